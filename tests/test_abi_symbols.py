"""The C entry points libfrt.so exports (`nm -D --defined-only`, the ` T frt_`
lines) are the committed list tests/abi_symbols.txt: moving code between the
library's translation units must neither drop an entry point nor export a
new one.  CPU only."""
import os
import subprocess

import first_raytracer_amd as frt

HERE = os.path.dirname(os.path.abspath(__file__))


def exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return sorted(l.split(" T ", 1)[1] for l in out.splitlines() if " T frt_" in l)


def test_exported_entry_points_are_the_committed_list():
    with open(os.path.join(HERE, "abi_symbols.txt")) as f:
        want = f.read().split()
    assert len(want) == 41 and want == sorted(set(want))
    got = exported(os.path.join(os.path.dirname(os.path.abspath(frt.__file__)), "libfrt.so"))
    assert got == want, {"missing": sorted(set(want) - set(got)), "new": sorted(set(got) - set(want))}
