"""The grow rule of the context's device buffers (csrc/frt_devbuf.hpp DevBuf::reserve) without a
device: csrc/tools/devbuf_check.cpp, a program of its own over a counting allocator, built by the
Makefile's devbuf_asan target under the address and undefined-behaviour sanitizers and run once.
It checks growth, no reallocation when the buffer is large enough, the 16-byte floor, an empty
buffer of capacity 0 after an allocation that fails and a fresh allocation at the next call,
release through the owner's list (twice), and that nothing is live at the end.  CPU only; nothing
is loaded into this process."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devbuf_rule_under_sanitizers(tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "first_raytracer_amd"), "devbuf_asan", "OBJDIR=" + str(tmp_path)],
                   check=True, timeout=300)
    p = subprocess.run([str(tmp_path / "devbuf_asan")], capture_output=True, text=True, timeout=60)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr
    m = re.search(r"devbuf_check: (\d+) allocations, (\d+) frees, (\d+) live, (\d+) checks failed", p.stdout)
    assert m and int(m.group(1)) == int(m.group(2)) > 0 and int(m.group(3)) == 0 and int(m.group(4)) == 0
