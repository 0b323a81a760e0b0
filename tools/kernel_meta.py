#!/usr/bin/env python3
"""Per-kernel build metadata of a libfrt.so, without a GPU: VGPR / AGPR / SGPR
counts, scratch (private segment) and static LDS (group segment) sizes and the
spill counts, read from the code objects' metadata notes.

  python tools/kernel_meta.py first_raytracer_amd/libfrt.so > new.json
  python tools/kernel_meta.py --diff parent.json new.json [--filter REGEX]

--diff lists the kernels of the first file whose VGPR / AGPR / scratch / LDS /
VGPR-spill figures differ in the second, and counts the kernels only one has.
A trailing `false` template argument that the second build added to the PSS-MLT
kernels (mlt_bootstrap / mlt_megakernel <..., ENV = false>) is ignored when
names are matched."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size",
        "vgpr_spill_count", "sgpr_spill_count", "kernarg_segment_size")
GATE = ("vgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count")


def notes_kernels(code_object):
    txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", code_object], capture_output=True,
                         text=True, check=True).stdout
    lines = txt.splitlines()
    start = [i for i, l in enumerate(lines) if l.strip() == "amdhsa.kernels:"]
    if not start:
        return {}
    out, cur, ind = [], None, None
    for l in lines[start[0] + 1:]:
        m = re.match(r"(\s*)- \.(\w+):\s*(.*)", l)
        if m and ind is None:
            ind = len(m.group(1))
        if m and len(m.group(1)) == ind:          # a new kernel's first key
            cur = {}
            out.append(cur)
            k, v = m.group(2), m.group(3)
        else:
            m = re.match(r"(\s+)\.(\w+):\s*(.*)", l)
            if not m or cur is None or len(m.group(1)) != ind + 2:
                continue
            k, v = m.group(2), m.group(3)
        cur[k] = v.strip().strip("'")
    return {d["name"]: {k: int(d[k]) for k in KEYS if k in d} for d in out if "name" in d}


def library_kernels(so):
    """Every gfx950 kernel of the library: its fat binary holds one bundle per translation unit."""
    res = {}
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", so,
                        os.path.join(d, "rest.o")], check=True)
        data = open(fat, "rb").read()
        offs = [m.start() for m in re.finditer(rb"__CLANG_OFFLOAD_BUNDLE__", data)]
        for n, o in enumerate(offs):
            part, co = os.path.join(d, f"b{n}.bin"), os.path.join(d, f"co{n}.o")
            with open(part, "wb") as f:
                f.write(data[o:offs[n + 1] if n + 1 < len(offs) else len(data)])
            subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={part}",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True,
                           stderr=subprocess.DEVNULL)
            res.update(notes_kernels(co))
    return res


def demangled(names):
    for tool in (os.path.join(LLVM, "llvm-cxxfilt"), "c++filt"):
        try:
            p = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
        except OSError:
            continue
        if p.returncode == 0:
            return dict(zip(names, p.stdout.splitlines()))
    return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="+")
    ap.add_argument("--diff", action="store_true")
    ap.add_argument("--filter", default="", help="regex on the demangled kernel name")
    a = ap.parse_args()
    if not a.diff:
        json.dump(library_kernels(a.files[0]), sys.stdout, indent=0, sort_keys=True)
        return 0
    old, new = (json.load(open(f)) for f in a.files[:2])
    strip = lambda k: re.sub(r"(mlt_(?:bootstrap|megakernel)I.*?)Lb0EEEv", r"\1EEv", k)   # noqa: E731
    by_old = {}
    for k, v in new.items():
        by_old.setdefault(strip(k) if strip(k) in old else k, v)
    names = demangled(sorted(old))
    changed = 0
    for k in sorted(old):
        if a.filter and not re.search(a.filter, names[k]):
            continue
        if k not in by_old:
            print("missing in the second build:", names[k])
            changed += 1
            continue
        d = {x: (old[k].get(x), by_old[k].get(x)) for x in GATE if old[k].get(x) != by_old[k].get(x)}
        if d:
            changed += 1
            print(names[k], d)
    print(f"{len(old)} kernels in the first build, {len(new)} in the second, "
          f"{len([k for k in by_old if k not in old])} new; {changed} differ")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
