#!/usr/bin/env python3
"""Per-kernel build metadata of a libfrt.so, without a GPU: VGPR / AGPR / SGPR
counts, scratch (private segment) and static LDS (group segment) sizes and the
spill counts, read from the code objects' metadata notes; a hash of each
kernel's instruction encodings (`insn_hash`: the encoding words of the
disassembly, without addresses, so it does not move with the function); and
the code objects each kernel name occurs in (`code_objects`; names in more
than one are listed on stderr).

  python tools/kernel_meta.py first_raytracer_amd/libfrt.so > new.json
  python tools/kernel_meta.py --diff parent.json new.json [--filter REGEX]

--diff lists the kernels of the first file whose VGPR / AGPR / scratch / LDS /
VGPR-spill figures, (where both files record one) instruction hash or code
objects (the translation units that hold the kernel, by link order) differ in
the second, and counts the kernels only one has.
A trailing `false` template argument that the second build added to the PSS-MLT
kernels (mlt_bootstrap / mlt_megakernel <..., ENV = false>) is ignored when
names are matched."""
import argparse
import hashlib
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


def insn_hashes(code_object, names):
    """sha256 (16 hex digits) over the encoding words of each named function, in order: the
    `// ADDRESS: WORDS` column of llvm-objdump -d up to the symbol's size (the alignment padding
    after it is not the kernel's), the address and the <symbol+offset> comments dropped."""
    tool = lambda t, *a: subprocess.run([os.path.join(LLVM, t), *a, code_object], capture_output=True,   # noqa: E731
                                        text=True, check=True).stdout
    size = {}
    for l in tool("llvm-readelf", "-s", "--wide").splitlines():
        f = l.split()
        if len(f) == 8 and f[3] == "FUNC" and f[7] in names:
            size[f[7]] = int(f[2])
    res, h, end = {}, None, 0
    for l in tool("llvm-objdump", "-d").splitlines():
        m = re.match(r"([0-9a-f]+) <(.+)>:$", l)
        if m:
            name = m.group(2)
            h = res.setdefault(name, hashlib.sha256()) if name in size else None
            end = int(m.group(1), 16) + size.get(name, 0)
            continue
        m = re.search(r"//\s*([0-9A-Fa-f]+):((?: [0-9A-Fa-f]{8})+)", l) if h else None
        if m and int(m.group(1), 16) < end:
            h.update(m.group(2).encode())
    return {k: v.hexdigest()[:16] for k, v in res.items()}


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
            kernels = notes_kernels(co)
            hashes = insn_hashes(co, set(kernels))
            for k, v in kernels.items():
                v["insn_hash"] = hashes.get(k)
                v["code_objects"] = [n]
                if k in res:                      # a second copy: the first one's figures stay
                    res[k]["code_objects"].append(n)
                    if res[k]["insn_hash"] != v["insn_hash"]:
                        res[k]["copies_differ"] = True
                else:
                    res[k] = v
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
        kernels = library_kernels(a.files[0])
        json.dump(kernels, sys.stdout, indent=0, sort_keys=True)
        dup = sorted(k for k, v in kernels.items() if len(v["code_objects"]) > 1)
        for k, name in demangled(dup).items():
            print("in more than one code object:", name, kernels[k]["code_objects"], file=sys.stderr)
        print(f"{len(kernels)} kernels, {len(dup)} in more than one code object", file=sys.stderr)
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
        gate = GATE + (("insn_hash",) if old[k].get("insn_hash") and by_old[k].get("insn_hash") else ())
        gate += ("code_objects",)             # the units link in one order: the indices compare
        d = {x: (old[k].get(x), by_old[k].get(x)) for x in gate if old[k].get(x) != by_old[k].get(x)}
        if d:
            changed += 1
            print(names[k], d)
    print(f"{len(old)} kernels in the first build, {len(new)} in the second, "
          f"{len([k for k in by_old if k not in old])} new; {changed} differ")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
