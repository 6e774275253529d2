"""Are the kernels of two builds of the library the same code?  Disassembles the gfx950 code objects of two
libcuberille_hip.so files and compares them kernel by kernel, instruction by instruction (branch targets and pc-relative literals aside,
which move with a kernel's place in the code object).  Written for cuberille_set_border: k_project gained a template parameter (PAD,
false for every instantiation that existed) and two trailing kernel arguments the unpadded instantiations never read.

    bash profiles/ab.sh            # csrc/libcuberille_prev.so from HEAD
    python profiles/compare_walk_isa.py midas-journal-740_amd/csrc/libcuberille_prev.so midas-journal-740_amd/csrc/libcuberille_hip.so

Result for the change that added the border (parent aab1e2c): 157 kernels identical; the 90 unpadded k_project instantiations
differ in ONE immediate only -- the offset of the hidden kernel arguments behind the explicit ones, 0x1f8 -> 0x208 (the two
new 8-byte arguments) in `s_load_dword s6, s[0:1], ...` and `s_add_u32 sN, s0, ...` -- and in nothing else; 30 padded
instantiations are new.  The change that added the region (cuberille_set_region: a REGION template parameter and two more
trailing arguments, the pitches): profiles/region_walk_isa.txt.
"""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")


def kernels(lib):
    """{demangled kernel name: [instruction text]} of the gfx950 code object inside `lib`."""
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(lib, os.path.join(tmp, "lib.so"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp, capture_output=True, check=True)
        co = glob.glob(os.path.join(tmp, "lib.so.*gfx950*"))[0]
        text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], capture_output=True, text=True,
                              check=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            t = re.sub(r"<[^>]*>", "", line.split("//")[0]).strip()
            t = re.sub(r"^(s_c?branch\w*|s_getpc\w*)\s.*", r"\1", t)
            # (the literal of a pc-relative address: s_getpc_b64 is followed by s_add_u32 sN, sN, <offset> / s_addc_u32)
            cur.append(re.sub(r"^(s_addc?_u32 (s\d+), \2), 0x[0-9a-f]+$", r"\1, PCREL", t))
    names = list(out)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {p: out[n] for p, n in zip(plain, names)}


def renamed(name):
    """The parent's name of a k_project instantiation in this tree.  The border change: k_project<T, MODE, GEOM>(...) became
    k_project<T, MODE, GEOM, false>(..., double, long long); the region change: k_project<T, MODE, GEOM, PAD>(..., double, long
    long) became k_project<T, MODE, GEOM, PAD, false>(..., double, long long, long long, long long)."""
    if "k_project<" not in name:
        return name
    if name.endswith("double, long long)"):
        return re.sub(r"k_project<([^>]*)>", lambda m: "k_project<%s, false>" % m.group(1), name).replace(
            "double, long long)", "double, long long, long long, long long)")
    return re.sub(r"k_project<([^>]*)>", lambda m: "k_project<%s, false>" % m.group(1), name).replace("int)", "int, double, long long)")


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    same, differ, kinds = 0, 0, set()
    for name, code in a.items():
        other = b.get(renamed(name))
        if other is None:
            print("MISSING in the second library:", name[:140])
            continue
        if other == code:
            same += 1
            continue
        differ += 1
        if len(other) != len(code):
            print("DIFFERENT LENGTH:", name[:140], len(code), len(other))
            continue
        for x, y in zip(code, other):
            if x != y:
                kinds.add((re.sub(r"0x[0-9a-f]+", "IMM", x), tuple(re.findall(r"0x[0-9a-f]+", x)), tuple(re.findall(r"0x[0-9a-f]+", y))))
    print("%d kernels identical, %d differ; new in the second library: %d" % (same, differ, len(set(b) - {renamed(n) for n in a})))
    for k in sorted(kinds):
        print("  differing instruction:", k[0], k[1], "->", k[2])


if __name__ == "__main__":
    main()
