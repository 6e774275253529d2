"""Are the kernels of two builds of the library the same code?  Disassembles the gfx950 code objects of two
libcuberille_hip.so files and compares them kernel by kernel, instruction by instruction (branch targets and pc-relative
literals aside, which move with a kernel's place in the code object).  It compares instructions only.

    python profiles/compare_isa.py <parent's libcuberille_hip.so> midas-journal-740_amd/csrc/libcuberille_hip.so

A kernel is matched by its canonical name: the kernel and its template arguments, argument lists aside.  Two rename rules are
kept here.  The row sweeps: the parent's six kernels by source (k_classify_span_rows / _pad_span_rows / _region_span_rows,
k_classify_rows / _pad_words / _region_words) are k_classify_span_rows<T, Rows<T>, BAND> and k_classify_words<T, Rows<T>, BAND>
here (ROW_SWEEPS; result: profiles/span_rows_isa.txt, where those 80 are meant to differ).  The source views: the walk's three trailing bools of the parent (PAD, REGION, BAND, at most one true)
are its one VIEW value here (0 whole, 1 border, 2 region, 3 band).  Results: profiles/view_isa.txt, profiles/point_normals_isa.txt,
profiles/view_sampler_isa.txt (the vertex side on one Sampler<T, VIEW>: no rename rule; every k_project, k_point_normals,
k_cell_pixels and k_gradient_image and everything outside the vertex side identical, the two lane-per-vertex walks
k_project_variant and k_project_bspline meant to differ; their registers in profiles/view_sampler_resource_usage.txt); the comparisons of the
changes that added the border, the region and the band (region_walk_isa.txt, band_isa.txt) were made by this script's
predecessors, which git history keeps (profiles/README.md).
"""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
VIEW_OF_BOOLS = {("false", "false", "false"): "0", ("true", "false", "false"): "1", ("false", "true", "false"): "2",
                 ("false", "false", "true"): "3"}
# the six row sweeps of the parent -> the two kernels here and their source of rows (<T[, BAND]> -> <T, Rows<T>, BAND>)
ROW_SWEEPS = {"k_classify_pad_span_rows": ("k_classify_span_rows", "RingRows"),
              "k_classify_region_span_rows": ("k_classify_span_rows", "PitchedRows"),
              "k_classify_rows": ("k_classify_words", "ContiguousRows"),
              "k_classify_pad_words": ("k_classify_words", "RingRows"),
              "k_classify_region_words": ("k_classify_words", "PitchedRows")}


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
            if line.strip() == "...":      # (zero bytes the disassembler elides: the padding behind a kernel's s_endpgm, which moves
                continue                   #  with what the linker places next)
            t = re.sub(r"<[^>]*>", "", line.split("//")[0]).strip()
            t = re.sub(r"^(s_c?branch\w*|s_getpc\w*)\s.*", r"\1", t)
            # (the literal of a pc-relative address: s_getpc_b64 is followed by s_add_u32 sN, sN, <offset> / s_addc_u32)
            cur.append(re.sub(r"^(s_addc?_u32 (s\d+), \2), 0x[0-9a-f]+$", r"\1, PCREL", t))
    names = list(out)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {p: out[n] for p, n in zip(plain, names)}


def canonical(name):
    """'void ns::kernel<args>(params)' -> (kernel, (template args)), the walk's three view bools as the view value."""
    m = re.match(r"^(?:void )?(?:cuberille::)?(\w+)<(.*)>\(.*\)$", name)
    if not m:
        return re.sub(r"\(.*\)$", "", name), ()
    args = [a.strip().replace("cuberille::", "") for a in m.group(2).split(",")]
    if m.group(1) == "k_project" and tuple(args[-3:]) in VIEW_OF_BOOLS:
        args[-3:] = [VIEW_OF_BOOLS[tuple(args[-3:])]]
    if m.group(1) == "k_classify_span_rows" and len(args) == 2:
        return m.group(1), (args[0], "ContiguousRows<%s>" % args[0], args[1])
    if m.group(1) in ROW_SWEEPS:
        kernel, rows = ROW_SWEEPS[m.group(1)]
        return kernel, (args[0], "%s<%s>" % (rows, args[0]), args[1] if len(args) > 1 else "false")
    return m.group(1), tuple(args)


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    mine = {}
    for name, code in b.items():
        assert canonical(name) not in mine, name
        mine[canonical(name)] = code
    per, kinds, missing = {}, set(), 0
    for name, code in a.items():
        k = canonical(name)
        other = mine.pop(k, None)
        if other is None:
            missing += 1
            print("MISSING in the second library:", name[:140])
            continue
        per.setdefault(k[0], [0, 0])[other != code] += 1
        if len(other) != len(code):
            print("DIFFERENT LENGTH:", name[:140], len(code), len(other))
        elif other != code:
            for x, y in zip(code, other):
                if x != y:
                    kinds.add((re.sub(r"0x[0-9a-f]+", "IMM", x), tuple(re.findall(r"0x[0-9a-f]+", x)), tuple(re.findall(r"0x[0-9a-f]+", y))))
    print("%d kernels of the first library identical in the second, %d differ, %d missing; new in the second: %d" % (
        sum(p[0] for p in per.values()), sum(p[1] for p in per.values()), missing, len(mine)))
    for k in sorted(per):
        print("  %-32s identical %3d, different %3d" % (k, per[k][0], per[k][1]))
    for k in sorted(kinds):
        print("  differing instruction:", k[0], k[1], "->", k[2])
    for k in mine:
        print("  new:", k)
    return 1 if missing or mine or any(p[1] for p in per.values()) else 0


if __name__ == "__main__":
    sys.exit(main())
