"""cuberille_set_band: are the kernels that existed before still the same code?  Disassembles the gfx950 code objects of the
parent's and this tree's libcuberille_hip.so (compare_walk_isa.kernels) and compares every kernel of the parent with its
instantiation here, instruction by instruction.  The change gave the five whole-volume sweep kernels and k_project a trailing
template parameter BAND (false for every instantiation that existed); the plain instantiations keep their scalar kernel
arguments as they were, and only the band instantiations take other types in the same argument places.  A kernel is matched by
its name and template arguments with that trailing `false` removed; argument lists are not part of the key.

    python profiles/compare_band_isa.py <parent's libcuberille_hip.so> midas-journal-740_amd/csrc/libcuberille_hip.so

Result: profiles/band_isa.txt.
"""
import re
import sys

from compare_walk_isa import kernels

BANDED = ("k_classify_flat", "k_classify_span", "k_classify_span_rows", "k_classify_tail", "k_classify_rows", "k_project")


def split_name(name):
    """'void ns::kernel<args>(params)' -> (kernel, [template args]); kernels without template arguments: (name, [])."""
    m = re.match(r"^(?:void )?(?:cuberille::)?(\w+)<(.*)>\(.*\)$", name)
    if not m:
        return re.sub(r"\(.*\)$", "", name), []
    return m.group(1), [a.strip() for a in m.group(2).split(",")]


def key(name, new):
    k, args = split_name(name)
    if new and k in BANDED:
        if args[-1] == "true":
            return None                              # a band instantiation: new
        assert args[-1] == "false", name
        args = args[:-1]
    if k == "k_classify_span" and len(args) == 1:    # (the parent's default span size is spelled out here)
        args.append("4096")
    return (k, tuple(args))


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    mine = {}
    new = 0
    for name, code in b.items():
        kk = key(name, True)
        if kk is None:
            new += 1
        else:
            assert kk not in mine, kk
            mine[kk] = code
    same, differ, kinds, per = 0, 0, set(), {}
    for name, code in a.items():
        kk = key(name, False)
        other = mine.pop(kk, None)
        if other is None:
            print("MISSING in the second library:", name[:140])
            continue
        if other == code:
            same += 1
            per.setdefault(kk[0], [0, 0])[0] += 1
            continue
        differ += 1
        per.setdefault(kk[0], [0, 0])[1] += 1
        if len(other) != len(code):
            print("DIFFERENT LENGTH:", name[:140], len(code), len(other))
            continue
        for x, y in zip(code, other):
            if x != y:
                kinds.add((re.sub(r"0x[0-9a-f]+", "IMM", x), tuple(re.findall(r"0x[0-9a-f]+", x)), tuple(re.findall(r"0x[0-9a-f]+", y))))
    print("%d kernels of the parent identical here, %d differ; band instantiations new here: %d; other new kernels: %d" % (
        same, differ, new, len(mine)))
    for k in sorted(per):
        print("  %-28s identical %3d, different %3d" % (k, per[k][0], per[k][1]))
    for k in sorted(kinds):
        print("  differing instruction:", k[0], k[1], "->", k[2])
    for kk in mine:
        print("  new:", kk)


if __name__ == "__main__":
    main()
