"""Kernel-by-kernel comparison of two gfx950 assembly files (hipcc --save-temps output):

    python tools/isa_diff.py base.s new.s [-v]

Per kernel symbol: "identical" (same instruction text, block labels renumbered), "reordered" (same count of every
mnemonic) or "differs" (with the per-mnemonic deltas), and any change of the resource lines (next_free_vgpr /
next_free_sgpr / accum_offset / LDS / scratch / spill counts).  Exit status 1 when the kernel sets differ, a kernel
differs, a resource line moves, or a kernel uses scratch or spills."""
import re
import sys
from collections import Counter

RES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")


def parse(path):
    text = open(path).read().splitlines()
    kernels, cur = {}, None
    for ln in text:
        m = re.match(r"\s*\.type\s+(\S+),@function", ln)
        if m:
            cur = kernels.setdefault(m.group(1), {"ins": [], "res": {}})
            continue
        if cur is not None and re.match(r"\.Lfunc_end\d+:", ln):
            cur = None
            continue
        if cur is not None:
            s = ln.split(";")[0].strip()
            if s and not s.startswith("."):
                cur["ins"].append(s)
            elif s.startswith(".L") and s.endswith(":"):
                cur["ins"].append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    sym = None
    for ln in text:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            sym = m.group(1)
        m = re.match(r"\s*\.amdhsa_(\w+)\s+(\d+)", ln)
        if sym in kernels and m and m.group(1) in RES:
            kernels[sym]["res"][m.group(1)] = int(m.group(2))
        m = re.match(r"\s*\.name:\s+(\S+)", ln)
        if m:
            sym = m.group(1)
        m = re.match(r"\s*\.(\w+_spill_count):\s+(\d+)", ln)
        if sym in kernels and m:
            kernels[sym]["res"][m.group(1)] = int(m.group(2))
    for k in kernels.values():
        k["ins"] = [re.sub(r"\.LBB\d+_", ".LBB_", i) for i in k["ins"]]
        k["mn"] = Counter(i.split()[0] for i in k["ins"] if not i.endswith(":"))
    return kernels


def main(argv):
    verbose = "-v" in argv
    a, b = (parse(p) for p in argv[1:3])
    bad = False
    if set(a) != set(b):
        bad = True
        for s in sorted(set(a) ^ set(b)):
            print(f"only in {'base' if s in a else 'new'}: {s}")
    tally = Counter()
    for s in sorted(set(a) & set(b)):
        ka, kb = a[s], b[s]
        if ka["ins"] == kb["ins"]:
            verdict = "identical"
        elif ka["mn"] == kb["mn"]:
            verdict = "reordered"
        else:
            verdict = "differs"
        tally[verdict] += 1
        notes = []
        if ka["res"] != kb["res"]:
            notes.append("resources " + ", ".join(f"{k} {ka['res'].get(k)} -> {kb['res'].get(k)}"
                                                   for k in sorted(set(ka["res"]) | set(kb["res"]))
                                                   if ka["res"].get(k) != kb["res"].get(k)))
        if kb["res"].get("private_segment_fixed_size") or kb["res"].get("vgpr_spill_count") or kb["res"].get("sgpr_spill_count"):
            notes.append("scratch / spills")
        if verdict == "differs":
            d = {m: kb["mn"][m] - ka["mn"][m] for m in set(ka["mn"]) | set(kb["mn"]) if kb["mn"][m] != ka["mn"][m]}
            notes.append(f"{len(ka['ins'])} -> {len(kb['ins'])} lines; " + " ".join(f"{m} {v:+d}" for m, v in sorted(d.items())))
        bad |= verdict == "differs" or bool(notes)
        if verbose or verdict != "identical" or notes:
            print(f"{verdict:9s} {s}" + ("".join(f"\n          {n}" for n in notes)))
    print(f"{argv[2]}: " + ", ".join(f"{n} {v}" for v, n in sorted(tally.items())) + f" of {len(set(a) & set(b))} kernels")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
