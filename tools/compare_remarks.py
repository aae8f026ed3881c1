"""Compare two MTG_BUILD_REMARKS directories (per-kernel resource usage of two builds): registers, scratch, spills, occupancy, LDS.
usage: python tools/compare_remarks.py <base_dir> <new_dir> [--all] [tu ...]
Prints the kernels that differ (--all: every kernel of the named translation units, or of all) and exits 1 if any kernel that both
builds have differs in VGPRs + AGPRs, scratch, occupancy or LDS; kernels only one build has are listed, not judged."""
import os
import re
import sys

FIELDS = {"TotalSGPRs": "sgpr", "VGPRs": "vgpr", "AGPRs": "agpr", r"ScratchSize \[bytes/lane\]": "scratch", "VGPRs Spill": "vspill",
          r"Occupancy \[waves/SIMD\]": "occ", r"LDS Size \[bytes/block\]": "lds"}
JUDGED = ("regs", "scratch", "occ", "lds")


def parse(d, only):
    out = {}
    for fn in sorted(os.listdir(d)):
        tu = fn[:-4]
        if not fn.endswith(".log") or (only and tu not in only):
            continue
        txt = open(os.path.join(d, fn), errors="replace").read()
        # "file:line:col: remark: Function Name: <mangled> [-Rpass-analysis=...]", then one remark line per figure (tools/kernel_resources.py)
        for block in re.split(r"remark: [^\n]*Function Name: ", txt)[1:]:
            row = {v: int((re.search(k + r": (\d+)", block) or [None, 0])[1]) for k, v in FIELDS.items()}
            row["regs"] = row["vgpr"] + row["agpr"]
            out[(tu, block.split()[0])] = row
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--all"]
    show_all = "--all" in sys.argv
    only = set(args[2:])
    a, b = parse(args[0], only), parse(args[1], only)
    differ = 0
    for key in sorted(b):
        tu, name = key
        if key not in a:
            print(f"{tu:18s} only in the new build   {name[:110]}")
            continue
        x, y = a[key], b[key]
        bad = any(x[f] != y[f] for f in JUDGED)
        differ += bad
        if show_all or bad or x["sgpr"] != y["sgpr"] or x["vspill"] != y["vspill"]:
            print(f"{tu:18s} " + " ".join(f"{f} {x[f]}->{y[f]}" for f in ("vgpr", "agpr", "sgpr", "scratch", "vspill", "occ", "lds"))
                  + ("  DIFFERS  " if bad else "  ") + name[:110])
    for tu, name in sorted(set(a) - set(b)):
        print(f"{tu:18s} only in the base build  {name[:110]}")
    print(f"{len(b)} kernels, {differ} that differ from the base in registers, scratch, occupancy or LDS")
    sys.exit(1 if differ else 0)


main()
