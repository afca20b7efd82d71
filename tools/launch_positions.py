#!/usr/bin/env python3
"""Diagnostic: assign every launch of a blocked fp32 inversion in a rocprofv3 kernel trace (csv) to its block and its
position in the block, and print the median durations by position.

    python tools/launch_positions.py <dir with *_kernel_trace.csv> [out.json]

The schedule is deterministic (blocked_invert): an inversion starts with blocked_init_kernel; a block is its panel
launches (gj_subpanel_kernel / gj_panel_multi_kernel / gj_diag_panel_kernel, one per sub-panel s, in order) and its
in-block update launches (gj_inblock_update_kernel), and ends with its rank-bw update.  The LAST in-block update launch
of a block is the one that carries strip(S-1), the outside-block strip tiles of the block's last sub-panel; panel launch
s > 0 carries strip(s-1).  The first inversion of the trace (cold caches, first-use initialisation) is left out.
"""
import csv
import glob
import json
import statistics
import sys


def spread(v):
    v = sorted(v)
    if not v:
        return None
    return {"n": len(v), "median_us": round(statistics.median(v), 2), "p10_us": round(v[len(v) // 10], 2),
            "p90_us": round(v[(9 * len(v)) // 10 - (1 if len(v) >= 10 else 0)], 2), "min_us": round(v[0], 2),
            "max_us": round(v[-1], 2)}


def short(name):
    return name.split("(")[0].replace("void ", "").replace("mi32::", "")


def main():
    f = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    inversions, cur = [], None
    for r in rows:
        name = short(r["Kernel_Name"])
        if name.startswith("blocked_init_kernel"):
            cur = []
            inversions.append(cur)
        if cur is not None:
            cur.append((name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    inversions = inversions[1:]
    ordinary, last = [], []
    last_by_block, panel = {}, {}  # block -> [us]; (block, s) -> (kernel, [us])
    by_kernel = {}
    for inv in inversions:
        blk, s, upd = 0, 0, []
        for name, us in inv:
            by_kernel.setdefault(name, []).append(us)
            if name.startswith(("gj_subpanel_kernel", "gj_panel_multi_kernel", "gj_diag_panel_kernel")):
                panel.setdefault((blk, s), (name, []))[1].append(us)
                s += 1
            elif name.startswith("gj_inblock_update_kernel"):
                upd.append(us)
            elif name.startswith("gj_rank_bw2_kernel"):
                if upd:
                    ordinary += upd[:-1]
                    last.append(upd[-1])
                    last_by_block.setdefault(blk, []).append(upd[-1])
                blk, s, upd = blk + 1, 0, []
    nblk = 1 + max(b for b, _ in panel)
    fused_by_s = {}
    for (b, s), (name, v) in panel.items():
        if name.endswith("true>"):
            fused_by_s.setdefault(s, []).extend(v)
    out = {
        "trace": f.split("/")[-1],
        "inversions": len(inversions),
        "update_ordinary": spread(ordinary),
        "update_block_last": spread(last),
        "update_block_last_median_us_by_block": [round(statistics.median(last_by_block[b]), 2) if b in last_by_block else None
                                                 for b in range(nblk)],
        "fused_panel_median_us_by_s": {str(s): round(statistics.median(v), 2) for s, v in sorted(fused_by_s.items())},
        "panel_median_us_by_block_and_s": [
            [round(statistics.median(panel[(b, s)][1]), 2) for s in range(1 + max(q for a, q in panel if a == b))]
            for b in range(nblk)],
        "panel_kernel_by_block": [sorted({panel[(a, s)][0] for a, s in panel if a == b}) for b in range(nblk)],
        "kernels": {k: spread(v) for k, v in sorted(by_kernel.items())},
    }
    for k in ("update_ordinary", "update_block_last"):
        print(k, out[k])
    print("block's last update, median by block:", out["update_block_last_median_us_by_block"])
    print("fused panel launches, median by s:", out["fused_panel_median_us_by_s"])
    for k, v in out["kernels"].items():
        print("%-52s n %5d median %8.2f us" % (k[:52], v["n"], v["median_us"]))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
