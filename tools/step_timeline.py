"""tools/step_timeline.py — the launch timeline of the LAST step of a `bench.py` run under `rocprofv3 --kernel-trace` (diagnostic).
Usage: python tools/step_timeline.py <kernel_trace.csv> [--json OUT]
A step is delimited by the host synchronisation between steps (the roots download): the longest idle gap between the last two DEEP-ALI merges
(k_ali_merge, one per step) starts the last step.  Prints every launch of that step (start / end relative to the step's first launch, duration,
queue, grid) and the critical-path summary: how long the chip ran one stream, both, or nothing, and what ran after the 2^23-leaf launch."""
import csv, json, sys


def load(path):
    rows = []
    for r in csv.DictReader(open(path)):
        rows.append({"name": r["Kernel_Name"], "s": int(r["Start_Timestamp"]), "e": int(r["End_Timestamp"]),
                     "q": r.get("Queue_Id", r.get("Stream_Id", "?")), "stream": r.get("Stream_Id", "?"),
                     "grid": int(r.get("Grid_Size", r.get("Grid_Size_X", 0)) or 0), "wg": int(r.get("Workgroup_Size", r.get("Workgroup_Size_X", 0)) or 0)})
    rows.sort(key=lambda r: r["s"])
    return rows


def last_step(rows):
    merges = [i for i, r in enumerate(rows) if "k_ali_merge" in r["name"]]
    if len(merges) < 2:
        return rows
    a, b = merges[-2], merges[-1]
    best, cut, end = -1, a + 1, rows[a]["e"]
    for i in range(a + 1, b + 1):
        gap = rows[i]["s"] - end
        if gap > best:
            best, cut = gap, i
        end = max(end, rows[i]["e"])
    return rows[cut:]


def short(name):
    n = name.split("(")[0]
    return n.replace("void ", "").replace("stark::", "")[:60]


def summarize(seq):
    t0 = seq[0]["s"]
    out = []
    for r in seq:
        out.append({"start_us": round((r["s"] - t0) / 1e3, 1), "end_us": round((r["e"] - t0) / 1e3, 1), "dur_us": round((r["e"] - r["s"]) / 1e3, 1),
                    "queue": r["q"], "grid": r["grid"], "wg": r["wg"], "kernel": short(r["name"])})
    # time with 0 / 1 / 2+ launches in flight
    ev = sorted([(r["s"], 1) for r in seq] + [(r["e"], -1) for r in seq])
    lvl, last, acc = 0, ev[0][0], {0: 0, 1: 0, 2: 0}
    for t, d in ev:
        acc[min(lvl, 2)] += t - last
        lvl += d; last = t
    end = max(r["e"] for r in seq)
    leaf = max((r for r in seq if "k_leaf_pair2" in r["name"]), key=lambda r: r["grid"], default=None)
    summ = {"step_us": round((end - t0) / 1e3, 1), "idle_us": round(acc[0] / 1e3, 1), "one_launch_us": round(acc[1] / 1e3, 1),
            "overlap_us": round(acc[2] / 1e3, 1), "launches": len(seq)}
    if leaf:
        summ["leaf0_start_us"] = round((leaf["s"] - t0) / 1e3, 1); summ["leaf0_end_us"] = round((leaf["e"] - t0) / 1e3, 1)
        summ["after_leaf0_us"] = round((end - leaf["e"]) / 1e3, 1)
    return out, summ


if __name__ == "__main__":
    rows = load(sys.argv[1])
    seq = last_step(rows)
    launches, summ = summarize(seq)
    for l in launches:
        print(f"{l['start_us']:10.1f} {l['end_us']:10.1f} dur {l['dur_us']:9.1f}  q {l['queue']:>3}  grid {l['grid']:>9}  {l['kernel']}")
    print(json.dumps(summ))
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump({"summary": summ, "launches": launches}, f, indent=0)
            f.write("\n")
