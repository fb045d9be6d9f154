"""Gaps between consecutive dense scans in a rocprofv3 kernel trace.

    python scripts/scan_gaps.py KERNEL_TRACE_CSV [--scan REGEX] [--keep STEPS --out CSV]

Reads the kernel_trace.csv of `rocprofv3 --kernel-trace`, takes the launches whose name matches --scan (default: the
dense prefilter's scan kernels) in start order and prints, over the second half of the run (the steady state), the
scan's duration, the gap from the end of scan i to the start of scan i+1 and the period start-to-start, plus the mean
duration of every other kernel.  --keep writes the last STEPS scans' worth of trace rows (all kernels, times relative
to the first kept row) to --out: small enough to keep under profiles/."""
import argparse
import csv
import re
import statistics as st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--scan", default=r"dense_prefilter(_i8)?_(scan|pair)_kernel")
    ap.add_argument("--keep", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = list(csv.DictReader(open(a.trace)))
    for r in rows:
        r["_s"], r["_e"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    rows.sort(key=lambda r: r["_s"])
    pat = re.compile(a.scan)
    scans = [r for r in rows if pat.search(r["Kernel_Name"])]
    if len(scans) < 4:
        raise SystemExit(f"only {len(scans)} launches match {a.scan!r}")
    half = scans[len(scans) // 2:]
    dur = [(r["_e"] - r["_s"]) / 1e3 for r in half]
    gap = [(b["_s"] - a_["_e"]) / 1e3 for a_, b in zip(half, half[1:])]
    per = [(b["_s"] - a_["_s"]) / 1e3 for a_, b in zip(half, half[1:])]

    def line(name, v):
        q = sorted(v)
        print(f"{name:28s} n={len(v):4d}  mean {st.mean(v):8.2f}  median {st.median(v):8.2f}  "
              f"p10 {q[len(q) // 10]:8.2f}  p90 {q[len(q) * 9 // 10]:8.2f}  us")

    print(f"scan launches: {len(scans)} (statistics over the last {len(half)}), queue ids: "
          f"{sorted({r.get('Queue_Id', '?') for r in half})}")
    line("scan duration", dur)
    line("gap scan i end -> i+1 start", gap)
    line("period start -> start", per)
    t0 = half[0]["_s"]
    other = {}
    for r in rows:
        if r["_s"] >= t0 and not pat.search(r["Kernel_Name"]):
            other.setdefault((r["Kernel_Name"], r.get("Queue_Id", "?")), []).append((r["_e"] - r["_s"]) / 1e3)
    for (name, q), v in sorted(other.items(), key=lambda kv: -sum(kv[1])):
        line(f"{name[:60]} [queue {q}]", v)
    if a.keep and a.out:
        first = scans[-a.keep]["_s"] if len(scans) > a.keep else scans[0]["_s"]
        cols = ["Queue_Id", "Kernel_Name", "Start_us", "End_us", "Workgroup_Size_X", "Grid_Size_X", "VGPR_Count",
                "LDS_Block_Size"]
        with open(a.out, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(cols)
            for r in rows:
                if r["_s"] < first:
                    continue
                w.writerow([r.get("Queue_Id", ""), r["Kernel_Name"], f"{(r['_s'] - first) / 1e3:.2f}",
                            f"{(r['_e'] - first) / 1e3:.2f}", r.get("Workgroup_Size_X", ""), r.get("Grid_Size_X", ""),
                            r.get("VGPR_Count", ""), r.get("LDS_Block_Size", "")])


if __name__ == "__main__":
    main()
