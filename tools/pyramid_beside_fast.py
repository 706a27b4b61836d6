#!/usr/bin/env python3
"""How k_pyramid_group fares beside k_fast_bands, from a rocprofv3 --kernel-trace csv of bench.py (several contexts in flight).

usage: pyramid_beside_fast.py <dir with *kernel_trace.csv> [skip_fraction]

A context's stream is serial and its pyramid comes before its FAST, so a FAST dispatch that overlaps a pyramid dispatch
always belongs to another context.  Prints
  - per pyramid launch of a pass (the groups differ in grid size): count, duration avg / min / max, and the same split by how
    much of the dispatch overlaps a k_fast_bands dispatch (none, under half, half or more);
  - the gap between the end of one FAST dispatch and the start of the next: avg / median / p90, which kernels fill it, and
    how often the next FAST's own pyramid (same stream) was still running after the previous FAST had ended -- i.e. the
    next FAST was waiting for its pyramid -- with the time from that pyramid's end to the FAST's start.
"""
import csv
import glob
import sys
from collections import defaultdict


def pct(v, p):
    v = sorted(v)
    return v[min(len(v) - 1, int(p * len(v)))] if v else 0


def overlap(s, e, iv):
    """length of [s, e) inside the sorted, disjoint intervals iv"""
    return sum(max(0, min(e, b) - max(s, a)) for a, b in iv if a < e and b > s)


def main():
    d = sys.argv[1]
    skip = float(sys.argv[2]) if len(sys.argv) > 2 else 0.3
    rows = []
    for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                q = r.get("Stream_Id") or r.get("Queue_Id") or "0"
                if q in ("0", "") and r.get("Queue_Id"):
                    q = r["Queue_Id"]
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].replace("void ", "").split("(")[0].split("<")[0],
                             q, int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0), int(r.get("LDS_Block_Size") or 0),
                             int(r.get("VGPR_Count") or 0)))
    rows.sort()
    t0, t1 = rows[0][0], max(r[1] for r in rows)
    lo = t0 + (t1 - t0) * skip  # start-up and warm-up
    rows = [r for r in rows if r[0] >= lo]
    fast = [r for r in rows if "k_fast_bands" in r[2]]
    pyr = [r for r in rows if "k_pyramid_group" in r[2]]
    if not fast or not pyr:
        print("no k_fast_bands / k_pyramid_group dispatches in the trace")
        return
    fiv = [(r[0], r[1]) for r in fast]
    us = 1e-3
    fd = [(e - s) * us for s, e in fiv]
    conc = sum(1 for i in range(1, len(fiv)) if fiv[i][0] < fiv[i - 1][1])
    print("k_fast_bands: n %d, avg %.1f us, min %.1f, max %.1f; dispatches that start before the previous one ended: %d"
          % (len(fd), sum(fd) / len(fd), min(fd), max(fd), conc))
    print()
    print("k_pyramid_group per launch of a pass (grid = workgroups x 256 threads)")
    print("%-26s %6s %9s %9s %9s" % ("", "n", "avg us", "min us", "max us"))
    for grid in sorted({r[4] for r in pyr}, reverse=True):
        P = [r for r in pyr if r[4] == grid]
        ov = [overlap(r[0], r[1], fiv) / max(1, r[1] - r[0]) for r in P]
        dur = [(r[1] - r[0]) * us for r in P]
        print("grid %d threads" % grid)
        for name, sel in (("all", lambda o: True), ("no FAST beside it", lambda o: o == 0),
                          ("FAST beside it < 50 %", lambda o: 0 < o < 0.5), ("FAST beside it >= 50 %", lambda o: o >= 0.5)):
            v = [x for x, o in zip(dur, ov) if sel(o)]
            if v:
                print("  %-24s %6d %9.1f %9.1f %9.1f" % (name, len(v), sum(v) / len(v), min(v), max(v)))
        top = sorted(zip(dur, ov), reverse=True)[:max(1, len(dur) // 10)]
        print("  the longest tenth: avg %.1f us, of which beside FAST %.0f %%" % (sum(x for x, _ in top) / len(top),
                                                                              100 * sum(o for _, o in top) / len(top)))
    print()
    gaps, fill, waited, wait_tail, own_start_late = [], defaultdict(float), 0, [], 0
    periods = []
    for i in range(1, len(fast)):
        a, b = fast[i - 1][1], fast[i][0]
        periods.append((fast[i][0] - fast[i - 1][0]) * us)
        gaps.append((b - a) * us)
        if b > a:
            for r in rows:
                if r[1] > a and r[0] < b and "k_fast_bands" not in r[2]:
                    fill[r[2]] += (min(b, r[1]) - max(a, r[0])) * us
        own = [r for r in pyr if r[3] == fast[i][3] and r[1] <= fast[i][0]]
        if own:
            last = max(own, key=lambda r: r[1])
            if last[1] > a:  # its own pyramid ended after the previous FAST had: the FAST could not have started at a
                waited += 1
                wait_tail.append((b - last[1]) * us)
                if last[0] >= a:
                    own_start_late += 1
    n = len(gaps)
    print("FAST to FAST: start-to-start %.1f us avg; gap (end of one to start of the next): avg %.1f us, median %.1f, p90 %.1f, max %.1f (n %d)"
          % (sum(periods) / n, sum(gaps) / n, pct(gaps, 0.5), pct(gaps, 0.9), max(gaps), n))
    tot = sum(max(0.0, g) for g in gaps)
    print("kernel time inside the gaps, per gap (kernels overlap, so the shares can add up to more than the gap):")
    for k, v in sorted(fill.items(), key=lambda kv: -kv[1])[:8]:
        print("  %-40s %7.1f us (%.0f %% of the gap time)" % (k, v / n, 100 * v / max(tot, 1e-9)))
    print("next FAST's own last pyramid launch ended after the previous FAST did: %d of %d gaps (%.0f %%); it even started after it: %d;"
          % (waited, n, 100.0 * waited / n, own_start_late))
    if wait_tail:
        print("  from that pyramid's end to the FAST's start: avg %.1f us, median %.1f" % (sum(wait_tail) / len(wait_tail), pct(wait_tail, 0.5)))


if __name__ == "__main__":
    main()
