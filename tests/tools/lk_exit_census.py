#!/usr/bin/env python3
"""Census of what the Lucas-Kanade yardstick (tests/lk_ref.py) reaches on the cases of tests/lk_cases.py (the hut_long crops) and
of tests/lk_edge_cases.py (synthetic): exits of a level by kind, edge and patch size, classes of inverse Hessians, classes of
patch fit at the boundary.  CPU only; lk_edge_cases.Census wraps the yardstick's functions and leaves its arithmetic alone.

    python tests/tools/lk_exit_census.py [--out profiles/lk_exit_census.txt]
"""
import argparse
import collections
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import lk_cases as LC  # noqa: E402
import lk_edge_cases as EC  # noqa: E402


def starts(n, prefix):
    return sum(v for k, v in n.items() if k.startswith(prefix))


def table(n):
    """the rows of the issue's census, in its order"""
    e = "leave-the-level exit, "
    return [("Inverse Hessians computed", n["inverse"]),
            ("  of them finite", starts(n, "inverse finite")),
            ("Singular Hessian (1/det = inf)", n["inverse singular (1/det = inf)"]),
            ("Arithmetic NaN in invH[0]", starts(n, "inverse nan0")),
            ("invH[0] = inf", starts(n, "inverse inf0")),
            ("Inf or NaN inverse used while tracking", n["inf or NaN inverse used while tracking"]),
            ("isnan(x) exit of the iteration loop", n["isnan(x) exit of the iteration loop"]),
            ("ft_floor_int saturation behind an inf position", n["ft_floor_int saturation behind an inf position"]),
            ("Leave-the-level exits at the bottom edge (v == h-half)", n[e + "bottom edge (v == h-half)"]),
            ("Leave-the-level exits at the right edge (u == w-half)", n[e + "right edge (u == w-half)"]),
            ("Leave-the-level exits at the left edge (u == half-1)", n[e + "left edge (u == half-1)"]),
            ("Leave-the-level exits at the top edge (v == half-1)", n[e + "top edge (v == half-1)"]),
            ("Leave-the-level exits further out", n[e + "further out"]),
            ("Patch-32 level runs", n["level runs, patch 32"]),
            ("Iteration exhaustion at patch 8", n["iteration exhaustion, patch 8"]),
            ("Iteration exhaustion at patch 16", n["iteration exhaustion, patch 16"]),
            ("Iteration exhaustion at patch 32", n["iteration exhaustion, patch 32"]),
            ("Converged at iteration one", n["converged at iteration one"]),
            ("Converged at the last iteration", n["converged at the last iteration"])]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    old, new, per_case = collections.Counter(), collections.Counter(), {}
    for name, (kind, opts, get) in LC.cases().items():
        with EC.Census() as c:
            LC.run_case(kind, opts, get())
        old.update(c.n)
        per_case["lk_cases: " + name] = c.n
    for name in EC.cases():
        n = EC.census(name)[0]
        new.update(n)
        per_case["lk_edge_cases: " + name] = n
    with EC.Census() as c:
        EC.bundle_uncached()
    new.update(c.n)
    per_case["lk_edge_cases: the bundle (%s)" % ", ".join(EC.BUNDLE["cameras"])] = c.n
    out = open(args.out, "w") if args.out else sys.stdout
    w = out.write
    w("Census of the Lucas-Kanade yardstick tests/lk_ref.py (tests/tools/lk_exit_census.py, CPU only).\n"
      "  existing = the ten cases of tests/lk_cases.py (384x256 hut_long crops, levels 0..4, default threshold)\n"
      "  new      = the %d cases of tests/lk_edge_cases.py and its bundle (synthetic frames of 192x176, 176x208 and 208x160)\n\n" % len(EC.cases()))
    w("%-58s %10s %10s\n" % ("what", "existing", "new"))
    for (what, a), (_, b) in zip(table(old), table(new)):
        w("%-58s %10d %10d\n" % (what, a, b))
    w("\nft_floor_int saturation stays at 0: an exactly singular H gives NaN updates, never +-inf (tests/test_lk_edge_cases_cpu.py,\n"
      "module docstring and test_exactly_singular_hessians_give_nan_updates_never_inf); a determinant that only rounds to zero on a\n"
      "regular H needs a template no detector selects.\n")
    w("\nEvery class, existing | new:\n")
    for k in sorted(set(old) | set(new)):
        w("  %-66s %8d %8d\n" % (k, old[k], new[k]))
    w("\nPer case (classes that occur):\n")
    for name, n in per_case.items():
        w("\n%s\n" % name)
        for k in sorted(n):
            w("  %-66s %8d\n" % (k, n[k]))
    if args.out:
        out.close()


if __name__ == "__main__":
    main()
