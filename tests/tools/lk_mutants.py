#!/usr/bin/env python3
"""Mutation instrument for the Lucas-Kanade tracker's kernels, k_ft_update and k_ft_track (an instrument, not a test).

Each mutant is a one-line change of vslam_featuretracker.hip (or of VSLAM_FT_MAX_ITER in its header).  The rule of the
list: a mutant may only refuse more, change a constant no address depends on, or reorder arithmetic.  None admits a
position or an index the original refuses, none removes a clamp, none touches an index or a loop bound over memory, so every
mutant library stays inside the buffers of the original.  The old text must occur exactly once in its file or the tool stops.
Build, run and report are tests/tools/mutant_driver.py's:

    python tests/tools/lk_mutants.py build --libs DIR [--jobs 16] [--parallel 1] [--only NAME ...]
    python tests/tools/lk_mutants.py run --libs DIR [--parent] [--out FILE] [--only NAME ...]
                                         [--json FILE --resume --limit N]   (a run split over several calls)
"""
import mutant_driver

FT, FH = "vslam_featuretracker.hip", "vslam_featuretracker.h"
NEW = ["tests/test_gpu_featuretracker_edges.py"]
PARENT = ["tests/test_gpu_featuretracker.py", "tests/test_gpu_featuretracker_bundle.py"]
TRACK = "if (u < half || v < half || u >= lg.w - half || v >= lg.h - half) {"
FIT = "if (x_tl < 0 || y_tl < 0 || x_tl >= lg.w - ps - 1 || y_tl >= lg.h - ps - 1) {"

# (name, [(file, old, new), ...], equivalent: why no input can tell it from the original, or None)
MUTANTS = [
    ("track-left-tight", [(FT, TRACK, TRACK.replace("u < half", "u <= half"))], None),
    ("track-top-tight", [(FT, TRACK, TRACK.replace("v < half", "v <= half"))], None),
    ("track-right-tight", [(FT, TRACK, TRACK.replace("u >= lg.w - half", "u >= lg.w - half - 1"))], None),
    ("track-bottom-tight", [(FT, TRACK, TRACK.replace("v >= lg.h - half", "v >= lg.h - half - 1"))], None),
    ("fit-left-tight", [(FT, FIT, FIT.replace("x_tl < 0", "x_tl < 1"))], None),
    ("fit-top-tight", [(FT, FIT, FIT.replace("y_tl < 0", "y_tl < 1"))], None),
    ("fit-right-tight", [(FT, FIT, FIT.replace("x_tl >= lg.w - ps - 1", "x_tl >= lg.w - ps - 2"))], None),
    ("fit-bottom-tight", [(FT, FIT, FIT.replace("y_tl >= lg.h - ps - 1", "y_tl >= lg.h - ps - 2"))], None),
    ("max-iter-29", [(FH, "#define VSLAM_FT_MAX_ITER 30 ", "#define VSLAM_FT_MAX_ITER 29 ")], None),
    ("converged-le", [(FT, "__fmul_rn(up[1], up[1])) < G.min_update_squared) {", "__fmul_rn(up[1], up[1])) <= G.min_update_squared) {")], None),
    ("skip-level-marker-word", [(FT, "if (isnan(hb[0])) continue;", "if (__float_as_uint(hb[0]) == FT_NAN) continue;")], None),
    ("jres-butterfly-ascending", [(FT, "for (int o = 16; o > 0; o >>= 1) /* the xor butterfly:", "for (int o = 1; o < 32; o <<= 1) /* the xor butterfly:")],
     None),
    ("disparity-from-template", [(FT, "const float dx = __fsub_rn(x, m[FT_FIRST]), dy = __fsub_rn(y, m[FT_FIRST + 1]);",
                                  "const float dx = __fsub_rn(x, m[FT_TEMPLATE]), dy = __fsub_rn(y, m[FT_TEMPLATE + 1]);")], None),
    ("inverse-by-division", [(FT, "o[0] = __fmul_rn(H[2], inv);", "o[0] = __fdiv_rn(H[2], s);"),
                             (FT, "o[2] = __fmul_rn(H[0], inv);", "o[2] = __fdiv_rn(H[0], s);")], None),
    ("gain-after-product", [(FT, "__fsub_rn(__fsub_rn(s, __fmul_rn(gain1, rv)), beta);",
                             "__fsub_rn(__fsub_rn(s, __fadd_rn(rv, __fmul_rn(alpha, rv))), beta);")], None),
    ("minus-one-reassociated", [(FT, "o[1] = __fmul_rn(__fmul_rn(-1.0f, H[1]), inv);", "o[1] = -__fmul_rn(H[1], inv);")],
     "a sign change commutes with a rounded product, so (-1 * H1) * inv and -(H1 * inv) are the same word for every pair that "
     "has no NaN; where the product is NaN (0 * inf) only the NaN's sign differs, the comparison does not read a NaN's bits, and "
     "the kernel only asks isnan() of it or turns the position into NaN, which is stored as the marker word"),
    ("no-isnan-break", [(FT, "if (isnan(x) || isnan(y)) break;", "")],
     "with a NaN position ft_floor_int gives INT_MIN (fmaxf drops the NaN), the bounds test refuses it and the level ends with "
     "go_to_next_level instead of ending the level loop; every later level does the same, the track is not converged either "
     "way, and nothing of a track that is not converged is stored but the marker word"),
]

SPEC = mutant_driver.Spec(MUTANTS, NEW, PARENT, "Mutants of the Lucas-Kanade tracker's kernels (tests/tools/lk_mutants.py)", "lk_mutants_",
                          300, 600)

if __name__ == "__main__":
    mutant_driver.main(SPEC, __doc__)
