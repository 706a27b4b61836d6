#!/usr/bin/env python3
"""Mutation instrument for the gates of the projecting matchers (an instrument, not a test).

Each mutant is a one-line change of the device code: a comparison operator, a literal or a literal's type; none removes a
clamp or touches an index (the tie-key mutant mirrors the index field in the encoder AND the decoder, so every index it
yields is the one that went in).  The old text must occur exactly once in its file or the tool stops.
Build, run and report are tests/tools/mutant_driver.py's (its docstring describes them); the report is
profiles/matcher_gate_mutants.txt.

    python tests/tools/matcher_gate_mutants.py build --libs DIR [--jobs 16] [--parallel 1] [--only NAME ...]
    python tests/tools/matcher_gate_mutants.py run --libs DIR [--parent] [--out FILE] [--only NAME ...]
                                                   [--json FILE --resume --limit N]   (a run split over several calls)
"""
import mutant_driver

PK, PJ, MD, BW = ("vslam_projection_kernels.hip", "vslam_projection.hip", "vslam_matchdev.h", "vslam_bow.hip")
NEW = ["tests/test_gpu_matcher_gates.py"]
PARENT = ["tests/test_gpu_projection.py", "tests/test_gpu_projection_bounds.py", "tests/test_gpu_mapping.py",
          "tests/test_gpu_bow_sparse.py"]

# (name, [(file, old, new), ...], equivalent: why no input can tell it from the original, or None)
MUTANTS = [
    ("chi2-7.8f", [(PK, "> 7.8) continue;", "> 7.8f) continue;")], None),
    ("chi2-5.99f", [(PK, "> 5.99) continue;", "> 5.99f) continue;")],
     "5.99f = 5.98999977 lies BELOW 5.99 and no float lies between them: x > 5.99 and x > 5.99f hold for the same floats x "
     "(7.8f, 3.84f * sigma2 and 0.998f lie on the other side of their literals, or are compared in double with one)"),
    ("epipolar-3.84f", [(BW, "__dmul_rn(3.84, (double)A.sigma2_2[oct2])", "__dmul_rn(3.84f, (double)A.sigma2_2[oct2])")], None),
    ("viewcos-0.998f", [(PK, "(double)mp.viewCos > 0.998 ?", "(double)mp.viewCos > 0.998f ?")], None),
    ("fuse-uright-gt", [(PK, "if (cd.uRight >= 0.f) {", "if (cd.uRight > 0.f) {")], None),
    ("frame-uright-ge", [(PK, "if (cd.uRight > 0.f) { /* CurrentFrame.mvuRight[i2] > 0 */",
                          "if (cd.uRight >= 0.f) { /* CurrentFrame.mvuRight[i2] > 0 */")], None),
    ("fuse-maxx-le", [(PK, "v = __fadd_rn(__fdiv_rn(__fmul_rn(A.fy, yc), zc), A.cy);\n"
                           "                go = u >= kbnd.minX && u < kbnd.maxX &&",
                       "v = __fadd_rn(__fdiv_rn(__fmul_rn(A.fy, yc), zc), A.cy);\n"
                       "                go = u >= kbnd.minX && u <= kbnd.maxX &&")], None),
    ("sim3dir-maxx-le", [(PK, "v = __fadd_rn(__fmul_rn(A.fy, __fmul_rn(yc, invz)), A.cy);\n"
                              "                go = u >= kbnd.minX && u < kbnd.maxX &&",
                          "v = __fadd_rn(__fmul_rn(A.fy, __fmul_rn(yc, invz)), A.cy);\n"
                          "                go = u >= kbnd.minX && u <= kbnd.maxX &&")], None),
    ("sim3proj-maxx-le", [(PK, "uv.x >= wbnd.minX && uv.x < wbnd.maxX &&", "uv.x >= wbnd.minX && uv.x <= wbnd.maxX &&")], None),
    ("frame-maxx-ge", [(PK, "!(uv.x < b.minX || uv.x > b.maxX)", "!(uv.x < b.minX || uv.x >= b.maxX)")], None),
    ("fuse-depth-gt", [(PK, "const float xc = pc.x, yc = pc.y, zc = pc.z;\n            go = !(zc < 0.0f);\n"
                            "            if (go) {\n                const float invz = __fdiv_rn(1.0f, zc);",
                        "const float xc = pc.x, yc = pc.y, zc = pc.z;\n            go = zc > 0.0f;\n"
                        "            if (go) {\n                const float invz = __fdiv_rn(1.0f, zc);")],
     "the two differ at zc == 0 (and NaN) only, where the projection is +-inf or NaN and KeyFrame::IsInImage fails anyway"),
    ("sim3dir-depth-gt", [(PK, "go = !(zc < 0.0f);\n            if (go) {\n                const float invz = (float)__ddiv_rn(",
                           "go = zc > 0.0f;\n            if (go) {\n                const float invz = (float)__ddiv_rn(")],
     "as fuse-depth-gt"),
    ("sim3proj-depth-gt", [(PK, "if (pc.z < 0.0f) return SbpProj{};", "if (!(pc.z > 0.0f)) return SbpProj{};")],
     "as fuse-depth-gt"),
    ("keyframe-depth-added", [(PK, "const float2 uv = sbp_pinhole(J, pc); /* no depth test here */",
                               "if (pc.z < 0.0f) return SbpProj{};\n    const float2 uv = sbp_pinhole(J, pc);")], None),
    ("range-min-strict", [(PK, "d.inRange = !(d.dist3D < kf.minDist[q] ||", "d.inRange = !(d.dist3D <= kf.minDist[q] ||")], None),
    ("range-max-strict", [(PK, "|| d.dist3D > d.maxDist);", "|| d.dist3D >= d.maxDist);")], None),
    ("sim3proj-angle-le", [(PK, "JS.kf.normals + 3 * q) < __dmul_rn(0.5,", "JS.kf.normals + 3 * q) <= __dmul_rn(0.5,")], None),
    ("fuse-angle-le", [(PK, "mp.normal) < __dmul_rn(0.5,", "mp.normal) <= __dmul_rn(0.5,")], None),
    ("kf-window-le", [(MD, "return fabsf(distx) < r && fabsf(disty) < r;", "return fabsf(distx) <= r && fabsf(disty) < r;")], None),
    ("frame-window-le", [(PK, "if (!(fabsf(distx) < pr.radius && fabsf(disty) < pr.radius)) return false;",
                          "if (!(fabsf(distx) <= pr.radius && fabsf(disty) < pr.radius)) return false;")], None),
    ("frame-er-ge", [(PK, "if (er > pr.radius) return false;", "if (er >= pr.radius) return false;")], None),
    ("level-upper-plus-one", [(PK, "pr.maxLevel = level + levelsUp;", "pr.maxLevel = level + levelsUp + 1;")], None),
    ("frame-level-upper-plus-one", [(PK, "else { pr.minLevel = oct - 1; pr.maxLevel = oct + 1; }",
                                     "else { pr.minLevel = oct - 1; pr.maxLevel = oct + 2; }")], None),
    ("tracked-level-upper-plus-one", [(PK, "pr.maxLevel = mp.level;", "pr.maxLevel = mp.level + 1;")], None),
    ("fuse-level-upper-plus-one", [(PK, "if (kpLevel < level - 1 || kpLevel > level) continue;",
                                    "if (kpLevel < level - 1 || kpLevel > level + 1) continue;")], None),
    ("forward-ge", [(PJ, "*forward = (tlc2 > mb && !mono) ? 1 : 0;", "*forward = (tlc2 >= mb && !mono) ? 1 : 0;")], None),
    ("backward-ge", [(PJ, "*backward = (-tlc2 > mb && !mono) ? 1 : 0;", "*backward = (-tlc2 >= mb && !mono) ? 1 : 0;")], None),
    ("th-high-99", [(PK, "#define SBP_TH_HIGH 100", "#define SBP_TH_HIGH 99")], None),
    ("th-low-49", [(BW, "#define SBOW_TH_LOW 50", "#define SBOW_TH_LOW 49")], None),
    ("ratio-hamming-ceil", [(PJ, "(int)floorf(lim);", "(int)ceilf(lim);")], None),
    ("ratio-resolve-ge", [(PK, "if (!(bl == sl && (float)bd > __fmul_rn(J.nnratio, (float)sd))) nc = best;",
                           "if (!(bl == sl && (float)bd >= __fmul_rn(J.nnratio, (float)sd))) nc = best;")], None),
    ("ratio-replay-ge", [(PK, "if (bl == sl && (float)bd > __fmul_rn(J.nnratio, (float)sd)) accept = false;",
                          "if (bl == sl && (float)bd >= __fmul_rn(J.nnratio, (float)sd)) accept = false;")], None),
    ("tie-larger-index", [(MD, "return (min(hamming, 255u) << 24) | (cell << 12) | index;",
                           "return (min(hamming, 255u) << 24) | (cell << 12) | (0xFFFu - index);"),
                          (MD, "{ return key & 0xFFFu; }", "{ return 0xFFFu - (key & 0xFFFu); }")], None),
    ("fuse-dist-256-found", [(PK, "if (dist > 255u) { /* `dist < bestDist`", "if (dist > 256u) { /* `dist < bestDist`")], None),
    ("triangulation-tie-first", [(BW, "(dist << 20) | (0xFFFFFu - (uint32_t)b));", "(dist << 20) | (uint32_t)b);"),
                                 (BW, "A.feat2[f0 + (int)(0xFFFFFu - (g & 0xFFFFFu))];", "A.feat2[f0 + (int)(g & 0xFFFFFu)];")], None),
    ("epipole-le", [(BW, "__fmul_rn(dey, dey)) < __fmul_rn(100.f, A.scale2[oct2])) continue;",
                     "__fmul_rn(dey, dey)) <= __fmul_rn(100.f, A.scale2[oct2])) continue;")], None),
    ("triangulation-uright-gt", [(BW, "const bool bStereo1 = A.uRight1[idx1] >= 0.f;", "const bool bStereo1 = A.uRight1[idx1] > 0.f;")],
     None),
]


SPEC = mutant_driver.Spec(MUTANTS, NEW, PARENT, "Mutants of the projecting matchers' gates (tests/tools/matcher_gate_mutants.py)",
                          "gate_mutants_", 300, 900)

if __name__ == "__main__":
    mutant_driver.main(SPEC, __doc__)
