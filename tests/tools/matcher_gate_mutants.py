#!/usr/bin/env python3
"""Mutation instrument for the gates of the projecting matchers (an instrument, not a test).

Each mutant is a one-line change of the device code: a comparison operator, a literal or a literal's type; none removes a
clamp or touches an index (the tie-key mutant mirrors the index field in the encoder AND the decoder, so every index it
yields is the one that went in).  The old text must occur exactly once in its file or the tool stops.

  build   every mutant is applied to a copy of vi_slam_amd/csrc (with include/) in a temporary directory OUTSIDE the tree
          and built there with `make -j N` (N <= 16; hipcc cross-compiles without a GPU); its libvslam_fe.so is copied to
          --libs DIR/<name>.so.
  run     per mutant one fresh child process per group of pytest files, under its own `timeout`, with VSLAM_FE_LIB naming
          the mutant's library: the new gate module, and (with --parent) the files that owned these gates before it.
          Exit status 0 = the files passed, the mutant SURVIVED them; 1 = noticed.  Any other status stops the tool.
  report  --out FILE (profiles/matcher_gate_mutants.txt)

    python tests/tools/matcher_gate_mutants.py build --libs DIR [--jobs 16] [--only NAME ...]
    python tests/tools/matcher_gate_mutants.py run --libs DIR [--parent] [--out FILE] [--only NAME ...]
                                                   [--json FILE --resume --limit N]   (a run split over several calls)
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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


def apply_edits(src_dir, edits):
    for fname, old, new in edits:
        path = os.path.join(src_dir, fname)
        with open(path) as f:
            text = f.read()
        if text.count(old) != 1:
            sys.exit("mutant text occurs %d times in %s (must be once): %r" % (text.count(old), fname, old))
        with open(path, "w") as f:
            f.write(text.replace(old, new))


def build(args):
    jobs = min(int(args.jobs), 16)
    os.makedirs(args.libs, exist_ok=True)
    work = tempfile.mkdtemp(prefix="gate_mutants_")
    try:
        for name, edits, _ in MUTANTS:
            if args.only and name not in args.only:
                continue
            top = os.path.join(work, name)
            shutil.copytree(os.path.join(ROOT, "vi_slam_amd", "csrc"), os.path.join(top, "vi_slam_amd", "csrc"))
            shutil.copytree(os.path.join(ROOT, "include"), os.path.join(top, "include"))
            csrc = os.path.join(top, "vi_slam_amd", "csrc")
            apply_edits(csrc, edits)
            t0 = time.time()
            subprocess.check_call(["make", "-s", "-C", csrc, "-j%d" % jobs, "../libvslam_fe.so"])
            shutil.copy(os.path.join(top, "vi_slam_amd", "libvslam_fe.so"), os.path.join(args.libs, name + ".so"))
            print("built %-32s %5.1f s" % (name, time.time() - t0), flush=True)
            shutil.rmtree(top)
    finally:
        shutil.rmtree(work, ignore_errors=True)


def run_files(lib, files, limit):
    """one fresh child under its own time limit -> exit status"""
    env = dict(os.environ, VSLAM_FE_LIB=os.path.abspath(lib))
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider"] + files
    return subprocess.call(cmd, cwd=ROOT, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def run(args):
    rows = []
    if args.resume and args.json and os.path.exists(args.json):  # a run split over several calls: keep what is there
        with open(args.json) as f:
            rows = json.load(f)
    done = {r["name"] for r in rows}
    verdict = {0: "survived", 1: "noticed"}
    for name, edits, equivalent in MUTANTS:
        if (args.only and name not in args.only) or name in done:
            continue
        if args.limit and len(rows) - len(done) >= args.limit:
            break
        lib = os.path.join(args.libs, name + ".so")
        if not os.path.exists(lib):
            sys.exit("no library for mutant %s in %s: run `build` first" % (name, args.libs))
        rec = dict(name=name, equivalent=equivalent, edits=[(f, o, n) for f, o, n in edits])
        groups = [("new", NEW, 300)] + ([("parent", PARENT, 900)] if args.parent else [])
        for key, files, limit in groups:
            t0 = time.time()
            rc = run_files(lib, files, limit)
            rec[key] = verdict.get(rc, "status %d" % rc)
            rec[key + "_s"] = round(time.time() - t0, 1)
            print("%-32s %-7s %-9s %6.1f s" % (name, key, rec[key], rec[key + "_s"]), flush=True)
            if rc not in (0, 1):
                rows.append(rec)
                write(args, rows)
                sys.exit("mutant %s: exit status %d from %s -- stopping" % (name, rc, " ".join(files)))
        rows.append(rec)
    write(args, rows)


def write(args, rows):
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    if not args.out:
        return
    live = [r for r in rows if not r["equivalent"]]
    with open(args.out, "w") as f:
        f.write("Mutants of the projecting matchers' gates (tests/tools/matcher_gate_mutants.py), one library per mutant,\n"
                "one fresh pytest process per mutant and file group on an MI355X.\n"
                "  new    = tests/test_gpu_matcher_gates.py\n"
                "  parent = %s\n" % ", ".join(os.path.basename(p) for p in PARENT))
        f.write("noticed = the files failed on the mutant; survived = they passed.\n\n")
        f.write("%-30s %-10s %-10s  change\n" % ("mutant", "parent", "new"))
        for r in rows:
            f.write("%-30s %-10s %-10s  " % (r["name"], r.get("parent", "-"), r["new"] + ("*" if r["equivalent"] else "")))
            f.write("; ".join("%s: %s -> %s" % (fn, " ".join(o.split())[-60:], " ".join(n.split())[-60:]) for fn, o, n in r["edits"]))
            f.write("\n")
        f.write("\n* equivalent mutants, not counted:\n")
        for r in rows:
            if r["equivalent"]:
                f.write("  %s: %s\n" % (r["name"], r["equivalent"]))
        f.write("\ncounted mutants: %d; noticed by the new module: %d; noticed by the parent's files: %s\n" % (
            len(live), sum(r["new"] == "noticed" for r in live),
            sum(r.get("parent") == "noticed" for r in live) if any("parent" in r for r in live) else "not run"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["build", "run", "list"])
    ap.add_argument("--libs", default=None, help="directory of the mutant libraries")
    ap.add_argument("--jobs", default=16)
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--parent", action="store_true", help="also run the files that owned these gates before")
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--resume", action="store_true", help="skip the mutants --json already lists")
    ap.add_argument("--limit", type=int, default=0, help="run at most this many mutants in this call")
    args = ap.parse_args()
    if args.what == "list":
        for name, edits, eq in MUTANTS:
            print(name, "(equivalent)" if eq else "")
        return
    if not args.libs:
        sys.exit("--libs DIR is required")
    build(args) if args.what == "build" else run(args)


if __name__ == "__main__":
    main()
