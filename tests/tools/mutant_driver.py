"""The build / run / report scheme shared by the mutation instruments (tests/tools/matcher_gate_mutants.py,
tests/tools/lk_mutants.py); an instrument, not a test.  An instrument is a Spec: its list of mutants, the pytest files that
are new and the ones that owned the code before, and the words of its report.

  build   every mutant is applied to a copy of vi_slam_amd/csrc (with include/) in a temporary directory OUTSIDE the tree
          and built there with `make -j N` (N <= 16; hipcc cross-compiles without a GPU); its libvslam_fe.so is copied to
          --libs DIR/<name>.so.  The old text of an edit must occur exactly once in its file or the tool stops.
  run     per mutant one fresh child process per group of pytest files, under its own `timeout`, with VSLAM_FE_LIB naming
          the mutant's library: the new module, and (with --parent) the parent's files.
          Exit status 0 = the files passed, the mutant SURVIVED them; 1 = noticed.  Any other status stops the tool.
  report  --out FILE

    python tests/tools/<instrument>.py build --libs DIR [--jobs 16] [--parallel 1] [--only NAME ...]
    python tests/tools/<instrument>.py run --libs DIR [--parent] [--out FILE] [--only NAME ...]
                                           [--json FILE --resume --limit N]   (a run split over several calls)
"""
import argparse
import collections
import concurrent.futures
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# mutants: (name, [(file, old, new), ...], equivalent: why no input can tell it from the original, or None); a file is
# looked up in vi_slam_amd/csrc, then in include.  title: the report's first words; tmp_prefix: of the build directory;
# new_limit, parent_limit: seconds a child process of either file group may take.
Spec = collections.namedtuple("Spec", "mutants new parent title tmp_prefix new_limit parent_limit")


def apply_edits(src_dir, edits, include_dir=None):
    for fname, old, new in edits:
        path = os.path.join(src_dir, fname)
        if not os.path.exists(path) and include_dir:
            path = os.path.join(include_dir, fname)
        with open(path) as f:
            text = f.read()
        if text.count(old) != 1:
            sys.exit("mutant text occurs %d times in %s (must be once): %r" % (text.count(old), fname, old))
        with open(path, "w") as f:
            f.write(text.replace(old, new))


def build(spec, args):
    parallel = max(1, int(args.parallel))
    jobs = max(1, min(int(args.jobs), 16) // parallel)
    os.makedirs(args.libs, exist_ok=True)
    work = tempfile.mkdtemp(prefix=spec.tmp_prefix)

    def one(name, edits):
        top = os.path.join(work, name)
        shutil.copytree(os.path.join(ROOT, "vi_slam_amd", "csrc"), os.path.join(top, "vi_slam_amd", "csrc"))
        shutil.copytree(os.path.join(ROOT, "include"), os.path.join(top, "include"))
        csrc = os.path.join(top, "vi_slam_amd", "csrc")
        apply_edits(csrc, edits, os.path.join(top, "include"))
        t0 = time.time()
        subprocess.check_call(["make", "-s", "-C", csrc, "-j%d" % jobs, "../libvslam_fe.so"])
        shutil.copy(os.path.join(top, "vi_slam_amd", "libvslam_fe.so"), os.path.join(args.libs, name + ".so"))
        print("built %-32s %5.1f s" % (name, time.time() - t0), flush=True)
        shutil.rmtree(top)

    try:
        todo = [(name, edits) for name, edits, _ in spec.mutants if not args.only or name in args.only]
        with concurrent.futures.ThreadPoolExecutor(parallel) as pool:
            for f in [pool.submit(one, *m) for m in todo]:
                f.result()
    finally:
        shutil.rmtree(work, ignore_errors=True)


def run_files(lib, files, limit):
    """one fresh child under its own time limit -> exit status"""
    env = dict(os.environ, VSLAM_FE_LIB=os.path.abspath(lib))
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider"] + files
    return subprocess.call(cmd, cwd=ROOT, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def run(spec, args):
    rows = []
    if args.resume and args.json and os.path.exists(args.json):  # a run split over several calls: keep what is there
        with open(args.json) as f:
            rows = json.load(f)
    done = {r["name"] for r in rows}
    verdict = {0: "survived", 1: "noticed"}
    for name, edits, equivalent in spec.mutants:
        if (args.only and name not in args.only) or name in done:
            continue
        if args.limit and len(rows) - len(done) >= args.limit:
            break
        lib = os.path.join(args.libs, name + ".so")
        if not os.path.exists(lib):
            sys.exit("no library for mutant %s in %s: run `build` first" % (name, args.libs))
        rec = dict(name=name, equivalent=equivalent, edits=[(f, o, n) for f, o, n in edits])
        groups = [("new", spec.new, spec.new_limit)] + ([("parent", spec.parent, spec.parent_limit)] if args.parent else [])
        for key, files, limit in groups:
            t0 = time.time()
            rc = run_files(lib, files, limit)
            rec[key] = verdict.get(rc, "status %d" % rc)
            rec[key + "_s"] = round(time.time() - t0, 1)
            print("%-32s %-7s %-9s %6.1f s" % (name, key, rec[key], rec[key + "_s"]), flush=True)
            if rc not in (0, 1):
                rows.append(rec)
                write(spec, args, rows)
                sys.exit("mutant %s: exit status %d from %s -- stopping" % (name, rc, " ".join(files)))
        rows.append(rec)
    write(spec, args, rows)


def write(spec, args, rows):
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    if not args.out:
        return
    live = [r for r in rows if not r["equivalent"]]
    with open(args.out, "w") as f:
        f.write("%s, one library per mutant,\n"
                "one fresh pytest process per mutant and file group on an MI355X.\n"
                "  new    = %s\n"
                "  parent = %s\n" % (spec.title, ", ".join(spec.new), ", ".join(os.path.basename(p) for p in spec.parent)))
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


def main(spec, doc):
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["build", "run", "list"])
    ap.add_argument("--libs", default=None, help="directory of the mutant libraries")
    ap.add_argument("--jobs", default=16)
    ap.add_argument("--parallel", default=1, help="mutants built at the same time (they share --jobs)")
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--parent", action="store_true", help="also run the files that owned this code before")
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--resume", action="store_true", help="skip the mutants --json already lists")
    ap.add_argument("--limit", type=int, default=0, help="run at most this many mutants in this call")
    args = ap.parse_args()
    if args.what == "list":
        for name, edits, eq in spec.mutants:
            print(name, "(equivalent)" if eq else "")
        return
    if not args.libs:
        sys.exit("--libs DIR is required")
    build(spec, args) if args.what == "build" else run(spec, args)
