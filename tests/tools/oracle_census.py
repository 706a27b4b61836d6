#!/usr/bin/env python3
"""Census of the CPU oracle's branches that a test run never took.

    make -C oracle COVERAGE=1                  # instrumented liborb_oracle.so in the normal library's place
    python -m pytest -q tests -m gpu           # ... and the CPU tests: every run adds to the same counters
    python -m pytest -q tests -m "not gpu"
    python tests/tools/oracle_census.py        # the report, on stdout
    make -C oracle clean all                   # back to the normal library

Plain Python plus gcov: runs `gcov -b -c` (JSON form) on the three oracle sources and prints one record per oracle
function with the lines that were never executed and the branches that were never taken, each with its line number
and source text.  Exception edges and the C-ABI glue (extern "C" entry points, orb_oracle_c.cpp) are dropped; lambdas
and OpenMP bodies count under the function that contains them.  Ordering is by source file, then by line, and no
execution count is printed, so two reports diff cleanly.

--functions RE       only functions whose name matches the regular expression
--dispositions FILE  JSON list of {"function": RE, "text": substring of the source line (optional), "line": int (optional),
                     "no_decision": true (optional: only branches on lines without if / loop / ?: / && / || / min / max,
                     i.e. edges the compiler made), "disposition": str}; the first rule that matches an entry is
                     appended to it; entries without one are marked NO DISPOSITION and make the exit status 1
--counts-only        only the per-function table
"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SOURCES = ("orb_oracle.cpp", "fastgrid_oracle.cpp", "orb_oracle_c.cpp")


def gcov_json(oracle_dir, src):
    stem = os.path.splitext(src)[0]
    gcda = os.path.join(oracle_dir, "liborb_oracle.so-%s.gcda" % stem)
    if not os.path.exists(gcda):
        sys.exit("oracle_census: %s has no counters: build with `make -C oracle COVERAGE=1`, then run the tests" % src)
    out = subprocess.run(["gcov", "-b", "-c", "-m", "--json-format", "--stdout", os.path.basename(gcda)], cwd=oracle_dir,
                         check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
    return json.loads(out)


def short_name(demangled):
    """orbo::compute_stereo_matches(orbo::Extractor const&, ...) -> orbo::compute_stereo_matches"""
    depth, out = 0, []
    for ch in demangled.replace("(anonymous namespace)", "{anonymous}"):
        if ch == "(" and depth == 0:
            break
        depth += ch == "<"
        depth -= ch == ">"
        out.append(ch)
    return "".join(out).strip() or demangled


def census(oracle_dir):
    """-> list of records dict(file, name, start, end, branches, entries=[(line, branch index or None, n branches, text)])"""
    records = []
    for src in SOURCES:
        doc = gcov_json(oracle_dir, src)
        with open(os.path.join(oracle_dir, src)) as f:
            text = f.read().split("\n")
        for fobj in doc["files"]:
            if os.path.basename(fobj["file"]) != src or os.path.dirname(fobj["file"]) not in ("", "."):
                continue
            # outermost functions: lambdas / OpenMP bodies / instantiations fold into the range that contains them
            funcs = sorted(fobj["functions"], key=lambda f: (f["start_line"], -f["end_line"], f["name"]))
            outer = []
            for f in funcs:
                if outer and f["start_line"] >= outer[-1]["start_line"] and f["end_line"] <= outer[-1]["end_line"]:
                    continue
                outer.append(f)
            # one entry per source line: counts of repeated instances add up
            lines = {}
            for ln in fobj["lines"]:
                cur = lines.setdefault(ln["line_number"], dict(count=0, branches=None))
                cur["count"] += ln["count"]
                br = [(b["count"], b["throw"]) for b in ln["branches"]]
                if cur["branches"] is None or len(cur["branches"]) != len(br):
                    cur["branches"] = br if cur["branches"] is None else cur["branches"]
                else:
                    cur["branches"] = [(a[0] + b[0], a[1]) for a, b in zip(cur["branches"], br)]
            for f in outer:
                glue = not f["name"].startswith("_Z") or src == "orb_oracle_c.cpp"
                if glue:
                    continue
                rec = dict(file=src, name=short_name(f["demangled_name"]), start=f["start_line"], end=f["end_line"],
                           branches=0, entries=[])
                for no in range(f["start_line"], f["end_line"] + 1):
                    ln = lines.get(no)
                    if ln is None:
                        continue
                    src_text = " ".join(text[no - 1].split()) if no - 1 < len(text) else ""
                    real = [c for c, throw in (ln["branches"] or []) if not throw]
                    rec["branches"] += len(real)
                    if ln["count"] == 0:
                        rec["entries"].append((no, None, len(real), src_text))
                        continue
                    for i, c in enumerate(real):
                        if c == 0:
                            rec["entries"].append((no, i, len(real), src_text))
                records.append(rec)
    return records


def load_rules(path):
    if not path:
        return None
    with open(path) as f:
        rules = json.load(f)
    for r in rules:
        r["_re"] = re.compile(r["function"])
    return rules


DECISION = re.compile(r"\b(if|for|while|switch|case|return)\b|\?|&&|\|\||\b(min|max)\b")


def disposition(rules, rec, entry):
    for r in rules:
        if not r["_re"].search(rec["name"]):
            continue
        if r.get("line") is not None and r["line"] != entry[0]:
            continue
        if r.get("text") and r["text"] not in entry[3]:
            continue
        if r.get("no_decision") and (entry[1] is None or DECISION.search(entry[3])):
            continue  # rule for compiler-made edges: only branches on lines without a decision in the source
        return r["disposition"]
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--oracle-dir", default=os.path.join(ROOT, "oracle"))
    ap.add_argument("--functions", default=None, help="regular expression on the function name")
    ap.add_argument("--dispositions", default=None)
    ap.add_argument("--counts-only", action="store_true")
    a = ap.parse_args()
    rules = load_rules(a.dispositions)
    want = re.compile(a.functions) if a.functions else None
    records = [r for r in census(a.oracle_dir) if want is None or want.search(r["name"])]
    missing = 0
    if not a.counts_only:
        for rec in records:
            if not rec["entries"]:
                continue
            print("%s: %s (lines %d-%d)" % (rec["file"], rec["name"], rec["start"], rec["end"]))
            for e in rec["entries"]:
                what = "never executed" if e[1] is None else "branch %d of %d never taken" % (e[1], e[2])
                line = "  %5d  %-28s %s" % (e[0], what, e[3])
                if rules is not None:
                    d = disposition(rules, rec, e)
                    if d is None:
                        missing += 1
                        d = "NO DISPOSITION"
                    line += "\n         -> " + d
                print(line)
            print()
    print("%-58s %9s %12s %15s" % ("function", "branches", "never taken", "lines never run"))
    tot = [0, 0, 0]
    for rec in records:
        nb = sum(1 for e in rec["entries"] if e[1] is not None) + sum(e[2] for e in rec["entries"] if e[1] is None)
        nl = sum(1 for e in rec["entries"] if e[1] is None)
        tot = [tot[0] + rec["branches"], tot[1] + nb, tot[2] + nl]
        print("%-58s %9d %12d %15d" % ("%s:%d %s" % (rec["file"].replace("_oracle.cpp", ""), rec["start"], rec["name"]),
                                       rec["branches"], nb, nl))
    print("%-58s %9d %12d %15d" % ("total", tot[0], tot[1], tot[2]))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
