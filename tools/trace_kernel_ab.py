"""`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- <program>` runs of the same program under two library builds:

    python tools/trace_kernel_ab.py --parent P_DIR [P_DIR2 ...] --head H_DIR [H_DIR2 ...] [--only REGEX]

Per kernel name: calls per run and the mean time per launch (us) of every run.  With several parent runs the margin is the spread of the
parent's own runs: a head run is `inside` it, `faster`, or `SLOWER` (above the parent's slowest run).  Exit status 1 when the sets of
kernel names or a call count differ between any two runs (a coverage check: the builds must launch the same kernels equally often)."""
import argparse
import csv
import glob
import os
import re
import sys


def stats(d):
    out = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = re.sub(r" \[clone .*\]$|\.kd$", "", row["Name"])
            calls, total = out.get(name, (0, 0.0))
            out[name] = (calls + int(row["Calls"]), total + float(row["TotalDurationNs"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", nargs="+", required=True)
    ap.add_argument("--head", nargs="+", required=True)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    P, H = [stats(d) for d in args.parent], [stats(d) for d in args.head]
    runs = P + H
    bad = 0
    for r in runs[1:]:
        for n in sorted(set(runs[0]) ^ set(r)):
            print("not in every run: %s" % n)
            bad = 1
    names = [n for n in sorted(set.intersection(*(set(r) for r in runs))) if not args.only or re.search(args.only, n)]
    print("runs: parent %d, head %d; kernel names %s; launches %s" % (len(P), len(H), [len(r) for r in runs],
                                                                      [sum(v[0] for v in r.values()) for r in runs]))
    print("%-44s %7s  %-28s %-28s %s" % ("kernel", "calls", "us/call parent runs", "us/call head runs", "head against the parent's runs"))
    for n in names:
        calls = [r[n][0] for r in runs]
        if len(set(calls)) != 1:
            bad = 1
        mp, mh = [r[n][1] / r[n][0] / 1e3 for r in P], [r[n][1] / r[n][0] / 1e3 for r in H]
        lo, hi = min(mp), max(mp)
        verdict = ", ".join("SLOWER" if x > hi else ("faster" if x < lo else "inside") for x in mh) if len(P) > 1 else "%.3f" % (mh[0] / mp[0])
        print("%-44s %7d  %-28s %-28s %s%s" % (re.sub(r"^void gdr::|^gdr::|\(.*", "", n.replace("(anonymous namespace)::", ""))[:44], calls[0], " ".join("%.2f" % x for x in mp),
                                                " ".join("%.2f" % x for x in mh), verdict, "" if len(set(calls)) == 1 else "  !! calls differ"))
    print("verdict: %s" % ("names and call counts equal" if not bad else "DIFFERENT names or call counts"))
    return bad


if __name__ == "__main__":
    sys.exit(main())
