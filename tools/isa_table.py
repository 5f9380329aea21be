"""Per-kernel comparison of device assembly between two revisions, no GPU:

    hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S FILE.hip -o FILE.s        (once per file and revision)
    python tools/isa_table.py --parent P1.s [P2.s ...] --head H1.s [H2.s ...] [--same REGEX] > profiles/NAME_isa.txt

Kernels are keyed by symbol, whichever file holds them (a refactor may move a kernel to another translation unit).  Per kernel: sha256[:16]
of the instruction text between its label and its .Lfunc_end (comments dropped, local labels renumbered in order of appearance), the
number of instruction lines, and VGPR / SGPR / LDS / scratch of its .amdhsa_kernel descriptor.  Exit status 1 when the sets of kernel
names differ, when a kernel matching --same differs in any column, or when a kernel with different text gained LDS or scratch."""
import argparse
import hashlib
import re
import subprocess
import sys

FIELDS = (("vgpr", ".amdhsa_next_free_vgpr"), ("sgpr", ".amdhsa_next_free_sgpr"), ("lds", ".amdhsa_group_segment_fixed_size"),
          ("scratch", ".amdhsa_private_segment_fixed_size"))


def kernels(paths):
    out = {}
    for path in paths:
        lines = open(path).read().split("\n")
        desc = {}
        cur = None
        for ln in lines:
            s = ln.strip()
            if s.startswith(".amdhsa_kernel "):
                cur = s.split()[1]
                desc[cur] = {}
            elif s == ".end_amdhsa_kernel":
                cur = None
            elif cur:
                for key, word in FIELDS:
                    if s.startswith(word + " "):
                        desc[cur][key] = s.split()[1]
        for name in desc:
            start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
            body, labels = [], {}
            for ln in lines[start + 1:]:
                s = ln.split(";")[0].strip()
                if s.startswith(".Lfunc_end"):
                    break
                if not s or (s.startswith(".") and not s.endswith(":")):
                    continue
                body.append(s)
            text = "\n".join(body)
            for lab in re.findall(r"\.LBB\d+_\d+", text):
                labels.setdefault(lab, ".L%d" % len(labels))
            text = re.sub(r"\.LBB\d+_\d+", lambda m: labels[m.group(0)], text)
            out[name] = dict(desc[name], text=hashlib.sha256(text.encode()).hexdigest()[:16],
                             instructions=sum(1 for s in body if not s.endswith(":")))
    return out


def demangle(names):
    try:
        res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, (r.replace("(anonymous namespace)::", "") for r in res)))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", nargs="+", required=True)
    ap.add_argument("--head", nargs="+", required=True)
    ap.add_argument("--same", default=None, help="kernels whose demangled name matches must be identical in every column")
    args = ap.parse_args()
    p, h = kernels(args.parent), kernels(args.head)
    bad = 0
    print("kernel symbols: parent %d, head %d, %s" % (len(p), len(h), "same set" if set(p) == set(h) else "DIFFERENT SETS"))
    for n in sorted(set(p) ^ set(h)):
        print("  only in %s: %s" % ("parent" if n in p else "head", n))
        bad = 1
    names = sorted(set(p) & set(h))
    pretty = demangle(names)
    cols = ("instructions",) + tuple(k for k, _ in FIELDS)
    changed = []
    for n in names:
        a, b = p[n], h[n]
        same = all(a[c] == b[c] for c in cols + ("text",))
        print(re.sub(r"\(.*", "", pretty[n]))
        print("    text %s / %s  %s" % (a["text"], b["text"], "identical" if same else "DIFFERENT"))
        print("    " + "  ".join("%s %s" % (c, a[c]) if a[c] == b[c] else "%s %s -> %s" % (c, a[c], b[c]) for c in cols))
        if not same:
            changed.append(pretty[n])
            if args.same and re.search(args.same, pretty[n]):
                print("    !! must be identical")
                bad = 1
            if int(b["lds"]) > int(a["lds"]) or int(b["scratch"]) > int(a["scratch"]):
                print("    !! gained LDS or scratch")
                bad = 1
    print("verdict: %d of %d kernels identical%s" % (len(names) - len(changed), len(names), "" if not changed else "; different: " +
                                                     ", ".join(re.sub(r"^void gdr::|\(.*", "", c) for c in changed)))
    return bad


if __name__ == "__main__":
    sys.exit(main())
