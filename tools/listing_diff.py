#!/usr/bin/env python3
"""Do two device listings hold the same kernels?  Per kernel: its name, both instruction counts, `same` or `different`.

    hipcc <the Makefile's flags of the object> --cuda-device-only -S file.hip -o new.s     (and the same of the parent commit)
    python tools/listing_diff.py parent.s new.s [--show KERNEL]

A listing is cut at its kernel symbols (the `.amdhsa_kernel` names); of a kernel's text the instructions and the labels are kept,
comments and directives dropped, and local labels (`.LBB12_3`, `.Ltmp7`) renumbered in the order in which the kernel first
names them, so that a kernel that moved in the file or got another function number still compares equal.  Nothing is said
about WHICH instructions a kernel holds: the two texts are equal or they are not.  `--show` prints a unified diff of one
kernel's two texts (a name or a part of one).  Exit status 1 if a kernel is `different` or is in one listing only.
"""
import argparse
import difflib
import re
import subprocess
import sys

LOCAL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def demangle(names):
    """the kernels' readable names, by c++filt where there is one (else the symbols as they are)"""
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}
    short = {}
    for n, d in zip(names, out):
        d = re.sub(r"\(anonymous namespace\)::", "", d)
        d = re.sub(r"^void ", "", d)
        short[n] = re.sub(r"\(.*$", "", d) if "(" in d else d
    return short


def kernels(path):
    """{symbol: [line, ...]} of the kernels of a listing, in the file's order"""
    lines = open(path).read().split("\n")
    symbols = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(lines), flags=re.M))
    out, cur, labels = {}, None, None
    for line in lines:
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if m and not m.group(1).startswith(".L"):
            cur = labels = None
            if m.group(1) in symbols:
                cur, labels = out.setdefault(m.group(1), []), {}
            continue
        if cur is None:
            continue
        if re.match(r"^\s*\.(section|end_amdhsa_kernel|rodata|text)\b", line) or line.startswith(".Lfunc_end"):
            cur = labels = None
            continue
        text = line.split(";")[0].strip()
        if not text or (text.startswith(".") and not LOCAL.match(text)):
            continue
        text = LOCAL.sub(lambda l: labels.setdefault(l.group(0), ".L%d" % len(labels)), text)
        cur.append(re.sub(r"\s+", " ", text))
    return out


def instructions(text):
    return sum(1 for t in text if not t.endswith(":"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--show", metavar="KERNEL", help="print the diff of the kernels whose name holds this")
    args = ap.parse_args()
    a, b = kernels(args.parent), kernels(args.new)
    names = demangle(list(dict.fromkeys(list(a) + list(b))))
    bad = 0
    for sym, name in names.items():
        if sym not in a or sym not in b:
            print("%-48s %s" % (name, "only in " + (args.parent if sym in a else args.new)))
            bad += 1
            continue
        same = a[sym] == b[sym]
        bad += not same
        print("%-48s %6d %6d  %s" % (name, instructions(a[sym]), instructions(b[sym]), "same" if same else "different"))
        if args.show and args.show in name and not same:
            sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(a[sym], b[sym], "parent", "new", lineterm="", n=2))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
