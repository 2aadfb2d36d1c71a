#!/usr/bin/env python3
"""isa_compare.py [--ordered] A.s B.s -- do two AMDGPU assembly files hold the same functions?

Splits each file (hipcc --cuda-device-only -S) into functions, symbol label to its .Lfunc_end,
and kernel descriptors (.amdhsa_kernel ... .end_amdhsa_kernel: registers, LDS, scratch), and
compares them by symbol, so moving a function within its source leaves the files equal.  Local
labels carry the function's ordinal in the file (.LBB<n>_, .LJTI<n>_, .Lfunc_end<n>) or a
file-wide counter (.Ltmp<n>, .Lpost_getpc<n>); both are rewritten per function.  __hip_cuid_* (a
hash of the source path) and .ident are ignored.  Prints symbols only in A, only in B, and those
whose text differs (with the first differing line); exit status 1 on any difference.  --ordered
also requires the same order.
"""
import re
import sys

LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
ORDINAL = re.compile(r"(\.L(?:BB|JTI|func_begin|func_end)|\bBB(?=\d+_))\d+")  # BB<n>_<k>: loop comments
COUNTER = re.compile(r"\.L(?:tmp|post_getpc)\d+")


def normalise(lines):
    seen = {}
    out = []
    for ln in lines:
        ln = " ".join(ORDINAL.sub(r"\1", ln).split())  # (a comment's column follows its label's width)
        out.append(COUNTER.sub(lambda m: ".Ln%d" % seen.setdefault(m.group(0), len(seen)), ln))
    return out


def split(path):
    """[(key, lines)] in file order: ("f", symbol) function text, ("k", symbol) kernel descriptor"""
    items, cur, kern, func = [], None, None, None
    for ln in open(path):
        ln = ln.rstrip()
        if "__hip_cuid_" in ln or ln.lstrip().startswith(".ident"):
            continue
        if kern is not None:
            kern[1].append(ln)
            if ln.strip() == ".end_amdhsa_kernel":
                kern = None
            continue
        if ln.lstrip().startswith(".amdhsa_kernel "):
            kern = (("k", ln.split()[1]), [ln])
            items.append(kern)
            continue
        if "@function" in ln and ln.lstrip().startswith(".type"):
            func = ln.split()[1].split(",")[0]
        m = LABEL.match(ln)
        if cur is None and m and m.group(1) == func:  # data labels start nothing
            cur = (("f", m.group(1)), [])
            items.append(cur)
        if cur is not None:
            cur[1].append(ln)
            if ln.startswith(".Lfunc_end"):
                cur = None
    return [(key, normalise(lines)) for key, lines in items]


def name(key):
    return ("kernel descriptor " if key[0] == "k" else "") + key[1]


def compare(a_path, b_path, ordered=False, out=sys.stdout):
    a, b = split(a_path), split(b_path)
    da, db = dict(a), dict(b)
    bad = 0
    for key, _ in a:
        if key not in db:
            print("only in A: " + name(key), file=out)
            bad += 1
    for key, _ in b:
        if key not in da:
            print("only in B: " + name(key), file=out)
            bad += 1
    for key, la in a:
        lb = db.get(key)
        if lb is not None and la != lb:
            i = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            print("differs: %s (line %d of it)" % (name(key), i + 1), file=out)
            print("  A: " + (la[i].strip() if i < len(la) else "<end>"), file=out)
            print("  B: " + (lb[i].strip() if i < len(lb) else "<end>"), file=out)
            bad += 1
    if ordered and not bad and [k for k, _ in a] != [k for k, _ in b]:
        i = next(i for i, (x, y) in enumerate(zip(a, b)) if x[0] != y[0])
        print("order differs from entry %d: A %s, B %s" % (i, name(a[i][0]), name(b[i][0])), file=out)
        bad += 1
    if not bad:
        nk = sum(1 for k, _ in a if k[0] == "k")
        print("identical: %d functions, %d kernel descriptors" % (len(a) - nk, nk), file=out)
    return 1 if bad else 0


if __name__ == "__main__":
    args = [x for x in sys.argv[1:] if x != "--ordered"]
    if len(args) != 2:
        sys.exit(__doc__)
    sys.exit(compare(args[0], args[1], "--ordered" in sys.argv[1:]))
