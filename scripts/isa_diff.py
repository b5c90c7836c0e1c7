#!/usr/bin/env python3
"""Compare the kernels of two builds, assembly against assembly.

    for f in csrc/*.hip; do
        hipcc --offload-arch=gfx950 --cuda-device-only -S -O3 -std=c++17 \\
            $f -o DIR/$(basename $f .hip).s
    done                                   # once per build, DIR = A and B
    python scripts/isa_diff.py A B

Prints one row per function symbol of every .s file in A or B: the
instruction counts, whether the instruction streams are equal, and
whether the .amdhsa_kernel blocks (registers, LDS, kernarg size) are
equal.  A stream is the function's lines with comments and directives
dropped and the local labels renumbered in order of appearance, so two
streams are equal exactly when the compiler emitted the same
instructions in the same order with the same operands.  Exits 1 when a
row differs or a symbol or file exists on one side only.

Text only: the script knows the layout of the compiler's .s output and
nothing about the instructions in it.
"""

import argparse
import os
import re
import sys

_LABEL = re.compile(r"\.L\w+")


def parse(path):
    """{symbol: (stream, kernel descriptor lines or None)} of one .s file."""
    funcs, descs = {}, {}
    is_func = set()
    sym = desc = None
    for raw in open(path):
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        word = line.split(None, 1)
        if word[0] == ".type" and line.endswith(",@function"):
            is_func.add(word[1].rsplit(",", 1)[0])
        elif word[0] == ".amdhsa_kernel":
            desc = descs.setdefault(word[1], [])
        elif word[0] == ".end_amdhsa_kernel":
            desc = None
        elif desc is not None:
            desc.append(line)
        elif line.endswith(":") and line[:-1] in is_func:
            sym = line[:-1]
            funcs[sym] = []
        elif line.startswith(".Lfunc_end"):
            sym = None
        elif sym is not None and (not line.startswith(".")
                                  or _LABEL.fullmatch(line[:-1])):
            funcs[sym].append(line)
    out = {}
    for sym, lines in funcs.items():
        names = {}
        stream = [_LABEL.sub(
            lambda m: names.setdefault(m.group(), ".L%d" % len(names)), ln)
            for ln in lines]
        out[sym] = (stream, descs.get(sym))
    return out


def n_instr(stream):
    return sum(not ln.endswith(":") for ln in stream)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("a", help="directory of .s files, first build")
    ap.add_argument("b", help="directory of .s files, second build")
    args = ap.parse_args()
    names = [sorted(f for f in os.listdir(d) if f.endswith(".s"))
             for d in (args.a, args.b)]
    bad = 0
    print("| file | symbol | instr A | instr B | stream | .amdhsa_kernel |")
    print("|---|---|---:|---:|---|---|")
    for fn in sorted(set(names[0]) | set(names[1])):
        if fn not in names[0] or fn not in names[1]:
            print(f"| {fn} | (file on one side only) | | | MISSING | MISSING |")
            bad += 1
            continue
        fa = parse(os.path.join(args.a, fn))
        fb = parse(os.path.join(args.b, fn))
        for sym in sorted(set(fa) | set(fb)):
            if sym not in fa or sym not in fb:
                na = n_instr(fa[sym][0]) if sym in fa else ""
                nb = n_instr(fb[sym][0]) if sym in fb else ""
                print(f"| {fn} | {sym} | {na} | {nb} | MISSING | MISSING |")
                bad += 1
                continue
            (sa, da), (sb, db) = fa[sym], fb[sym]
            same_s, same_d = sa == sb, da == db
            bad += not (same_s and same_d)
            print(f"| {fn} | {sym} | {n_instr(sa)} | {n_instr(sb)} | "
                  f"{'equal' if same_s else 'DIFFERENT'} | "
                  f"{'equal' if same_d else 'DIFFERENT'} |")
    print(f"\n{bad} difference(s)" if bad else "\nall kernels identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
