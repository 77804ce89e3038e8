"""Compare the gfx950 code of two builds kernel by kernel, without a GPU: one line per kernel whose mangled name
contains the substring -- instruction counts, whether the disassembly is textually identical, whether at least the
opcode sequence is, the opcode-histogram delta (b - a), every code-object resource field that differs and, when the
text differs, how many lines do: in all, inside a run of MFMAs (a K loop), and naming an AGPR.

    python scripts/kernel_isa_diff.py A B substr [substr ...]     # A, B: libmacaw_hip.so or an object file (gemm_v9.o)

The project pins bit-identity between code paths (mk_gemm against mk_gemm_grouped, a refactored kernel against its
parent): identical text here is that, for every shape at once.  Exit status 1 when any kernel's text differs."""
import collections
import difflib
import re
import subprocess
import sys

import kernel_resources as kr

LOOP_GAP = 100      # MFMAs further apart than this many instructions belong to different loops


def in_loops(lines):
    """per line: does it lie between the first and the last MFMA of one loop"""
    at = [i for i, ins in enumerate(lines) if ins.startswith("v_mfma_")]
    inside = [False] * len(lines)
    for a, b in zip(at, at[1:]):
        if b - a <= LOOP_GAP:
            inside[a:b + 1] = [True] * (b + 1 - a)
    return inside


def changed(la, lb):
    """(differing lines, of them inside a loop, of them naming an AGPR), counted on both sides"""
    n = loop = agpr = 0
    for tag, a0, a1, b0, b1 in difflib.SequenceMatcher(None, la, lb, autojunk=False).get_opcodes():
        if tag == "equal":
            continue
        for lines, lo, hi in ((la, a0, a1), (lb, b0, b1)):
            inside = in_loops(lines)
            n += hi - lo
            loop += sum(inside[lo:hi])
            agpr += sum(bool(re.search(r"\ba(\d+|\[\d+:\d+\])", ins)) for ins in lines[lo:hi])
    return n, loop, agpr


def diff(a, b, substr):
    """yield (kernel, n_a, n_b, text identical, opcode sequence identical, histogram delta, resource delta, changed)"""
    da, db = kr.disassemble(substr, a), kr.disassemble(substr, b)
    ra, rb = kr.kernels(a), kr.kernels(b)
    syms = sorted(set(da) | set(db))
    dem = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True,
                         text=True).stdout.replace("(anonymous namespace)::", "").split("\n")
    for sym, name in zip(syms, dem):
        la, lb = da.get(sym, []), db.get(sym, [])
        oa, ob = [i.split()[0] for i in la], [i.split()[0] for i in lb]
        ha, hb = collections.Counter(oa), collections.Counter(ob)
        hist = {o: hb[o] - ha[o] for o in sorted(set(ha) | set(hb)) if hb[o] != ha[o]}
        res = {f: (ra.get(name, {}).get(f), rb.get(name, {}).get(f)) for f in kr.FIELDS
               if ra.get(name, {}).get(f) != rb.get(name, {}).get(f)}
        yield name, len(la), len(lb), la == lb, oa == ob, hist, res, (0, 0, 0) if la == lb else changed(la, lb)


if __name__ == "__main__":
    if len(sys.argv) < 4:
        sys.exit(__doc__)
    same = True
    for substr in sys.argv[3:]:
        for name, na, nb, text, ops, hist, res, (n, loop, agpr) in diff(sys.argv[1], sys.argv[2], substr):
            same &= text
            print(f"{name[:64]:64s} {na:5d} -> {nb:5d}  text {'identical' if text else 'DIFFERS'}  "
                  f"opcodes {'identical' if ops else 'DIFFER'}  histogram {hist or '{}'}  resources {res or '{}'}"
                  + ("" if text else f"  lines {n} (in a loop {loop}, naming an AGPR {agpr})"))
    sys.exit(0 if same else 1)
