#!/usr/bin/env python3
"""Generate tests/golden/nfa_cases.json by running the REFERENCE coder on its NFA predictor.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_nfa.py

Imports /root/reference (read-only, never copied).  Each case is a finite-state model --
``tables`` [K][V] integer pmf rows and ``next`` [K][V] transitions -- a start state and symbols,
coded by ``A_to_bin(NFA(state, transitions), prec)`` with ``transitions[q] = (cdf, next[q])``
(arith_code.py:423-434; ``dcache = None`` is set on the instance, which the reference's
``NFA.__init__`` omits).  Recorded: the bytes and bit count of ``bits(symbols)``, what
``A_from_bin.run(bits, stop=0)`` emits for the whole stream and for a truncated prefix, and the
state the model ends in.  An order-1 byte model's ``next`` is stored as the string "symbol"
(next[q][s] = s).  Output: data only.
"""
from __future__ import annotations

import itertools
import json
import os
import random
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, "/root/reference")

import arith_code as ref  # noqa: E402  (the reference, read-only)

OUT = os.path.join(REPO, "tests", "golden", "nfa_cases.json")


def nfa(state, tables, nxt):
    p = ref.NFA(state, [(list(itertools.accumulate(r)), n) for r, n in zip(tables, nxt)])
    p.dcache = None
    return p


def row(rng, V, kind):
    """One pmf row with at least two positive entries (a one-symbol row makes the reference's
    bit-driven decoder loop forever)."""
    while True:
        if kind == "small":           # totals far below 2^(prec-1): never fudged
            r = [rng.choice([0, 1, 1, 2, 3, 5, 8, 13]) for _ in range(V)]
        elif kind == "heavy":         # minp = 1 and a total past 2^16: fudged at prec 16 on every step
            r = [rng.choice([1, 1, 2, 7, 900, 30000, 70000]) for _ in range(V)]
            r[rng.randrange(V)] = 1
            r[rng.randrange(V)] = 90000
        elif kind == "peaked":
            r = [1] * V
            r[rng.randrange(V)] = 1 << 14
        elif kind == "zeros":
            r = [rng.choice([0, 0, 0, 4, 9, 100]) for _ in range(V)]
        elif kind == "big":           # u64 entries, totals near 2^40
            r = [rng.randrange(1, 1 << 36) for _ in range(V)]
        else:
            raise ValueError(kind)
        if sum(1 for p in r if p > 0) >= 2:
            return r


def walk(rng, tables, nxt, state, n):
    syms, q = [], state
    for _ in range(n):
        r = tables[q]
        s = rng.choices(range(len(r)), weights=[min(p, 1000) + (1 if p else 0) for p in r])[0]
        syms.append(s)
        q = nxt[q][s]
    return syms, q


def run_reference(tables, nxt, state, syms, prec):
    bits = list(ref.A_to_bin(nfa(state, tables, nxt), prec).bits(syms))
    assert all(b in (0, 1) for b in bits)
    rec = {"L": len(bits), "bytes": bytes(ref.group_bits(iter(bits))).hex()}
    dec = list(ref.A_from_bin(nfa(state, tables, nxt), prec).run(iter(bits), stop=0))
    assert dec[:len(syms)] == syms, "reference round trip failed"
    rec["decoded_count"] = len(dec)
    rec["decoded"] = dec
    cut = len(bits) // 2
    pre = list(ref.A_from_bin(nfa(state, tables, nxt), prec).run(iter(bits[:cut]), stop=0))
    assert pre == dec[:len(pre)]
    rec["prefix_bits"] = cut
    rec["prefix_decoded_count"] = len(pre)
    return rec


# (name, seed, V, K, prec, pmf_bits, row kinds by state (cycled), symbols)
CASES = [
    ("v2_k1_p16", 1, 2, 1, 16, 32, ["small"], 40),
    ("v2_k3_p24", 2, 2, 3, 24, 32, ["small", "peaked"], 70),
    ("v5_k4_p16_fudged", 3, 5, 4, 16, 32, ["heavy"], 90),
    ("v17_k8_p16_fudged", 4, 17, 8, 16, 32, ["heavy"], 130),
    ("v12_k6_p16_mixed", 5, 12, 6, 16, 32, ["small", "heavy", "peaked"], 150),
    ("v64_k16_p24", 6, 64, 16, 24, 32, ["small", "zeros", "peaked"], 100),
    ("v100_k10_p48_zeros", 7, 100, 10, 48, 32, ["zeros", "small"], 65),
    ("v256_k2_p24", 8, 256, 2, 24, 32, ["peaked", "small"], 64),
    ("v3_k256_p16", 9, 3, 256, 16, 32, ["small", "peaked"], 200),
    ("v31_k5_p48_u64", 10, 31, 5, 48, 64, ["big", "small"], 80),
    ("v7_k3_p24_u64", 11, 7, 3, 24, 64, ["small", "zeros"], 63),
    ("order1_bytes_p48", 12, 256, 256, 48, 32, ["small", "zeros", "peaked"], 300),
]


def main():
    out = []
    for name, seed, V, K, prec, bits, kinds, n in CASES:
        rng = random.Random(seed)
        tables = [row(rng, V, kinds[q % len(kinds)]) for q in range(K)]
        order1 = name.startswith("order1")
        nxt = [list(range(V)) for _ in range(K)] if order1 else [[rng.randrange(K) for _ in range(V)] for _ in range(K)]
        state = rng.randrange(K)
        syms, end = walk(rng, tables, nxt, state, n)
        rec = {"name": name, "V": V, "K": K, "prec": prec, "pmf_bits": bits, "state": state, "tables": tables,
               "next": "symbol" if order1 else nxt, "syms": syms, "end_state": end}
        rec.update(run_reference(tables, nxt, state, syms, prec))
        out.append(rec)
        print(name, rec["L"], rec["decoded_count"], rec["prefix_decoded_count"], flush=True)
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
