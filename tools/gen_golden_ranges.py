#!/usr/bin/env python3
"""Generate tests/golden/range_cases.json by running the REFERENCE coder on implicit CDFs.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_ranges.py

Imports /root/reference (read-only, never copied).  Each case is a CDF given by a formula -- never
written out -- and symbols, coded by ``AC(CDFPredictor(lazy), prec)``: the reference's
``symbol_to_range`` indexes ``dist[s-1]``, ``dist[s]`` and ``dist[-1]`` only (arith_code.py:98-110),
so a lazy sequence serves it, and every total here is at most 2^(prec-1), so no step fudges.
Formulas (tests/ranges.py restates them):

    quad     c_i = (i + 1) (i + 1 + K)      i < V     T = V (V + K)
    uniform  c_i = (i + 1) step             i < V     T = V step

Recorded: the formula's parameters, the symbols, the bit count ``L`` and bytes of ``bits(symbols)``
and ``decoded_count``, the number of symbols ``A_from_bin.run(bits, stop=0)`` emits (0 for a stream
of no bits: the reference decides only when a bit arrives).  Output: data only.
"""
from __future__ import annotations

import json
import os
import random
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, "/root/reference")

import arith_code as ref  # noqa: E402  (the reference, read-only)

OUT = os.path.join(REPO, "tests", "golden", "range_cases.json")


class Lazy:
    """A CDF as a sequence that computes its entries."""

    def __init__(self, kind, V, par):
        self.kind, self.V, self.par = kind, V, par

    def __len__(self):
        return self.V

    def __getitem__(self, i):
        if i < 0:
            i += self.V
        if not 0 <= i < self.V:
            raise IndexError(i)
        return (i + 1) * (i + 1 + self.par) if self.kind == "quad" else (i + 1) * self.par


class Model(ref.CDFPredictor):
    """CDFPredictor over a lazy dist; minp from the formula (its __init__ walks all V entries)."""

    def __init__(self, dist):
        self.dist = dist
        self.minp = dist[0] if dist.kind == "uniform" or len(dist) == 1 else min(dist[0], dist[1] - dist[0])


# (name, kind, V, parameter, prec, steps, seed)
CASES = [
    ("quad_v16_k3_p34_n64", "quad", 1 << 16, 3, 34, 64, 1),
    ("quad_v16_half_p34_n65", "quad", 1 << 16, 1 << 16, 34, 65, 2),        # T = 2^33 = 2^(prec-1) exactly
    ("quad_v16_k7_p48_n130", "quad", 1 << 16, 7, 48, 130, 3),
    ("quad_v16_k1_p61_n64", "quad", 1 << 16, 1, 61, 64, 4),
    ("quad_v16_k9_p40_n1", "quad", 1 << 16, 9, 40, 1, 5),
    ("quad_v20_k5_p48_n65", "quad", 1 << 20, 5, 48, 65, 6),
    ("quad_v20_k1000_p61_n130", "quad", 1 << 20, 1000, 61, 130, 7),
    ("uni_half_p16_n64", "uniform", 1 << 15, 1, 16, 64, 8),                # T = 2^15 = 2^(prec-1)
    ("uni_half_p16_n1", "uniform", 32, 1 << 10, 16, 1, 9),
    ("uni_half_p48_n65", "uniform", 1 << 12, 1 << 35, 48, 65, 10),         # T = 2^47 = 2^(prec-1)
    ("uni_half_p48_n130", "uniform", 1 << 40, 1 << 7, 48, 130, 11),
    ("one_p16_n64", "uniform", 1, 1, 16, 64, 12),                          # V = 1, T = 1: zero bits per symbol
    ("one_p48_n1", "uniform", 1, 1, 48, 1, 13),
    ("one_p61_n130", "uniform", 1, 1, 61, 130, 14),
]


def main():
    out = []
    for name, kind, V, par, prec, n, seed in CASES:
        rng = random.Random(seed)
        syms = [rng.randrange(V) for _ in range(n)]
        syms[0] = V - 1                                            # symbols 0 and V - 1 present
        syms[-1 if n > 1 else 0] = 0 if n > 1 else V - 1
        if n > 2:
            syms[n // 2] = 0
        dist = Lazy(kind, V, par)
        assert dist[-1] <= 1 << (prec - 1), name
        # the shortcut for minp is the reference's own value (walked where V allows)
        if V <= 1 << 16:
            assert Model(dist).minp == ref.CDFPredictor(dist).minp, name
        bits = list(ref.AC(Model(dist), prec).to_bin.bits(syms))
        assert all(b in (0, 1) for b in bits)
        dec = list(ref.AC(Model(dist), prec).from_bin.run(iter(bits), stop=0))
        assert dec[:n] == syms[:len(dec)] and (not bits or len(dec) >= n), name
        out.append({"name": name, "kind": kind, "V": V, "par": par, "prec": prec, "syms": syms, "L": len(bits),
                    "bytes": bytes(ref.group_bits(iter(bits))).hex(), "decoded_count": len(dec)})
        print(name, len(bits), len(dec), flush=True)
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
