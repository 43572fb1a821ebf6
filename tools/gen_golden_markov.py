#!/usr/bin/env python3
"""Generate tests/golden/markov_cases.json by running the REFERENCE coder on its adaptive
n-gram predictor.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_markov.py

Imports /root/reference (read-only, never copied).  Each case is a count model -- V symbols, an
order, integer weights W -- and symbols, coded by
``A_to_bin(Markov_up_to_n(V, order, lfunc), prec)`` with ``lfunc(c, o, n, m) = c * W[o]``
(arith_code.py:443-464).  Recorded: the bytes and bit count of ``bits(symbols)``, what
``A_from_bin.run(bits, stop=0)`` emits for the whole stream and for a half-length prefix, and the
``past`` the model ends with.  No tables are stored: the counts follow from the symbols.  One
case has a non-linear ``lfunc`` (named, restated by the test) for the per-token path, and the
default-``lfunc`` case is also run with the default argument itself.  The symbol draw repeats
the symbol two back with probability 1/2 and is uniform otherwise, so contexts recur.
Output: data only.
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

OUT = os.path.join(REPO, "tests", "golden", "markov_cases.json")

# the non-linear lfuncs, by name (tests/counts.py restates them)
LFUNCS = {"square": lambda c, o, n, m: c * c * (o + 1) + (7 if c else 0)}


def draw(rng, V, n):
    syms = []
    for t in range(n):
        syms.append(syms[t - 2] if t >= 2 and rng.random() < 0.5 else rng.randrange(V))
    return syms


def model(V, order, W, lfunc):
    if lfunc is not None:
        return ref.Markov_up_to_n(V, order, LFUNCS[lfunc])
    return ref.Markov_up_to_n(V, order, lambda c, o, n, m, W=tuple(W): c * W[o])


def always_fudged_share(V, order, W, prec, syms):
    """Share of steps whose row has T > 2 w0 minp, w0 = 2^(prec-1): fudged at every width."""
    p = model(V, order, W, None)
    n = 0
    for s in syms:
        row = [p.prob(x) for x in range(V)]
        n += sum(row) > (2 << (prec - 1)) * min(row)
        p.accept(s)
    return n / len(syms)


def run_reference(V, order, W, lfunc, syms, prec):
    mk = lambda: model(V, order, W, lfunc)  # noqa: E731
    enc = mk()
    bits = list(ref.A_to_bin(enc, prec).bits(syms))
    assert all(b in (0, 1) for b in bits)
    rec = {"L": len(bits), "bytes": bytes(ref.group_bits(iter(bits))).hex(), "past": list(enc.past)}
    dec = list(ref.A_from_bin(mk(), prec).run(iter(bits), stop=0))
    assert dec[:len(syms)] == syms, "reference round trip failed"
    rec["decoded_count"] = len(dec)
    rec["decoded"] = dec
    cut = len(bits) // 2
    pre = list(ref.A_from_bin(mk(), prec).run(iter(bits[:cut]), stop=0))
    assert pre == dec[:len(pre)]
    rec["prefix_bits"] = cut
    rec["prefix_decoded_count"] = len(pre)
    return rec


# (name, seed, V, order, W (or the name of a non-linear lfunc), prec, pmf_bits, symbols)
CASES = [
    ("v2_o1_p16", 1, 2, 1, [1], 16, 32, 64),
    ("v4_o2_p16", 2, 4, 2, [1, 9], 16, 32, 200),
    ("v17_o2_p16", 3, 17, 2, [3, 7000], 16, 32, 300),
    ("v40_o2_p16_fudged", 4, 40, 2, [900, 1], 16, 32, 200),
    ("v64_o1_p16_fudged", 5, 64, 1, [5000], 16, 32, 150),
    ("v12_o3_p16_default", 6, 12, 3, [0, 12, 96], 16, 32, 200),
    ("v100_o2_p16", 7, 100, 2, [1, 30000], 16, 32, 120),
    ("v300_o2_p16_two_passes", 8, 300, 2, [2000, 1], 16, 32, 90),
    ("v256_o2_p48", 9, 256, 2, [1, 300], 48, 32, 130),
    ("v256_o1_p24", 10, 256, 1, [1], 24, 32, 70),
    ("v5_o3_p16", 11, 5, 3, [1, 40, 5000], 16, 32, 260),
    ("v31_o3_p48_u64", 12, 31, 3, [1, 1 << 20, 1 << 29], 48, 64, 100),
    ("v3_o4_p16", 13, 3, 4, [1, 5, 50, 700], 16, 32, 240),
    ("v129_o2_p48_u64", 14, 129, 2, [1 << 29, 3], 48, 64, 110),
    ("v9_o2_p24_square", 15, 9, 2, "square", 24, 32, 150),
]


def main():
    out = []
    for name, seed, V, order, W, prec, bits, n in CASES:
        rng = random.Random(seed)
        syms = draw(rng, V, n)
        lfunc = W if isinstance(W, str) else None
        rec = {"name": name, "V": V, "order": order, "weights": None if lfunc else W, "lfunc": lfunc, "prec": prec,
               "pmf_bits": bits, "syms": syms}
        rec.update(run_reference(V, order, W, lfunc, syms, prec))
        share = None
        if lfunc is None:
            share = always_fudged_share(V, order, W, prec, syms)
        if name.endswith("_default"):                             # the default argument is these weights
            assert W == [V * o ** 3 for o in range(order)]
            d = list(ref.A_to_bin(ref.Markov_up_to_n(V, order), prec).bits(syms))
            assert d == list(ref.A_to_bin(model(V, order, W, None), prec).bits(syms))
            rec["default_lfunc"] = True
        out.append(rec)
        print(name, rec["L"], rec["decoded_count"], rec["prefix_decoded_count"], share, flush=True)
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
