#!/usr/bin/env python3
"""Generate tests/golden/history_cases.json by running the REFERENCE coder on its match-history
predictor.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_history.py

Imports /root/reference (read-only, never copied).  Each case is a history model -- V symbols, a
ring of P past symbols, an ``lfunc`` -- and symbols, coded by ``A_to_bin(History(V, P, lfunc), prec)``
(arith_code.py:364-398).  ``lfunc`` is the reference's default argument ("default"), a table
``(r, i, n, p) -> table[i][r]`` (stored), or a named function that the tests restate.  Recorded: the
bytes and bit count of ``bits(symbols)``, the ring and write index the model ends with, and -- where
the reference's ``A_from_bin.run(bits, stop=0)`` returns within the time limit -- what it emits.  At
prec 48 it does not (it was left running for 40 s on the two cases here), so those cases carry
``decoded: null``.  Every reference call runs under a time limit.  The symbols are phases of random
symbols, a period-3 run and a constant run, each longer than the ring where the case's length allows.
Output: data only.
"""
from __future__ import annotations

import json
import os
import random
import signal
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, "/root/reference")

import arith_code as ref  # noqa: E402  (the reference, read-only)

OUT = os.path.join(REPO, "tests", "golden", "history_cases.json")
LIMIT_S = 20

# the non-table lfuncs, by name (tests/history.py restates them)
LFUNCS = {"hyper": lambda r, i, n, p: (r * r + 3) * n // (i + 1) + (r > 2)}


class TimeUp(Exception):
    pass


def limited(f, seconds=LIMIT_S):
    """f() under a time limit; TimeUp when it runs out."""
    def ring(*_):
        raise TimeUp()
    old = signal.signal(signal.SIGALRM, ring)
    signal.alarm(seconds)
    try:
        return f()
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def draw(rng, V, n, phases):
    """n symbols in equal phases: 'r' random, '3' period 3, 'c' one symbol, '0' symbol 0."""
    syms, per = [], -(-n // len(phases))
    for k, ph in enumerate(phases):
        for t in range(per):
            if ph == "r":
                syms.append(rng.randrange(V))
            elif ph == "3":
                syms.append((V - 1, 1 % V, V // 2)[t % 3])
            elif ph == "c":
                syms.append(V - 1)
            else:
                syms.append(0)
    return syms[:n]


def model(V, P, weights, lfunc):
    if lfunc is not None:
        return ref.History(V, P, LFUNCS[lfunc])
    if weights == "default":
        return ref.History(V, P)
    return ref.History(V, P, lambda r, i, n, p, W=weights: W[i][r])


def totals(V, P, weights, lfunc, syms):
    """T of every step's row."""
    p, out = model(V, P, weights, lfunc), []
    for s in syms:
        out.append(p.calc_dist()[-1])
        p.accept(s)
    return out


def run_reference(V, P, weights, lfunc, syms, prec, decode):
    mk = lambda: model(V, P, weights, lfunc)  # noqa: E731
    enc = mk()
    bits = limited(lambda: list(ref.A_to_bin(enc, prec).bits(syms)))
    assert all(b in (0, 1) for b in bits)
    rec = {"L": len(bits), "bytes": bytes(ref.group_bits(iter(bits))).hex(), "ring": list(enc.past),
           "pasti": enc.pasti, "decoded": None, "decoded_count": None}
    if decode:
        dec = limited(lambda: list(ref.A_from_bin(mk(), prec).run(iter(bits), stop=0)))
        assert dec[:len(syms)] == syms, "reference round trip failed"
        rec["decoded"] = dec
        rec["decoded_count"] = len(dec)
    return rec


def table(P, f):
    return [[f(r, i) for r in range(P)] for i in range(P)]


# (name, seed, V, P, weights ("default", a table, or the name of a function), prec, pmf_bits, symbols,
#  phases, whether the reference's decoder is run, the band the share of fudged steps must lie in)
CASES = [
    ("v3_p5_p16", 1, 3, 5, "default", 16, 32, 60, "r3cr", True, None),
    ("v2_p1_p12", 2, 2, 1, "default", 12, 32, 30, "rc0r", True, None),
    ("v5_p8_p16", 3, 5, 8, "default", 16, 32, 80, "r3c", True, None),
    ("v17_p16_p24_plain", 4, 17, 16, "default", 24, 32, 80, "rc3", True, (0.0, 0.0)),
    ("v256_p64_p20", 5, 256, 64, "default", 20, 32, 60, "rc", True, None),
    ("v256_p64_p48", 6, 256, 64, "default", 48, 32, 60, "rc", False, None),
    ("v256_p256_p48_u64", 7, 256, 256, "default", 48, 64, 40, "rc", False, None),
    ("v9_p6_p16_table", 8, 9, 6, table(6, lambda r, i: (r + 1) * (i + 2) * 7 if (r + i) % 4 else 0), 16, 32, 70, "r3cr",
     True, None),
    ("v7_p5_p16_hyper", 9, 7, 5, "hyper", 16, 32, 60, "rc3", True, None),
    ("v5_p8_p11_fudged", 10, 5, 8, "default", 11, 32, 90, "rcr", True, (0.1, 0.9)),
]


def main():
    out = []
    for name, seed, V, P, W, prec, bits, n, phases, decode, band in CASES:
        rng = random.Random(seed)
        syms = draw(rng, V, n, phases)
        lfunc = W if isinstance(W, str) and W != "default" else None
        rec = {"name": name, "V": V, "P": P, "weights": None if lfunc else W, "lfunc": lfunc, "prec": prec,
               "pmf_bits": bits, "syms": syms}
        rec.update(run_reference(V, P, W, lfunc, syms, prec, decode))
        # a step fudges when T > w minp with minp = 1 and 2^(prec-1) < w <= 2^prec: surely when
        # T > 2^prec, surely not when T <= 2^(prec-1)
        T = totals(V, P, W, lfunc, syms)
        sure = sum(t > 1 << prec for t in T) / n
        maybe = sum(t > 1 << (prec - 1) for t in T) / n
        if band is not None:
            assert band[0] <= sure and maybe <= band[1], (name, sure, maybe)
            rec["fudged_band"] = list(band)
        out.append(rec)
        print(name, rec["L"], rec["decoded_count"], f"fudged {sure:.2f}..{maybe:.2f}", flush=True)
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
