#!/usr/bin/env python3
"""Generate tests/golden/sparse_cases.json by running the REFERENCE coder on the dense rows of
sparse cases.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_sparse.py

Imports /root/reference (read-only, never copied).  A sparse row is at most K (symbol, weight)
pairs over a uniform floor ``base``; its dense row is ``pmf[s] = base + wt_j where s == idx_j``,
so its CDF is ``c_i = base (i + 1) + sum_{idx_j <= i} wt_j`` -- computed on demand, never written
out, which is all ``AC(CDFPredictor(lazy), prec)`` needs: ``symbol_to_range`` indexes ``dist[s-1]``,
``dist[s]`` and ``dist[-1]`` only (arith_code.py:98-110), ``val_to_symbol`` bisects (:94-97), and
every total here is at most 2^(prec-1), so no step fudges.  The row changes with every step
(``accept``).

Recorded per case: prec, V, base, K, the pairs of every step (``rows[t] = [idx list, wt list]``,
the pads implied), the symbols, the bit count ``L`` and bytes of ``bits(symbols)`` and
``decoded_count``, the number of symbols ``A_from_bin.run(bits, stop=0)`` emits.  Output: data only.
"""
from __future__ import annotations

import bisect
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

OUT = os.path.join(REPO, "tests", "golden", "sparse_cases.json")


class Lazy:
    """The CDF of one sparse row as a sequence that computes its entries."""

    def __init__(self, V, base, idx, wt):
        self.V, self.base, self.idx = V, base, idx
        self.pre = [0, *itertools.accumulate(wt)]

    def __len__(self):
        return self.V

    def __getitem__(self, i):
        if i < 0:
            i += self.V
        if not 0 <= i < self.V:
            raise IndexError(i)
        return self.base * (i + 1) + self.pre[bisect.bisect_right(self.idx, i)]


class Model(ref.CDFPredictor):
    """CDFPredictor over the lazy rows of a job, one per step; minp from the pairs (its __init__
    walks all V entries)."""

    def __init__(self, V, base, rows):
        self.V, self.base, self.rows, self.i = V, base, rows, 0
        self._load()

    def _load(self):
        idx, wt = self.rows[min(self.i, len(self.rows) - 1)]
        self.dist = Lazy(self.V, self.base, idx, wt)
        self.minp = self.base if len(idx) < self.V else self.base + min(wt)

    def accept(self, symbol):
        self.i += 1
        self._load()

    def copy(self):
        return Model(self.V, self.base, self.rows)


def spread(rng, total, n, cap=(1 << 32) - 1):
    """n weights in [0, cap] that sum to total."""
    assert 0 <= total <= n * cap
    w = [0] * n
    left = total
    for j in range(n):
        hi = min(cap, left)
        lo = max(0, left - (n - 1 - j) * cap)
        w[j] = left if j == n - 1 else rng.randint(lo, max(lo, min(hi, 2 * left // (n - j) + 1)))
        left -= w[j]
    assert left == 0 and all(0 <= x <= cap for x in w)
    return w


def make_row(rng, V, base, K, prec, n, t, exact):
    """n pairs, ascending; by turns adjacent pairs, pairs at 0 and V - 1, weights of 0."""
    n = min(n, V, K)
    room = (1 << (prec - 1)) - base * V
    assert room >= 0
    if n == 0:
        return [[], []]
    picks = set()
    if t % 3 == 0 and n >= 2:                                      # adjacent pairs (i, i + 1)
        i = rng.randrange(V - 1)
        picks |= {i, i + 1}
    if t % 3 == 1 and n >= 2:                                      # pairs at symbols 0 and V - 1
        picks |= {0, V - 1}
    while len(picks) < n:
        picks.add(rng.randrange(V))
    idx = sorted(picks)
    cap = min((1 << 32) - 1, room)
    if exact:
        wt = spread(rng, room, n)
    else:
        wt = [rng.choice((0, 1, rng.randrange(cap // (2 * n) + 1), cap // n)) for _ in range(n)]
    assert base * V + sum(wt) <= 1 << (prec - 1)
    return [idx, wt]


def pick_symbol(rng, V, idx, t):
    """By turns: at a pair, directly before and after one, first and last in a gap, 0, V - 1."""
    gaps = []                                                      # (first, last) of every run of plain entries
    prev = -1
    for i in [*idx, V]:
        if i - prev > 1:
            gaps.append((prev + 1, i - 1))
        prev = i
    kind = t % 8
    if idx and kind == 0:
        return rng.choice(idx)
    if idx and kind == 1:
        return max(0, rng.choice(idx) - 1)
    if idx and kind == 2:
        return min(V - 1, rng.choice(idx) + 1)
    if gaps and kind == 3:
        return rng.choice(gaps)[0]
    if gaps and kind == 4:
        return rng.choice(gaps)[1]
    if kind == 5:
        return 0
    if kind == 6:
        return V - 1
    return rng.randrange(V)


# (name, V, prec, base, K, steps, pair counts by step (cycled), total exactly 2^(prec-1))
CASES = [
    ("v5_p16_b1_k4", 5, 16, 1, 4, 16, (0, 1, 4, 2, 3), False),
    ("v5_p34_b65537_k4_half", 5, 34, 65537, 4, 16, (3, 4, 2), True),
    ("v5_p61_b3_k8", 5, 61, 3, 8, 16, (5, 0, 1, 2), False),
    ("v5_p48_b3_k4", 5, 48, 3, 4, 9, (4, 1, 0), False),
    ("v300_p16_b3_k8_half", 300, 16, 3, 8, 16, (5, 8, 1), True),
    ("v300_p34_b1_k8_full", 300, 34, 1, 8, 16, (8,), False),
    ("v300_p48_b1_k64", 300, 48, 1, 64, 12, (64, 0, 1, 20), False),
    ("v300_p61_b70000_k4", 300, 61, 70000, 4, 16, (4, 2, 0, 1), False),
    ("v300_p48_b1_k256", 300, 48, 1, 256, 6, (256, 1, 0, 255), False),
    ("v300_p16_b1_k4_n1", 300, 16, 1, 4, 16, (1,), False),
    ("v18_p34_b1_k8", 1 << 18, 34, 1, 8, 16, (8, 3, 0, 1), False),
    ("v18_p48_bbig_k8_half", 1 << 18, 48, (1 << 29) - 1, 8, 16, (8, 1, 5), True),
    ("v18_p61_b3_k64", 1 << 18, 61, 3, 64, 12, (64, 17, 1, 0), False),
    ("v18_p48_b1_k4_n0", 1 << 18, 48, 1, 4, 8, (0,), False),
]


def main():
    out = []
    for ci, (name, V, prec, base, K, steps, counts, exact) in enumerate(CASES):
        rng = random.Random(100 + ci)
        rows = [make_row(rng, V, base, K, prec, counts[t % len(counts)], t, exact) for t in range(steps)]
        syms = [pick_symbol(rng, V, rows[t][0], t + ci) for t in range(steps)]
        for idx, wt in rows:
            assert len(idx) <= K and idx == sorted(set(idx)) and all(0 <= i < V for i in idx)
            assert base * V + sum(wt) <= 1 << (prec - 1), name
            assert not exact or base * V + sum(wt) == 1 << (prec - 1), name
        bits = list(ref.AC(Model(V, base, rows), prec).to_bin.bits(syms))
        assert all(b in (0, 1) for b in bits)
        dec = list(ref.AC(Model(V, base, rows), prec).from_bin.run(iter(bits), stop=0))
        assert dec[:steps] == syms[:len(dec)] and (not bits or len(dec) >= steps), name
        out.append({"name": name, "prec": prec, "V": V, "base": base, "K": K, "rows": rows, "syms": syms,
                    "L": len(bits), "bytes": bytes(ref.group_bits(iter(bits))).hex(), "decoded_count": len(dec)})
        print(name, len(bits), len(dec), flush=True)
    with open(OUT, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
