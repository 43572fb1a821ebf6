"""Shared by the sparse-row tests (test_sparse_host.py, test_gpu_sparse.py): the fixtures of
tests/golden/sparse_cases.json as slot arrays, the rules of lac_amd/csrc/lac_sparse.h restated in
Python integers on the dense row, random rows, and the census of the existing fixtures that are
sparse rows with every symbol a pair."""
import random

import numpy as np

from conftest import load_golden

SPARSE_CASES = load_golden("sparse_cases.json")


# ------------------------------------------------------------------ slot arrays
def slots(pairs, K):
    """[[idx list], [wt list]] -> (idx int32 [K], wt uint32 [K]), pads -1 / 0."""
    idx = np.full(K, -1, dtype=np.int32)
    wt = np.zeros(K, dtype=np.uint32)
    idx[:len(pairs[0])] = pairs[0]
    wt[:len(pairs[1])] = pairs[1]
    return idx, wt


def job_slots(rows, K):
    """rows[t] = [[idx], [wt]] -> (idx int32 [steps, K], wt uint32 [steps, K])."""
    got = [slots(r, K) for r in rows]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def case_slots(case):
    return job_slots(case["rows"], case["K"])


# ------------------------------------------------------------------ Python integers on the dense row
def dense(pairs, base, V):
    """One dense row in Python integers."""
    row = [base] * V
    for i, w in zip(*pairs):
        row[i] += int(w)
    return row


def dense_job(rows, base, V):
    return np.array([dense(r, base, V) for r in rows], dtype=np.uint64).reshape(len(rows), V)


def total(pairs, base, V):
    return base * V + sum(int(w) for w in pairs[1])


def triple(pairs, base, s):
    """(lo, hi) of symbol s: c_{s-1}, c_s of the dense row, without writing it."""
    lo = base * s + sum(int(w) for i, w in zip(*pairs) if i < s)
    return lo, lo + base + sum(int(w) for i, w in zip(*pairs) if i == s)


def triples(rows, base, V, syms):
    """The Python-integer triples of a job (lac_encode_ranges' inputs)."""
    lo, hi = zip(*(triple(r, base, s) for r, s in zip(rows, syms)))
    return list(lo), list(hi), [total(r, base, V) for r in rows]


def row_valid(idx, wt, base, V, prec):
    """The whole-row validity rule on slot arrays."""
    idx = [int(x) for x in idx]
    n = 0
    while n < len(idx) and idx[n] >= 0:
        n += 1
    if any(x != -1 for x in idx[n:]) or any(x >= V for x in idx[:n]):
        return False
    if any(a >= b for a, b in zip(idx[:n], idx[1:n])):
        return False
    return base * V + sum(int(w) for w in wt[:n]) <= 1 << (prec - 1)


def search_targets(pairs, base, V):
    """t = 0, T - 1 and every A_j - 1, A_j, B_j - 1, B_j that lies in [0, T)."""
    T = total(pairs, base, V)
    ts = {0, T - 1}
    P = 0
    for i, w in zip(*pairs):
        A = base * i + P
        B = A + base + int(w)
        ts |= {A - 1, A, B - 1, B}
        P += int(w)
    return sorted(t for t in ts if 0 <= t < T)


def dense_search(row, t):
    """bisect_right(cdf, t) on a dense row: -> (s, c_{s-1}, c_s)."""
    c = 0
    for s, p in enumerate(row):
        if c + p > t:
            return s, c, c + p
        c += p
    raise AssertionError("target past the total")


# ------------------------------------------------------------------ random rows
def random_pairs(rng, V, base, K, prec, n=None, full=False):
    """n (default random) ascending pairs with weights whose total stays valid; ``full``: the total
    is exactly 2^(prec-1) where the weights can reach it."""
    n = rng.randrange(0, min(K, V) + 1) if n is None else min(n, K, V)
    room = (1 << (prec - 1)) - base * V
    assert room >= 0
    if n == 0:
        return [[], []]
    picks = set()
    if n >= 2 and rng.random() < 0.5:
        i = rng.randrange(V - 1)
        picks |= {i, i + 1}                                  # adjacent pairs
    if n >= 2 and rng.random() < 0.3:
        picks |= {0, V - 1}
    while len(picks) < n:
        picks.add(rng.randrange(V))
    idx = sorted(picks)[:n]
    cap = min((1 << 32) - 1, room // n)
    wt = [rng.choice((0, min(1, cap), cap, rng.randrange(cap + 1))) for _ in range(n)]
    if full and room <= n * ((1 << 32) - 1):
        wt = [min((1 << 32) - 1, room // n)] * n
        left = room - sum(wt)
        for j in range(n):
            add = min(left, (1 << 32) - 1 - wt[j])
            wt[j] += add
            left -= add
        assert left == 0
    return [idx, wt]


def random_job(seed, V, base, K, prec, steps, n=None):
    rng = random.Random(seed)
    rows = [random_pairs(rng, V, base, K, prec, n=n, full=(t % 11 == 3)) for t in range(steps)]
    syms = []
    for t, r in enumerate(rows):
        c = [0, V - 1, rng.randrange(V)]
        for i in r[0]:
            c += [x for x in (i - 1, i, i + 1) if 0 <= x < V]
        syms.append(c[rng.randrange(len(c))])
    return rows, syms


# ------------------------------------------------------------------ census of the existing fixtures
def census_qualifies(c):
    """A small_cases.json fixture that is a sparse row job with every symbol a pair: every entry
    >= 1, V <= 256, every total <= 2^(prec-1) -- coded with base 1, wt = entry - 1 and K = V rounded
    up to a multiple of 4."""
    rows = c["rows"]
    if not c["syms"] or not rows or len(rows[0]) > 256:
        return False
    return all(all(1 <= int(x) <= 1 << 32 for x in r) and sum(int(x) for x in r) <= 1 << (c["prec"] - 1) for r in rows)


def census():
    small = load_golden("small_cases.json")
    return {kind: [c for c in small[kind] if census_qualifies(c)] for kind in ("static", "perstep")}


def census_slots(c):
    """-> (idx [rows, K], wt [rows, K], base = 1, K) of a census fixture."""
    V = len(c["rows"][0])
    K = (V + 3) // 4 * 4
    rows = [[list(range(V)), [int(x) - 1 for x in r]] for r in c["rows"]]
    return (*job_slots(rows, K), 1, K)
