"""The match-history models restated on the host (include/lac.h lac_hist_*; helper of
tests/test_history_host.py, tests/test_gpu_history.py, tests/test_gpu_history_limits.py and
tests/test_gpu_history_dropin.py).

A model: V symbols, a ring of P past symbols and weights L[i][r] (lag i, run r).  A stream keeps
``ring`` (P integers, -1 at the start) and the write index ``pasti``.  Literally as the
reference's History.runs / calc_dist / accept (arith_code.py:371-393):

    for i in range(P):
        p = ring[pasti-1-i]                               (Python's indexing: a negative index wraps)
        r = number of j = 1, 2, .. < P-i, while ring[pasti-1-i-j] == ring[pasti-j]
        if p > 0:  row[p] += L[i][r]                      (row starts as all ones)
    accept(s):  ring[pasti] = s;  pasti = (pasti+1) % P

``Stream.runs`` is those loops as they stand; ``Stream.runs_np`` the same comparisons as one
[P, P] array, for the shapes where the loops would take minutes (test_history_host.py holds the two
to each other).
"""
import functools

import numpy as np

# the non-table lfuncs of the fixtures, by name (tools/gen_golden_history.py)
LFUNCS = {"hyper": lambda r, i, n, p: (r * r + 3) * n // (i + 1) + (r > 2)}


def default_weights(V, P):
    """The reference's default lfunc, n*r**3 + 1, as a table."""
    return [[V * r ** 3 + 1 for r in range(P)] for _ in range(P)]


def table_of(lfunc, V, P):
    return [[int(lfunc(r, i, V, P)) for r in range(P)] for i in range(P)]


class Stream:
    """One stream's ring and write index, and the rows they give."""

    def __init__(self, V, P, L, ring=None, pasti=0):
        self.V, self.P, self.L = V, P, L
        self.ring = [-1] * P if ring is None else [int(x) for x in ring]
        self.pasti = int(pasti)
        assert len(self.ring) == P and 0 <= self.pasti < P

    def runs(self):
        """(p, r, i) for every lag with p > 0: the reference's loops."""
        P, ring, pasti = self.P, self.ring, self.pasti
        for i in range(P):
            p = ring[pasti - 1 - i]
            r = 0
            for j in range(1, P - i):
                if ring[pasti - 1 - i - j] != ring[pasti - j]:
                    break
                r += 1
            if p > 0:
                yield (p, r, i)

    def runs_np(self):
        """The same triples from one [P, P] comparison."""
        P = self.P
        ring = np.array(self.ring, dtype=np.int64)
        i = np.arange(P)[:, None]
        j = np.arange(1, P)[None, :] if P > 1 else np.zeros((1, 0), dtype=np.int64)
        eq = (ring[(self.pasti - 1 - i - j) % P] == ring[(self.pasti - j) % P]) & (j < P - i)
        r = np.where(eq.all(axis=1), eq.shape[1], np.argmin(eq, axis=1)) if P > 1 else np.zeros(P, dtype=np.int64)
        p = ring[(self.pasti - 1 - i[:, 0]) % P]
        return [(int(p[k]), int(r[k]), k) for k in range(P) if p[k] > 0]

    def row(self, fast=None):
        """The step's row as Python integers (exact)."""
        out = [1] * self.V
        fast = self.P > 16 if fast is None else fast
        for p, r, i in (self.runs_np() if fast else self.runs()):
            out[p] += int(self.L[i][r])
        return out

    def accept(self, s):
        self.ring[self.pasti] = int(s)
        self.pasti = (self.pasti + 1) % self.P


def pmf_rows(rows, bits, V=None):
    """Rows of Python integers as the pmf path takes them: an array in the entries' type; a row
    with an entry that does not fit becomes the empty row (LAC_E_TABLE at that step, as it is for
    the history model)."""
    dt = np.uint32 if bits == 32 else np.uint64
    out = np.zeros((len(rows), len(rows[0]) if rows else V), dtype=dt)
    for t, r in enumerate(rows):
        if max(r) < (1 << bits) and sum(r) < (1 << 64):
            out[t] = np.array(r, dtype=np.uint64).astype(dt)
    return out


def walk(V, P, L, syms, bits=32, ring=None, pasti=0, extra_row=False):
    """One stream: the rows [T (+ 1), V] its symbols are coded with, and the Stream afterwards.  A
    symbol outside [0, V) or a row with an entry that does not fit ends the walk there (the stream
    fails at that step, nothing moves); the rows after it repeat the failing step's."""
    st = Stream(V, P, L, ring, pasti)
    rows, dead = [], False
    for s in syms:
        rows.append(st.row() if not dead else rows[-1])
        row_ok = max(rows[-1]) < (1 << bits)
        if dead or not (0 <= s < V and row_ok):
            dead = True
        else:
            st.accept(s)
    if extra_row:
        rows.append(st.row())
    return pmf_rows(rows, bits, V), st


def walk_batch(V, P, L, sym, bits=32, states=None):
    """sym [T, B] -> (rows [T, B, V], [Stream] * B); ``states``: the streams to continue (copied)."""
    T, B = sym.shape
    rows = np.zeros((T, B, V), dtype=np.uint32 if bits == 32 else np.uint64)
    out = []
    for b in range(B):
        r, p = (None, 0) if states is None else (states[b].ring, states[b].pasti)
        rows[:, b], st = walk(V, P, L, sym[:, b].tolist(), bits, r, p)
        out.append(st)
    return rows, out


def pattern(kind, rng, V, T):
    """One stream's symbols: a constant run, a period-3 run, random symbols, or symbol 0 only
    (every row all ones)."""
    if kind == "constant":
        return np.full(T, V - 1, dtype=np.int32)
    if kind == "period3":
        return (np.array([V - 1, 1 % V, V // 2])[np.arange(T) % 3]).astype(np.int32)
    if kind == "zeros":
        return np.zeros(T, dtype=np.int32)
    return rng.integers(0, V, size=T).astype(np.int32)


PATTERNS = ("constant", "period3", "random", "zeros")


def draw(rng, V, T, B=1):
    """Symbols [T, B]: stream b follows PATTERNS[b % 4]."""
    return np.stack([pattern(PATTERNS[b % 4], rng, V, T) for b in range(B)], axis=1)


def fudged_share(V, P, L, prec, syms):
    """Share of a stream's steps whose row has T > 2 w0 (minp is 1), w0 = 2^(prec-1): fudged at
    every width."""
    st, n = Stream(V, P, L), 0
    for s in syms:
        n += sum(st.row()) > (2 << (prec - 1))
        st.accept(s)
    return n / len(syms)


# ------------------------------------------------------------------ jobs at the kernels' limits
# (tests/test_history_host.py holds each to what it is meant to reach; tests/test_gpu_history_limits.py codes them)
W48 = (1 << 48) - 1                                                   # the largest weight a model takes


def wide_weights(P):
    """Weights over the whole range a table may hold -- 0, 1, both sides of 2^32, 2^47 and up to
    the limit 2^48 - 1 --, and the limit itself at every lag's clamped run: a constant stream's
    row reaches the documented maximum V + P (2^48 - 1)."""
    L = [[(0, 1, (1 << 32) - 1, 1 << 32, (1 << 47) + i, W48 - r)[(7 * i + 3 * r) % 6] for r in range(P)]
         for i in range(P)]
    for i in range(P):
        L[i][P - i - 1] = W48
    return L


def seam_weights(P, add=0):
    """Weights that tell every lag and every run apart."""
    return [[add + 1 + (257 * i + 13 * r) % 3001 for r in range(P)] for i in range(P)]


def wide_symbols(V, P, seed=0):
    """[2 P + 9, 5]: the four PATTERNS, and a stream that is constant for P + 3 steps, then random."""
    rng = np.random.default_rng(1000 * V + P + seed)
    T = 2 * P + 9
    sym = draw(rng, V, T, 5)
    sym[:P + 3, 4] = V - 2
    sym[P + 3:, 4] = rng.integers(0, V, size=T - P - 3)
    return sym


def totals(rows):
    """Exact totals of rows [..., V] as Python integers, in an object array."""
    return rows.astype(object).sum(axis=-1)


def fudge_classes(tot, prec):
    """Shares of the steps that always fudge (T > 2^prec), sometimes, and never (T <= 2^(prec-1)):
    minp is 1 and the coder's width lies in (2^(prec-1), 2^prec]."""
    t = np.array(tot, dtype=object).reshape(-1)
    always = sum(int(x) > (1 << prec) for x in t) / len(t)
    never = sum(int(x) <= (1 << (prec - 1)) for x in t) / len(t)
    return always, 1.0 - always - never, never


def edge32_weights(lags, P=192):
    """``lags`` = (a, b, c): L[a][*] = L[b][*] = 2^31 - 1, L[c][*] = 1, every other weight 0.  A
    symbol at lags a and b has the entry 2^32 - 1, the last that fits u32; at c as well, 2^32."""
    L = [[0] * P for _ in range(P)]
    L[lags[0]] = [(1 << 31) - 1] * P
    L[lags[1]] = [(1 << 31) - 1] * P
    L[lags[2]] = [1] * P
    return L


def edge32_symbols(V=6, T=140):
    """[T, 4]: constant 5; constant 5 for 100 steps, then 1 + t % 4; constant 5 with the symbol V
    at step 129; zeros."""
    sym = np.full((T, 4), 5, dtype=np.int32)
    sym[100:, 1] = 1 + np.arange(100, T) % 4
    sym[129, 2] = V
    sym[:, 3] = 0
    return sym


def seam_symbols(V, P):
    """[2 P + 9, 3]: constant, period 3, random."""
    return draw(np.random.default_rng(31 * P + V), V, 2 * P + 9, 3)[:, :3]


def seam_positions(V, bits):
    """The entries at the edges of the decoder's search: the first and last entry of a lane's
    vector, of a pass of 64 lanes and of the row."""
    vec = 16 // (bits // 8)
    S = {0, 1, vec - 1, vec, 64 * vec - 1, 64 * vec, 64 * vec + 1, 128 * vec - 1, 128 * vec, V - 2, V - 1}
    return sorted(s for s in S if 0 <= s < V)


def steered_symbols(V, bits, P):
    """[T, 2]: one stream cycles through the seam positions, the other through them reversed, for
    2 P + 3 steps and two cycles more (the ring is full for more than half of them): with P = 4 a
    coded symbol is never in the ring, with P = 64 always after the first cycle."""
    S = seam_positions(V, bits)
    T = 2 * P + 2 * len(S) + 3
    k = np.arange(T) % len(S)
    return np.stack([np.array(S)[k], np.array(S[::-1])[k]], axis=1).astype(np.int32)


def probe_ring(V, bits, P=16):
    """The ring of the exact-bounds probes: the seam positions strictly inside (0, V - 1) in
    order, the rest -1, and pasti their count."""
    inside = [s for s in seam_positions(V, bits) if 0 < s < V - 1]
    assert len(inside) < P
    return inside + [-1] * (P - len(inside)), len(inside)


def bound_probes(row, V, bits, prec):
    """(s, x) for s in the seam positions and their successors: x the first and the last value of
    the coder's full width w = 2^prec that decodes to s, from the restatement's exact ranges."""
    from oracle import restate
    cdf, w = restate.cdf_of(row), 1 << prec
    S = seam_positions(V, bits)
    out = []
    for s in sorted(set(S) | {s + 1 for s in S if s + 1 < V}):
        a, b = restate.symbol_to_range(cdf, 1, s, w)
        assert b > a, (s, a, b)
        out += [(s, a)] + ([(s, b - 1)] if b - 1 > a else [])
    return out


JOBS = {
    # kind: (V, P, weights, entry bits, symbols) of its arguments
    "wide": lambda V, P: (V, P, wide_weights(P), 64, wide_symbols(V, P)),
    "edge32": lambda bits, a, b, c: (6, 192, edge32_weights((a, b, c)), bits, edge32_symbols()),
    "edge32_clean": lambda bits, a, b, c: (6, 192, edge32_weights((a, b, c)), bits, np.where(edge32_symbols() == 6, 5, edge32_symbols())),
    "edge32_lanes": lambda bits: (6, 192, edge32_weights((0, 1, 2)), bits,
                                  np.stack([np.full(12, 5), np.zeros(12)], axis=1).astype(np.int32)),
    "seam": lambda P: (5, P, seam_weights(P), 32, seam_symbols(5, P)),
    "steered": lambda V, bits, P: (V, P, seam_weights(P), bits, steered_symbols(V, bits, P)),
}


@functools.lru_cache(maxsize=None)
def job(kind, *args):
    """(V, P, L, bits, sym, rows, streams afterwards) of a job of JOBS: walked once, and left as it
    is by every test that shares it."""
    V, P, L, bits, sym = JOBS[kind](*args)
    rows, sts = walk_batch(V, P, L, sym, bits)
    return V, P, L, bits, sym, rows, sts


@functools.lru_cache(maxsize=None)
def job_verdict(prec, kind, *args):
    """The C oracle's verdict (tests/errors.py) on the job's restated rows."""
    import types

    import errors
    _, _, _, _, sym, rows, _ = job(kind, *args)
    return errors.verdict(types.SimpleNamespace(B=sym.shape[1], prec=prec), rows, sym)
