"""The match-history models restated on the host (include/lac.h lac_hist_*; helper of
tests/test_history_host.py, tests/test_gpu_history.py and tests/test_gpu_history_dropin.py).

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
