"""The adaptive n-gram count models restated on the host (include/lac.h lac_count_*; helper of
tests/test_counts_host.py, tests/test_gpu_counts.py, tests/test_gpu_counts_limits.py and
tests/test_gpu_counts_dropin.py).

A model: V symbols, an order k in [1, 4], integer weights W[0..k-1].  A stream keeps ``past``,
its last <= k accepted symbols, and one count per n-gram of length i + 1 (i < k).  With
m = len(past):  row[s] = 1 + sum_{i<m} W[i] * C_i[(last i symbols of past), s];  accept(s) adds 1
to those m counts and appends s to past -- unless one of them is 0xffffffff: then the step is
refused and nothing changes.  The counts are held dense, in the layout the device
uses (lac_amd/csrc/lac_count.h): per stream ``stride`` uint32 words, section i at word off[i],
V^i rows of Vc = 4 ceil(V / 4) counts, the row of a context its symbols read oldest first as
base-V digits.
"""
import numpy as np

# the non-linear lfuncs of the fixtures, by name (tools/gen_golden_markov.py)
LFUNCS = {"square": lambda c, o, n, m: c * c * (o + 1) + (7 if c else 0)}
COUNT_FULL = 0xffffffff                                           # a count here cannot be incremented (kCountFull)


def layout(V, order):
    Vc = -(-V // 4) * 4
    off, o = [], 0
    for i in range(order):
        off.append(o)
        o += V ** i * Vc
    return {"V": V, "Vc": Vc, "order": order, "off": off, "words": o, "stride": -(-o // 64) * 64}


def ngrams(V, order):
    return sum(V ** (i + 1) for i in range(order))


def row_index(ctx, V):
    """Row of a context (a tuple of symbols, oldest first) in its section."""
    r = 0
    for s in ctx:
        r = r * V + s
    return r


class Stream:
    """One stream's counts and past, and the rows they give."""

    def __init__(self, V, order, W, counts=None, past=()):
        self.V, self.order, self.W = V, order, [int(w) for w in W]
        self.y = layout(V, order)
        self.counts = np.zeros(self.y["stride"], dtype=np.uint32) if counts is None else np.array(counts, dtype=np.uint32)
        self.past = tuple(int(s) for s in past)

    def _at(self, i, s=0):
        ctx = self.past[len(self.past) - i:]
        return self.y["off"][i] + row_index(ctx, self.V) * self.y["Vc"] + s

    def row(self):
        """The step's row as Python integers (exact)."""
        out = [1] * self.V
        for i in range(len(self.past)):
            a = self._at(i)
            c = self.counts[a:a + self.V]
            if self.W[i]:
                for s in np.flatnonzero(c):
                    out[s] += self.W[i] * int(c[s])
        return out

    def accept(self, s):
        """Count s under the m current contexts and append it to past.  False, and nothing
        changes, when one of those counts is full (count_accept, lac_amd/csrc/lac_count.h)."""
        at = [self._at(i, s) for i in range(len(self.past))]
        if any(int(self.counts[a]) == COUNT_FULL for a in at):
            return False
        for a in at:
            self.counts[a] += 1
        self.past = (self.past + (int(s),))[-self.order:]
        return True

    def past_row(self):
        """past as the device holds it: [order], most recent last, -1 absent."""
        return [-1] * (self.order - len(self.past)) + list(self.past)

    def table(self):
        """The counts as the reference's dict: n-gram tuple -> count."""
        t = {}
        for i in range(self.order):
            for r in range(self.V ** i):
                a = self.y["off"][i] + r * self.y["Vc"]
                for s in np.flatnonzero(self.counts[a:a + self.V]):
                    ctx, x = [], r
                    for _ in range(i):
                        ctx.append(x % self.V)
                        x //= self.V
                    t[tuple(reversed(ctx)) + (int(s),)] = int(self.counts[a + s])
        return t


def pmf_rows(rows, bits, V=None):
    """Rows of Python integers as the pmf path takes them: an array in the entries' type; a row
    with an entry that does not fit, or a total >= 2^64, becomes the empty row (LAC_E_TABLE at
    that step, as it is for the count model)."""
    dt = np.uint32 if bits == 32 else np.uint64
    out = np.zeros((len(rows), len(rows[0]) if rows else V), dtype=dt)
    for t, r in enumerate(rows):
        if max(r) < (1 << bits) and sum(r) < (1 << 64):
            out[t] = np.array(r, dtype=np.uint64).astype(dt)
    return out


def walk(V, order, W, syms, bits=32, counts=None, past=(), extra_row=False):
    """One stream: the rows [T (+ 1), V] its symbols are coded with, and the Stream afterwards.  A
    symbol outside [0, V) ends the walk there (the stream fails at that step, nothing moves);
    the rows after it repeat the failing step's.  So does a symbol one of whose counts is full:
    that step's row is the empty row (LAC_E_TABLE there, as for a bad row)."""
    st = Stream(V, order, W, counts, past)
    rows, dead = [], False
    for s in syms:
        rows.append(st.row() if not dead else rows[-1])
        row_ok = max(rows[-1]) < (1 << bits) and sum(rows[-1]) < (1 << 64)
        if dead or not (0 <= s < V and row_ok):
            dead = True
        elif not st.accept(s):
            rows[-1] = [0] * V
            dead = True
    if extra_row:
        rows.append(st.row())
    return pmf_rows(rows, bits, V), st


def walk_batch(V, order, W, sym, bits=32, states=None):
    """sym [T, B] -> (rows [T, B, V], [Stream] * B); ``states``: the streams to continue (copied)."""
    T, B = sym.shape
    rows = np.zeros((T, B, V), dtype=np.uint32 if bits == 32 else np.uint64)
    out = []
    for b in range(B):
        c, p = (None, ()) if states is None else (states[b].counts, states[b].past)
        rows[:, b], st = walk(V, order, W, sym[:, b].tolist(), bits, c, p)
        out.append(st)
    return rows, out


def draw(rng, V, T, B=1):
    """Symbols [T, B]: the symbol two back with probability 1/2, else uniform -- contexts recur."""
    sym = rng.integers(0, V, size=(T, B)).astype(np.int32)
    rep = rng.random((T, B)) < 0.5
    for t in range(2, T):
        sym[t] = np.where(rep[t], sym[t - 2], sym[t])
    return sym


def always_fudged_share(case):
    """Share of a fixture's steps whose row has T > 2 w0 minp, w0 = 2^(prec-1)."""
    st = Stream(case["V"], case["order"], case["weights"])
    n = 0
    for s in case["syms"]:
        r = st.row()
        n += sum(r) > (2 << (case["prec"] - 1)) * min(r)
        st.accept(s)
    return n / len(case["syms"])
