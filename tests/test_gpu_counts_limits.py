"""Adaptive n-gram count models at their arithmetic limits (include/lac.h lac_count_*): counts
loaded with set_count_state that are full or nearly so, u64 rows with entries of 2^52 and more and
totals up to 2^64 - 1 and at 2^64, the u32 entry at 2^32 - 1, two defects in one step, and the
``trace`` argument of encode_counts.

Every expected value comes from outside the count-model path: the C oracle on the rows of the
host restatement (tests/counts.py, which knows the full-count rule), built from exact Python
integers, and -- for registers, plane words and traces -- the pmf path (encode / decode) of this
library on those rows.  What a job is meant to reach (the step a count is full at, the class of a
wide row, the share of fudged steps) is asserted on the host before the device is touched.
"""
import functools

import numpy as np
import pytest

import counts as K
import errors as E
from test_gpu_counts import DEC_FIELDS, DEV, ENC_FIELDS, Model, _coder, _comp_job, dev_i32, same_fields, same_state, verdict

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
FULL = K.COUNT_FULL
SENTINEL = -7


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


# ------------------------------------------------------------------ host side
class Unsaturated(K.Stream):
    """The walk with the full-count rule ignored: counts as 64-bit integers, never refused."""

    def __init__(self, V, order, W, counts=None, past=()):
        super().__init__(V, order, W, None, past)
        if counts is not None:
            self.counts = np.array(counts, dtype=np.uint64)
        else:
            self.counts = self.counts.astype(np.uint64)

    def accept(self, s):
        for i in range(len(self.past)):
            self.counts[self._at(i, s)] += np.uint64(1)
        self.past = (self.past + (int(s),))[-self.order:]
        return True


def valid_past(row, V):
    """A stored past's trailing run of symbols (include/lac.h lac_count_set_state)."""
    out = []
    for s in reversed([int(x) for x in row]):
        if not 0 <= s < V:
            break
        out.append(s)
    return tuple(reversed(out))


def streams_of(m, counts, past, cls=K.Stream):
    return [cls(m.V, m.order, m.W, counts[b], valid_past(past[b], m.V)) for b in range(len(counts))]


def int_rows(st, syms):
    """The rows (Python integers) of one stream's steps; a refused step or a bad symbol ends it."""
    rows = []
    for s in syms:
        rows.append(st.row())
        if not (0 <= s < st.V and sum(rows[-1]) < 1 << 64 and st.accept(s)):
            break
    return rows


def row_fits(row, bits):
    return max(row) < 1 << bits and sum(row) < 1 << 64


def pmf_array(rows_by_stream, bits, V):
    """[stream][step] rows of Python integers -> [T, B, V] in the entries' type."""
    return np.stack([K.pmf_rows(r, bits, V) for r in rows_by_stream], axis=1)


def encode_both(c, ref, m, sym, rows, counts, past, trace=None, rtrace=None):
    c.reset()
    c.set_count_state(counts, past)
    c.encode_counts(dev_i32(sym), trace=trace)
    ref.reset()
    ref.encode(E.dev_pmf(rows, DEV), dev_i32(sym), trace=rtrace)


def frozen_like_the_pmf_path(c, ref, v, what):
    rc, err, es = c.status()
    assert np.array_equal(err, v["code"]) and np.array_equal(es, v["step"]) and rc == E.first_code(v["code"]), (what, err, es)
    a, b = c.checkpoint(), ref.checkpoint()
    same_fields(a["state"], b["state"], ENC_FIELDS, what)
    assert np.array_equal(E.written(a), E.written(b)), what
    return a


# ------------------------------------------------------------------ saturation
SAT_V, SAT_S, SAT_A, SAT_O = 7, 3, 5, 1                           # the symbol whose count is full, its context, another
SAT_REST = (1, 2, 4, 5, 6)                                        # neither that symbol nor symbol 0
SAT_FORMS = ((32, (0, 5), 0), (32, (3, 0), 1), (64, (1, 1), 0), (64, (1, 1), 1))
SAT_IDS = [f"u{b}w{w[0]}_{w[1]}s{s}" for b, w, s in SAT_FORMS]


@functools.lru_cache(maxsize=None)
def _sat_job(bits, W, sec, prec):
    """Order 2, V = 7, five streams of 24 steps; the preset counts sit in section `sec` (for u32 the
    section whose weight is 0: the row does not show the count), in the row of context (5,) * sec:
      0  symbol 3's count 0xfffffffd; with history present 3 is coded there three times -- the third
         is refused, at step 4 + 2 sec
      1  symbol 3's count 0xffffffff, a full preset past: 3 at step 0 is refused
      2  the same counts and past, other symbols: clean
      3  symbol 0's count 0xffffffff; the symbol V at step 2, under that context: LAC_E_SYMBOL_RANGE
      4  no presets, clean
    -> model, sym, counts, past, the streams they start from, the failing steps of streams 0, 1, 3."""
    m = Model(SAT_V, 2, list(W), prec, bits)
    rng = np.random.default_rng(100 * bits + 10 * sec + prec)
    T, B = 24, 5
    y = K.layout(m.V, m.order)
    ctx = (SAT_A,) * sec
    slot = lambda s: y["off"][sec] + K.row_index(ctx, m.V) * y["Vc"] + s   # noqa: E731
    sym = rng.choice(SAT_REST, size=(T, B)).astype(np.int32)
    sym[:, 4] = K.draw(rng, m.V, T)[:, 0]
    counts = np.zeros((B, y["stride"]), dtype=np.uint32)
    past = np.full((B, m.order), -1, dtype=np.int32)
    past[:4] = (SAT_O, SAT_A)                                     # (ends in the context)
    three = ((list(ctx) + [SAT_S]) * 3)[sec:]
    sym[:2 + len(three), 0] = [SAT_O, SAT_A] + three
    counts[0, slot(SAT_S)] = 0xfffffffd
    counts[1, slot(SAT_S)] = counts[2, slot(SAT_S)] = FULL
    sym[0, 1] = SAT_S
    counts[3, slot(0)] = FULL
    sym[:3, 3] = [SAT_O, SAT_A, m.V]
    return m, sym, counts, past, slot, (1 + len(three), 0, 2)


def _sat_classes(m, sym, counts, past, slot, steps, code3):
    """The host assertions of a saturation job; -> (restated rows, streams, verdict)."""
    rows, sts = m.walk(sym, streams_of(m, counts, past))
    v = verdict(m, rows, sym)
    assert v["code"].tolist() == [E.LAC_E_TABLE, E.LAC_E_TABLE, 0, code3, 0], v["code"]
    assert v["step"].tolist() == [steps[0], steps[1], -1, steps[2] if code3 else -1, -1], v["step"]
    # the refused steps' rows are good rows: the count alone refuses them
    for b in (0, 1):
        t = steps[b]
        true_row = int_rows(streams_of(m, counts, past, Unsaturated)[b], sym[:t + 1, b].tolist())[t]
        assert row_fits(true_row, m.bits) and not rows[t, b].any(), (b, true_row)
        assert int(sts[b].counts[slot(SAT_S)]) == FULL           # two accepts went through (stream 0); none (stream 1)
    assert int(sts[0].counts.astype(np.uint64).sum()) > int(counts[0].astype(np.uint64).sum())
    assert np.array_equal(sts[1].counts, counts[1]) and sts[1].past_row() == past[1].tolist()
    assert int(sts[3].counts[slot(0)]) == FULL
    return rows, sts, v


def _fudged_at(m, row):
    """Does this row fudge at every width a coder has (w <= 2^prec), at none (w > 2^(prec-1)), or
    at some?"""
    T, mn = sum(row), min(row)
    if T > (mn << m.prec):
        return "always"
    return "never" if T <= (mn << (m.prec - 1)) else "some"


@pytest.mark.parametrize("prec", (48, 16))
@pytest.mark.parametrize("bits,W,sec", SAT_FORMS, ids=SAT_IDS)
def test_saturation_encode(bits, W, sec, prec):
    m, sym, counts, past, slot, steps = _sat_job(bits, W, sec, prec)
    rows, sts, v = _sat_classes(m, sym, counts, past, slot, steps, E.LAC_E_SYMBOL_RANGE)
    B = sym.shape[1]
    sym2 = np.concatenate([sym, sym[:3]])                         # the job and three more steps: the sticky call
    rows2, sts2 = m.walk(sym2, streams_of(m, counts, past))
    v2 = verdict(m, rows2, sym2)
    assert np.array_equal(v2["code"], v["code"]) and np.array_equal(v2["step"], v["step"])
    for b in (0, 1, 3):
        assert np.array_equal(sts2[b].counts, sts[b].counts) and sts2[b].past == sts[b].past
    with _coder(m, B) as c, _coder(m, B, load=False) as ref:
        encode_both(c, ref, m, sym, rows, counts, past)
        a = frozen_like_the_pmf_path(c, ref, v, "frozen")
        same_state(c, sts, "counts and past as of the failing step")
        c.encode_counts(dev_i32(sym[:3]))                         # sticky: more steps change nothing of a failed stream
        rc, err, es = c.status()
        assert np.array_equal(err, v["code"]) and np.array_equal(es, v["step"])
        a2 = c.checkpoint()
        for b in (0, 1, 3):
            assert a2["state"][b].tobytes() == a["state"][b].tobytes(), b
            assert np.array_equal(E.written(a2)[:, b], E.written(a)[:, b]), b
        same_state(c, sts2, "sticky")
        c.finish()
        got, n = E.stream_bytes(c)
        for b in range(B):                                        # the neighbours' bytes are the oracle's
            if v2["code"][b]:
                assert n[b] == 0, b
            else:
                assert got[b] == v2["data"][b] and n[b] == v2["nbits"][b], b


@pytest.mark.parametrize("prec", (48, 16))
@pytest.mark.parametrize("bits,W,sec", SAT_FORMS, ids=SAT_IDS)
def test_saturation_decode(bits, W, sec, prec):
    """The count encoder cannot produce bits past a refused step: the pmf path of a second context
    encodes the rows of the walk with the rule ignored, decode_counts reads those bits with the
    preset counts."""
    m, sym, counts, past, slot, steps = _sat_job(bits, W, sec, prec)
    sym = sym.copy()
    sym[2, 3] = SAT_O                                             # a decoder returns no symbol >= V: stream 3 is clean here
    T, B = sym.shape
    rows, sts, v = _sat_classes(m, sym, counts, past, slot, steps, 0)
    free = streams_of(m, counts, past, Unsaturated)
    free_rows = [int_rows(free[b], sym[:, b].tolist()) for b in range(B)]
    assert all(len(r) == T and all(row_fits(x, bits) for x in r) for r in free_rows)
    for b in (0, 1):                                              # the full slot is passed once, and never met again
        assert int(free[b].counts[slot(SAT_S)]) == 1 << 32
    # the refused step: fudged at every width in u64 at prec 16 (the counts are read back from
    # memory there), at none at prec 48
    kind = [_fudged_at(m, free_rows[b][steps[b]]) for b in (0, 1)]
    assert kind == (["always"] * 2 if (bits, prec) == (64, 16) else ["never"] * 2), kind
    if (bits, prec, sec) == (64, 16, 0):                          # section 0 is in every row: every step fudges
        share = np.mean([_fudged_at(m, r) == "always" for b in (0, 1, 2, 3) for r in free_rows[b]])
        assert share == 1.0, share
    free_pmf = pmf_array(free_rows, bits, m.V)
    vf = verdict(m, free_pmf, sym)
    assert not vf["code"].any()
    with _coder(m, B) as c, _coder(m, B, load=False) as ref:
        ref.encode_job(E.dev_pmf(free_pmf, DEV), dev_i32(sym))
        got, n = E.stream_bytes(ref)
        assert got == vf["data"] and np.array_equal(n, vf["nbits"])
        bits_t, nb = ref.bits_tensor(), ref.nbits_tensor().clone()
        c.decode_open(bits_t, nb)
        c.set_count_state(counts, past)
        out = c.decode_counts(T).cpu().numpy()
        rc, err, es = c.status()
        assert np.array_equal(err, v["code"]) and np.array_equal(es, v["step"]) and rc == E.LAC_E_TABLE, (err, es)
        for b in range(B):
            k = T if v["code"][b] == 0 else int(v["step"][b])
            assert np.array_equal(out[:k, b], sym[:k, b]) and (out[k:, b] == -1).all(), (b, out[:, b])
        ref.decode_open(bits_t, nb)
        want = ref.decode(E.dev_pmf(rows, DEV)).cpu().numpy()
        assert np.array_equal(out, want)
        same_fields(E.dec_state(c), E.dec_state(ref), DEC_FIELDS, "decoder")
        same_state(c, sts, "counts and past frozen")


# ------------------------------------------------------------------ wide u64 rows
WIDE_V, WIDE_M = 6, (1 << 30) - 1
WIDE_PAST = (1, 2, 3, 4)


@functools.lru_cache(maxsize=None)
def _wide_job(prec):
    """V = 6, order 4, W = [1, 2^30 - 1, 2^30 - 1, 2^30 - 1], every past (1, 2, 3, 4), 20 steps:
      a  every count of sections 1..3 below 2^24: entries >= 2^52, totals < 2^62
      b  every count of sections 1..3 in [0.12, 0.2) 2^32: totals in [2^63, 2^64)
      c  b's kind of counts, but the 18 counts of the step-0 contexts hold N = (2^64 - V) // (2^30 - 1)
         between them and symbol 0 of section 0 holds R - 1: the total of step 0 is 2^64 - 1
      d  c with R there: 2^64"""
    V, M = WIDE_V, WIDE_M
    m = Model(V, 4, [1, M, M, M], prec, 64)
    rng = np.random.default_rng(64 + prec)
    T, B = 20, 4
    y = K.layout(V, 4)

    def fill(lo, hi):
        cs = np.zeros(y["stride"], dtype=np.uint32)
        for i in range(1, 4):
            for r in range(V ** i):
                at = y["off"][i] + r * y["Vc"]
                cs[at:at + V] = rng.integers(lo, hi, size=V)
        cs[:V] = rng.integers(0, 100, size=V)
        return cs
    counts = np.stack([fill(0, 1 << 24), fill(int(0.12 * 2 ** 32), int(0.2 * 2 ** 32)),
                       fill(int(0.12 * 2 ** 32), int(0.2 * 2 ** 32)), np.zeros(y["stride"], dtype=np.uint32)])
    N, R = divmod((1 << 64) - V, M)
    assert R >= 1
    each, more = divmod(N, 18)
    assert each + 1 <= (1 << 32) - 2
    k = 0
    for i in range(1, 4):
        at = y["off"][i] + K.row_index(WIDE_PAST[4 - i:], V) * y["Vc"]
        for s in range(V):
            counts[2, at + s] = each + (1 if k < more else 0)
            k += 1
    counts[2, :V] = 0
    counts[2, 0] = R - 1
    counts[3] = counts[2]
    counts[3, 0] = R
    past = np.tile(np.array(WIDE_PAST, dtype=np.int32), (B, 1))
    sym = K.draw(rng, V, T, B)
    sym[:, 2] = rng.choice((0, 1, 2, 3, 5), size=T)               # c never comes back to a context that holds a 4
    sym[0, 2] = 5
    sym[:, 3] = sym[:, 2]
    return m, sym, counts, past, (N, R)


def _wide_classes(m, sym, counts, past):
    """-> per stream the rows as Python integers, with the classes asserted."""
    T, B = sym.shape
    sts = streams_of(m, counts, past)
    rows = [int_rows(sts[b], sym[:, b].tolist()) for b in range(B)]
    assert [len(r) for r in rows] == [T, T, T, 1]
    assert all(max(r) >= 1 << 52 and sum(r) < 1 << 62 for r in rows[0])
    assert all(1 << 63 <= sum(r) < 1 << 64 for r in rows[1])
    assert sum(rows[2][0]) == (1 << 64) - 1 and all(sum(r) < 1 << 64 for r in rows[2])
    assert sum(rows[3][0]) == 1 << 64 and max(rows[3][0]) < 1 << 64
    assert sum(1 for r in rows[2] if sum(r) >= 1 << 63) == T      # (c stays on wide rows throughout)
    for b in range(3):                                            # counts the job itself wrote are read again
        fixed = streams_of(m, counts, past)[b]
        seen = False
        for t in range(T):
            seen = seen or fixed.row() != rows[b][t]
            fixed.past = (fixed.past + (int(sym[t, b]),))[-m.order:]
        assert seen, b
    return rows


@pytest.mark.parametrize("prec", (60, 48))
def test_wide_u64_rows(prec):
    m, sym, counts, past, _ = _wide_job(prec)
    T, B = sym.shape
    _wide_classes(m, sym, counts, past)
    rows, sts = m.walk(sym, streams_of(m, counts, past))
    v = verdict(m, rows, sym)
    assert v["code"].tolist() == [0, 0, 0, E.LAC_E_TABLE] and v["step"].tolist() == [-1, -1, -1, 0]
    assert np.array_equal(sts[3].counts, counts[3]) and sts[3].past == WIDE_PAST
    with _coder(m, B) as c, _coder(m, B, load=False) as ref:
        encode_both(c, ref, m, sym, rows, counts, past)
        frozen_like_the_pmf_path(c, ref, v, "encoder")
        same_state(c, sts, "after encode")
        c.finish()
        got, n = E.stream_bytes(c)
        assert got[:3] == v["data"][:3] and n.tolist() == v["nbits"][:3].tolist() + [0]
        bits_t, nb = c.bits_tensor(), c.nbits_tensor().clone()
        c.decode_open(bits_t, nb)
        c.set_count_state(counts, past)
        out = c.decode_counts(T).cpu().numpy()
        rc, err, es = c.status()
        assert np.array_equal(err, v["code"]) and np.array_equal(es, v["step"]), (err, es)
        assert np.array_equal(out[:, :3], sym[:, :3]) and (out[:, 3] == -1).all()
        ref.decode_open(bits_t, nb)
        assert np.array_equal(ref.decode(E.dev_pmf(rows, DEV)).cpu().numpy(), out)
        same_fields(E.dec_state(c), E.dec_state(ref), DEC_FIELDS, "decoder")
        same_state(c, sts, "after decode")


# ------------------------------------------------------------------ the u32 edge
def _edge_job():
    """V = 4, order 1, W = [1], symbol 2's count 0xfffffffe: the entry 2^32 - 1 codes, the accept
    fills the count, the next row's entry is 2^32.  Stream 1 codes other symbols under that row."""
    m = Model(4, 1, [1], 48, 32)
    counts = np.zeros((2, K.layout(4, 1)["stride"]), dtype=np.uint32)
    counts[:, 2] = 0xfffffffe
    past = np.array([[1], [1]], dtype=np.int32)
    sym = np.array([[2, 1, 0, 3, 1, 0, 3, 3, 1, 0], [0, 1, 3, 3, 0, 1, 0, 3, 1, 1]], dtype=np.int32).T.copy()
    return m, sym, counts, past


def test_u32_entry_at_2_32_minus_1():
    m, sym, counts, past = _edge_job()
    T = len(sym)
    first = streams_of(m, counts, past)[0].row()
    assert first[2] == (1 << 32) - 1 and sum(first) > 1 << 32     # the entry fits, the total passes 2^32: legal
    rows, sts = m.walk(sym, streams_of(m, counts, past))
    v = verdict(m, rows, sym)
    assert v["code"].tolist() == [E.LAC_E_TABLE, 0] and v["step"].tolist() == [1, -1]
    assert int(sts[0].counts[2]) == FULL and int(sts[1].counts[2]) == 0xfffffffe
    m64 = Model(4, 1, [1], 48, 64)                                # (for the decode below: u64 entries code the whole job)
    rows64, _ = m64.walk(sym, streams_of(m64, counts, past))
    v64 = verdict(m64, rows64, sym)
    assert not v64["code"].any() and np.array_equal(rows64[0], rows[0])
    with _coder(m, 2) as c, _coder(m, 2, load=False) as ref:
        encode_both(c, ref, m, sym, rows, counts, past)
        frozen_like_the_pmf_path(c, ref, v, "encoder")
        same_state(c, sts, "after encode")
        c.finish()
        got, n = E.stream_bytes(c)
        assert got[1] == v["data"][1] and n.tolist() == [0, v["nbits"][1]]
    # decode: the u32 context reads the u64 job's bits and meets the bad row
    buf =np.zeros((2, 128), dtype=np.uint8)
    for b, d in enumerate(v64["data"]):
        buf[b, :len(d)] = np.frombuffer(d, dtype=np.uint8)
    with _coder(m, 2) as c:
        c.decode_open(torch.from_numpy(buf).to(DEV), torch.from_numpy(v64["nbits"].copy()).to(DEV))
        c.set_count_state(counts, past)
        out = c.decode_counts(T).cpu().numpy()
        rc, err, es = c.status()
        assert err.tolist() == [E.LAC_E_TABLE, 0] and es.tolist() == [1, -1]
        assert out[:, 0].tolist() == [2] + [-1] * (T - 1) and np.array_equal(out[:, 1], sym[:, 1])
        same_state(c, sts, "after decode")


# ------------------------------------------------------------------ two defects in one step
def _bad_row_jobs():
    """(model, counts, past) whose first row is bad: a u32 entry of 2^32, and twin d's total 2^64."""
    m, _, counts, past = _edge_job()
    counts = counts.copy()
    counts[:, 2] = FULL
    assert streams_of(m, counts, past)[0].row()[2] == 1 << 32
    mw, _, cw, pw, _ = _wide_job(48)
    return (m, counts, past), (mw, np.stack([cw[3], cw[3]]), pw[:2])


@pytest.mark.parametrize("which", (0, 1), ids=("u32_entry", "total_2_64"))
def test_precedence_at_one_step(which):
    """include/lac.h: an encode step tests the symbol's range before the table; a decode step the
    table before the registers."""
    m, counts, past = _bad_row_jobs()[which]
    sym = np.array([[m.V, 1], [0, 1]], dtype=np.int32)            # stream 0: a symbol out of range on the bad row
    rows, sts = m.walk(sym, streams_of(m, counts, past))
    assert not rows.any()                                         # (the restatement: the bad row, nothing moves)
    code, step = np.array([E.LAC_E_SYMBOL_RANGE, E.LAC_E_TABLE], dtype=np.int32), np.array([0, 0])
    with _coder(m, 2) as c, _coder(m, 2, load=False) as ref:
        encode_both(c, ref, m, sym, rows, counts, past)
        frozen_like_the_pmf_path(c, ref, {"code": code, "step": step}, "encode")
        same_state(c, sts, "encode")
        c.finish()
        c.decode_open(torch.zeros((2, 64), dtype=torch.uint8, device=DEV), torch.full((2,), 64, dtype=torch.int64, device=DEV))
        c.set_count_state(counts, past)
        st = E.dec_state(c)
        st["x"][0], st["x"][1] = st["l"][0] - 1, st["h"][1] + 1   # registers out of range on the bad row
        E.set_dec_state(c, st)
        out = c.decode_counts(2).cpu().numpy()
        rc, err, es = c.status()
        assert err.tolist() == [E.LAC_E_TABLE] * 2 and es.tolist() == [0, 0] and (out == -1).all(), (err, es)
        after = E.dec_state(c)
        for f in ("l", "h", "x", "pos", "nsym"):
            assert np.array_equal(after[f], st[f]), f
        same_state(c, sts, "decode")


# ------------------------------------------------------------------ traces
def _symbol_error_job():
    m, sym, _, _, _ = _comp_job()
    sym = sym.copy()
    for b, (t, s) in {0: (0, m.V), 1: (63, -1), 3: (64, 2 ** 31 - 1)}.items():
        sym[t, b] = s
    return m, sym, None, None, [E.LAC_E_SYMBOL_RANGE, E.LAC_E_SYMBOL_RANGE, 0, E.LAC_E_SYMBOL_RANGE, 0], [0, 63, -1, 64, -1]


@pytest.mark.parametrize("job", ("composition", "saturating", "bad_symbol"))
def test_traces_are_the_pmf_paths(job):
    """encode_counts(sym, trace=...) writes {E, k} of every coded step as encode does on the restated
    rows; the failing step's entry and every later one is not written."""
    if job == "composition":
        m, sym, _, _, _ = _comp_job()
        counts = past = None
        code, step = [0] * 5, [-1] * 5
    elif job == "saturating":
        m, sym, counts, past, slot, steps = _sat_job(64, (1, 1), 0, 48)
        code = [E.LAC_E_TABLE, E.LAC_E_TABLE, 0, E.LAC_E_SYMBOL_RANGE, 0]
        step = [steps[0], steps[1], -1, steps[2], -1]
    else:
        m, sym, counts, past, code, step = _symbol_error_job()
    T, B = sym.shape
    start = None if counts is None else streams_of(m, counts, past)
    rows, _ = m.walk(sym, start)
    v = verdict(m, rows, sym)
    assert v["code"].tolist() == code and v["step"].tolist() == step
    with _coder(m, B) as c, _coder(m, B, load=False) as ref:
        tr = torch.full((T, B, 2), SENTINEL, dtype=torch.int64, device=DEV)
        rt = torch.full((T, B, 2), SENTINEL, dtype=torch.int64, device=DEV)
        encode_both(c, ref, m, sym, rows, counts, past, trace=tr, rtrace=rt)
        a = frozen_like_the_pmf_path(c, ref, v, job)
        t, r = tr.cpu().numpy(), rt.cpu().numpy()
        assert np.array_equal(t, r)
        for b in range(B):
            n = T if code[b] == 0 else step[b]
            assert (t[n:, b] == SENTINEL).all(), (job, b)
            assert (t[:n, b, 1] >= 0).all() and (t[:n, b, 1] <= 64).all(), (job, b)
            assert int(t[:n, b, 1].sum()) == int(a["state"]["L"][b]), (job, b)
