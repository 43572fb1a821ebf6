"""Adaptive n-gram count models on the device (include/lac.h lac_count_*, BatchCoder.load_counts /
encode_counts / decode_counts): the kernel keeps the counts, builds each step's row from them,
codes, and updates them.

Every expected value comes from outside the count-model path: the reference's own bits for its
Markov_up_to_n predictor (tests/golden/markov_cases.json), the C oracle on the rows of the dense
host restatement (tests/counts.py), and -- for registers, and for corrupt bits -- the pmf path
(encode / decode) of this library on those rows.
"""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import counts as K
import errors as E
from test_counts_host import CASES, IDS

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENC_FIELDS = ("l", "h", "L", "wa", "wc", "nsym", "err", "nflush", "err_step")
DEC_FIELDS = ("l", "h", "x", "pos", "nsym", "err", "det", "err_step", "ndet")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _lib():
    from lac_amd import _lib
    return _lib


class Model:
    def __init__(self, V, order, W, prec, bits):
        self.V, self.order, self.W, self.prec, self.bits = V, order, list(W), prec, bits

    def walk(self, sym, states=None):
        return K.walk_batch(self.V, self.order, self.W, sym, self.bits, states)


def _coder(m, B, cap=None, load=True):
    from lac_amd.batch import BatchCoder
    c = BatchCoder(m.V, B, prec=m.prec, pmf_bits=m.bits, capacity_bits=cap or 140 * (m.prec + 2) + 256, device=DEV)
    if load:
        c.load_counts(m.order, m.W)
    return c


def verdict(m, pmf, sym):
    return E.verdict(types.SimpleNamespace(B=sym.shape[1], prec=m.prec), pmf, sym)


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def same_fields(got, want, fields, what):
    for f in fields:
        assert np.array_equal(got[f], want[f]), (what, f, got[f], want[f])


def same_state(c, sts, what=""):
    """The coder's counts and past against the host walk's streams."""
    counts, past = c.count_state()
    for b, st in enumerate(sts):
        assert np.array_equal(counts[b], st.counts), (what, b, "counts")
        assert past[b].tolist() == st.past_row(), (what, b, past[b], st.past_row())


def job_equals_oracle(c, m, sym, what="", rows=None, sts=None):
    """encode_counts_job against the oracle on the restated rows, decode_counts of its own output,
    and the counts and past both leave."""
    if rows is None:
        rows, sts = m.walk(sym)
    v = verdict(m, rows, sym)
    assert not v["code"].any(), what
    c.encode_counts_job(dev_i32(sym))
    assert c.status()[0] == 0, what
    got, n = E.stream_bytes(c)
    assert np.array_equal(n, v["nbits"]) and got == v["data"], what
    same_state(c, sts, (what, "after encode"))
    c.decode_open()
    c.set_count_state()
    out = c.decode_counts(sym.shape[0]).cpu().numpy()
    assert c.status()[0] == 0 and np.array_equal(out, sym), what
    same_state(c, sts, (what, "after decode"))
    return got, n


# ------------------------------------------------------------------ the reference's fixtures
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixture(case):
    """encode_counts_job gives the reference's bytes and bit count, decode_counts its symbols, the
    final past and counts are the host walk's; with set_decode_stop the stream stops where the
    reference's run(bits, stop=0) stops, on the whole stream and on the truncated prefix."""
    m = Model(case["V"], case["order"], case["weights"], case["prec"], case["pmf_bits"])
    sym = np.array(case["syms"], dtype=np.int32)[:, None]
    N = len(sym)
    _, sts = m.walk(sym)
    with _coder(m, 1, cap=(N + 8) * (m.prec + 2) + 256) as c:
        c.encode_counts_job(dev_i32(sym))
        data, n = c.to_bytes()
        assert int(n[0]) == case["L"] and data[0].hex() == case["bytes"]
        same_state(c, sts, "encode")
        assert c.count_state()[1][0].tolist()[-len(case["past"]):] == case["past"]
        c.decode_open()
        c.set_count_state()
        assert np.array_equal(c.decode_counts(N).cpu().numpy(), sym)
        assert c.status()[0] == 0
        same_state(c, sts, "decode")
        bits = c.bits_tensor()
        c.set_decode_stop(True)
        for nbits, count in ((case["L"], case["decoded_count"]), (case["prefix_bits"], case["prefix_decoded_count"])):
            c.decode_open(bits, torch.tensor([nbits], dtype=torch.int64, device=DEV))
            c.set_count_state()
            out = c.decode_counts(case["decoded_count"] + 5).cpu().numpy()[:, 0]
            rc, err, step = c.status()
            assert rc == _lib().LAC_E_UNDETERMINED and step[0] == count, (nbits, rc, step)
            assert out[:count].tolist() == case["decoded"][:count] and (out[count:] == -1).all()
            assert c.determined().tolist() == [count]
            stop = m.walk(np.array(case["decoded"][:count], dtype=np.int32).reshape(-1, 1))[1]
            same_state(c, stop, "frozen at the stop")


# ------------------------------------------------------------------ boundaries
T_EDGES = (1, 63, 64, 65, 130)
EDGE_FORMS = (
    (2, 1, [1], 48, 32), (2, 4, [1, 3, 0, 9], 16, 32),                       # V = 2; order 4 with a zero weight
    (255, 2, [1, 300], 48, 32), (256, 2, [1, 300], 48, 32), (257, 2, [1, 300], 48, 32),   # one u32 vector per lane
    (127, 2, [1 << 29, 5], 60, 64), (128, 1, [1 << 29], 60, 64), (129, 2, [3, 1 << 29], 60, 64),   # and one u64
    (7, 3, [0, 4, 77], 24, 32), (64, 1, [5000], 16, 32), (40, 2, [900, 1], 16, 32),     # prec 16: rows that fudge
    (300, 2, [2000, 1], 16, 32), (9, 4, [1, 2, 3, 4], 24, 64),
)


@pytest.mark.parametrize("V,order,W,prec,bits", EDGE_FORMS, ids=[f"v{f[0]}o{f[1]}p{f[3]}u{f[4]}" for f in EDGE_FORMS])
def test_boundaries(V, order, W, prec, bits):
    """B = 5 (a stream in a second workgroup), jobs of 1 .. 130 steps (the 64-step blocks), rows
    just under / at / over one 64-vector pass.  Stream 0 repeats one symbol (the same counts are
    re-read the step after they are written), stream 1 alternates two."""
    rng = np.random.default_rng(1000 * V + prec + order)
    m, B = Model(V, order, W, prec, bits), 5
    sym = K.draw(rng, V, max(T_EDGES), B)
    sym[:, 0] = V - 1
    sym[:, 1] = np.arange(len(sym)) % 2
    rows, _ = m.walk(sym)
    if prec == 16 and max(W) >= 900:                              # (the fudging forms do fudge)
        w0 = 1 << (prec - 1)
        assert (rows.sum(axis=2, dtype=np.uint64) > 2 * w0 * rows.min(axis=2).astype(np.uint64)).mean() > 0.3
    with _coder(m, B) as c:
        for T in T_EDGES:
            job_equals_oracle(c, m, sym[:T], what=(V, order, T), rows=rows[:T], sts=m.walk(sym[:T])[1])


@pytest.mark.parametrize("B", (1, 64))
def test_stream_counts(B):
    rng = np.random.default_rng(B)
    m = Model(17, 2, [3, 7000], 16, 32)
    sym = K.draw(rng, m.V, 70, B)
    with _coder(m, B) as c:
        job_equals_oracle(c, m, sym, what=B)


@pytest.mark.parametrize("bits,prec", ((32, 48), (64, 60)))
def test_widest_vocabulary(bits, prec):
    """V = 4096, the limit: 16 passes of u32 entries, 32 of u64; the first and last entries coded."""
    rng = np.random.default_rng(4096 + bits)
    m, B, T = Model(4096, 1, [700], prec, bits), 2, 66
    sym = K.draw(rng, m.V, T, B)
    sym[::5, 0] = [4095, 0, 4094, 255, 256, 4095, 1023, 1024, 4095, 0, 2048, 4095, 3, 4092]
    with _coder(m, B) as c:
        job_equals_oracle(c, m, sym, what=("V=4096", bits))


def test_u32_rows_whose_total_passes_2_32():
    m, B, T = Model(64, 2, [1 << 29, 1 << 29], 48, 32), 5, 40
    sym = ((np.arange(T)[:, None] * 7 + np.arange(B)[None, :] * 3) % m.V).astype(np.int32)   # no symbol twice
    rows, sts = m.walk(sym)
    assert (rows.sum(axis=2, dtype=np.uint64)[20:] > 1 << 32).all() and rows.max() < 1 << 32
    with _coder(m, B) as c:
        job_equals_oracle(c, m, sym, what="wide", rows=rows, sts=sts)


# ------------------------------------------------------------------ registers are the pmf path's
@functools.lru_cache(maxsize=None)
def _comp_job():
    rng = np.random.default_rng(21)
    m, B, T = Model(50, 3, [2, 90, 4000], 48, 32), 5, 130
    sym = K.draw(rng, m.V, T, B)
    rows, sts = m.walk(sym)
    return m, sym, rows, sts, verdict(m, rows, sym)


@pytest.mark.parametrize("V,order,W,prec,bits", ((40, 2, [900, 1], 16, 32), (50, 3, [2, 90, 4000], 48, 32),
                                                  (31, 3, [1, 1 << 20, 1 << 29], 60, 64)))
def test_registers_equal_the_pmf_path(V, order, W, prec, bits):
    rng = np.random.default_rng(V)
    m, B, T = Model(V, order, W, prec, bits), 5, 100
    sym = K.draw(rng, V, T, B)
    rows, sts = m.walk(sym)
    pmf = E.dev_pmf(rows, DEV)
    with _coder(m, B) as c, _coder(m, B, load=False) as ref:
        c.reset()
        c.set_count_state()
        c.encode_counts(dev_i32(sym))
        ref.reset()
        ref.encode(pmf, dev_i32(sym))
        a, b = c.checkpoint(), ref.checkpoint()
        same_fields(a["state"], b["state"], ENC_FIELDS, "encoder")
        assert np.array_equal(E.written(a), E.written(b))
        c.finish()
        ref.finish()
        assert E.stream_bytes(c)[0] == E.stream_bytes(ref)[0]
        bits_t, nb = c.bits_tensor(), c.nbits_tensor().clone()
        c.decode_open(bits_t, nb)
        c.set_count_state()
        out = c.decode_counts(T).cpu().numpy()
        ref.decode_open(bits_t, nb)
        want = ref.decode(pmf).cpu().numpy()
        assert np.array_equal(out, want) and np.array_equal(out, sym)
        same_fields(E.dec_state(c), E.dec_state(ref), DEC_FIELDS, "decoder")


# ------------------------------------------------------------------ composition
def test_stream_lengths_over_split_calls():
    m, sym, rows, _, _ = _comp_job()
    T = sym.shape[0]
    lengths = np.array([0, 1, 64, T, 65])
    sts = [m.walk(sym[:k, b:b + 1])[1][0] for b, k in enumerate(lengths)]
    with _coder(m, 5) as c:
        c.set_stream_lengths(lengths)
        c.reset()
        c.set_count_state()
        for a, b in ((0, 1), (1, 65), (65, 130)):                   # calls of 1, 64 and 65 steps
            c.encode_counts(dev_i32(sym[a:b]))
        c.finish()
        got, n = E.stream_bytes(c)
        for b, k in enumerate(lengths):
            d, nb = E.oracle_prefix(rows[:, b], sym[:, b], int(k), m.prec)
            assert got[b] == d and n[b] == nb, b
        same_state(c, sts, "encode")
        c.decode_open()
        c.set_count_state()
        out = np.concatenate([c.decode_counts(b - a).cpu().numpy() for a, b in ((0, 1), (1, 65), (65, 130))])
        for b, k in enumerate(lengths):
            assert np.array_equal(out[:k, b], sym[:k, b]) and (out[k:, b] == -1).all(), b
        assert c.status()[0] == 0
        same_state(c, sts, "decode")


def test_three_calls_with_drains_equal_the_one_shot():
    m, sym, rows, sts, v = _comp_job()
    B = 5
    with _coder(m, B, cap=70 * (m.prec + 2) + 256) as c:
        slots = torch.zeros((B, 1024), dtype=torch.uint8, device=DEV)
        fill = torch.zeros(B, dtype=torch.int64, device=DEV)
        c.reset()
        c.set_count_state()
        for a, b in ((0, 1), (1, 65), (65, 130)):
            c.encode_counts(dev_i32(sym[a:b]))
            c.drain(slots, fill)
        c.finish()
        assert c.status()[0] == 0
        tail, n = E.stream_bytes(c)
        head, f = slots.cpu().numpy(), fill.cpu().numpy()
        for b in range(B):
            assert head[b, :f[b]].tobytes() + tail[b] == v["data"][b] and 8 * f[b] + n[b] == v["nbits"][b], b
        assert f.max() > 0
        same_state(c, sts)


def test_window_of_four_positions_with_refills():
    m, sym, rows, sts, v = _comp_job()
    B, T, N = 5, sym.shape[0], 4
    stride = (max(len(d) for d in v["data"]) + 7) // 8 * 8 + 8
    buf = np.zeros((B, stride), dtype=np.uint8)
    for b, d in enumerate(v["data"]):
        buf[b, :len(d)] = np.frombuffer(d, dtype=np.uint8)
    bits, nb = torch.from_numpy(buf).to(DEV), torch.from_numpy(v["nbits"].copy()).to(DEV)
    with _coder(m, B, cap=N * (m.prec + 2) + 256) as c:
        c.decode_open_window(bits, nb)
        c.set_count_state()
        out = torch.empty((T, B), dtype=torch.int32, device=DEV)
        for t in range(0, T, N):
            c.decode_counts(min(N, T - t), out=out[t:t + N])
            c.refill()
        c.refill()
        assert c.status()[0] == 0 and np.array_equal(out.cpu().numpy(), sym)
        same_state(c, sts)


def test_checkpoint_continues_in_a_fresh_context():
    m, sym, rows, sts, v = _comp_job()
    B, half = 5, 65
    with _coder(m, B) as c, _coder(m, B) as d:
        c.reset()
        c.set_count_state()
        c.encode_counts(dev_i32(sym[:half]))
        ck = c.checkpoint()
        counts, past = c.count_state()
        same_state(c, m.walk(sym[:half])[1], "first half")
        d.restore(ck)
        d.set_count_state(counts, past)
        d.encode_counts(dev_i32(sym[half:]))
        d.finish()
        got, n = E.stream_bytes(d)
        assert got == v["data"] and np.array_equal(n, v["nbits"])
        same_state(d, sts, "second half")
        # the same through device tensors (lac_count_get_state -> lac_count_set_state)
        cd, pd = c.count_state(device=True)
        d.restore(ck)
        d.set_count_state(cd, pd)
        d.encode_counts(dev_i32(sym[half:]))
        d.finish()
        assert E.stream_bytes(d)[0] == v["data"]


def test_valid_history_is_the_trailing_run():
    m = Model(9, 3, [1, 20, 300], 24, 32)
    rng = np.random.default_rng(5)
    sym = K.draw(rng, m.V, 30, 3)
    past = np.array([[4, -1, 2], [7, 9, 3], [1, 2, 3]], dtype=np.int32)      # a hole; a symbol out of range; whole
    start = [K.Stream(m.V, m.order, m.W, past=p) for p in ((2,), (3,), (1, 2, 3))]
    rows, sts = m.walk(sym, start)
    v = verdict(m, rows, sym)
    with _coder(m, 3) as c:
        c.reset()
        c.set_count_state(None, past)
        c.encode_counts(dev_i32(sym))
        c.finish()
        got, n = E.stream_bytes(c)
        assert got == v["data"] and np.array_equal(n, v["nbits"])
        same_state(c, sts)


# ------------------------------------------------------------------ errors
def test_symbol_errors_freeze_the_stream_at_their_step():
    """A symbol >= V or < 0 at the first, last and next-to-last step of a 64-step block."""
    m, sym, _, _, _ = _comp_job()
    sym = sym.copy()
    B, T = sym.shape[1], sym.shape[0]
    bad = {0: (0, m.V), 1: (63, -1), 2: (62, 2 ** 31 - 1), 3: (64, -2 ** 31)}
    for b, (t, s) in bad.items():
        sym[t, b] = s
    rows, sts = m.walk(sym)
    v = verdict(m, rows, sym)
    code = np.array([E.LAC_E_SYMBOL_RANGE] * 4 + [0], dtype=np.int32)
    step = np.array([0, 63, 62, 64, -1], dtype=np.int64)
    assert np.array_equal(v["code"], code) and np.array_equal(v["step"], step)      # the yardstick itself
    with _coder(m, B) as c, _coder(m, B, load=False) as ref:
        c.reset()
        c.set_count_state()
        c.encode_counts(dev_i32(sym))
        ref.reset()
        ref.encode(E.dev_pmf(rows, DEV), dev_i32(sym))
        rc, err, es = c.status()
        assert np.array_equal(err, code) and np.array_equal(es, step) and rc == E.first_code(code)
        a, b = c.checkpoint(), ref.checkpoint()
        same_fields(a["state"], b["state"], ENC_FIELDS, "frozen")
        assert np.array_equal(E.written(a), E.written(b))
        same_state(c, sts, "counts and past as of the failing step")
        c.encode_counts(dev_i32(sym[:3]))                         # sticky: more steps change nothing of a failed stream
        assert np.array_equal(c.status()[1][:4], code[:4])
        same_state(c, sts[:4], "sticky")
        c.finish()
        got, n = E.stream_bytes(c)
        assert n[:4].tolist() == [0, 0, 0, 0]
        c.encode_counts_job(dev_i32(sym[:, 4:5].repeat(B, axis=1)))   # a reset clears it
        assert c.status()[0] == 0 and E.stream_bytes(c)[0][0] == v["data"][4]


def test_capacity_overflow():
    m, sym, rows, _, _ = _comp_job()
    B = sym.shape[1]
    cap = 5 * (m.prec + 2)
    with _coder(m, B, cap=cap) as c, _coder(m, B, cap=cap, load=False) as ref:
        c.reset()
        c.set_count_state()
        c.encode_counts(dev_i32(sym))
        ref.reset()
        ref.encode(E.dev_pmf(rows, DEV), dev_i32(sym))
        rc, err, es = c.status()
        rc2, err2, es2 = ref.status()
        assert (err == E.LAC_E_CAPACITY).all() and np.array_equal(err, err2) and np.array_equal(es, es2) and rc == rc2
        same_fields(c.checkpoint()["state"], ref.checkpoint()["state"], ENC_FIELDS, "frozen")
        sts = [m.walk(sym[:es[b], b:b + 1])[1][0] for b in range(B)]
        same_state(c, sts, "as of the failing step")


def test_entry_past_2_32_in_a_u32_context():
    """1 + 2^29 c does not fit u32 from c = 8: LAC_E_TABLE at the step the restatement predicts;
    the u64 context codes the same job."""
    m = Model(4, 1, [1 << 29], 24, 32)
    sym = np.ones((20, 2), dtype=np.int32)
    sym[:, 1] = np.arange(20) % 4                                  # stream 1 never gets there
    rows, sts = m.walk(sym)
    v = verdict(m, rows, sym)
    assert v["code"].tolist() == [E.LAC_E_TABLE, 0] and v["step"].tolist() == [9, -1]
    with _coder(m, 2) as c:
        c.reset()
        c.set_count_state()
        c.encode_counts(dev_i32(sym))
        rc, err, es = c.status()
        assert err.tolist() == [E.LAC_E_TABLE, 0] and es.tolist() == [9, -1] and rc == E.LAC_E_TABLE
        same_state(c, sts)
        c.finish()
        got, n = E.stream_bytes(c)
        assert got[1] == v["data"][1] and n.tolist() == [0, v["nbits"][1]]
        # decode: stream 1's bytes in both slots; stream 0 now walks stream 1's symbols, cleanly
        bits = c.bits_tensor()
        bits[0] = bits[1]
        nb = torch.full((2,), int(n[1]), dtype=torch.int64, device=DEV)
        c.decode_open(bits, nb)
        c.set_count_state()
        out = c.decode_counts(20).cpu().numpy()
        assert c.status()[0] == 0 and np.array_equal(out[:, 0], sym[:, 1]) and np.array_equal(out[:, 1], sym[:, 1])
    m64 = Model(4, 1, [1 << 29], 24, 64)
    with _coder(m64, 2) as c:
        job_equals_oracle(c, m64, sym, what="u64")
    # the decoder meets the bad row too: the u64 job's bytes, decoded in a u32 context
    rows64, _ = m64.walk(sym)
    v64 = verdict(m64, rows64, sym)
    buf = np.zeros((2, 64), dtype=np.uint8)
    for b, d in enumerate(v64["data"]):
        buf[b, :len(d)] = np.frombuffer(d, dtype=np.uint8)
    with _coder(m, 2) as c:
        c.decode_open(torch.from_numpy(buf).to(DEV), torch.from_numpy(v64["nbits"].copy()).to(DEV))
        c.set_count_state()
        out = c.decode_counts(20).cpu().numpy()
        rc, err, es = c.status()
        assert err.tolist() == [E.LAC_E_TABLE, 0] and es.tolist() == [9, -1]
        assert np.array_equal(out[:9, 0], sym[:9, 0]) and (out[9:, 0] == -1).all() and np.array_equal(out[:, 1], sym[:, 1])
        same_state(c, sts, "decode")


@pytest.mark.parametrize("V,order,W,prec,bits", ((40, 2, [900, 1], 16, 32), (50, 2, [3, 200], 48, 32),
                                                  (129, 2, [1 << 29, 3], 48, 64)))
def test_corrupt_bits_equal_the_per_position_loop(V, order, W, prec, bits):
    """One flipped bit per stream: symbols, -1 fills, codes, steps and registers are those of the
    per-position pmf decode with the rows rebuilt on the host from the symbols read back."""
    rng = np.random.default_rng(V + prec)
    m, B, T = Model(V, order, W, prec, bits), 5, 100
    sym = K.draw(rng, V, T, B)
    with _coder(m, B) as c, _coder(m, B, load=False) as ref:
        c.encode_counts_job(dev_i32(sym))
        assert c.status()[0] == 0
        bits_t, nb = c.bits_tensor(), c.nbits_tensor().clone()
        n = nb.cpu().numpy()
        for b in range(1, 4):                                     # streams 1..3: one flipped bit each
            at = int(rng.integers(8, int(n[b]) // 2))
            bits_t[b, at // 8] ^= 0x80 >> (at % 8)
        c.decode_open(bits_t, nb)
        c.set_count_state()
        out = c.decode_counts(T).cpu().numpy()
        rc, err, es = c.status()
        assert all(int(e) in _lib().STATUS_NAMES for e in err)    # the status is a code
        ref.decode_open(bits_t, nb)
        sts = [K.Stream(V, order, W) for _ in range(B)]
        want = np.zeros((T, B), dtype=np.int32)
        for t in range(T):
            rows = K.pmf_rows([st.row() for st in sts], bits)[None]
            want[t] = ref.decode(E.dev_pmf(rows, DEV)).cpu().numpy()[0]
            for b, st in enumerate(sts):
                if want[t, b] >= 0:
                    st.accept(want[t, b])
        assert np.array_equal(out, want)
        rc2, err2, es2 = ref.status()
        assert rc == rc2 and np.array_equal(err, err2) and np.array_equal(es, es2)
        same_fields(E.dec_state(c), E.dec_state(ref), DEC_FIELDS, "registers")
        assert np.array_equal(out[:, 0], sym[:, 0]) and np.array_equal(out[:, 4], sym[:, 4])   # clean neighbours
        assert not np.array_equal(out[:, 1:4], sym[:, 1:4])       # (the corruption did change something)
        same_state(c, sts, "counts of the symbols read")


# ------------------------------------------------------------------ one launch whatever the steps
def test_one_launch_each_way():
    L = _lib()
    rng = np.random.default_rng(31)
    m, B = Model(20, 2, [1, 50], 48, 32), 5
    sym = K.draw(rng, m.V, 700, B)
    counts = {}
    for T in (70, 700):
        with _coder(m, B, cap=T * (m.prec + 2) + 256) as c:
            L.check(c.lib.lac_profile_enable(c.ctx, 1))
            c.encode_counts_job(dev_i32(sym[:T]))
            c.decode_open()
            c.set_count_state()
            out = c.decode_counts(T).cpu().numpy()
            assert np.array_equal(out, sym[:T])
            ms, n = np.zeros(8), np.zeros(8, dtype=np.int64)
            L.check(c.lib.lac_profile_read(c.ctx, ms.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p), 0))
            counts[T] = n.tolist()
    enc, dec = L.KERNEL_IDS["encode"], L.KERNEL_IDS["decode_step"]
    assert counts[70][enc] == counts[700][enc] == 1 and counts[70][dec] == counts[700][dec] == 1, counts


# ------------------------------------------------------------------ refusals and limits
def test_refusals_and_limits():
    from lac_amd._lib import LacError
    L = _lib()

    def refused(code, f):
        with pytest.raises(LacError) as e:
            f()
        assert e.value.code == code, e.value

    m = Model(16, 2, [1, 9], 24, 32)
    with _coder(m, 3, load=False) as c:
        sym = dev_i32(np.zeros((4, 3)))
        refused(L.LAC_E_STATE, lambda: c.encode_counts(sym))                   # no model yet
        refused(L.LAC_E_STATE, lambda: c.decode_counts(4))
        refused(L.LAC_E_STATE, lambda: c.set_count_state())
        refused(L.LAC_E_STATE, lambda: c.count_state())
        for order, W in ((0, []), (5, [1] * 5), (2, [1, 1 << 30])):            # the order; a weight >= 2^30
            refused(L.LAC_E_ARG, lambda: c.load_counts(order, W))
        c.set_mapping("floor")
        refused(L.LAC_E_ARG, lambda: c.load_counts(2, [1, 9]))                 # the floor mapping
        c.set_mapping("ceil")
        c.load_counts(2, [1, (1 << 30) - 1])
        c.load_counts(m.order, m.W)
        assert c.count_layout == {k: K.layout(m.V, m.order)[k] for k in ("Vc", "stride", "off")}
        refused(L.LAC_E_STATE, lambda: c.decode_counts(4))                     # no decode open
        c.set_mapping("floor")
        refused(L.LAC_E_STATE, lambda: c.encode_counts(sym))
        c.set_mapping("ceil")
        c.reset()
        c.encode_counts(sym)
        refused(L.LAC_E_STATE, lambda: c.load_counts(m.order, m.W))            # in mid-job
        c.finish()
        c.load_counts(m.order, m.W)                                            # between jobs: fine
        c.decode_open()
        refused(L.LAC_E_STATE, lambda: c.encode_counts(sym))                   # decoding
        c.decode_counts(4)
        refused(L.LAC_E_STATE, lambda: c.load_counts(m.order, m.W))            # a decode job is running
        c.decode_open()
        c.load_counts(m.order, m.W)
    for V, order, ok in ((4096, 1, True), (4097, 1, False), (75, 4, True), (76, 4, False), (256, 4, False)):
        big = Model(V, order, [1] * order, 48, 32)
        with _coder(big, 1, load=False) as c:
            if ok:
                c.load_counts(order, big.W)
            else:
                refused(L.LAC_E_ARG, lambda: c.load_counts(order, big.W))


def test_a_context_holds_both_kinds_of_model():
    rng = np.random.default_rng(8)
    m = Model(12, 2, [1, 40], 24, 32)
    sym = K.draw(rng, m.V, 70, 2)
    tables = rng.integers(1, 50, size=(3, m.V)).astype(np.uint32)
    nxt = rng.integers(0, 3, size=(3, m.V)).astype(np.int32)
    with _coder(m, 2) as c:
        c.load_fsm(tables, nxt)
        c.encode_fsm_job(dev_i32(sym))
        fsm = E.stream_bytes(c)
        got = job_equals_oracle(c, m, sym, what="counts after an fsm job")
        c.encode_fsm_job(dev_i32(sym))
        assert E.stream_bytes(c)[0] == fsm[0] and fsm[0] != got[0]


def test_order3_byte_model_at_the_limit():
    """16.8 M counts per stream: contexts index the far end of the block."""
    m = Model(256, 3, [1, 16, 300], 48, 32)
    rng = np.random.default_rng(3)
    sym = K.draw(rng, m.V, 65, 1)
    sym[:6, 0] = [255, 255, 255, 255, 0, 255]                     # the last rows of every section
    with _coder(m, 1) as c:
        c.encode_counts_job(dev_i32(sym))
        rows, sts = m.walk(sym)
        v = verdict(m, rows, sym)
        got, n = E.stream_bytes(c)
        assert got == v["data"] and np.array_equal(n, v["nbits"])
        c.decode_open()
        c.set_count_state()
        assert np.array_equal(c.decode_counts(65).cpu().numpy(), sym) and c.status()[0] == 0
        same_state(c, sts)
