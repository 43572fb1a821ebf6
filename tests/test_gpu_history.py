"""Match-history models on the device (include/lac.h lac_hist_*, BatchCoder.load_history /
encode_history / decode_history): the kernel keeps the ring and the match lengths, builds each
step's row from them, codes, and moves them.

Every expected value comes from outside the history-model path: the reference's own bits for its
History predictor (tests/golden/history_cases.json), the C oracle on the rows of the literal host
restatement (tests/history.py), and -- for registers, and for corrupt bits -- the pmf path
(encode / decode) of this library on those rows.
"""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import errors as E
import history as H
from test_history_host import CASES, IDS, weights_of

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
    def __init__(self, V, P, L, prec, bits):
        self.V, self.P, self.L, self.prec, self.bits = V, P, L, prec, bits

    def walk(self, sym, states=None):
        return H.walk_batch(self.V, self.P, self.L, sym, self.bits, states)


def _coder(m, B, cap=None, load=True, steps=140):
    from lac_amd.batch import BatchCoder
    c = BatchCoder(m.V, B, prec=m.prec, pmf_bits=m.bits, capacity_bits=cap or (steps + 8) * (m.prec + 2) + 256, device=DEV)
    if load:
        c.load_history(m.P, m.L)
    return c


def verdict(m, pmf, sym):
    return E.verdict(types.SimpleNamespace(B=sym.shape[1], prec=m.prec), pmf, sym)


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def same_fields(got, want, fields, what):
    for f in fields:
        assert np.array_equal(got[f], want[f]), (what, f, got[f], want[f])


def same_state(c, sts, what=""):
    """The coder's rings and write indices against the host walk's streams."""
    ring, pasti = c.history_state()
    for b, st in enumerate(sts):
        assert ring[b].tolist() == st.ring and int(pasti[b]) == st.pasti, (what, b, ring[b], st.ring, pasti[b], st.pasti)


def padded(data, nbits):
    stride = (max(len(d) for d in data) + 7) // 8 * 8 + 8
    buf = np.zeros((len(data), stride), dtype=np.uint8)
    for b, d in enumerate(data):
        buf[b, :len(d)] = np.frombuffer(d, dtype=np.uint8)
    return torch.from_numpy(buf).to(DEV), torch.from_numpy(np.asarray(nbits, dtype=np.int64).copy()).to(DEV)


# ------------------------------------------------------------------ the reference's fixtures
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixture(case):
    """encode_history_job gives the reference's bytes and bit count and ends with its ring,
    decode_history its symbols; with set_decode_stop the stream stops where the reference's
    run(bits, stop=0) stops (the cases whose reference decode finishes)."""
    m = Model(case["V"], case["P"], weights_of(case), case["prec"], case["pmf_bits"])
    sym = np.array(case["syms"], dtype=np.int32)[:, None]
    N = len(sym)
    more = (case["decoded_count"] or N) + 5
    with _coder(m, 1, steps=more) as c:
        c.encode_history_job(dev_i32(sym))
        data, n = c.to_bytes()
        assert int(n[0]) == case["L"] and data[0].hex() == case["bytes"]
        ring, pasti = c.history_state()
        assert ring[0].tolist() == case["ring"] and int(pasti[0]) == case["pasti"]
        c.decode_open()
        c.set_history_state()
        assert np.array_equal(c.decode_history(N).cpu().numpy(), sym)
        assert c.status()[0] == 0
        ring, pasti = c.history_state()
        assert ring[0].tolist() == case["ring"] and int(pasti[0]) == case["pasti"]
        if case["decoded"] is None:
            return
        count = case["decoded_count"]
        c.set_decode_stop(True)
        c.decode_open(c.bits_tensor(), torch.tensor([case["L"]], dtype=torch.int64, device=DEV))
        c.set_history_state()
        out = c.decode_history(more).cpu().numpy()[:, 0]
        rc, err, step = c.status()
        assert rc == _lib().LAC_E_UNDETERMINED and step[0] == count, (rc, step)
        assert out[:count].tolist() == case["decoded"] and (out[count:] == -1).all()
        assert c.determined().tolist() == [count]
        stop = m.walk(np.array(case["decoded"], dtype=np.int32).reshape(-1, 1))[1]
        same_state(c, stop, "frozen at the stop")


# ------------------------------------------------------------------ against the pmf path
def small_weights(P, seed):
    return np.random.default_rng(seed).integers(0, 3000, size=(P, P)).tolist()


# (V, P, streams, prec, entry bits, weights): every P, V, stream count, prec and entry width of the
# issue at least once, the long rings with few streams (the host restatement is O(P^2) a step)
SHAPES = (
    (2, 1, 1, 16, 32, "default"), (3, 2, 3, 16, 64, "default"), (255, 5, 3, 48, 32, "default"),
    (256, 63, 3, 16, 32, "default"), (260, 64, 65, 48, 64, "small"), (4096, 65, 1, 48, 32, "small"),
    (4096, 5, 3, 16, 64, "default"), (3, 256, 3, 48, 32, "default"), (256, 256, 1, 16, 64, "default"),
    (255, 64, 3, 16, 64, "small"), (2, 65, 65, 48, 32, "default"),
)


@functools.lru_cache(maxsize=None)
def shape_job(V, P, B, prec, bits, wk):
    """The shape's model, its symbols (3 P + 5 steps: the ring wraps and M saturates; stream b
    follows pattern b % 4 -- constant, period 3, random, symbol 0 -- and a lone stream changes
    pattern every P + 2 steps), the restated rows and the oracle's verdict: computed once, and
    left as they are by every test that shares them."""
    rng = np.random.default_rng(V * 1000 + P)
    m = Model(V, P, H.default_weights(V, P) if wk == "default" else small_weights(P, P), prec, bits)
    T = 3 * P + 5
    sym = H.draw(rng, V, T, B)
    if B == 1:
        for k, t0 in enumerate(range(0, T, P + 2)):
            sym[t0:t0 + P + 2, 0] = H.pattern(H.PATTERNS[k % 4], rng, V, T)[t0:t0 + P + 2]
    rows, sts = m.walk(sym)
    return m, sym, rows, sts, verdict(m, rows, sym)


@pytest.mark.parametrize("shape", SHAPES, ids=[f"v{s[0]}P{s[1]}b{s[2]}p{s[3]}u{s[4]}" for s in SHAPES])
def test_history_job_equals_the_pmf_job(shape):
    """encode_history equals the oracle and encode_job on the restated rows; decode_history gives
    the symbols; each path decodes the other's output; the rings are the host walk's."""
    m, sym, rows, sts, v = shape_job(*shape)
    B, T = shape[2], sym.shape[0]
    assert not v["code"].any()
    pmf = E.dev_pmf(rows, DEV)
    with _coder(m, B, steps=T) as c, _coder(m, B, steps=T, load=False) as ref:
        c.encode_history_job(dev_i32(sym))
        assert c.status()[0] == 0
        got, n = E.stream_bytes(c)
        assert np.array_equal(n, v["nbits"]) and got == v["data"]
        same_state(c, sts, "after encode")
        ref.encode_job(pmf, dev_i32(sym))
        assert E.stream_bytes(ref)[0] == got
        # the history path decodes the pmf path's output ...
        c.decode_open(ref.bits_tensor(), ref.nbits_tensor().clone())
        c.set_history_state()
        out = c.decode_history(T).cpu().numpy()
        assert c.status()[0] == 0 and np.array_equal(out, sym)
        same_state(c, sts, "after decode")
        # ... and the pmf path the history path's
        c.encode_history_job(dev_i32(sym))
        ref.decode_open(c.bits_tensor(), c.nbits_tensor().clone())
        assert np.array_equal(ref.decode(pmf).cpu().numpy(), sym) and ref.status()[0] == 0


def test_the_fudging_shapes_do_fudge():
    """minp is 1: a step surely fudges when T > 2^prec.  The prec-16 byte shapes mix both kinds."""
    for shape in (s for s in SHAPES if s[3] == 16 and s[0] >= 255):
        m, sym, rows, _, _ = shape_job(*shape)
        T = rows.sum(axis=2, dtype=np.uint64)
        assert 0.05 < float((T > 1 << m.prec).mean()) and float((T <= 1 << (m.prec - 1)).mean()) > 0.05, shape


# ------------------------------------------------------------------ registers are the pmf path's
@functools.lru_cache(maxsize=None)
def _comp_job():
    return shape_job(50, 40, 5, 48, 32, "small")                  # 125 steps, five streams


@pytest.mark.parametrize("V,P,prec,bits,wk", ((256, 20, 16, 32, "default"), (50, 40, 48, 32, "small"),
                                              (31, 7, 60, 64, "default")))
def test_registers_equal_the_pmf_path(V, P, prec, bits, wk):
    m, sym, rows, sts, _ = shape_job(V, P, 5, prec, bits, wk)
    T = sym.shape[0]
    pmf = E.dev_pmf(rows, DEV)
    with _coder(m, 5, steps=T) as c, _coder(m, 5, steps=T, load=False) as ref:
        c.reset()
        c.set_history_state()
        c.encode_history(dev_i32(sym))
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
        c.set_history_state()
        out = c.decode_history(T).cpu().numpy()
        ref.decode_open(bits_t, nb)
        want = ref.decode(pmf).cpu().numpy()
        assert np.array_equal(out, want) and np.array_equal(out, sym)
        same_fields(E.dec_state(c), E.dec_state(ref), DEC_FIELDS, "decoder")


def test_trace_is_the_pmf_paths():
    m, sym, rows, _, _ = _comp_job()
    T, B = sym.shape
    with _coder(m, B, steps=T) as c, _coder(m, B, steps=T, load=False) as ref:
        ta = torch.zeros((T, B, 2), dtype=torch.int64, device=DEV)
        tb = torch.zeros((T, B, 2), dtype=torch.int64, device=DEV)
        c.reset()
        c.set_history_state()
        c.encode_history(dev_i32(sym), trace=ta)
        ref.reset()
        ref.encode(E.dev_pmf(rows, DEV), dev_i32(sym), trace=tb)
        assert torch.equal(ta, tb)


# ------------------------------------------------------------------ state
@pytest.mark.parametrize("V,P,prec,bits,wk", ((50, 40, 48, 32, "small"), (256, 20, 16, 32, "default")))
def test_state_continues_in_a_fresh_context(V, P, prec, bits, wk):
    """Encode k steps, read the state, restore it into a fresh context and go on: the uninterrupted
    job, for k on both sides of a ring wrap (and 1, and a 64-step block's edge)."""
    m, sym, rows, sts, v = shape_job(V, P, 5, prec, bits, wk)
    T = sym.shape[0]
    with _coder(m, 5, steps=T) as c, _coder(m, 5, steps=T) as d:
        for k in (1, P - 1, P, P + 1, 64, 2 * P + 3):
            c.reset()
            c.set_history_state()
            c.encode_history(dev_i32(sym[:k]))
            ck = c.checkpoint()
            ring, pasti = c.history_state()
            same_state(c, m.walk(sym[:k])[1], ("first part", k))
            d.restore(ck)
            d.set_history_state(ring, pasti)
            d.encode_history(dev_i32(sym[k:]))
            d.finish()
            got, n = E.stream_bytes(d)
            assert got == v["data"] and np.array_equal(n, v["nbits"]), k
            same_state(d, sts, ("second part", k))


def test_checkpoint_and_restore_in_mid_job():
    """BatchCoder.checkpoint / restore around a detour: the coder's registers come back with the
    checkpoint, the model's with set_history_state."""
    m, sym, rows, sts, v = _comp_job()
    T, B = sym.shape
    with _coder(m, B, steps=2 * T) as c:
        c.reset()
        c.set_history_state()
        c.encode_history(dev_i32(sym[:70]))
        ck, (ring, pasti) = c.checkpoint(), c.history_state()
        c.encode_history(dev_i32(sym[:33]))                        # the detour
        c.restore(ck)
        c.set_history_state(ring, pasti)
        c.encode_history(dev_i32(sym[70:]))
        c.finish()
        got, n = E.stream_bytes(c)
        assert got == v["data"] and np.array_equal(n, v["nbits"])
        same_state(c, sts)


def test_a_state_no_walk_produced():
    """Any ring over [-1, V) and any write index: M is rebuilt from them by the literal rule."""
    rng = np.random.default_rng(77)
    V, P, B = 9, 12, 4
    m = Model(V, P, small_weights(P, 3), 24, 32)
    ring = rng.integers(-1, V, size=(B, P)).astype(np.int32)
    ring[1] = 4                                                       # one symbol everywhere
    pasti = np.array([0, 5, P - 1, 7], dtype=np.int32)
    start = [H.Stream(V, P, m.L, ring[b], pasti[b]) for b in range(B)]
    sym = H.draw(rng, V, 3 * P + 5, B)
    rows, sts = m.walk(sym, start)
    v = verdict(m, rows, sym)
    with _coder(m, B) as c:
        c.reset()
        c.set_history_state(ring, pasti)
        c.encode_history(dev_i32(sym))
        c.finish()
        got, n = E.stream_bytes(c)
        assert c.status()[0] == 0 and got == v["data"] and np.array_equal(n, v["nbits"])
        same_state(c, sts)
        c.decode_open()
        c.set_history_state(ring, pasti)
        assert np.array_equal(c.decode_history(len(sym)).cpu().numpy(), sym)
        same_state(c, sts, "decode")


# ------------------------------------------------------------------ composition
def test_stream_lengths_over_split_calls():
    m, sym, rows, _, _ = _comp_job()
    T = sym.shape[0]
    cuts = ((0, 1), (1, 65), (65, T))
    lengths = np.array([0, 1, 64, T, 65])
    sts = [m.walk(sym[:k, b:b + 1])[1][0] for b, k in enumerate(lengths)]
    with _coder(m, 5) as c:
        c.set_stream_lengths(lengths)
        c.reset()
        c.set_history_state()
        for a, b in cuts:
            c.encode_history(dev_i32(sym[a:b]))
        c.finish()
        got, n = E.stream_bytes(c)
        for b, k in enumerate(lengths):
            d, nb = E.oracle_prefix(rows[:, b], sym[:, b], int(k), m.prec)
            assert got[b] == d and n[b] == nb, b
        same_state(c, sts, "encode")
        c.decode_open()
        c.set_history_state()
        out = np.concatenate([c.decode_history(b - a).cpu().numpy() for a, b in cuts])
        for b, k in enumerate(lengths):
            assert np.array_equal(out[:k, b], sym[:k, b]) and (out[k:, b] == -1).all(), b
        assert c.status()[0] == 0
        same_state(c, sts, "decode")


def test_stream_lengths_shorter_than_the_job():
    m, sym, rows, _, _ = _comp_job()
    T = sym.shape[0]
    lengths = np.array([T - 1, 3, 0, 70, T])
    sts = [m.walk(sym[:k, b:b + 1])[1][0] for b, k in enumerate(lengths)]
    with _coder(m, 5) as c:
        c.set_stream_lengths(lengths)
        c.encode_history_job(dev_i32(sym))
        got, n = E.stream_bytes(c)
        for b, k in enumerate(lengths):
            d, nb = E.oracle_prefix(rows[:, b], sym[:, b], int(k), m.prec)
            assert got[b] == d and n[b] == nb, b
        same_state(c, sts)
        assert c.status()[0] == 0


def test_three_calls_with_drains_equal_the_one_shot():
    m, sym, rows, sts, v = _comp_job()
    T, B = sym.shape
    with _coder(m, B, cap=70 * (m.prec + 2) + 256) as c:
        slots = torch.zeros((B, 1024), dtype=torch.uint8, device=DEV)
        fill = torch.zeros(B, dtype=torch.int64, device=DEV)
        c.reset()
        c.set_history_state()
        for a, b in ((0, 1), (1, 65), (65, T)):
            c.encode_history(dev_i32(sym[a:b]))
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
    (T, B), N = sym.shape, 4
    bits, nb = padded(v["data"], v["nbits"])
    with _coder(m, B, cap=N * (m.prec + 2) + 256) as c:
        c.decode_open_window(bits, nb)
        c.set_history_state()
        out = torch.empty((T, B), dtype=torch.int32, device=DEV)
        for t in range(0, T, N):
            c.decode_history(min(N, T - t), out=out[t:t + N])
            c.refill()
        c.refill()
        assert c.status()[0] == 0 and np.array_equal(out.cpu().numpy(), sym)
        same_state(c, sts)


# ------------------------------------------------------------------ errors
def test_entry_past_2_32_in_a_u32_context():
    """A constant run under weights of 2^30: the symbol's entry is 1 + t 2^30 at step t < P, past
    u32 from t = 4.  LAC_E_TABLE at exactly that step, the ring frozen, the other streams
    unaffected; the u64 context codes the same job, and a u32 decoder of its bytes stops there too."""
    V, P = 6, 8
    m = Model(V, P, [[1 << 30] * P for _ in range(P)], 24, 32)
    sym = np.full((20, 3), 5, dtype=np.int32)
    sym[:, 1] = np.arange(20) % 5 + 1                              # period 5: a symbol is in the ring twice at most
    sym[:, 2] = 0                                                     # symbol 0 gains no weight
    rows, sts = m.walk(sym)
    v = verdict(m, rows, sym)
    assert v["code"].tolist() == [E.LAC_E_TABLE, 0, 0] and v["step"].tolist() == [4, -1, -1]
    assert sts[0].ring == [5, 5, 5, 5, -1, -1, -1, -1] and sts[0].pasti == 4
    with _coder(m, 3) as c:
        c.reset()
        c.set_history_state()
        c.encode_history(dev_i32(sym))
        rc, err, es = c.status()
        assert err.tolist() == [E.LAC_E_TABLE, 0, 0] and es.tolist() == [4, -1, -1] and rc == E.LAC_E_TABLE
        same_state(c, sts)
        c.encode_history(dev_i32(sym[:3]))                          # sticky: nothing of the failed stream moves
        assert c.status()[1].tolist() == [E.LAC_E_TABLE, 0, 0]
        same_state(c, sts[:1], "sticky")
    m64 = Model(V, P, m.L, 24, 64)
    rows64, sts64 = m64.walk(sym)
    v64 = verdict(m64, rows64, sym)
    assert not v64["code"].any()
    with _coder(m64, 3) as c:
        c.encode_history_job(dev_i32(sym))
        got, n = E.stream_bytes(c)
        assert c.status()[0] == 0 and got == v64["data"] and np.array_equal(n, v64["nbits"])
        same_state(c, sts64)
    with _coder(m, 3) as c:                                         # the u64 job's bytes in a u32 context
        c.decode_open(*padded(v64["data"], v64["nbits"]))
        c.set_history_state()
        out = c.decode_history(20).cpu().numpy()
        rc, err, es = c.status()
        assert err.tolist() == [E.LAC_E_TABLE, 0, 0] and es.tolist() == [4, -1, -1]
        assert np.array_equal(out[:4, 0], sym[:4, 0]) and (out[4:, 0] == -1).all()
        assert np.array_equal(out[:, 1:], sym[:, 1:])
        same_state(c, sts, "decode")


def test_u32_rows_whose_total_passes_2_32():
    V, P = 40, 16
    m = Model(V, P, [[1 << 29] * P for _ in range(P)], 48, 32)
    sym = ((np.arange(60)[:, None] * 7 + np.arange(3)[None, :] * 3) % (V - 1) + 1).astype(np.int32)   # no symbol twice in a ring
    rows, sts = m.walk(sym)
    assert (rows.sum(axis=2, dtype=np.uint64)[20:] > 1 << 32).all() and rows.max() < 1 << 32
    v = verdict(m, rows, sym)
    with _coder(m, 3) as c:
        c.encode_history_job(dev_i32(sym))
        got, n = E.stream_bytes(c)
        assert c.status()[0] == 0 and got == v["data"] and np.array_equal(n, v["nbits"])
        c.decode_open()
        c.set_history_state()
        assert np.array_equal(c.decode_history(60).cpu().numpy(), sym) and c.status()[0] == 0


def test_symbol_errors_freeze_the_stream_at_their_step():
    """A symbol >= V or < 0 at the first, last and next-to-last step of a 64-step block."""
    m, sym, _, _, _ = _comp_job()
    sym = sym.copy()
    B = sym.shape[1]
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
        c.set_history_state()
        c.encode_history(dev_i32(sym))
        ref.reset()
        ref.encode(E.dev_pmf(rows, DEV), dev_i32(sym))
        rc, err, es = c.status()
        assert np.array_equal(err, code) and np.array_equal(es, step) and rc == E.first_code(code)
        a, b = c.checkpoint(), ref.checkpoint()
        same_fields(a["state"], b["state"], ENC_FIELDS, "frozen")
        assert np.array_equal(E.written(a), E.written(b))
        same_state(c, sts, "ring as of the failing step")
        c.encode_history(dev_i32(sym[:3]))                          # sticky
        assert np.array_equal(c.status()[1][:4], code[:4])
        same_state(c, sts[:4], "sticky")
        c.encode_history_job(dev_i32(sym[:, 4:5].repeat(B, axis=1)))   # a reset clears it
        assert c.status()[0] == 0 and E.stream_bytes(c)[0][0] == v["data"][4]


def test_capacity_overflow_in_mid_job():
    """250 bits of room: the random and the symbol-0 stream run out of it in mid-job, the constant
    streams, whose matches make them cheap, finish (the period-3 stream as the pmf path has it)."""
    m, sym, rows, _, v = _comp_job()
    (T, B), cap = sym.shape, 5 * (m.prec + 2)
    assert (v["nbits"][[0, 4]] < cap // 2).all() and (v["nbits"][[2, 3]] > 2 * cap).all()
    with _coder(m, B, cap=cap) as c, _coder(m, B, cap=cap, load=False) as ref:
        c.reset()
        c.set_history_state()
        c.encode_history(dev_i32(sym))
        ref.reset()
        ref.encode(E.dev_pmf(rows, DEV), dev_i32(sym))
        rc, err, es = c.status()
        rc2, err2, es2 = ref.status()
        assert err[[0, 2, 3, 4]].tolist() == [0, E.LAC_E_CAPACITY, E.LAC_E_CAPACITY, 0]
        assert np.array_equal(err, err2) and np.array_equal(es, es2) and rc == rc2 and (es[2:4] > 0).all()
        same_fields(c.checkpoint()["state"], ref.checkpoint()["state"], ENC_FIELDS, "frozen")
        sts = [m.walk(sym[:es[b] if err[b] else T, b:b + 1])[1][0] for b in range(B)]
        same_state(c, sts, "as of the failing step")


@pytest.mark.parametrize("V,P,prec,bits,wk", ((256, 20, 16, 32, "default"), (50, 40, 48, 32, "small"),
                                              (31, 7, 48, 64, "default")))
def test_corrupt_bits_equal_the_per_position_loop(V, P, prec, bits, wk):
    """One flipped bit per stream: symbols, -1 fills, codes, steps and registers are those of the
    per-position pmf decode with the rows rebuilt on the host from the symbols read back."""
    m, sym, _, _, v = shape_job(V, P, 5, prec, bits, wk)
    rng = np.random.default_rng(V + prec)
    T, B = sym.shape
    bits_t, nb = padded(v["data"], v["nbits"])
    for b in range(1, 4):                                           # streams 1..3: one flipped bit each
        at = int(rng.integers(4, max(int(v["nbits"][b]) // 2, 6)))
        bits_t[b, at // 8] ^= 0x80 >> (at % 8)
    with _coder(m, B, steps=T) as c, _coder(m, B, steps=T, load=False) as ref:
        c.decode_open(bits_t, nb)
        c.set_history_state()
        out = c.decode_history(T).cpu().numpy()
        rc, err, es = c.status()
        assert all(int(e) in _lib().STATUS_NAMES for e in err)      # the status is a code
        ref.decode_open(bits_t, nb)
        sts = [H.Stream(V, P, m.L) for _ in range(B)]
        want = np.zeros((T, B), dtype=np.int32)
        for t in range(T):
            rows = H.pmf_rows([st.row() for st in sts], bits)[None]
            want[t] = ref.decode(E.dev_pmf(rows, DEV)).cpu().numpy()[0]
            for b, st in enumerate(sts):
                if want[t, b] >= 0:
                    st.accept(want[t, b])
        assert np.array_equal(out, want)
        rc2, err2, es2 = ref.status()
        assert rc == rc2 and np.array_equal(err, err2) and np.array_equal(es, es2)
        same_fields(E.dec_state(c), E.dec_state(ref), DEC_FIELDS, "registers")
        assert np.array_equal(out[:, 0], sym[:, 0]) and np.array_equal(out[:, 4], sym[:, 4])   # clean neighbours
        same_state(c, sts, "rings of the symbols read")


# ------------------------------------------------------------------ one launch whatever the steps
def test_one_launch_each_way():
    L = _lib()
    rng = np.random.default_rng(31)
    m, B = Model(20, 9, small_weights(9, 1), 48, 32), 5
    sym = H.draw(rng, m.V, 700, B)
    counts = {}
    for T in (70, 700):
        with _coder(m, B, steps=T) as c:
            L.check(c.lib.lac_profile_enable(c.ctx, 1))
            c.encode_history_job(dev_i32(sym[:T]))
            c.decode_open()
            c.set_history_state()
            out = c.decode_history(T).cpu().numpy()
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

    V, P = 16, 6
    m = Model(V, P, small_weights(P, 2), 24, 32)
    with _coder(m, 3, load=False) as c:
        sym = dev_i32(np.zeros((4, 3)))
        refused(L.LAC_E_STATE, lambda: c.encode_history(sym))                  # no model yet
        refused(L.LAC_E_STATE, lambda: c.decode_history(4))
        refused(L.LAC_E_STATE, lambda: c.set_history_state())
        refused(L.LAC_E_STATE, lambda: c.history_state())
        for p in (0, 257):                                                     # P in [1, 256]
            refused(L.LAC_E_ARG, lambda: c.load_history(p, [[1] * p] * p))
        big = [[1] * P for _ in range(P)]
        big[P - 1][P - 1] = 1 << 48
        refused(L.LAC_E_ARG, lambda: c.load_history(P, big))                   # a weight >= 2^48
        c.set_mapping("floor")
        refused(L.LAC_E_ARG, lambda: c.load_history(P, m.L))                   # the floor mapping
        c.set_mapping("ceil")
        big[P - 1][P - 1] = (1 << 48) - 1
        c.load_history(P, big)
        c.load_history(256, [[1] * 256] * 256)
        c.load_history(P, m.L)
        ring = np.full((3, P), -1, dtype=np.int32)
        pasti = np.zeros(3, dtype=np.int32)
        for at, x in (((2, P - 1), V), ((0, 0), -2)):                          # ring entries in [-1, V)
            r = ring.copy()
            r[at] = x
            refused(L.LAC_E_ARG, lambda: c.set_history_state(r, pasti))
        for x in (P, -1):                                                      # pasti in [0, P)
            q = pasti.copy()
            q[2] = x
            refused(L.LAC_E_ARG, lambda: c.set_history_state(ring, q))
            refused(L.LAC_E_ARG, lambda: c.set_history_state(None, q))
        ring[1, 3] = V - 1
        pasti[1] = P - 1
        c.set_history_state(ring, pasti)
        got = c.history_state()
        assert np.array_equal(got[0], ring) and np.array_equal(got[1], pasti)
        refused(L.LAC_E_ARG, lambda: c.set_history_state(ring, np.array([0, P, 0], dtype=np.int32)))
        got = c.history_state()                                                # a refused state changes nothing
        assert np.array_equal(got[0], ring) and np.array_equal(got[1], pasti)
        refused(L.LAC_E_STATE, lambda: c.decode_history(4))                    # no decode open
        c.set_mapping("floor")
        refused(L.LAC_E_STATE, lambda: c.encode_history(sym))
        c.set_mapping("ceil")
        c.reset()
        c.encode_history(sym)
        refused(L.LAC_E_STATE, lambda: c.load_history(P, m.L))                 # in mid-job
        c.finish()
        c.load_history(P, m.L)                                                 # between jobs: fine
        c.decode_open()
        refused(L.LAC_E_STATE, lambda: c.encode_history(sym))                  # decoding
        c.decode_history(4)
        refused(L.LAC_E_STATE, lambda: c.load_history(P, m.L))                 # a decode job is running
        c.decode_open()
        c.load_history(P, m.L)
    for V, ok in ((4096, True), (4097, False)):
        with _coder(Model(V, 2, None, 48, 32), 1, load=False) as c:
            if ok:
                c.load_history(2, [[1, 2], [3, 4]])
            else:
                refused(L.LAC_E_ARG, lambda: c.load_history(2, [[1, 2], [3, 4]]))


def test_a_context_holds_all_three_kinds_of_model():
    rng = np.random.default_rng(8)
    m, sym, rows, sts, v = shape_job(12, 7, 2, 24, 32, "small")
    tables = rng.integers(1, 50, size=(3, m.V)).astype(np.uint32)
    nxt = rng.integers(0, 3, size=(3, m.V)).astype(np.int32)
    with _coder(m, 2) as c:
        c.load_fsm(tables, nxt)
        c.load_counts(2, [1, 40])
        c.encode_fsm_job(dev_i32(sym))
        fsm = E.stream_bytes(c)[0]
        c.encode_counts_job(dev_i32(sym))
        cnt = E.stream_bytes(c)[0]
        c.encode_history_job(dev_i32(sym))
        assert E.stream_bytes(c)[0] == v["data"]
        same_state(c, sts)
        c.encode_fsm_job(dev_i32(sym))
        assert E.stream_bytes(c)[0] == fsm
        c.encode_counts_job(dev_i32(sym))
        assert E.stream_bytes(c)[0] == cnt and len({tuple(fsm), tuple(cnt), tuple(v["data"])}) == 3
