"""The match-history kernels (lac_amd/csrc/lac_history.hip) where their own arithmetic is at its
limits: weights of 2^48 - 1 and totals of 2^56 in the three wave sums, both division forms of the
decoder at totals next to 2^50, the u32 entry test at 2^32 - 1 and at 2^32 with the deciding weights
in one lane and in three, last lags on each side of the lanes' seams (lags k, k + 64, k + 128,
k + 192 belong to lane k) under weights that tell the lags apart, and the decoder's search steered
onto the seams of its lanes and passes and onto the exact bounds of a symbol's range.

Every expected value comes from outside the history path: the C oracle on the rows of the literal
host restatement (tests/history.py), this library's pmf path on those rows for registers, plane
words, traces and per-stream status, and oracle/restate.py for exact range bounds.  What each job
reaches is asserted without a device in tests/test_history_host.py.
"""
import numpy as np
import pytest

import errors as E
import history as H
from test_gpu_history import DEC_FIELDS, ENC_FIELDS, Model, _coder, dev_i32, padded, same_fields, same_state, verdict  # noqa: F401
from test_history_host import PROBES, SEAM_P, STEER_V, WIDE_PRECS, WIDE_SHAPES, probe_model

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _job(prec, kind, *args):
    V, P, L, bits, sym, rows, sts = H.job(kind, *args)
    return Model(V, P, L, prec, bits), sym, rows, sts, H.job_verdict(prec, kind, *args)


def job_equals_the_yardsticks(prec, kind, *args, split=False):
    """encode_history_job gives the oracle's bytes and bit counts and the bytes of encode_job on
    the restated rows, and leaves the host walk's rings; decode_history returns the symbols with
    the pmf decoder's registers, status and determined() and leaves the same rings.  ``split``: a
    reset / encode_history / checkpoint run as well -- the encoder's registers, the written plane
    words and the trace are the pmf path's."""
    m, sym, rows, sts, v = _job(prec, kind, *args)
    T, B = sym.shape
    what = (kind, args, prec)
    assert not v["code"].any()
    pmf, dsym = E.dev_pmf(rows, DEV), dev_i32(sym)
    with _coder(m, B, steps=T) as c, _coder(m, B, steps=T, load=False) as ref:
        c.encode_history_job(dsym)
        assert c.status()[0] == 0, what
        got, n = E.stream_bytes(c)
        assert np.array_equal(n, v["nbits"]) and got == v["data"], what
        same_state(c, sts, (what, "after encode"))
        ref.encode_job(pmf, dsym)
        assert E.stream_bytes(ref)[0] == got, what
        bits_t, nb = ref.bits_tensor(), ref.nbits_tensor().clone()
        c.decode_open(bits_t, nb)
        c.set_history_state()
        out = c.decode_history(T).cpu().numpy()
        ref.decode_open(bits_t, nb)
        want = ref.decode(pmf).cpu().numpy()
        assert np.array_equal(want, sym) and np.array_equal(out, sym), what
        same_fields(E.dec_state(c), E.dec_state(ref), DEC_FIELDS, (what, "decoder"))
        sc, sr = c.status(), ref.status()
        assert sc[0] == sr[0] == 0 and np.array_equal(sc[1], sr[1]) and np.array_equal(sc[2], sr[2]), what
        assert np.array_equal(c.determined(), ref.determined()), what
        same_state(c, sts, (what, "after decode"))
        if not split:
            return
        ta = torch.zeros((T, B, 2), dtype=torch.int64, device=DEV)
        tb = torch.zeros((T, B, 2), dtype=torch.int64, device=DEV)
        c.reset()
        c.set_history_state()
        c.encode_history(dsym, trace=ta)
        ref.reset()
        ref.encode(pmf, dsym, trace=tb)
        a, b = c.checkpoint(), ref.checkpoint()
        same_fields(a["state"], b["state"], ENC_FIELDS, (what, "encoder"))
        assert np.array_equal(E.written(a), E.written(b)), what
        assert torch.equal(ta, tb), what


# ------------------------------------------------------------------ 1. wide weights in a u64 context
@pytest.mark.parametrize("prec", WIDE_PRECS)
@pytest.mark.parametrize("V,P", WIDE_SHAPES)
def test_wide_weights(V, P, prec):
    """Weights up to 2^48 - 1 and totals up to V + P (2^48 - 1) (2^56 + 44 at P = 256): never fudged
    at prec 61, partly at 57, mostly at 48 and 16."""
    job_equals_the_yardsticks(prec, "wide", V, P, split=(V, P) == (300, 256) and prec in (57, 48))


# ------------------------------------------------------------------ 2. the division forms at T near 2^50
@pytest.mark.parametrize("prec", (50, 51))
def test_division_forms_at_totals_near_2_50(prec):
    """Totals in [2^47, 2^50): at prec 50 the decoder's small form, at prec 51 the general one."""
    job_equals_the_yardsticks(prec, "wide", 300, 4, split=True)


@pytest.mark.parametrize("prec", (50, 51))
def test_division_forms_with_decode_stop(prec):
    """Streams cut short by different amounts, LAC_OPT_DECODE_STOP on: the symbols, the verdicts,
    err_step and the registers are the pmf path's."""
    from lac_amd._lib import LAC_E_UNDETERMINED
    m, sym, rows, sts, v = _job(prec, "wide", 300, 4)
    T, B = sym.shape
    bits_t, nb = padded(v["data"], v["nbits"])
    cut = torch.clamp(nb - dev_i32(np.arange(B) * 37).to(torch.int64), min=0)
    with _coder(m, B, steps=T) as c, _coder(m, B, steps=T, load=False) as ref:
        for k in (c, ref):
            k.set_decode_stop(True)
            k.decode_open(bits_t, cut)
        c.set_history_state()
        out, want = c.decode_history(T).cpu().numpy(), ref.decode(E.dev_pmf(rows, DEV)).cpu().numpy()
        sc, sr = c.status(), ref.status()
        print("stops", sr[1].tolist(), sr[2].tolist())
        assert (sr[1][1:] == LAC_E_UNDETERMINED).all() and len(set(sr[2][1:].tolist())) >= 2    # the yardstick's reach
        assert np.array_equal(out, want)
        assert sc[0] == sr[0] == LAC_E_UNDETERMINED and np.array_equal(sc[1], sr[1]) and np.array_equal(sc[2], sr[2])
        same_fields(E.dec_state(c), E.dec_state(ref), DEC_FIELDS, "stopped")
        assert np.array_equal(c.determined(), ref.determined())
        stop = [m.walk(sym[:sr[2][b] if sr[1][b] else T, b:b + 1])[1][0] for b in range(B)]
        same_state(c, stop, "frozen at the stop")


# ------------------------------------------------------------------ 3. the u32 entry at 2^32 - 1 and at 2^32
def frozen_like_the_pmf_path(m, sym, rows, sts, code, step):
    """A split encode: codes and err_step as expected and as the pmf path's on the restated rows
    (a refused row is the empty row there), the frozen registers and written plane words the pmf
    path's, the rings those of the failing step.  -> the finished streams' bytes."""
    T, B = sym.shape
    with _coder(m, B, steps=T) as c, _coder(m, B, steps=T, load=False) as ref:
        c.reset()
        c.set_history_state()
        c.encode_history(dev_i32(sym))
        ref.reset()
        ref.encode(E.dev_pmf(rows, DEV), dev_i32(sym))
        rc, err, es = c.status()
        assert err.tolist() == code and es.tolist() == step and rc == E.first_code(np.array(code)), (err, es)
        rr, rerr, res = ref.status()
        assert rerr.tolist() == code and res.tolist() == step and rr == rc          # the contract: the pmf path's
        a, b = c.checkpoint(), ref.checkpoint()
        same_fields(a["state"], b["state"], ENC_FIELDS, "frozen")
        assert np.array_equal(E.written(a), E.written(b))
        same_state(c, sts, "ring as of the failing step")
        c.finish()
        return E.stream_bytes(c)


@pytest.mark.parametrize("prec", (48, 16))
def test_u32_entry_at_the_last_value_that_fits(prec):
    """Lags 0, 64 and 128 -- one lane's -- carry 2^31 - 1, 2^31 - 1 and 1: a constant stream's entry
    is 2^32 - 1 from step 65 on, coded 64 times, and 2^32 at step 129: LAC_E_TABLE there and not
    before.  Stream 2 has the symbol V at that step: LAC_E_SYMBOL_RANGE, the symbol is tested
    before the table (include/lac.h; the oracle, which builds the row first, says LAC_E_TABLE)."""
    m, sym, rows, sts, v = _job(prec, "edge32", 32, 0, 64, 128)
    assert v["code"].tolist() == [E.LAC_E_TABLE, 0, E.LAC_E_TABLE, 0] and v["step"].tolist() == [129, -1, 129, -1]
    code, step = [E.LAC_E_TABLE, 0, E.LAC_E_SYMBOL_RANGE, 0], [129, -1, 129, -1]
    got, n = frozen_like_the_pmf_path(m, sym, rows, sts, code, step)
    for b in (1, 3):
        assert got[b] == v["data"][b] and n[b] == v["nbits"][b], b
    # the u64 context codes the whole job (stream 2 with 5 in the place of V) ...
    m64, sym64, rows64, sts64, v64 = _job(prec, "edge32_clean", 64, 0, 64, 128)
    T, B = sym64.shape
    with _coder(m64, B, steps=T) as c:
        c.encode_history_job(dev_i32(sym64))
        got, n = E.stream_bytes(c)
        assert c.status()[0] == 0 and got == v64["data"] and np.array_equal(n, v64["nbits"])
        same_state(c, sts64)
    # ... and a u32 decoder of its bytes stops at step 129 on the constant streams, as the pmf decoder does
    _, _, rows32, sts32, _ = _job(prec, "edge32_clean", 32, 0, 64, 128)
    with _coder(m, B, steps=T) as c, _coder(m, B, steps=T, load=False) as ref:
        bits_t, nb = padded(v64["data"], v64["nbits"])
        c.decode_open(bits_t, nb)
        c.set_history_state()
        out = c.decode_history(T).cpu().numpy()
        ref.decode_open(bits_t, nb)
        want = ref.decode(E.dev_pmf(rows32, DEV)).cpu().numpy()
        rc, err, es = c.status()
        assert err.tolist() == [E.LAC_E_TABLE, 0, E.LAC_E_TABLE, 0] and es.tolist() == [129, -1, 129, -1], (err, es)
        assert np.array_equal(ref.status()[1], err) and np.array_equal(ref.status()[2], es)
        for b in (0, 2):
            assert (out[:129, b] == 5).all() and (out[129:, b] == -1).all(), b
        assert np.array_equal(out[:, [1, 3]], sym64[:, [1, 3]]) and np.array_equal(out, want)
        same_fields(E.dec_state(c), E.dec_state(ref), DEC_FIELDS, "decoder")
        same_state(c, sts32, "decode")


@pytest.mark.parametrize("prec", (48, 16))
def test_u32_entry_with_the_deciding_weights_in_three_lanes(prec):
    """The same weights at lags 0, 1 and 2: 2^31 at step 1, 2^32 - 1 at step 2, refused at step 3."""
    m, sym, rows, sts, v = _job(prec, "edge32_lanes", 32)
    assert v["code"].tolist() == [E.LAC_E_TABLE, 0] and v["step"].tolist() == [3, -1]
    got, n = frozen_like_the_pmf_path(m, sym, rows, sts, [E.LAC_E_TABLE, 0], [3, -1])
    assert got[1] == v["data"][1] and n[1] == v["nbits"][1]
    m64, sym64, _, sts64, v64 = _job(prec, "edge32_lanes", 64)
    with _coder(m64, 2, steps=len(sym64)) as c:
        c.encode_history_job(dev_i32(sym64))
        got, n = E.stream_bytes(c)
        assert c.status()[0] == 0 and got == v64["data"] and np.array_equal(n, v64["nbits"])
        same_state(c, sts64)


# ------------------------------------------------------------------ 4. lag seams
@pytest.mark.parametrize("P,prec", [(P, 48) for P in SEAM_P] + [(129, 16), (193, 16)])
def test_last_lag_on_each_side_of_a_lane_seam(P, prec):
    """Weights that differ in every lag and run (test_history_host.py: the bytes change when two
    lags across a seam change places, and when the last lag is dropped)."""
    job_equals_the_yardsticks(prec, "seam", P)


# ------------------------------------------------------------------ 5. search edges of the decoder
@pytest.mark.parametrize("bits,V", [(b, V) for b in (32, 64) for V in STEER_V[b]])
def test_symbols_steered_onto_the_search_seams(bits, V):
    """The coded symbols cycle, forwards and backwards, through the first and last entry of a
    lane's vector, of a pass and of the row -- with the entry 1 (P = 4) and above 1 (P = 64); at
    V = 4096 also at prec 16, where most steps fudge."""
    for P in (4, 64):
        job_equals_the_yardsticks(48, "steered", V, bits, P)
    if V == 4096:
        job_equals_the_yardsticks(16, "steered", V, bits, 64)


@pytest.mark.parametrize("bits,V,prec", PROBES)
def test_targets_exactly_on_the_cdf_bounds(bits, V, prec):
    """One step from the full width w = 2^prec with x set to the first and to the last value of a
    symbol's range: unfudged (w >= T) the target is exactly c_{s-1}, and c_s - 1.  The symbol and
    the registers afterwards are the restatement's and the pmf path's."""
    L, ring, pasti, row, probes = probe_model(bits, V, prec)
    B = len(probes)
    m = Model(V, 16, L, prec, bits)
    rows = H.pmf_rows([row] * B, bits)[None]
    zeros = torch.zeros((B, 64), dtype=torch.uint8, device=DEV)
    nb = torch.full((B,), 512, dtype=torch.int64, device=DEV)
    with _coder(m, B) as c, _coder(m, B, load=False) as ref:
        for k in (c, ref):
            k.decode_open(zeros, nb)
            st = E.dec_state(k)
            assert (st["l"] == 0).all() and (st["h"] == (1 << prec) - 1).all() and (st["x"] == 0).all()
            st["x"] = np.array([x for _, x in probes], dtype=st["x"].dtype)
            E.set_dec_state(k, st)
        c.set_history_state(np.array([ring] * B, dtype=np.int32), np.full(B, pasti, dtype=np.int32))
        out = c.decode_history(1).cpu().numpy()[0]
        want = ref.decode(E.dev_pmf(rows, DEV)).cpu().numpy()[0]
        assert want.tolist() == [s for s, _ in probes] and out.tolist() == want.tolist(), (out, want)
        assert c.status()[0] == 0 and ref.status()[0] == 0
        same_fields(E.dec_state(c), E.dec_state(ref), ("l", "h", "x", "pos", "nsym", "det", "ndet", "err"), "after the step")
        after = [H.Stream(V, 16, L, ring, pasti) for _ in probes]
        for st, (s, _) in zip(after, probes):
            st.accept(s)
        same_state(c, after, "the ring accepted s")
