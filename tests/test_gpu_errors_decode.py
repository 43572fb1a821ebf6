"""The sticky per-stream error contract of include/lac.h on every decode kernel form: k_decode_step
(split), k_decode_wave_fine / k_decode_wave (fused / fused_chunk), k_dec_stats + k_decode_seq
(stats), k_decode_block at 4 / 8 / 16 waves, the k_decode_lean <-> k_decode_seq hand-over (stats
with few streams) -- in one call and in calls cut at 1 and 65 -- and windowed runs whose windows
slide (long streams, a refill every 32 steps).

A clean job is encoded and checked against the C oracle's bytes; it is then decoded against tables
in which one row per failing stream is bad (tests/errors.py decode_case: all zero, or a u64 total
of 2^64 / 2^65) at the first, last and next-to-last step of a 64-step chunk.  Expected symbols are
the encoded ones, expected codes and steps those the oracle gives for the same tables
(tests/test_errors_host.py).  A failed stream's registers are compared with a split-path context
that decoded exactly err_step steps of that stream (per-stream counts), byte for byte."""
import numpy as np
import pytest

import errors as E
from test_gpu_layouts import DECODE_FORMS

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REG_FIELDS = ("l", "h", "x", "pos", "nsym", "det", "ndet")
ONE = ((0, E.T_STEPS),)
# bits, prec, rotation: u32 tables (stats takes the lean step), u64 at prec 56 (stats is k_decode_seq
# alone: the lean step needs prec <= 50) and at prec 48 with the other kinds at each position
CASES = ((32, 32, 0), (64, 56, 0), (64, 48, 1))
FORM_IDS = [f"{p}{w or ''}" for p, w in DECODE_FORMS]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _coder(case, cap=None):
    from lac_amd.batch import BatchCoder
    return BatchCoder(case.V, case.B, prec=case.prec, pmf_bits=case.bits,
                      capacity_bits=cap or case.capacity_bits, device=DEV)


def _set_decode(c, path, waves):
    c.set_decode_path(path)
    c.set_block_waves(waves)


_setup_cache = {}


def _setup(case):
    """-> the oracle's streams on the device (bits [B, stride], nbits), the bad and the clean
    tables on the device, and the reference registers: a split-path context whose per-stream
    counts end stream b after its first `position` symbols."""
    if id(case) in _setup_cache:
        return _setup_cache[id(case)]
    v = E.verdict(case, case.clean_pmf, case.clean_sym)
    assert not v["code"].any()
    clean, bad, ds = E.dev_pmf(case.clean_pmf, DEV), E.dev_pmf(case.pmf, DEV), E.dev_sym(case.sym, DEV)
    c = _coder(case)
    c.encode_job(clean, ds)                                       # the clean job, against the oracle
    assert c.status()[0] == 0
    got, gn = E.stream_bytes(c)
    assert np.array_equal(gn, v["nbits"]) and got == v["data"]
    stride = (max(len(d) for d in v["data"]) + 7) // 8 * 8 + 8
    buf = np.zeros((case.B, stride), dtype=np.uint8)
    for b, d in enumerate(v["data"]):
        buf[b, :len(d)] = np.frombuffer(d, dtype=np.uint8)
    bits, nbits = torch.from_numpy(buf).to(DEV), torch.from_numpy(v["nbits"].copy()).to(DEV)
    pos = np.array([p if p >= 0 else case.T for _, _, p in case.streams], dtype=np.int64)
    c.set_decode_path("split")
    c.set_stream_lengths(pos)
    c.decode_open(bits, nbits)
    out = c.decode(bad).cpu().numpy()
    rc, err, _ = c.status()
    assert rc == 0 and not err.any()
    ref = E.dec_state(c)
    c.close()
    assert np.array_equal(ref["nsym"], pos)
    for b in range(case.B):
        assert np.array_equal(out[:pos[b], b], case.sym[:pos[b], b]) and (out[pos[b]:, b] == -1).all()
    _setup_cache[id(case)] = (bits, nbits, bad, clean, ref, pos)
    return _setup_cache[id(case)]


def _expected(case):
    code = np.array([E.EXPECT_CODE[k] for k, _, _ in case.streams], dtype=np.int32)
    step = np.array([p for _, _, p in case.streams], dtype=np.int64)
    return code, step


def _check_run(case, out, status, st, ref, pos, what, base=None):
    code, step = _expected(case)
    rc, err, es = status
    assert np.array_equal(err, code), (what, err)
    assert np.array_equal(es, step), (what, es)
    assert rc == E.first_code(code), (what, rc)
    for b in range(case.B):
        n = int(pos[b])
        assert np.array_equal(out[:n, b], case.sym[:n, b]), (what, b, np.flatnonzero(out[:n, b] != case.sym[:n, b])[:4])
        assert (out[n:, b] == -1).all(), (what, b, out[n:, b])
    assert np.array_equal(st["err"], code) and np.array_equal(st["err_step"], step), (what, st)
    for f in REG_FIELDS:
        got = st[f] + np.uint64(64) * base.astype(np.uint64) if (f == "pos" and base is not None) else st[f]
        assert np.array_equal(got, ref[f]), (what, f, got, ref[f])


def _decode(c, tables, cuts):
    return torch.cat([c.decode(tables[a:b]) for a, b in cuts]).cpu().numpy()


@pytest.mark.parametrize("form", DECODE_FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("bits,prec,k", CASES)
def test_decode_bad_rows(bits, prec, k, form):
    """Symbols before the bad step, -1 from it on (across the 64-step chunks and the later
    calls), LAC_E_TABLE at the position, clean neighbours decoded in full -- among them streams
    whose neighbour's bad row sits at t + 1 under the block path's look-ahead --, registers frozen
    before the failing step; then sticky, and cleared by decode_open."""
    case = E.decode_case(bits, prec, k)
    bits_d, nbits_d, bad, clean, ref, pos = _setup(case)
    c = _coder(case)
    _set_decode(c, *form)
    for cuts in (ONE, E.CUTS):
        what = (form, len(cuts))
        c.decode_open(bits_d, nbits_d)
        out = _decode(c, bad, cuts)
        st = E.dec_state(c)
        _check_run(case, out, c.status(), st, ref, pos, what)
        more = c.decode(clean[:1]).cpu().numpy()                  # sticky: one more step of valid rows
        st2 = E.dec_state(c)
        for b in case.failing:
            assert more[0, b] == -1 and st2[b].tobytes() == st[b].tobytes(), (what, b)
        for b in case.clean:
            assert st2["nsym"][b] == case.T + 1 and st2["err"][b] == 0, (what, b)
    c.decode_open(bits_d, nbits_d)                                # cleared by the next open
    rc, err, es = c.status()
    assert rc == 0 and not err.any() and (es == -1).all()
    assert np.array_equal(_decode(c, clean, ONE), case.sym), form
    c.close()


@pytest.mark.parametrize("cuts", [ONE, E.CUTS], ids=["one", "cuts"])
def test_decode_bad_rows_lean_handover(cuts):
    """stats with 5 u32 streams at prec 48: k_decode_lean, which leaves a stream to k_decode_seq
    for one step at a bad row (resume[b]) -- and, legally, at stream 1's rows of total 2^33 just
    before stream 2's bad row at 64."""
    case = E.decode_case(32, 48, lean=True)
    bits_d, nbits_d, bad, clean, ref, pos = _setup(case)
    c = _coder(case)
    _set_decode(c, "stats", 0)
    c.decode_open(bits_d, nbits_d)
    out = _decode(c, bad, cuts)
    _check_run(case, out, c.status(), E.dec_state(c), ref, pos, ("lean", len(cuts)))
    c.close()


def window_capacity(N, prec):
    """The smallest capacity_bits whose window holds N steps between two refills by include/lac.h's
    rule: W = ceil(capacity_bits / 64) + 1 words with 64 W >= (N + 1) prec + 63."""
    W = ((N + 1) * prec + 63 + 63) // 64
    return 64 * (W - 1), W


@pytest.mark.parametrize("path", ["auto", "split", "fused", "block"])
@pytest.mark.parametrize("bits,prec,k", CASES[:2])
def test_decode_bad_rows_windowed(bits, prec, k, path):
    """decode_open_window with a refill every 32 steps and the smallest window include/lac.h's
    rule allows for them, over streams of ~21 bits per symbol (errors._rows 'skew': ~2700 bits
    against a window of 18 / 30 words), so every stream that gets past its first refills slides:
    window_base() > 0 for the clean streams and the ones failing at 63 and later.  The same
    symbols, status and registers as the whole-stream decode, with pos + 64 base; a failed
    stream's window, base and registers stay where they were through the later refills and one
    more decode call."""
    case = E.decode_case(bits, prec, k, flavour="skew")
    bits_d, nbits_d, bad, clean, ref, pos = _setup(case)
    N = 32
    cap, W = window_capacity(N, case.prec)
    assert int(nbits_d.min()) > 64 * W + 64 * 8                   # the streams outgrow the window by words
    c = _coder(case, cap=cap)
    assert c.bits_stride() == 8 * W
    c.set_decode_path(path)
    c.decode_open_window(bits_d, nbits_d)
    out = []
    for t in range(0, case.T, N):
        out.append(c.decode(bad[t:t + N]))
        c.refill()
    c.refill()
    out = torch.cat(out).cpu().numpy()
    base, st = c.window_base(), E.dec_state(c)
    _check_run(case, out, c.status(), st, ref, pos, ("window", path), base=base)
    for b in range(case.B):
        if pos[b] >= 63:
            assert base[b] > 0, (path, b, base)
    assert c.decode(clean[:1]).cpu().numpy()[0, case.failing].tolist() == [-1] * len(case.failing)
    c.refill()
    base2, st2 = c.window_base(), E.dec_state(c)
    for b in case.failing:
        assert base2[b] == base[b] and st2[b].tobytes() == st[b].tobytes(), (path, b)
    c.close()


@pytest.mark.parametrize("form", DECODE_FORMS + (("stats-lean", 0),), ids=FORM_IDS + ["stats-lean"])
def test_decode_range_error_between_calls(form):
    """x set to l - 1 for one stream and to h + 1 for another between two calls
    (lac_decode_set_state): LAC_E_DECODE_RANGE with err_step = nsym at the call boundary, -1 from
    there on, the registers as they were set, the neighbours intact."""
    lean = form[0] == "stats-lean"
    case = E.decode_case(32, 48, lean=True) if lean else E.decode_case(64, 48, 1)
    bits_d, nbits_d, bad, clean, ref, pos = _setup(case)
    lo_b, hi_b = 1, case.B - 2
    c = _coder(case)
    _set_decode(c, "stats" if lean else form[0], form[1])
    c.decode_open(bits_d, nbits_d)
    out = [c.decode(clean[:65])]
    st = E.dec_state(c)
    st["x"][lo_b] = st["l"][lo_b] - 1
    st["x"][hi_b] = st["h"][hi_b] + 1
    E.set_dec_state(c, st)
    out.append(c.decode(clean[65:]))
    out = torch.cat(out).cpu().numpy()
    rc, err, es = c.status()
    after = E.dec_state(c)
    c.close()
    for b in range(case.B):
        if b in (lo_b, hi_b):
            assert err[b] == E.LAC_E_DECODE_RANGE and es[b] == 65, (form, b, err, es)
            assert np.array_equal(out[:65, b], case.sym[:65, b]) and (out[65:, b] == -1).all(), (form, b)
            for f in REG_FIELDS:
                assert after[f][b] == st[f][b], (form, b, f)
        else:
            assert err[b] == 0 and es[b] == -1 and np.array_equal(out[:, b], case.sym[:, b]), (form, b)
    assert rc == E.LAC_E_DECODE_RANGE


@pytest.mark.parametrize("form", DECODE_FORMS + (("stats-lean", 0),), ids=FORM_IDS + ["stats-lean"])
def test_decode_open_refuses_an_overlong_stream(form):
    """One stream with nbits > 8 * stride: the sticky LAC_E_ARG with err_step 0 and all T outputs
    -1, the other streams decoded in full."""
    lean = form[0] == "stats-lean"
    case = E.decode_case(32, 48, lean=True) if lean else E.decode_case(32, 32, 0)
    bits_d, nbits_d, bad, clean, ref, pos = _setup(case)
    victim = 2
    nb = nbits_d.clone()
    nb[victim] = 8 * bits_d.shape[1] + 1
    c = _coder(case)
    _set_decode(c, "stats" if lean else form[0], form[1])
    for cuts in (ONE, E.CUTS):
        c.decode_open(bits_d, nb)
        out = _decode(c, clean, cuts)
        rc, err, es = c.status()
        assert rc == E.LAC_E_ARG, (form, rc)
        for b in range(case.B):
            if b == victim:
                assert err[b] == E.LAC_E_ARG and es[b] == 0 and (out[:, b] == -1).all(), (form, b, err, es)
            else:
                assert err[b] == 0 and es[b] == -1 and np.array_equal(out[:, b], case.sym[:, b]), (form, b)
    c.close()


@pytest.mark.parametrize("form", DECODE_FORMS + (("stats-lean", 0),), ids=FORM_IDS + ["stats-lean"])
def test_decode_precedence_table_before_range(form):
    """Two defects in one decode step: x set outside [l, h] just before the stream's bad row.
    Every form reports include/lac.h's order -- the table before the registers -- so LAC_E_TABLE
    at the row's step, the registers as they were set."""
    lean = form[0] == "stats-lean"
    case = E.decode_case(32, 48, lean=True) if lean else E.decode_case(64, 48, 1)
    bits_d, nbits_d, bad, clean, ref, pos = _setup(case)
    cut = 64 if lean else 65
    victims = [b for b in range(case.B) if pos[b] == cut]
    assert len(victims) == 1
    v = victims[0]
    c = _coder(case)
    _set_decode(c, "stats" if lean else form[0], form[1])
    for off in (-1, 1):                                           # x = l - 1, then x = h + 1
        c.decode_open(bits_d, nbits_d)
        out = [c.decode(bad[:cut])]
        st = E.dec_state(c)
        assert st["err"][v] == 0 and st["nsym"][v] == cut
        st["x"][v] = st["l"][v] - 1 if off < 0 else st["h"][v] + 1
        E.set_dec_state(c, st)
        out.append(c.decode(bad[cut:]))
        out = torch.cat(out).cpu().numpy()
        rc, err, es = c.status()
        after = E.dec_state(c)
        assert err[v] == E.LAC_E_TABLE and es[v] == cut, (form, off, err, es)
        assert np.array_equal(out[:cut, v], case.sym[:cut, v]) and (out[cut:, v] == -1).all(), (form, off)
        for f in REG_FIELDS:
            assert after[f][v] == st[f][v], (form, off, f)
        for b in case.clean:
            assert err[b] == 0 and np.array_equal(out[:, b], case.sym[:, b]), (form, off, b)
    c.close()
