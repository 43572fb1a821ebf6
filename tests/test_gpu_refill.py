"""Windowed decode (include/lac.h lac_decode_open_window / lac_decode_refill / lac_decode_window_base,
BatchCoder.decode_open_window / refill / window_base, lac_amd.batch.HostBits): a coder whose
capacity holds only the bits between two refills decodes what lac_decode_open decodes on the whole
streams -- symbols, status, every register with pos + 64 * base, determined().  Every comparison
is against the whole-stream decode in a plain context and the coded symbols, never against the
windowed coder itself."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAC_E_ARG, LAC_E_CAPACITY, LAC_E_STATE, LAC_E_UNDETERMINED = -1, -7, -9, -12
SENTINEL = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _dec_dtype():
    from lac_amd.coder import _DEC_STATE
    return _DEC_STATE


def _state(c):
    from lac_amd import _lib
    st = np.zeros(c.streams, dtype=_dec_dtype())
    _lib.check(c.lib.lac_decode_get_state(c.ctx, st.ctypes.data_as(C.c_void_p), c._stream))
    return st


def _set_state(c, st):
    from lac_amd import _lib
    st = np.ascontiguousarray(st)
    _lib.check(c.lib.lac_decode_set_state(c.ctx, st.ctypes.data_as(C.c_void_p), c._stream))


def _absolute(st, base=None):
    """The state with pos made absolute: pos + 64 * base."""
    st = st.copy()
    if base is not None:
        st["pos"] += np.uint64(64) * base.astype(np.uint64)
    return st


def _same_states(a, b):
    for f in a.dtype.names:
        assert np.array_equal(a[f], b[f]), (f, a[f], b[f])


def _dev(pmf):
    it = np.int32 if pmf.dtype == np.uint32 else np.int64
    return torch.from_numpy(np.ascontiguousarray(pmf).view(it)).to(DEV)


def _cap(N, prec):
    return N * (prec + 2) + 256


@functools.lru_cache(maxsize=None)
def _case(bits, prec, V=64, B=5, T=400, seed=0):
    """Skewed tables (entries 2^0 .. 2^19 / 2^39, symbols uniform: ~12 / ~22 bits per symbol),
    coded by encode_job -> tables, symbols, the streams on the device, their counts, their bytes."""
    from lac_amd.batch import BatchCoder
    rng = np.random.default_rng(1000 * bits + prec + seed)
    ex = rng.integers(0, 20 if bits == 32 else 40, size=(T, B, V))
    pmf = (np.uint64(1) << ex.astype(np.uint64)).astype(np.uint32 if bits == 32 else np.uint64)
    sym = rng.integers(0, V, size=(T, B)).astype(np.int32)
    dp, ds = _dev(pmf), torch.from_numpy(sym).to(DEV)
    with BatchCoder(V, B, prec=prec, pmf_bits=bits, capacity_bits=T * (prec + 2) + 256, device=DEV) as c:
        c.encode_job(dp, ds)
        assert c.status()[0] == 0
        dbits, dn = c.bits_tensor(), c.nbits_tensor().clone()
        data, nb = c.to_bytes()
    return dp, ds, dbits, dn, data, np.asarray(nb).astype(np.int64)


def _run(bits, prec, dp, T, N, path, src, nbits, cap, window, lengths=None, stop=False, probe=None, V=64):
    """Decode T steps in calls of N steps (a refill after each call and one at the end when
    `window`) -> symbols [T, B], status, absolute state, determined()."""
    from lac_amd.batch import BatchCoder
    B = dp.shape[1]
    with BatchCoder(V, B, prec=prec, pmf_bits=bits, capacity_bits=cap, device=DEV) as c:
        c.set_decode_path(path)
        if lengths is not None:
            c.set_stream_lengths(lengths)
        if stop:
            c.set_decode_stop(True)
        if window:
            c.decode_open_window(src, nbits)
        else:
            c.decode_open(src, nbits)
        out = torch.empty((T, B), dtype=torch.int32, device=DEV)
        for t in range(0, T, N):
            c.decode(dp[t:t + N], out[t:min(t + N, T)])
            if window:
                c.refill()
            if probe is not None:
                probe(c, min(t + N, T))
        if window:
            c.refill()
        rc, err, step = c.status()
        st = _absolute(_state(c), c.window_base() if window else None)
        return out.cpu().numpy(), (rc, err.copy(), step.copy()), st, c.determined()


def _same_run(got, want):
    assert np.array_equal(got[0], want[0])
    assert got[1][0] == want[1][0] and np.array_equal(got[1][1], want[1][1]) and np.array_equal(got[1][2], want[1][2])
    _same_states(got[2], want[2])
    assert np.array_equal(got[3], want[3])


# ------------------------------------------------------------------ 1. equality with the whole-stream decode
@functools.lru_cache(maxsize=None)
def _whole(bits, prec, path, N):
    dp, ds, dbits, dn, _, _ = _case(bits, prec)
    T = dp.shape[0]
    r = _run(bits, prec, dp, T, N, path, dbits, dn, T * (prec + 2) + 256, window=False)
    assert r[1][0] == 0 and np.array_equal(r[0], ds.cpu().numpy())
    return r


@pytest.mark.parametrize("path", ["split", "fused", "stats", "block", "auto"])
@pytest.mark.parametrize("prec", [16, 48, 61])
@pytest.mark.parametrize("bits", [32, 64])
def test_windowed_decode_equals_whole_stream_decode(bits, prec, path):
    from lac_amd.batch import HostBits
    dp, ds, dbits, dn, data, nb = _case(bits, prec)
    T = dp.shape[0]
    host = HostBits(data, nb, DEV)
    try:
        for N in (1, 7, 64):
            want = _whole(bits, prec, path, N)
            _same_run(_run(bits, prec, dp, T, N, path, dbits, dn, _cap(N, prec), window=True), want)
            _same_run(_run(bits, prec, dp, T, N, path, host, None, _cap(N, prec), window=True), want)
    finally:
        torch.cuda.synchronize()
        host.close()


# ------------------------------------------------------------------ 2. stream ends; more than one block of words
LV, LB, LT, LPREC, LBITS = 64, 6, 1000, 48, 64


@functools.lru_cache(maxsize=None)
def _long_case():
    return _case(LBITS, LPREC, V=LV, B=LB, T=LT, seed=5)


def _window_bits(N):
    from lac_amd.batch import BatchCoder
    with BatchCoder(LV, LB, prec=LPREC, pmf_bits=LBITS, capacity_bits=_cap(N, LPREC), device=DEV) as c:
        return 8 * c.bits_stride()


def test_stream_ends():
    """Counts of 0, below prec, exactly the window, one bit more, a multiple of 64, and a stream
    some 50 windows long, side by side: truncated streams decode zeros past their end, and the
    registers, status and determined counts are the whole-stream decode's."""
    dp, ds, dbits, dn, _, nb = _long_case()
    wb = _window_bits(1)
    assert int(nb.min()) > 30 * wb
    counts = np.array([0, LPREC - 5, wb, wb + 1, 64 * 100, int(nb[5])], dtype=np.int64)
    dn2 = torch.from_numpy(counts).to(DEV)
    want = _run(LBITS, LPREC, dp, LT, 1, "auto", dbits, dn2, LT * (LPREC + 2) + 256, window=False)
    got = _run(LBITS, LPREC, dp, LT, 1, "auto", dbits, dn2, _cap(1, LPREC), window=True)
    _same_run(got, want)
    assert np.array_equal(got[0][:, 5], ds.cpu().numpy()[:, 5])
    assert 0 < got[3][4] < LT                                    # determined(): by the bits held


def test_stream_lengths_and_decode_stop():
    dp, ds, dbits, dn, _, nb = _long_case()
    lengths = np.array([LT, 100, 0, LT, 333, LT], dtype=np.int64)
    bases = {}

    def probe(c, t):
        if t in (150, LT):
            bases[t] = c.window_base()

    want = _run(LBITS, LPREC, dp, LT, 1, "auto", dbits, dn, LT * (LPREC + 2) + 256, window=False, lengths=lengths)
    got = _run(LBITS, LPREC, dp, LT, 1, "auto", dbits, dn, _cap(1, LPREC), window=True, lengths=lengths, probe=probe)
    _same_run(got, want)
    sym = ds.cpu().numpy()
    for b in range(LB):
        assert np.array_equal(got[0][:lengths[b], b], sym[:lengths[b], b]) and (got[0][lengths[b]:, b] == -1).all()
    assert bases[150][1] == bases[LT][1] and bases[150][2] == bases[LT][2] == 0   # an ended stream's window stays
    assert bases[150][0] < bases[LT][0]
    # LAC_OPT_DECODE_STOP on truncated streams: the same step, LAC_E_UNDETERMINED
    cut = torch.from_numpy(np.array([int(nb[0]), 3000, 64 * 50, 777, int(nb[4]), 64 * 200 + 1], dtype=np.int64)).to(DEV)
    want = _run(LBITS, LPREC, dp, LT, 7, "auto", dbits, cut, LT * (LPREC + 2) + 256, window=False, stop=True)
    got = _run(LBITS, LPREC, dp, LT, 7, "auto", dbits, cut, _cap(7, LPREC), window=True, stop=True)
    _same_run(got, want)
    assert (got[1][1][[1, 2, 3, 5]] == LAC_E_UNDETERMINED).all()


@pytest.mark.parametrize("path", ["auto", "fused"])
def test_windows_of_more_than_one_block(path):
    """300 steps of ~22 bits between refills: a window of 240 words that drops ~100 words per
    refill -- k_dec_refill's move and fetch loops run more than one block of 64 words."""
    dp, ds, dbits, dn, data, nb = _long_case()
    N = 300
    assert _window_bits(N) // 64 > 128 and int(nb.min()) > _window_bits(N) + 64 * 20
    bases = {}
    want = _run(LBITS, LPREC, dp, LT, N, path, dbits, dn, LT * (LPREC + 2) + 256, window=False)
    got = _run(LBITS, LPREC, dp, LT, N, path, dbits, dn, _cap(N, LPREC), window=True,
               probe=lambda c, t: bases.setdefault(t, c.window_base()))
    _same_run(got, want)
    assert np.array_equal(got[0], ds.cpu().numpy())
    # the refill after step 300 dropped and fetched more than 64 words and moved more than 64
    # (the next one finds the stream's end inside the window, which then stays)
    assert int(bases[300].min()) > 64 and _window_bits(N) // 64 - int(bases[300].max()) > 64


# ------------------------------------------------------------------ 3. a stream that outruns its window
def test_dry_stream_is_flagged_at_the_refill():
    """Uniform rows over 32768 symbols at prec 48: 15 bits per symbol, so 40 steps with no refill
    consume 600 bits against a window of capacity_bits = 256.  The long stream is flagged at the
    refill; the stream beside it, whole inside its window, is not."""
    from lac_amd.batch import BatchCoder
    V, prec, steps = 32768, 48, 40
    pmf = torch.ones((1, 1, V), dtype=torch.int32, device=DEV)
    rng = np.random.default_rng(9)
    sym = torch.from_numpy(rng.integers(0, V, size=(60, 2)).astype(np.int32)).to(DEV)
    lengths = np.array([60, 15], dtype=np.int64)
    with BatchCoder(V, 2, prec=prec, capacity_bits=60 * (prec + 2) + 256, device=DEV) as c:
        c.set_stream_lengths(lengths)
        c.encode_job(pmf.expand(60, 2, V), sym)
        assert c.status()[0] == 0
        bits, nb = c.bits_tensor(), c.nbits_tensor().clone()
    stride = bits.shape[1]
    framed = torch.full((4, stride), SENTINEL, dtype=torch.uint8, device=DEV)   # sentinel rows around the source
    framed[1:3] = bits
    before = framed.clone()
    with BatchCoder(V, 2, prec=prec, capacity_bits=256, device=DEV) as c:
        wbits = 8 * c.bits_stride()
        assert int(nb[0]) > 2 * wbits and int(nb[1]) <= wbits and 15 * steps + prec > wbits
        c.set_stream_lengths(lengths)
        c.decode_open_window(framed[1:3], nb)
        out = c.decode(pmf.expand(steps, 2, V))
        assert c.status()[0] == 0                                # not detected by the steps
        c.refill()
        rc, err, step = c.status()
        st = _state(c)
        assert rc == LAC_E_CAPACITY and err.tolist() == [LAC_E_CAPACITY, 0]
        assert st["nsym"].tolist() == [steps, 15] and step[0] == steps
        got = out.cpu().numpy()
        assert np.array_equal(got[:15, 1], sym.cpu().numpy()[:15, 1]) and (got[15:, 1] == -1).all()
        c.refill()                                               # sticky: the stream is left alone
        _same_states(_state(c), st)
    torch.cuda.synchronize()
    assert torch.equal(framed, before)


# ------------------------------------------------------------------ 4. untrusted counts, refusals
def test_untrusted_counts_fail_their_stream_alone():
    from lac_amd.batch import BatchCoder
    bits, prec = 32, 48
    dp, ds, dbits, dn, _, nb = _case(bits, prec)
    T, B = ds.shape
    N = 7
    sym = ds.cpu().numpy()
    stride = dbits.shape[1]
    # stream 1 claims more bits than its row holds; stream 3's window would start past its end
    claimed = nb.copy()
    claimed[1] = 8 * stride + 1
    base = np.zeros(B, dtype=np.int64)
    base[3] = nb[3] // 64 + 1
    with BatchCoder(64, B, prec=prec, pmf_bits=bits, capacity_bits=_cap(N, prec), device=DEV) as c:
        c.decode_open_window(dbits, torch.from_numpy(claimed).to(DEV), base=base)
        out = torch.empty((T, B), dtype=torch.int32, device=DEV)
        for t in range(0, T, N):
            c.decode(dp[t:t + N], out[t:t + N])
            c.refill()
        rc, err, step = c.status()
        assert rc == LAC_E_ARG and err.tolist() == [0, LAC_E_ARG, 0, LAC_E_ARG, 0]
        got = out.cpu().numpy()
        assert (got[:, [1, 3]] == -1).all() and np.array_equal(got[:, [0, 2, 4]], sym[:, [0, 2, 4]])
        assert c.window_base()[[1, 3]].tolist() == [0, 0]


def test_refusals_change_nothing():
    from lac_amd import _lib
    from lac_amd.batch import BatchCoder
    bits, prec = 32, 48
    dp, ds, dbits, dn, _, nb = _case(bits, prec)
    T, B = ds.shape
    sym = ds.cpu().numpy()

    def refused(code, call):
        with pytest.raises(_lib.LacError) as e:
            call()
        assert e.value.code == code

    with BatchCoder(64, B, prec=prec, pmf_bits=bits, capacity_bits=T * (prec + 2) + 256, device=DEV) as c:
        # an encoding context
        c.reset()
        c.encode(dp[:10], ds[:10])
        ck = c.checkpoint()
        refused(LAC_E_STATE, c.refill)
        refused(LAC_E_STATE, c.window_base)
        ck2 = c.checkpoint()
        assert ck["state"].tobytes() == ck2["state"].tobytes() and np.array_equal(ck["planes"], ck2["planes"])
        # a plain decode_open
        c.decode_open(dbits, dn)
        c.decode(dp[:20])
        st = _state(c)
        refused(LAC_E_STATE, c.refill)
        # misaligned source / stride: nothing opened, the plain decode goes on
        odd = torch.zeros((B, dbits.shape[1] + 8), dtype=torch.uint8, device=DEV)
        refused(LAC_E_ARG, lambda: c.decode_open_window(odd[:, 4:], dn))
        skew = torch.zeros((B, dbits.shape[1] + 4), dtype=torch.uint8, device=DEV)
        refused(LAC_E_ARG, lambda: c.decode_open_window(skew, dn))
        assert c.lib.lac_decode_open_window(c.ctx, None, 8, C.c_void_p(dn.data_ptr()), None, c._stream) == LAC_E_ARG
        refused(LAC_E_STATE, c.refill)
        _same_states(_state(c), st)
        assert np.array_equal(c.decode(dp[20:40]).cpu().numpy(), sym[20:40])
        # after decode_open_packed
        payload = torch.cat([dbits[b, :(int(nb[b]) + 7) // 8] for b in range(B)])
        c.decode_open_packed(payload, 0, counts=dn)
        c.decode(dp[:20])
        st = _state(c)
        refused(LAC_E_STATE, c.refill)
        _same_states(_state(c), st)
        assert np.array_equal(c.decode(dp[20:40]).cpu().numpy(), sym[20:40])
        # a windowed open, then a plain one: the window is gone
        c.decode_open_window(dbits, dn)
        c.refill()
        c.decode_open(dbits, dn)
        refused(LAC_E_STATE, c.refill)


# ------------------------------------------------------------------ 5. resume
@pytest.mark.parametrize("at", [200, 210])                      # between two refills, and right after one
def test_resume_from_state_and_window_base(at):
    from lac_amd.batch import BatchCoder
    bits, prec, N = 32, 48, 7
    dp, ds, dbits, dn, _, nb = _case(bits, prec)
    T, B = ds.shape
    want = _whole(bits, prec, "auto", N)
    saved = {}

    def probe(c, t):
        if t == at:
            saved["st"], saved["base"] = _state(c), c.window_base()

    # the first part, in calls that end at `at`
    with BatchCoder(64, B, prec=prec, pmf_bits=bits, capacity_bits=_cap(N, prec), device=DEV) as c:
        c.decode_open_window(dbits, dn)
        out = torch.empty((T, B), dtype=torch.int32, device=DEV)
        for t in range(0, at, N):
            c.decode(dp[t:min(t + N, at)], out[t:min(t + N, at)])
            if t + N <= at:
                c.refill()
        probe(c, at)
    assert saved["base"].min() > 0
    with BatchCoder(64, B, prec=prec, pmf_bits=bits, capacity_bits=_cap(N, prec), device=DEV) as c:
        c.decode_open_window(dbits, dn, base=saved["base"])
        _set_state(c, saved["st"])
        c.refill()
        for t in range(at, T, N):
            c.decode(dp[t:t + N], out[t:min(t + N, T)])
            c.refill()
        assert c.status()[0] == 0
        _same_states(_absolute(_state(c), c.window_base()), want[2])
        assert np.array_equal(c.determined(), want[3])
    assert np.array_equal(out.cpu().numpy(), ds.cpu().numpy())


# ------------------------------------------------------------------ 6. the logits decode
@functools.lru_cache(maxsize=None)
def _logits_case():
    from lac_amd.batch import BatchCoder
    V, B, T, prec = 512, 3, 200, 48
    g = torch.Generator().manual_seed(21)
    lg = (torch.randn((T, B, V), generator=g) * 4).to(torch.bfloat16).to(DEV)
    sym = torch.randint(0, V, (T, B), generator=g, dtype=torch.int32).to(DEV)
    with BatchCoder(V, B, prec=prec, capacity_bits=T * (prec + 2) + 256, device=DEV) as c:
        c.encode_logits_job(lg, sym)
        bits, nb = c.bits_tensor(), c.nbits_tensor().clone()
        c.decode_open(bits, nb)
        whole = c.decode_logits(lg).cpu().numpy()
        st, det = _state(c), c.determined()
        assert c.status()[0] == 0
    assert np.array_equal(whole, sym.cpu().numpy())
    return V, B, T, prec, lg, bits, nb, whole, st, det


@pytest.mark.parametrize("N", [1, 16])
@pytest.mark.parametrize("mode", ["fused", "split"])
def test_logits_step_with_refills_equals_whole_logits_decode(mode, N):
    from lac_amd.batch import BatchCoder
    V, B, T, prec, lg, bits, nb, whole, st, det = _logits_case()
    with BatchCoder(V, B, prec=prec, capacity_bits=_cap(N, prec), device=DEV) as c:
        assert int(nb.min()) > 8 * c.bits_stride()
        c.set_q1_step(mode)
        c.decode_open_window(bits, nb)
        out = torch.empty((T, B), dtype=torch.int32, device=DEV)
        for t in range(T):
            c.decode_logits_step(lg[t], out[t:t + 1])
            if (t + 1) % N == 0:
                c.refill()
        c.refill()
        assert c.status()[0] == 0
        assert np.array_equal(out.cpu().numpy(), whole)
        _same_states(_absolute(_state(c), c.window_base()), st)
        assert np.array_equal(c.determined(), det)


def test_logits_compressor_decompresses_through_a_window():
    from lac_amd.llm import LogitsCompressor, TinyCausalLM
    V, B, T, N = 512, 2, 100, 16
    model = TinyCausalLM(vocab=V, max_len=128, seed=3, d=32, layers=1, heads=2).to(DEV).eval()
    tokens = torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(4))
    lengths = np.array([T, 37])
    lc = LogitsCompressor(model, V, prec=48, device=DEV, drain_every=N)
    data, nbits = lc.compress(tokens, lengths=lengths)
    plain = LogitsCompressor(model, V, prec=48, device=DEV)
    strides = []
    for comp in (lc, plain):
        make = comp._coder

        def recording(*a, _make=make, **k):
            coder = _make(*a, **k)
            strides.append(coder.bits_stride())
            return coder

        comp._coder = recording
    got = lc.decompress(data, nbits, T, lengths=lengths).cpu()
    want = plain.decompress(data, nbits, T, lengths=lengths).cpu()
    assert torch.equal(got, want)
    assert torch.equal(got[0], tokens[0]) and torch.equal(got[1, :37], tokens[1, :37]) and bool((got[1, 37:] == -1).all())
    n_words = (N * (48 + 2) + 256 + lc.DRAIN_KEEP_BITS + 63) // 64 + 1
    t_words = (T * (48 + 2) + 256 + 63) // 64 + 1
    assert strides == [8 * n_words, 8 * t_words] and n_words < t_words
    assert int(np.asarray(nbits).max()) > 0
