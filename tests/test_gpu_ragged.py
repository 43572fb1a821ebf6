"""Streams of different lengths in one batch (lac_set_stream_lengths, include/lac.h):
stream b codes only its first len[b] symbols, every later step is a no-op for it.

The expected bits of stream b are the C oracle's for that stream alone, over its first
len[b] rows; the expected decode is its symbols, then -1.  Everything dead is poisoned so
that a kernel consuming it cannot pass: dead integer rows are all zero (LAC_E_TABLE if
consumed), dead symbols are -1 (LAC_E_SYMBOL_RANGE if consumed).  T = 130 crosses the
64-step straight block and, at 70 streams, nothing else; the counts sit on both sides of
64 and 128, at 0, at T and past it."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 130
COUNTS = [0, 1, 63, 64, 65, 128, 130, 1000]
DECODE_PATHS = ("auto", "split", "fused", "fused_chunk", "stats", "block")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _counts(B):
    return np.array([COUNTS[b % len(COUNTS)] for b in range(B)], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _case(kind, B, prec):
    """-> (pmf [T, B, V] or [V], sym [T, B] with -1 where dead, counts, live lengths,
    expected bytes per stream, expected bit counts), computed once and shared."""
    from oracle import oracle
    rng = np.random.default_rng(zlib.crc32(f"{kind}/{B}/{prec}".encode()))
    cnt = _counts(B)
    live = np.minimum(cnt, T)
    if kind == "u64_512":
        V = 512
        pmf = rng.integers(1 << 50, 1 << 51, size=(T, B, V), dtype=np.uint64)      # totals near 2^60
    elif kind == "static":
        V = 1000
        pmf = rng.integers(1, 5000, size=(V,)).astype(np.uint32)
    else:
        V = 999 if kind == "u32_999" else 1000
        pmf = rng.integers(1, 1000, size=(T, B, V)).astype(np.uint32)
        if kind == "fudge":
            # a fudging row (T = 2^31 with minp 1: T > w * minp at prec <= 31) before the end
            # of the streams with counts 63 .. 1000, the construction of
            # test_gpu_lean.test_lean_hands_over_mid_stream
            for b in range(B):
                if live[b] > 40:
                    pmf[40, b, :] = (1 << 31) // V + 1
                    pmf[40, b, 5] = 1
    sym = rng.integers(0, V, size=(T, B)).astype(np.int32)
    want, wbits = [], []
    for b in range(B):
        n = int(live[b])
        if kind == "static":
            data, L, _ = oracle.encode(pmf, sym[:n, b], prec, static=True)
        else:
            data, L, _ = oracle.encode(pmf[:max(n, 1), b], sym[:n, b], prec)
        want.append(data)
        wbits.append(L)
        sym[n:, b] = -1                                         # poison
        if kind != "static":
            pmf[n:, b, :] = 0
    return pmf, sym, cnt, live, want, np.array(wbits, dtype=np.uint64)


def _device_tables(pmf, B):
    it = np.int32 if pmf.dtype == np.uint32 else np.int64
    d = torch.from_numpy(np.ascontiguousarray(pmf).view(it)).to(DEV)
    if d.dim() == 1:
        d = d.view(1, 1, -1).expand(T, B, -1)                   # a static model: strides 0
    return d


def _coder(V, B, prec, bits):
    from lac_amd.batch import BatchCoder
    return BatchCoder(V, B, prec=prec, pmf_bits=bits, capacity_bits=T * (prec + 34) + 256, device=DEV)


def _clean(c):
    rc, err, _ = c.status()
    assert rc == 0 and not err.any(), (rc, err)


def _expected_out(sym):
    return sym                                                  # the live symbols, -1 past each count


CASES = [(k, B, p) for k in ("u32_1000", "u32_999", "u64_512") for B in (5, 70) for p in (24, 40, 48)]
CASES += [("static", 5, 40), ("static", 70, 24), ("fudge", 5, 24), ("fudge", 70, 24), ("fudge", 5, 48)]


@pytest.mark.parametrize("kind,B,prec", CASES)
def test_ragged_job_matches_oracle_on_every_path(kind, B, prec):
    pmf, sym, cnt, live, want, wbits = _case(kind, B, prec)
    V = pmf.shape[-1]
    dp, ds = _device_tables(pmf, B), torch.from_numpy(sym).to(DEV)
    c = _coder(V, B, prec, 64 if pmf.dtype == np.uint64 else 32)
    c.set_stream_lengths(cnt)
    for enc in ("split", "fused"):
        c.set_path(enc)
        trace = torch.full((T, B, 2), -7, dtype=torch.int64, device=DEV)
        c.encode_job(dp, ds, trace=trace)
        _clean(c)
        got, gbits = c.to_bytes()
        assert (gbits == wbits).all(), (enc, gbits, wbits)
        assert got == want, enc
        tr = trace.cpu().numpy()
        for b in range(B):                                      # no trace entry of a dead step is written
            assert (tr[live[b]:, b] == -7).all(), (enc, b)
            assert (tr[:live[b], b, 1] >= 0).all(), (enc, b)
        for path in DECODE_PATHS:
            c.set_decode_path(path)
            c.decode_open()                                     # counts persist: set once
            out = c.decode(dp).cpu().numpy()
            _clean(c)
            assert np.array_equal(out, _expected_out(sym)), (enc, path)
    c.close()


def test_ragged_job_across_launch_chunks():
    """From 512 streams the split encode and the stats decode launch 64 steps at a time:
    T = 130 is three launch chunks, and a row of a later chunk is live iff the symbols
    its stream has coded (read at the chunk's start) plus its index stay below the count."""
    B, prec = 514, 40
    pmf, sym, cnt, live, want, wbits = _case("u32_1000", B, prec)
    dp, ds = _device_tables(pmf, B), torch.from_numpy(sym).to(DEV)
    c = _coder(1000, B, prec, 32)
    c.set_stream_lengths(cnt)
    c.set_path("split")
    c.encode_job(dp, ds)
    _clean(c)
    got, gbits = c.to_bytes()
    assert (gbits == wbits).all() and got == want
    for path in ("stats", "block", "auto"):
        c.set_decode_path(path)
        c.decode_open()
        out = c.decode(dp).cpu().numpy()
        _clean(c)
        assert np.array_equal(out, sym), path
    c.close()


def test_counts_with_decode_stop_on_a_truncated_stream():
    """Counts and LAC_OPT_DECODE_STOP: a stream stops at whichever comes first.  Stream 6
    (count 130) gets half its bits: it ends LAC_E_UNDETERMINED before its count; the
    others end clean at theirs."""
    from lac_amd import _lib
    kind, B, prec = "u32_1000", 8, 40
    pmf, sym, cnt, live, want, wbits = _case(kind, B, prec)
    dp, ds = _device_tables(pmf, B), torch.from_numpy(sym).to(DEV)
    c = _coder(1000, B, prec, 32)
    c.set_stream_lengths(cnt)
    c.encode_job(dp, ds)
    bits, nb = c.bits_tensor(), c.nbits_tensor()
    assert int(nb[6]) == int(wbits[6]) > 200
    nb[6] = nb[6] // 2
    c.set_decode_stop(True)
    c.decode_open(bits, nb)
    out = c.decode(dp).cpu().numpy()
    rc, err, _ = c.status()
    assert err[6] == _lib.LAC_E_UNDETERMINED and not np.delete(err, 6).any(), err
    ok = np.delete(np.arange(B), 6)
    assert np.array_equal(out[:, ok], sym[:, ok])
    n6 = int((out[:, 6] >= 0).sum())
    assert 0 < n6 < live[6] and np.array_equal(out[:n6, 6], sym[:n6, 6]) and (out[n6:, 6] == -1).all()
    c.close()


@pytest.mark.parametrize("B,enc", [(5, "split"), (70, "split"), (70, "fused")])
def test_incremental_calls_count_symbols_not_steps(B, enc):
    """The base of a count is the symbols coded, not the step index of a call: encode in
    calls of 50 + 80 steps equals the job, decode in two calls equals one."""
    pmf, sym, cnt, live, want, wbits = _case("u32_1000", B, 40)
    dp, ds = _device_tables(pmf, B), torch.from_numpy(sym).to(DEV)
    c = _coder(1000, B, 40, 32)
    c.set_path(enc)
    c.set_stream_lengths(torch.from_numpy(cnt))                 # a tensor is accepted too
    c.reset()
    c.encode(dp[:50], ds[:50])
    c.encode(dp[50:], ds[50:])
    c.finish()
    _clean(c)
    got, gbits = c.to_bytes()
    assert got == want and (gbits == wbits).all()
    for path in ("stats", "fused", "block", "split"):
        c.set_decode_path(path)
        c.decode_open()
        out = torch.cat([c.decode(dp[:50]), c.decode(dp[50:])]).cpu().numpy()
        _clean(c)
        assert np.array_equal(out, sym), path
    c.close()


@pytest.mark.parametrize("B", [5, 70])
def test_clearing_counts_restores_rectangular_jobs(B):
    """set_stream_lengths(None) after a ragged job: a rectangular job gives a fresh coder's
    bits, and decodes in full."""
    pmf, sym, cnt, *_ = _case("u32_1000", B, 40)
    rng = np.random.default_rng(5)
    full = rng.integers(1, 1000, size=(T, B, 1000)).astype(np.uint32)
    fsym = rng.integers(0, 1000, size=(T, B)).astype(np.int32)
    dfull, dfs = _device_tables(full, B), torch.from_numpy(fsym).to(DEV)
    fresh = _coder(1000, B, 40, 32)
    fresh.encode_job(dfull, dfs)
    want = fresh.to_bytes()
    fresh.close()
    c = _coder(1000, B, 40, 32)
    c.set_stream_lengths(list(cnt))                             # a plain sequence is accepted
    c.encode_job(_device_tables(pmf, B), torch.from_numpy(sym).to(DEV))
    _clean(c)
    c.set_stream_lengths(None)
    c.encode_job(dfull, dfs)
    got = c.to_bytes()
    assert got[0] == want[0] and (got[1] == want[1]).all()
    for path in ("auto", "fused"):
        c.set_decode_path(path)
        c.decode_open()
        assert np.array_equal(c.decode(dfull).cpu().numpy(), fsym), path
    c.close()


def test_set_stream_lengths_validates_on_the_host():
    c = _coder(1000, 5, 40, 32)
    with pytest.raises(ValueError):
        c.set_stream_lengths([1, 2, 3])
    with pytest.raises(ValueError):
        c.set_stream_lengths(np.zeros((5, 1), dtype=np.int64))
    with pytest.raises(ValueError):
        c.set_stream_lengths([1, 2, -1, 4, 5])
    with pytest.raises(TypeError):
        c.set_stream_lengths([1.5, 2, 3, 4, 5])
    c.set_stream_lengths(np.arange(5, dtype=np.int32))          # any integer dtype
    c.close()


def test_capi_tail_refuses_counts_and_null_clears():
    """lac_decode_tail_step returns LAC_E_STATE while counts are set; setting counts, then
    NULL, then decoding behaves as with none ever set."""
    from lac_amd import _lib
    B, prec = 5, 40
    rng = np.random.default_rng(9)
    full = rng.integers(1, 1000, size=(T, B, 1000)).astype(np.uint32)
    fsym = rng.integers(0, 1000, size=(T, B)).astype(np.int32)
    dp, ds = _device_tables(full, B), torch.from_numpy(fsym).to(DEV)
    c = _coder(1000, B, prec, 32)
    c.encode_job(dp, ds)
    c.decode_open()
    lib, st = c.lib, c._stream
    lens = torch.from_numpy(_counts(B)).to(DEV)
    assert lib.lac_set_stream_lengths(c.ctx, C.c_void_p(lens.data_ptr()), st) == 0
    so = torch.zeros(B, dtype=torch.int64, device=DEV)
    co = torch.zeros(B, dtype=torch.int32, device=DEV)
    args = (c.ctx, C.c_void_p(dp.data_ptr()), dp.stride(1), _lib.LAC_TAIL_DECIDE, C.c_void_p(so.data_ptr()),
            C.c_void_p(co.data_ptr()), st)
    assert lib.lac_decode_tail_step(*args) == _lib.LAC_E_STATE
    assert lib.lac_decode_tail_begin(c.ctx, st) == _lib.LAC_E_STATE
    assert lib.lac_set_stream_lengths(c.ctx, None, st) == 0
    c.decode_open()
    assert np.array_equal(c.decode(dp).cpu().numpy(), fsym)
    _clean(c)
    c.close()


# ------------------------------------------------------------------ container
def test_container_ragged_roundtrip():
    from lac_amd import container
    pmf, sym, cnt, live, want, wbits = _case("u32_1000", 5, 40)
    dp, ds = _device_tables(pmf, 5), torch.from_numpy(sym).to(DEV)
    c = _coder(1000, 5, 40, 32)
    blob = container.compress_batch(c, dp, ds, n_symbols=live)
    c.close()
    h = container.unpack(blob)
    assert h["n_symbols"] == [int(n) for n in live] and h["streams"] == want
    out, n = container.decompress_batch(blob, dp)
    assert n == [int(x) for x in live]
    assert np.array_equal(out.cpu().numpy(), sym[:int(live.max())])


def test_container_ragged_blob_from_oracle_bits_decodes_clean():
    """A short stream is not decoded past its end: its dead rows are all zero, which
    decoding max(n_symbols) steps for every stream would turn into LAC_E_TABLE."""
    from lac_amd import container
    pmf, sym, cnt, live, want, wbits = _case("u32_999", 5, 48)
    blob = container.pack(want, [int(n) for n in live], [int(x) for x in wbits], 48, 999)
    out, n = container.decompress_batch(blob, _device_tables(pmf, 5))
    assert np.array_equal(out.cpu().numpy(), sym[:int(live.max())])


def test_container_equal_lengths_decode_as_before():
    from lac_amd import container
    rng = np.random.default_rng(3)
    B, steps = 5, 20
    full = rng.integers(1, 1000, size=(steps, B, 1000)).astype(np.uint32)
    fsym = rng.integers(0, 1000, size=(steps, B)).astype(np.int32)
    dp, ds = torch.from_numpy(full.view(np.int32)).to(DEV), torch.from_numpy(fsym).to(DEV)
    c = _coder(1000, B, 40, 32)
    blob = container.compress_batch(c, dp, ds)
    c.close()
    assert container.unpack(blob)["n_symbols"] == [steps] * B
    out, n = container.decompress_batch(blob, dp)
    assert n == [steps] * B and np.array_equal(out.cpu().numpy(), fsym)
