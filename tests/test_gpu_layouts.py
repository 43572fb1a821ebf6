"""The pmf kernels on strided, padded, offset and broadcast tables (tests/layouts.py).

The C ABI takes a base pointer and two element strides (include/lac.h); every kernel does
its own address arithmetic, and the library picks the 16-byte-vector or the scalar family
by the base's alignment and the strides (encode_dispatch, decode_plan).  On a contiguous
[T, B, V] tensor b*stream_stride, b*V and (t*B + b)*V - t*step_stride coincide, and so do
row + step_stride and row + B*V; here they do not, and everything around the rows is
poison.  Expected bytes, bit counts and symbols are the C oracle's on the view's
materialised values -- never the GPU's own output on another layout.  All exact.

    case  dtype  V     B    T   prec  reaches
    A     u32    1000  5    70  40    lean step with helpers; few-stream per-step form; ragged last
                                      iteration of a row
    B     u32    1000  70   20  24    fudged rows: k_encode re-reads the row, decode_fudged;
                                      k_decode_seq without lean
    C     u64    512   6    12  48    llama64 rows, fudged at prec 48; VEC = 2
    D     u32    64    512  70  40    64-step launch chunks (t0 > 0) of the split encode and the stats
                                      decode; many-stream per-step form
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"

from layouts import LAYOUTS, layout_view

#        V, B, T, prec, synth kind, exp_range, seed
CASES = {"A": (1000, 5, 70, 40, "loguniform", 16, 101),
         "B": (1000, 70, 20, 24, "loguniform", 24, 102),
         "C": (512, 6, 12, 48, "llama64", 24, 103),
         "D": (64, 512, 70, 40, "loguniform", 16, 104)}
ENCODE_PATHS = ("split", "fused", "auto")
# decode path, block waves
DECODE_FORMS = (("split", 0), ("fused", 0), ("fused_chunk", 0), ("stats", 0), ("block", 4), ("block", 8),
                ("block", 16))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _materialised(pmf, layout):
    """The values a layout's view holds (layouts.py: the broadcasts hold one step / stream)."""
    if layout == "step_bcast":
        return np.ascontiguousarray(np.broadcast_to(pmf[:1], pmf.shape))
    if layout == "stream_bcast":
        return np.ascontiguousarray(np.broadcast_to(pmf[:, :1], pmf.shape))
    return pmf


@functools.lru_cache(maxsize=None)
def _tables(case):
    from lac_amd import synth
    V, B, T, prec, kind, er, seed = CASES[case]
    pmf, sym = synth.make_batch(seed, T, B, V, kind, er, sym_mode="uniform")   # every entry > 0: any symbol codes
    tot = pmf.astype(object).sum(axis=-1) if pmf.dtype == np.uint64 else pmf.sum(axis=-1, dtype=np.uint64)
    minp = pmf.min(axis=-1)
    # the coder's width stays in (2^(prec-2), 2^prec]: what the case is meant to reach
    if case in ("A", "D"):          # the lean step: totals below 2^32, never fudged (T <= w * minp)
        assert int(tot.max()) < 1 << 32 and (tot <= (1 << (prec - 2)) * minp.astype(np.uint64)).all()
    if case == "B":                 # every row fudged, whatever the width
        assert (tot > (1 << prec) * minp.astype(np.uint64)).all()
    if case == "C":                 # most rows fudged (those with a hot entry)
        assert sum(int(t) > (int(m) << prec) for t, m in zip(tot.ravel(), minp.ravel())) > T * B // 2
    pmf.setflags(write=False)
    sym.setflags(write=False)
    return pmf, sym


@functools.lru_cache(maxsize=None)
def _expected(case, kind):
    """-> (per-stream bytes, bit counts) of the oracle on the materialised values of the
    full table ('full') or of a broadcast; computed once and shared."""
    from oracle import oracle
    pmf, sym = _tables(case)
    prec = CASES[case][3]
    out, nb, status, rc = oracle.encode_batch(_materialised(pmf, kind), sym, prec, nthreads=8)
    assert rc == 0 and not status.any()
    return [out[b, :(int(nb[b]) + 7) // 8].tobytes() for b in range(pmf.shape[1])], nb


def _want(case, layout):
    return _expected(case, layout if layout in ("step_bcast", "stream_bcast") else "full")


def _coder(case):
    from lac_amd.batch import BatchCoder
    V, B, T, prec = CASES[case][:4]
    return BatchCoder(V, B, prec=prec, pmf_bits=64 if case == "C" else 32, capacity_bits=T * (prec + 34) + 256,
                      device=DEV)


def _cuts(T):
    a, b = (1, 65) if T > 65 else (1, T - 1)
    return (0, a), (a, b), (b, T)


def _clean(c):
    rc, err, _ = c.status()
    assert rc == 0 and not err.any(), (rc, err)


def _check_bytes(c, want, what):
    _clean(c)
    got, gbits = c.to_bytes()
    assert (gbits == want[1]).all(), (what, gbits, want[1])
    assert got == want[0], what


def _set_decode(c, path, waves):
    c.set_decode_path(path)
    c.set_block_waves(waves)


def _oracle_bits(want, B):
    """Decode the oracle's bytes, not the encoder's own."""
    data, nb = want
    stride = (max(len(d) for d in data) + 7) // 8 * 8 + 8
    buf = np.zeros((B, stride), dtype=np.uint8)
    for b, d in enumerate(data):
        buf[b, :len(d)] = np.frombuffer(d, dtype=np.uint8)
    return torch.from_numpy(buf).to(DEV), torch.from_numpy(nb.astype(np.int64)).to(DEV)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", list(CASES))
def test_encode_bytes_on_layout(case, layout):
    """Every encode path, as one job and as three incremental calls over slices of the view."""
    pmf, sym = _tables(case)
    T = pmf.shape[0]
    view = layout_view(pmf, DEV, layout)
    ds = torch.from_numpy(sym.copy()).to(DEV)
    want = _want(case, layout)
    c = _coder(case)
    for path in ENCODE_PATHS:
        c.set_path(path)
        c.encode_job(view, ds)
        _check_bytes(c, want, (path, "job"))
        c.reset()
        for a, b in _cuts(T):
            c.encode(view[a:b], ds[a:b])
        c.finish()
        _check_bytes(c, want, (path, "slices"))
    c.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", list(CASES))
def test_decode_symbols_on_layout(case, layout):
    """Every decode path on the oracle's bits, in one call and in three; determined() agrees."""
    pmf, sym = _tables(case)
    T, B, _ = pmf.shape
    view = layout_view(pmf, DEV, layout)
    bits, nbits = _oracle_bits(_want(case, layout), B)
    c = _coder(case)
    det = None
    for path, waves in DECODE_FORMS:
        _set_decode(c, path, waves)
        for cuts in (((0, T),), _cuts(T)):
            c.decode_open(bits, nbits)
            out = torch.cat([c.decode(view[a:b]) for a, b in cuts]).cpu().numpy()
            _clean(c)
            assert np.array_equal(out, sym), (path, waves, len(cuts), np.argwhere(out != sym)[:4])
            d = c.determined()
            det = d if det is None else det
            assert (d == det).all() and (d <= T).all(), (path, waves, len(cuts))
    c.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", ["A", "C"])
def test_decode_one_step_per_call_on_layout(case, layout):
    pmf, sym = _tables(case)
    T, B, _ = pmf.shape
    view = layout_view(pmf, DEV, layout)
    bits, nbits = _oracle_bits(_want(case, layout), B)
    c = _coder(case)
    for path in ("auto", "stats"):
        c.set_decode_path(path)
        c.decode_open(bits, nbits)
        out = torch.cat([c.decode(view[t:t + 1]) for t in range(T)]).cpu().numpy()
        _clean(c)
        assert np.array_equal(out, sym), (path, np.argwhere(out != sym)[:4])
    c.close()


@pytest.mark.parametrize("case", ["A", "C"])
def test_vector_and_scalar_families_mixed_in_one_stream(case):
    """The coder state handed between the families mid-stream: encode's three calls take
    their slices from a contig (vector), an offset_1 (scalar) and a pad_vec (vector) view
    of the same values, decode's from pad_odd (scalar), transposed and contig (vector) --
    at case A lean -> scalar k_decode_seq -> lean."""
    pmf, sym = _tables(case)
    T, B, _ = pmf.shape
    views = {n: layout_view(pmf, DEV, n) for n in ("contig", "offset_1", "pad_vec", "pad_odd", "transposed")}
    ds = torch.from_numpy(sym.copy()).to(DEV)
    want = _want(case, "contig")
    cuts = _cuts(T)
    c = _coder(case)
    for path in ENCODE_PATHS:
        c.set_path(path)
        c.reset()
        for (a, b), n in zip(cuts, ("contig", "offset_1", "pad_vec")):
            c.encode(views[n][a:b], ds[a:b])
        c.finish()
        _check_bytes(c, want, path)
    for order in (("pad_odd", "transposed", "contig"), ("contig", "pad_odd", "transposed")):
        for path, waves in DECODE_FORMS:
            _set_decode(c, path, waves)
            c.decode_open()
            out = torch.cat([c.decode(views[n][a:b]) for (a, b), n in zip(cuts, order)]).cpu().numpy()
            _clean(c)
            assert np.array_equal(out, sym), (order, path, waves)
    c.close()


def test_lean_launch_groups_on_a_transposed_table():
    """u32 V = 32768, 33 streams, 66 steps: the 512 MB lean buffer takes 64 steps of these
    rows per launch group (lac_select.h decode_plan), so the second group starts at t0 = 64
    with 2 steps.  The table is generated as [B, T, V] and coded transposed (step_stride <
    stream_stride).  The bytes of 4 streams are the oracle's; both decode paths return the
    symbols."""
    from lac_amd import synth
    from lac_amd.batch import BatchCoder
    from oracle import oracle
    V, B, T, prec = 32768, 33, 66, 48
    store, sym_bt = synth.softmax_tables(B, T, V, seed=41, device=DEV)       # "steps" = streams here
    view, sym = store.transpose(0, 1), sym_bt.transpose(0, 1).contiguous()
    assert view.stride(0) == V and view.stride(1) == T * V
    c = BatchCoder(V, B, prec=prec, capacity_bits=T * (prec + 2) + 256, device=DEV)
    c.encode_job(view, sym)
    _clean(c)
    data, nb = c.to_bytes()
    hs = sym.cpu().numpy()
    for b in (0, 13, 31, 32):
        rows = store[b].cpu().numpy().view(np.uint32)
        wd, wl, _ = oracle.encode(rows, hs[:, b], prec)
        assert int(nb[b]) == wl and data[b] == wd, b
    for path in ("stats", "fused"):
        c.set_decode_path(path)
        c.decode_open()
        out = c.decode(view)
        _clean(c)
        assert torch.equal(out, sym), path
    c.close()


# ---- per-stream counts (lac_set_stream_lengths) on a layout; counts as tests/test_gpu_ragged.py
COUNTS = [0, 1, 63, 64, 65, 128, 130, 1000]


@functools.lru_cache(maxsize=None)
def _ragged():
    """Case A with counts: dead rows all zero (LAC_E_TABLE if consumed), dead symbols -1
    (LAC_E_SYMBOL_RANGE if consumed); expected bytes per stream from the oracle over the
    stream's live prefix alone."""
    from oracle import oracle
    pmf, sym = _tables("A")
    T, B, _ = pmf.shape
    prec = CASES["A"][3]
    pmf, sym = pmf.copy(), sym.copy()
    cnt = np.array([COUNTS[b % len(COUNTS)] for b in range(B)], dtype=np.int64)     # 0, 1, 63, 64, 65 of T = 70
    live = np.minimum(cnt, T)
    want, wbits = [], []
    for b in range(B):
        n = int(live[b])
        data, L, _ = oracle.encode(pmf[:max(n, 1), b], sym[:n, b], prec)
        want.append(data)
        wbits.append(L)
        sym[n:, b] = -1
        pmf[n:, b, :] = 0
    return pmf, sym, cnt, want, np.array(wbits, dtype=np.uint64)


@pytest.mark.parametrize("layout", ["transposed", "pad_odd"])
def test_ragged_counts_on_layout(layout):
    pmf, sym, cnt, want, wbits = _ragged()
    view = layout_view(pmf, DEV, layout)
    ds = torch.from_numpy(sym.copy()).to(DEV)
    c = _coder("A")
    c.set_stream_lengths(cnt)
    for enc in ENCODE_PATHS:
        c.set_path(enc)
        c.encode_job(view, ds)
        _check_bytes(c, (want, wbits), enc)
        for path, waves in DECODE_FORMS + (("auto", 0),):
            _set_decode(c, path, waves)
            c.decode_open()
            out = c.decode(view).cpu().numpy()
            _clean(c)
            assert np.array_equal(out, sym), (enc, path, waves)
    c.close()
