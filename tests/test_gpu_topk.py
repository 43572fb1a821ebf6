"""Top-k rows straight from logits on the device (include/lac.h lac_topk_logits,
BatchCoder.topk_logits / set_topk_form, lac_amd.sparse.topk_rows_q1, TopKCompressor(rule="q1")).

The yardstick is Python integers on the C oracle's q1 tables (topk.yardstick: lexsort by
(-g, symbol), take k, sort by symbol, shift), compared element for element including pads; both
kernel forms are forced at small shapes, the seams of their layout come from lac_topk.h through the
native library, and the end-to-end checks hold the coded bytes to the pmf path on the yardstick's
dense rows and to the C oracle.  Integer work: everything is compared bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import topk as TK
from oracle import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LAC_OK, LAC_E_ARG = 0, -1
SENT_I, SENT_W = -77, 0x5EAD5EAD
FORMS = (TK.FORM_REGS, TK.FORM_STREAM)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _coder(V, B, prec=48, form=TK.FORM_AUTO, **kw):
    from lac_amd.batch import BatchCoder
    c = BatchCoder(V, B, prec=prec, capacity_bits=kw.pop("cap", 4096), device=DEV, **kw)
    c.set_topk_form(form)
    return c


def _dev(rows):
    """typed rows (uint16 bf16 bit patterns or float32) -> the device tensor a call takes"""
    t = torch.from_numpy(np.ascontiguousarray(rows).view(np.int16) if rows.dtype == np.uint16 else np.ascontiguousarray(rows))
    return (t.view(torch.bfloat16) if rows.dtype == np.uint16 else t).to(DEV)


def _host(idx, wt):
    return idx.cpu().numpy(), wt.cpu().numpy().view(np.uint32)


def _check(c, rows, k, wb, K=None):
    """rows [T, B, V] typed: the kernel's rows against the yardstick"""
    Kk = (k + 3) // 4 * 4 if K is None else K
    idx, wt = _host(*c.topk_logits(_dev(rows), k, wb, K))
    want_i, want_w = TK.yardstick(rows, k, wb, Kk)
    assert idx.shape == want_i.shape and idx.dtype == np.int32
    assert np.array_equal(idx, want_i), (k, wb, Kk, np.argwhere(idx != want_i)[:4])
    assert np.array_equal(wt, want_w), (k, wb, Kk, np.argwhere(wt != want_w)[:4])
    return idx, wt


def _batch(rng, T, B, V, tb, k):
    """[T, B, V] typed rows: the rows built to tie, a row with survivors only in its last vector,
    random rows for the rest"""
    rows = TK.random_rows(rng, T * B, V, spread=float(rng.choice((6.0, 30.0))))
    special = list(TK.special_rows(rng, V, k).values()) + [TK.last_vector_row(V, tb, k)[0]]
    for n, r in enumerate(special[:T * B - 2]):
        rows[n] = r
    return TK.as_type(rows.reshape(T, B, V), tb)


# ------------------------------------------------------------------ shapes, parameters, special rows
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tb", (2, 4))
@pytest.mark.parametrize("V", (8, 64, 520, 4104))
def test_both_forms_at_small_shapes(V, tb, form):
    rng = np.random.default_rng(100 * V + 10 * tb + form)
    T, B = 3, 4
    dtype = torch.bfloat16 if tb == 2 else torch.float32
    with _coder(V, B, form=form) as c:
        assert c.topk_form(dtype) == form
        for k in sorted({1, 3, min(64, V), min(256, V), V if V <= 64 else 1}):
            rows = _batch(rng, T, B, V, tb, k)
            for wb in (0, 16, 24):
                _check(c, rows, k, wb)
        _check(c, _batch(rng, T, B, V, tb, 5), 5, 24, 256)       # K = 256 with k = 5
        _check(c, _batch(rng, 1, B, V, tb, 1), 1, 24, 4)         # one step


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tb", (2, 4))
@pytest.mark.parametrize("V", (64, 520, 4104))
def test_tie_classes_across_every_seam(V, tb, form):
    """Thread, register-round, wave and tile seams of the forced form: a tie class with members on
    both sides, the cut exactly at the seam, one before it and one after it; survivors only in the
    last thread's last vector."""
    seen = 0
    with _coder(V, 1, form=form) as c:
        for seam in TK.seams(V, tb, form):
            for row, k in TK.seam_rows(V, seam):
                _check(c, TK.as_type(row[None, None], tb), k, 24, 256)
                seen += 1
        for k in (1, 3, 64):
            row, kk = TK.last_vector_row(V, tb, k)
            _check(c, TK.as_type(row[None, None], tb), kk, 24)
    assert seen >= 3
    if V == 4104:
        assert len(TK.seams(V, tb, form)) >= (3 if tb == 2 or form == TK.FORM_STREAM else 2)


@pytest.mark.parametrize("V,tb,form", ((32000, 2, TK.FORM_REGS), (128256, 2, TK.FORM_REGS), (128256, 4, TK.FORM_STREAM)))
def test_real_vocabularies_under_auto(V, tb, form):
    """One row each of a Llama-2 and a Llama-3 vocabulary: the form AUTO picks, the same rows under
    the other form where it can hold them, and the seams of the large layout."""
    from lac_amd._lib import LacError
    rng = np.random.default_rng(V + tb)
    dtype = torch.bfloat16 if tb == 2 else torch.float32
    with _coder(V, 1) as c:
        assert c.topk_form(dtype) == form == TK.plan(V, tb)[1]
        rows = TK.as_type(TK.random_rows(rng, 1, V)[None], tb)
        got = _check(c, rows, 64, 24)
        for seam in TK.seams(V, tb, TK.FORM_AUTO)[-2:]:          # the wave seam and, streamed, the tile seam
            row, k = TK.seam_rows(V, seam)[1]
            _check(c, TK.as_type(row[None, None], tb), k, 24)
        if form == TK.FORM_REGS:
            c.set_topk_form(TK.FORM_STREAM)
            assert c.topk_form(dtype) == TK.FORM_STREAM
            other = _host(*c.topk_logits(_dev(rows), 64, 24))
            assert np.array_equal(other[0], got[0]) and np.array_equal(other[1], got[1])
        else:
            c.set_topk_form(TK.FORM_REGS)                        # a forced form that cannot hold the row
            with pytest.raises(LacError) as e:
                c.topk_logits(_dev(rows), 64, 24)
            assert e.value.code == LAC_E_ARG


# ------------------------------------------------------------------ layout
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tb", (2, 4))
def test_strides_offsets_and_untouched_neighbours(tb, form):
    V, T, B, k, K = 520, 3, 4, 7, 8
    n = 16 // tb
    rng = np.random.default_rng(7 + tb)
    with _coder(V, B, form=form) as c:
        typ = TK.BF16 if tb == 2 else TK.F32

        def call(buf, off, ss, bs, want_rows):
            """lac_topk_logits on the flat typed buffer `buf` at element `off`, into sentinel-filled
            outputs one row longer on each side"""
            d = _dev(buf)
            oi = torch.full(((T * B + 2) * K,), SENT_I, dtype=torch.int32, device=DEV)
            ow = torch.full(((T * B + 2) * K,), SENT_W, dtype=torch.int32, device=DEV)
            rc = c.lib.lac_topk_logits(c.ctx, C.c_void_p(d.data_ptr() + off * tb), typ, ss, bs, T, k, 24, K,
                                       C.c_void_p(oi.data_ptr() + 4 * K), C.c_void_p(ow.data_ptr() + 4 * K), c._stream)
            assert rc == LAC_OK
            gi, gw = oi.cpu().numpy(), ow.cpu().numpy().view(np.uint32)
            assert (gi[:K] == SENT_I).all() and (gi[-K:] == SENT_I).all()
            assert (gw[:K] == SENT_W).all() and (gw[-K:] == SENT_W).all()
            want_i, want_w = TK.yardstick(want_rows, k, 24, K)
            assert np.array_equal(gi[K:-K].reshape(T, B, K), want_i) and np.array_equal(gw[K:-K].reshape(T, B, K), want_w)

        rows = TK.as_type(TK.random_rows(rng, T * B, V).reshape(T, B, V), tb)
        call(rows.reshape(-1), 0, B * V, V, rows)                                     # contiguous
        call(rows[0].reshape(-1), 0, 0, V, np.broadcast_to(rows[0], (T, B, V)))       # step_stride = 0
        call(rows[:, 0].reshape(-1), 0, V, 0, np.broadcast_to(rows[:, :1], (T, B, V)))   # stream_stride = 0
        call(rows[0, 0], 0, 0, 0, np.broadcast_to(rows[0, 0], (T, B, V)))             # one row for all
        # padded strides and a base 16 bytes into the buffer
        pad_b, pad_t = V + 3 * n, B * (V + 3 * n) + 5 * n
        buf = TK.as_type(TK.random_rows(rng, 1, n + T * pad_t)[0], tb)
        want = np.stack([np.stack([buf[n + t * pad_t + b * pad_b:][:V] for b in range(B)]) for t in range(T)])
        call(buf, n, pad_t, pad_b, want)


# ------------------------------------------------------------------ refusals
def test_refusals_launch_nothing_and_write_nothing():
    from lac_amd._lib import LacError
    V, T, B, k, K = 64, 2, 3, 8, 8
    rng = np.random.default_rng(3)
    rows = TK.as_type(TK.random_rows(rng, T * B, V).reshape(T, B, V), 2)
    rows32 = TK.as_type(TK.random_rows(rng, T * B, V).reshape(T, B, V), 4)
    d, d32 = _dev(rows), _dev(rows32)
    oi = torch.full((T * B * 256 + 8,), SENT_I, dtype=torch.int32, device=DEV)
    ow = torch.full((T * B * 256 + 8,), SENT_W, dtype=torch.int32, device=DEV)
    prof, cnt = (C.c_double * 8)(), (C.c_int64 * 8)()
    p = lambda x, off=0: C.c_void_p(x.data_ptr() + off)  # noqa: E731
    with _coder(V, B) as c:
        c.lib.lac_profile_enable(c.ctx, 1)
        c.lib.lac_profile_read(c.ctx, prof, cnt, 1)

        def call(lg=None, typ=TK.BF16, ss=B * V, bs=V, steps=T, k=k, wb=24, K=K, idx=None, wt=None, nul=()):
            a = [p(d) if lg is None else lg, typ, ss, bs, steps, k, wb, K, p(oi) if idx is None else idx,
                 p(ow) if wt is None else wt]
            for i in nul:
                a[i] = None
            return c.lib.lac_topk_logits(c.ctx, *a, c._stream)

        def untouched():
            torch.cuda.synchronize()
            c.lib.lac_profile_read(c.ctx, prof, cnt, 1)
            assert list(cnt) == [0] * 8
            assert bool((oi == SENT_I).all()) and bool((ow == SENT_W).all())

        for nul in ((0,), (8,), (9,)):                                  # NULL arrays with steps > 0
            assert call(nul=nul) == LAC_E_ARG
        for typ in (0, 3):
            assert call(typ=typ) == LAC_E_ARG
        assert call(lg=p(d, 2)) == LAC_E_ARG and call(lg=p(d, 8)) == LAC_E_ARG          # the layouts logits_check refuses
        assert call(ss=B * V + 4) == LAC_E_ARG and call(bs=V + 2) == LAC_E_ARG
        assert call(lg=p(d32), typ=TK.F32, bs=V + 2) == LAC_E_ARG
        for bad_k in (0, -1, V + 1, 257):
            assert call(k=bad_k, K=256) == LAC_E_ARG, bad_k
        for bad_K in (6, 4, 0, 260, 7, -8):                             # not a multiple of 4, below k, above 256
            assert call(K=bad_K) == LAC_E_ARG, bad_K
        for bad_wb in (-1, 25, 32):
            assert call(wb=bad_wb) == LAC_E_ARG, bad_wb
        assert call(idx=p(oi, 4)) == LAC_E_ARG and call(wt=p(ow, 8)) == LAC_E_ARG      # outputs off 16 bytes
        assert call(steps=-1) == LAC_E_ARG and call(ss=-8) == LAC_E_ARG and call(bs=-8) == LAC_E_ARG
        assert call(steps=0) == LAC_OK and call(steps=0, nul=(0, 8, 9)) == LAC_OK      # no launch
        assert call(steps=0, k=0) == LAC_E_ARG
        untouched()
        assert c.lib.lac_set_option(c.ctx, 11, 3) == LAC_E_ARG and c.lib.lac_set_option(c.ctx, 11, -1) == LAC_E_ARG
        # the Python layer
        for bad in (dict(k=0), dict(k=V + 1), dict(k=8, K=6), dict(k=8, weight_bits=25)):
            with pytest.raises(LacError) as e:
                c.topk_logits(d, **bad)
            assert e.value.code == LAC_E_ARG
        with pytest.raises(TypeError):
            c.topk_logits(d.to(torch.float16), 8)
        with pytest.raises(ValueError):
            c.topk_logits(d, 8, out=(oi[:T * B * 8].view(T, B, 8), ow[:T * B * 4].view(T, B, 4)))
        untouched()
        # it touches no stream state, works while decoding and under any mapping / termination, ignores counts,
        # and is one launch in slot 6 whatever the steps
        c.reset()
        ck = c.checkpoint()
        c.set_mapping("floor")
        c.set_termination("acsampler")
        c.set_stream_lengths([0, 1, 0])
        want = TK.yardstick(rows, k, 24, K)
        got = _host(*c.topk_logits(d, k))
        c.lib.lac_profile_read(c.ctx, prof, cnt, 1)
        assert list(cnt) == [0, 0, 0, 0, 0, 0, 1, 0]
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        after = c.checkpoint()
        for f in ck["state"].dtype.names:
            assert np.array_equal(ck["state"][f], after["state"][f]), f
        c.set_stream_lengths(None)
        out = (oi[:T * B * K].view(T, B, K), ow[:T * B * K].view(T, B, K))
        ri, rw = c.topk_logits(d32, k, out=out)
        assert ri.data_ptr() == oi.data_ptr() and np.array_equal(_host(ri, rw)[0], TK.yardstick(rows32, k, 24, K)[0])


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize("V,tb,k,wb,base", ((64, 2, 8, 24, 1), (520, 4, 64, 16, 3), (520, 2, 5, 24, 1)))
def test_coded_bytes_equal_the_pmf_path_and_the_oracle_on_the_yardstick_rows(V, tb, k, wb, base):
    from lac_amd.sparse import dense_rows, topk_rows_q1
    T, B, prec = 12, 3, 48
    K = (k + 3) // 4 * 4
    rng = np.random.default_rng(V + k)
    rows = TK.as_type(TK.random_rows(rng, T * B, V, spread=8.0).reshape(T, B, V), tb)
    rows[2, 1] = TK.as_type(np.full(V, 1.5, dtype=np.float32), tb)                      # an all-tie row among them
    want_i, want_w = TK.yardstick(rows, k, wb, K)
    sym = rng.integers(0, V, size=(T, B)).astype(np.int32)
    sym[::2] = np.take_along_axis(want_i[::2], rng.integers(0, k, size=(T, B, 1))[::2], -1)[..., 0]   # at a pair, too
    ds = torch.from_numpy(sym).to(DEV)
    a = _coder(V, B, prec, pmf_bits=64, cap=T * (prec + 2) + 256)
    p = _coder(V, B, prec, pmf_bits=64, cap=T * (prec + 2) + 256)
    try:
        idx, wt, b = topk_rows_q1(a, _dev(rows), k, wb, base)
        assert b == base and np.array_equal(idx.cpu().numpy(), want_i)
        a.encode_sparse_job(idx, wt, base, ds)
        dense = dense_rows(want_i, want_w, base, V)                                      # the yardstick's rows
        p.encode_job(torch.from_numpy(dense.view(np.int64)).to(DEV), ds)
        da, na = a.to_bytes()
        dp, npp = p.to_bytes()
        assert da == dp and np.array_equal(np.asarray(na, dtype=np.uint64), np.asarray(npp, dtype=np.uint64))
        for s in range(B):
            data, nbits, _ = oracle.encode(dense[:, s], sym[:, s].tolist(), prec)
            assert da[s] == data and int(na[s]) == nbits
        a.decode_open()
        assert np.array_equal(a.decode_sparse(idx, wt, base).cpu().numpy(), sym)
        with pytest.raises(ValueError):                                                  # rows that could fudge are refused
            topk_rows_q1(a, _dev(rows), k, 24, base=(1 << (prec - 1)) // V)
    finally:
        a.close()
        p.close()


def test_topk_compressor_rules():
    """rule="q1" round-trips with TinyCausalLM at B = 3, T = 20 and codes the rows topk_logits gives;
    rule="float" is byte-identical to a TopKCompressor built without the argument."""
    from lac_amd.llm import TinyCausalLM
    from lac_amd.sparse import TopKCompressor, dense_rows
    V, k, B, T = 1000, 20, 3, 20
    model = TinyCausalLM(vocab=V, d=32, layers=1, heads=2, max_len=64, seed=3)
    tokens = torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(5))
    comp = TopKCompressor(model, V, k, device=DEV, rule="q1")
    data, nbits = comp.compress(tokens)
    assert torch.equal(comp.decompress(data, nbits, T).cpu(), tokens)
    idx, wt, base = comp.rows(tokens)
    assert idx.shape == (T, B, k) and idx.dtype == torch.int32 and wt.dtype == torch.int32 and base == 1
    assert bool((idx[..., 1:] > idx[..., :-1]).all()) and int(wt.max()) == 1 << 24
    p = _coder(V, B, comp.prec, pmf_bits=64, cap=T * (comp.prec + 2) + 256)
    p.encode_job(dense_rows(idx, wt, base, V), tokens.t().contiguous().to(torch.int32).to(DEV))
    want, nb = p.to_bytes()
    p.close()
    assert data == want and np.array_equal(np.asarray(nbits, dtype=np.uint64), np.asarray(nb, dtype=np.uint64))
    plain = TopKCompressor(model, V, k, device=DEV).compress(tokens)
    named = TopKCompressor(model, V, k, device=DEV, rule="float").compress(tokens)
    assert plain[0] == named[0] and np.array_equal(np.asarray(plain[1]), np.asarray(named[1]))
    with pytest.raises(ValueError):
        TopKCompressor(model, V, k, device=DEV, rule="exact")
    with pytest.raises(ValueError):
        TopKCompressor(model, V, k, weight_bits=25, prec=60, device=DEV, rule="q1")
