"""The logits path on strided, padded, offset and broadcast logits (tests/layouts.py).

The row-statistics kernels do their own address arithmetic from the base pointer and the
two element strides, with LDS-DMA offsets hoisted out of their loops; around every row
lies +inf, so one logit read from outside a row changes its maximum and the whole table.
Expected tables are ``oracle.q1_quantize`` of the view's materialised bits, expected bytes
``oracle.encode_batch`` of those tables.  Layouts the path cannot take -- a misaligned base
or strides that are no multiple of a 16-byte vector -- are refused with LAC_E_ARG by all
four entry points (include/lac.h), and the context stays usable.

    dtype  V      B   T  prec
    bf16   32000  12  3  48     4000 vectors: AUTO shape 6, the single-block and tiled forms hold the
                                row, forced group shapes split it
    f32    65540  6   3  48     16385 vectors: AUTO shape 22; forced 19 / 20 / 21 / 23 split it into
                                real segments
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"

from layouts import layout_view

LAYOUTS = ("contig", "pad_vec", "step_pad", "transposed", "offset_vec", "step_bcast", "stream_bcast")
REFUSED = ("pad_odd", "offset_1")
SHAPES = {"bf16": (32000, 12, 3, 48, 6), "f32": (65540, 6, 3, 48, 3)}      # V, B, T, prec, fewest accepted shapes


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _logits(seed, steps, B, V, scale=3.0):
    """Normal logits with a few sharp peaks (LLM-like) and the special values of
    tests/test_gpu_logits.py (_logits(..., specials=True)), f32 host array."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((steps, B, V)) * scale).astype(np.float32)
    hot = rng.integers(0, V, size=(steps, B))
    np.put_along_axis(x, hot[..., None], np.float32(scale * 6), axis=2)
    x[0, 0, :3] = [np.nan, -np.inf, 1e30]
    x[0, 1, :] = -np.inf                                      # all -inf row: uniform table
    x[1, 0, 5] = np.inf                                       # +inf max: every other entry 1
    x[2, 0, 7] = 262143.5                                     # largest max of the GPU fast path
    x[2, 0, 9] = 262143.5 - 3.0
    x[2, B - 1, 3] = 3.0e5                                    # just past it: capped (slow) path
    x[2, B - 1, 4] = 3.0e5 - 0.25
    x[1, B - 1, 8] = np.float32(np.nan)                       # NaN in a normal row
    return x


def _sample(pmf, seed):
    """Symbols drawn from the tables themselves (inverse CDF), int32 [steps, B]."""
    rng = np.random.default_rng(seed)
    c = np.cumsum(pmf.astype(np.uint64), axis=-1)
    r = (rng.random(pmf.shape[:-1]) * c[..., -1]).astype(np.uint64)
    s = np.empty(pmf.shape[:-1], dtype=np.int32)
    for idx in np.ndindex(*pmf.shape[:-1]):
        s[idx] = np.searchsorted(c[idx], r[idx], side="right")
    return np.minimum(s, pmf.shape[-1] - 1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _inputs(dtype):
    """-> host logits [T, B, V] (f32, or bf16 bit patterns as uint16) and symbols."""
    from oracle import oracle
    V, B, T, prec, _ = SHAPES[dtype]
    x = _logits(V + B, T, B, V)
    if dtype == "bf16":
        x = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).copy()
    sym = _sample(oracle.q1_quantize(x, prec), V + 1)
    x.setflags(write=False)
    sym.setflags(write=False)
    return x, sym


@functools.lru_cache(maxsize=None)
def _expected(dtype, kind):
    """-> (q1 tables, per-stream bytes, bit counts) of the oracle on the materialised values
    of the full logits ('full') or of a broadcast; computed once and shared."""
    from oracle import oracle
    x, sym = _inputs(dtype)
    prec = SHAPES[dtype][3]
    if kind == "step_bcast":
        x = np.ascontiguousarray(np.broadcast_to(x[:1], x.shape))
    elif kind == "stream_bcast":
        x = np.ascontiguousarray(np.broadcast_to(x[:, :1], x.shape))
    pmf = oracle.q1_quantize(x, prec)
    out, nb, status, rc = oracle.encode_batch(pmf, sym, prec, nthreads=8)
    assert rc == 0 and not status.any()
    return pmf, [out[b, :(int(nb[b]) + 7) // 8].tobytes() for b in range(x.shape[1])], nb


def _want(dtype, layout):
    return _expected(dtype, layout if layout in ("step_bcast", "stream_bcast") else "full")


def _coder(dtype):
    from lac_amd.batch import BatchCoder
    V, B, T, prec, _ = SHAPES[dtype]
    return BatchCoder(V, B, prec=prec, pmf_bits=32, capacity_bits=T * (prec + 2) + 256, device=DEV)


def _check_bytes(c, want, what):
    rc, err, _ = c.status()
    assert rc == 0 and not err.any(), (what, rc, err)
    got, gbits = c.to_bytes()
    assert (gbits == want[2]).all(), (what, gbits, want[2])
    assert got == want[1], what


def _accepted(c, view, ds, want, what):
    """Run AUTO and every forced shape 1..23 on the view -> the set of shapes that took it;
    each of them gives the oracle's bytes and decodes to the symbols."""
    from lac_amd._lib import LacError, LAC_E_ARG
    took = set()
    for sh in range(0, 24):
        try:
            c.set_q1_shape(sh)                     # retired shapes are refused here
            c.encode_logits_job(view, ds)          # and shapes that cannot hold the row here
        except LacError as e:
            assert e.code == LAC_E_ARG, (what, sh)
            continue
        _check_bytes(c, want, (what, sh))
        c.decode_open()
        assert torch.equal(c.decode_logits(view), ds), (what, sh)
        rc, err, _ = c.status()
        assert rc == 0 and not err.any(), (what, sh)
        took.add(sh)
    c.set_q1_shape(0)
    return took


@functools.lru_cache(maxsize=None)
def _contig_accepts(dtype):
    """The shapes that take the contiguous tensor: what holds the row depends on V and the
    type alone (q1_plan), so every accepted layout must be taken by exactly these."""
    x, sym = _inputs(dtype)
    c = _coder(dtype)
    took = _accepted(c, layout_view(x, DEV, "contig"), torch.from_numpy(sym.copy()).to(DEV), _want(dtype, "contig"),
                     "contig")
    c.close()
    assert 0 in took and len(took - {0}) >= SHAPES[dtype][4], took
    return frozenset(took)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", list(SHAPES))
def test_logits_on_layout(dtype, layout):
    x, sym = _inputs(dtype)
    T = x.shape[0]
    want = _want(dtype, layout)
    view = layout_view(x, DEV, layout)
    ds = torch.from_numpy(sym.copy()).to(DEV)
    c = _coder(dtype)
    got_pmf = c.quantize_logits(view).cpu().numpy().view(np.uint32)
    assert np.array_equal(got_pmf, want[0]), np.argwhere(got_pmf != want[0])[:4]
    took = _accepted(c, view, ds, want, layout)
    assert took == _contig_accepts(dtype), (sorted(took), sorted(_contig_accepts(dtype)))
    c.reset()                                                   # AUTO, one step per call
    for t in range(T):
        c.encode_logits(view[t:t + 1], ds[t:t + 1])
    c.finish()
    _check_bytes(c, want, (layout, "incremental"))
    c.decode_open()
    out = torch.cat([c.decode_logits(view[t:t + 1]) for t in range(T)])
    assert torch.equal(out, ds), layout
    c.close()


@pytest.mark.parametrize("layout", REFUSED)
@pytest.mark.parametrize("dtype", list(SHAPES))
def test_misaligned_logits_are_refused(dtype, layout):
    """An odd stream stride (pad_odd) or a base one element off 16 bytes (offset_1): every
    entry point returns LAC_E_ARG and leaves the context as it was."""
    from lac_amd._lib import LacError, LAC_E_ARG
    x, sym = _inputs(dtype)
    want = _want(dtype, "contig")
    bad, good = layout_view(x, DEV, layout), layout_view(x, DEV, "contig")
    ds = torch.from_numpy(sym.copy()).to(DEV)
    c = _coder(dtype)

    def refused(call, *args):
        with pytest.raises(LacError) as e:
            call(*args)
        assert e.value.code == LAC_E_ARG, call.__name__

    refused(c.encode_logits_job, bad, ds)
    refused(c.quantize_logits, bad)
    c.reset()
    c.encode_logits(good[:1], ds[:1])
    refused(c.encode_logits, bad[1:], ds[1:])                   # mid-stream: the stream goes on after it
    c.encode_logits(good[1:], ds[1:])
    c.finish()
    _check_bytes(c, want, "incremental around a refusal")
    c.decode_open()
    refused(c.decode_logits, bad)
    assert torch.equal(c.decode_logits(good), ds)               # the refused call decoded nothing
    rc, err, _ = c.status()
    assert rc == 0 and not err.any()
    c.encode_logits_job(good, ds)
    _check_bytes(c, want, "job after the refusals")
    assert np.array_equal(c.quantize_logits(good).cpu().numpy().view(np.uint32), want[0])
    c.close()
