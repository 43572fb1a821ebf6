"""The one-position logits calls (lac_decode_logits_step / lac_encode_logits_step,
BatchCoder.decode_logits_step / encode_logits_step) on the GPU: the fused one-launch step
(LAC_OPT_Q1_STEP 1) against the C oracle (``oracle.q1_quantize`` + ``oracle.encode_batch``, as
tests/test_gpu_logits.py) and, observable for observable, against the two-launch path (mode 2),
which is the `steps = 1` call of the existing entry points.  Everything is bit-exact.
"""
import ctypes as C
import functools
import os
import subprocess
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO                                          # noqa: E402
from errors import dec_state as _dec_state, set_dec_state as _set_dec_state   # noqa: E402
from test_gpu_logits import _device_logits, _host_bits, _logits, _sample   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [
    # V, B, steps, prec, dtype
    (24, 3, 50, 24, "f32"),                # 6 vectors: nearly every thread empty
    (1000, 5, 30, 40, "bf16"),             # 125 vectors, a partial wave; the special rows
    (32000, 4, 8, 48, "bf16"),             # the serving shapes: not a multiple of the block
    (32000, 1, 8, 48, "f32"),
    (128256, 2, 4, 48, "bf16"),            # 16032 vectors: the last register partly filled
    (65536, 1, 3, 48, "f32"),              # exactly the cap
    (1000, 4, 20, 56, "bf16"),             # prec > 50: the 128-bit division form
]
IDS = ["-".join(str(v) for v in s) for s in SHAPES]


def _coder(V, B, prec, steps, mode=None, cap=None):
    from lac_amd.batch import BatchCoder
    c = BatchCoder(V, B, prec=prec, pmf_bits=32, capacity_bits=cap or steps * (prec + 2) + 256, device=DEV)
    if mode is not None:
        c.set_q1_step(mode)
    return c


@functools.lru_cache(maxsize=None)
def _case(V, B, steps, prec, dtype, shared=False):
    """Logits, the oracle's tables, symbols drawn from them, the oracle's bytes; computed once.
    shared: one row per step for all streams (stream stride 0)."""
    from oracle import oracle as coracle
    x = _logits(V + B + prec, steps, 1 if shared else B, V, specials=True)
    dl = _device_logits(x, dtype)
    pmf = coracle.q1_quantize(_host_bits(dl), prec)
    if shared:
        pmf = np.ascontiguousarray(np.broadcast_to(pmf, (steps, B, V)))
    sym = _sample(pmf, V + 1)
    out, nb, status, rc = coracle.encode_batch(pmf, sym, prec, nthreads=16)
    assert rc == 0 and not status.any()
    want = [out[b, :(int(nb[b]) + 7) // 8].tobytes() for b in range(B)]
    return types.SimpleNamespace(V=V, B=B, steps=steps, prec=prec, dl=dl, pmf=pmf, sym=sym,
                                 dsym=torch.from_numpy(sym).to(DEV), want=want, nb=nb)


def _padded(dl):
    """The same rows, padded by one 16-B vector each."""
    n = 16 // dl.element_size()
    buf = torch.full(dl.shape[:2] + (dl.shape[2] + n,), float("nan"), dtype=dl.dtype, device=dl.device)
    buf[..., :dl.shape[2]] = dl
    return buf[..., :dl.shape[2]]


def _written(ck):
    """A checkpoint's planes with the words past each stream's L bits (never written: whatever the
    allocation held) zeroed."""
    p = ck["planes"].copy()
    for b, L in enumerate(ck["state"]["L"]):
        p[:, b, (int(L) + 63) // 64:] = 0
    return p


def _same_ckpt(a, b):
    for f in a["state"].dtype.names:
        assert np.array_equal(a["state"][f], b["state"][f]), (f, a["state"][f], b["state"][f])
    assert np.array_equal(_written(a), _written(b))
    return True


def _launches(c, fn):
    """Kernel launches per profile slot (lac_profile_read) while fn runs."""
    cnt = (C.c_int64 * 8)()
    ms = (C.c_double * 8)()
    c.lib.lac_profile_read(c.ctx, None, None, 1)
    c.lib.lac_profile_enable(c.ctx, 1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        c.lib.lac_profile_enable(c.ctx, 0)
    c.lib.lac_profile_read(c.ctx, C.cast(ms, C.c_void_p), C.cast(cnt, C.c_void_p), 1)
    return [int(v) for v in cnt]


def _encode_steps(c, dl, dsym, trace=None):
    c.reset()
    for t in range(dsym.shape[0]):
        c.encode_logits_step(dl[t], dsym[t], trace=None if trace is None else trace[t])
    c.finish()


def _decode_steps(c, dl, steps):
    out = torch.empty((steps, c.streams), dtype=torch.int32, device=DEV)
    for t in range(steps):
        got = c.decode_logits_step(dl[t], out=out[t:t + 1])
        assert got.shape == (1, c.streams) and got.dtype == torch.int32
    return out


@functools.lru_cache(maxsize=None)
def _stream_cap():
    """The most streams the fused step takes here: min(kQ1StepMaxStreams, compute units)."""
    so = os.path.join(REPO, "tests", "native", "libstepselectcheck.so")
    src = os.path.join(REPO, "tests", "native", "step_select_check.cpp")
    deps = [src, os.path.join(REPO, "lac_amd", "csrc", "lac_select.h"), os.path.join(REPO, "include", "lac.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(REPO, "lac_amd", "csrc"),
                        "-I", os.path.join(REPO, "include"), src, "-o", so], check=True)
    lib = C.CDLL(so)
    k = (C.c_int64 * 4)()
    lib.ssc_consts.argtypes = [C.POINTER(C.c_int64)]
    lib.ssc_consts.restype = None
    lib.ssc_consts(k)
    return min(int(k[1]), torch.cuda.get_device_properties(0).multi_processor_count)


# ------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("layout", ["rows", "shared", "padded"])
@pytest.mark.parametrize("V,B,steps,prec,dtype", SHAPES, ids=IDS)
def test_step_encode_decode_vs_oracle(V, B, steps, prec, dtype, layout):
    k = _case(V, B, steps, prec, dtype, shared=layout == "shared")
    dl = _padded(k.dl) if layout == "padded" else k.dl
    if layout == "shared":
        assert dl.shape[1] == 1                                    # [steps, 1, V]: stream stride 0
    c = _coder(V, B, prec, steps, "fused")
    trace = torch.zeros((steps, B, 2), dtype=torch.int64, device=DEV)
    _encode_steps(c, dl, k.dsym, trace)
    data, n = c.to_bytes()
    assert [int(v) for v in n] == [int(v) for v in k.nb]
    assert data == k.want
    # the traces: the job's, which tests/test_gpu_logits.py pins to the pmf path's
    ref = _coder(V, B, prec, steps)
    rtrace = torch.zeros_like(trace)
    ref.encode_logits_job(dl, k.dsym, trace=rtrace)
    assert ref.to_bytes()[0] == k.want
    assert torch.equal(trace, rtrace)
    # decode: the coded symbols, and determined() as the two-launch path reports it
    c.decode_open()
    got = _decode_steps(c, dl, steps)
    assert torch.equal(got, k.dsym)
    c.raise_on_error()
    ref.decode_open()
    assert torch.equal(ref.decode_logits(dl), k.dsym)
    assert np.array_equal(c.determined(), ref.determined())
    assert _dec_state(c).tobytes() == _dec_state(ref).tobytes()
    c.close()
    ref.close()


# ------------------------------------------------------------------ fused against two launches
@pytest.mark.parametrize("V,B,steps,prec,dtype", SHAPES, ids=IDS)
def test_fused_equals_two_launch_state_for_state(V, B, steps, prec, dtype):
    k = _case(V, B, steps, prec, dtype)
    a, b = _coder(V, B, prec, steps, "fused"), _coder(V, B, prec, steps, "split")
    ta = torch.zeros((steps, B, 2), dtype=torch.int64, device=DEV)
    tb = torch.zeros_like(ta)
    a.reset()
    b.reset()
    for t in range(steps):
        a.encode_logits_step(k.dl[t], k.dsym[t], trace=ta[t])
        b.encode_logits_step(k.dl[t], k.dsym[t], trace=tb[t])
        assert _same_ckpt(a.checkpoint(), b.checkpoint()), t        # state and planes
    assert torch.equal(ta, tb)
    a.finish()
    b.finish()
    assert a.to_bytes()[0] == b.to_bytes()[0] == k.want
    bits, nb = a.bits_tensor(), a.nbits_tensor()
    a.decode_open(bits, nb)
    b.decode_open(bits, nb)
    for t in range(steps):
        sa, sb = a.decode_logits_step(k.dl[t]), b.decode_logits_step(k.dl[t])
        assert torch.equal(sa, sb) and torch.equal(sa[0], k.dsym[t]), t
        assert _dec_state(a).tobytes() == _dec_state(b).tobytes(), t
    # past the end of the streams' bits both decode on over zero padding alike
    for t in range(2):
        assert torch.equal(a.decode_logits_step(k.dl[t]), b.decode_logits_step(k.dl[t]))
        assert _dec_state(a).tobytes() == _dec_state(b).tobytes()
    assert a.status()[0] == b.status()[0]
    a.close()
    b.close()


# ------------------------------------------------------------------ one launch
def test_fused_step_is_one_launch():
    V, B, steps, prec, dtype = SHAPES[2]
    k = _case(V, B, steps, prec, dtype)
    for mode, stats in (("fused", 0), ("split", steps)):
        c = _coder(V, B, prec, steps, mode)
        c.reset()
        n = _launches(c, lambda: [c.encode_logits_step(k.dl[t], k.dsym[t]) for t in range(steps)])
        assert (n[6], n[1], n[7]) == (stats, steps, 0), (mode, n)
        c.finish()
        assert c.to_bytes()[0] == k.want
        c.decode_open()
        n = _launches(c, lambda: _decode_steps(c, k.dl, steps))
        assert (n[6], n[7], n[1]) == (stats, steps, 0), (mode, n)
        c.close()


# ------------------------------------------------------------------ mixing with the other calls
def test_step_calls_mix_in_one_session():
    V, B, steps, prec, dtype = SHAPES[1]
    k = _case(V, B, steps, prec, dtype)
    c = _coder(V, B, prec, steps, "fused")
    pmf = c.quantize_logits(k.dl)                                  # the materialised tables
    assert np.array_equal(pmf.cpu().numpy().view(np.uint32), k.pmf)
    # encode: steps, pmf steps, multi-step logits calls, and a checkpoint / restore in the middle
    c.reset()
    t = 0
    while t < steps:
        c.encode_logits_step(k.dl[t], k.dsym[t])
        t += 1
        if t < steps:
            c.encode(pmf[t:t + 1], k.dsym[t:t + 1])
            t += 1
        if t == 8:
            ck = c.checkpoint()
            c.encode_logits_step(k.dl[0], k.dsym[0])               # thrown away by the restore
            c.reset()
            c.restore(ck)
        n = min(3, steps - t)
        if n:
            c.encode_logits(k.dl[t:t + n], k.dsym[t:t + n])
            t += n
    c.finish()
    data, nb = c.to_bytes()
    assert data == k.want and [int(v) for v in nb] == [int(v) for v in k.nb]
    # decode: steps, decode_logits of 3 steps and pmf steps alternate; equal to decode_logits alone
    ref = _coder(V, B, prec, steps)
    bits, nbt = c.bits_tensor(), c.nbits_tensor()
    ref.decode_open(bits, nbt)
    want = ref.decode_logits(k.dl)
    assert torch.equal(want, k.dsym)
    c.decode_open()
    got = torch.empty_like(want)
    t = 0
    while t < steps:
        c.decode_logits_step(k.dl[t], out=got[t:t + 1])
        t += 1
        n = min(3, steps - t)
        if n:
            c.decode_logits(k.dl[t:t + n], out=got[t:t + n])
            t += n
        if t < steps:
            c.decode(pmf[t:t + 1], out=got[t:t + 1])
            t += 1
    assert torch.equal(got, want)
    assert _dec_state(c).tobytes() == _dec_state(ref).tobytes()
    assert np.array_equal(c.determined(), ref.determined())
    c.close()
    ref.close()


# ------------------------------------------------------------------ per-stream counts
@pytest.mark.parametrize("dtype,V", [("bf16", 1000), ("f32", 32000)])
def test_step_with_stream_lengths(dtype, V):
    from oracle import oracle as coracle
    B, steps, prec = 3, 6, 40
    counts = [0, 2, steps]
    x = _logits(V + 17, steps, B, V)
    dl = _device_logits(x, dtype).clone()
    host = _host_bits(dl)
    rng = np.random.default_rng(V)
    sym = np.full((steps, B), -1, dtype=np.int32)
    want, wbits = [], []
    for b, n in enumerate(counts):
        pmf = coracle.q1_quantize(host[:max(n, 1), b], prec)
        sym[:n, b] = _sample(pmf[:n], int(rng.integers(1 << 30))) if n else sym[:n, b]
        data, L, _ = coracle.encode(pmf, sym[:n, b], prec)
        want.append(data)
        wbits.append(L)
        dl[n:, b, :] = float("nan")                                 # an ended stream's rows
    dsym = torch.from_numpy(sym).to(DEV)
    res = {}
    for mode in ("fused", "split"):
        c = _coder(V, B, prec, steps, mode)
        c.set_stream_lengths(counts)
        c.reset()
        for t in range(steps):
            before = c.checkpoint()["state"]
            c.encode_logits_step(dl[t], dsym[t])
            after = c.checkpoint()["state"]
            for b, n in enumerate(counts):
                if t >= n:                                         # an ended stream: state unchanged
                    assert before[b].tobytes() == after[b].tobytes(), (mode, t, b)
        c.finish()
        rc, err, _ = c.status()
        assert rc == 0 and not err.any()
        data, nb = c.to_bytes()
        assert data == want and [int(v) for v in nb] == wbits, mode
        c.decode_open()
        states = []
        for t in range(steps):
            before = _dec_state(c)
            got = c.decode_logits_step(dl[t]).cpu().numpy()[0]
            after = _dec_state(c)
            assert np.array_equal(got, sym[t]), (mode, t)           # -1 for the ended streams
            for b, n in enumerate(counts):
                if t >= n:
                    assert before[b].tobytes() == after[b].tobytes(), (mode, t, b)
            states.append(after.tobytes())
        rc, err, _ = c.status()
        assert rc == 0 and not err.any()
        res[mode] = states
        c.close()
    assert res["fused"] == res["split"]


# ------------------------------------------------------------------ errors, each as mode 2 reports it
def _both(V, B, prec, steps, cap=None):
    return [_coder(V, B, prec, steps, m, cap=cap) for m in ("fused", "split")]


def test_decode_range_error_matches_two_launch():
    from lac_amd._lib import LAC_E_DECODE_RANGE
    V, B, steps, prec, dtype = SHAPES[1]
    k = _case(V, B, steps, prec, dtype)
    enc = _coder(V, B, prec, steps)
    enc.encode_logits_job(k.dl, k.dsym)
    bits, nb = enc.bits_tensor(), enc.nbits_tensor()
    seen = []
    for c in _both(V, B, prec, steps):
        c.decode_open(bits, nb)
        outs = [c.decode_logits_step(k.dl[0]).cpu().numpy()]
        st = _dec_state(c)
        st["x"][1] = st["l"][1] - 1                                # x < l
        _set_dec_state(c, st)
        for t in (1, 2, 3):
            outs.append(c.decode_logits_step(k.dl[t]).cpu().numpy())
        rc, err, step = c.status()
        assert rc == LAC_E_DECODE_RANGE and list(err != 0) == [b == 1 for b in range(B)]
        assert err[1] == LAC_E_DECODE_RANGE and step[1] == 1
        assert all(o[0, 1] == -1 for o in outs[1:])                # the failing step and every later one
        assert all(np.array_equal(np.delete(o[0], 1), np.delete(k.sym[t], 1)) for t, o in enumerate(outs))
        seen.append((np.concatenate(outs).tobytes(), err.tobytes(), step.tobytes(), _dec_state(c).tobytes()))
        c.close()
    assert seen[0] == seen[1]


def test_symbol_range_error_matches_two_launch():
    from lac_amd._lib import LAC_E_SYMBOL_RANGE
    V, B, steps, prec, dtype = SHAPES[1]
    k = _case(V, B, steps, prec, dtype)
    bad = k.dsym[1].clone()
    bad[0], bad[3] = -1, V
    seen = []
    for c in _both(V, B, prec, steps):
        c.reset()
        c.encode_logits_step(k.dl[0], k.dsym[0])
        c.encode_logits_step(k.dl[1], bad)
        c.encode_logits_step(k.dl[2], k.dsym[2])                   # the failed streams stay where they are
        rc, err, step = c.status()
        assert rc == LAC_E_SYMBOL_RANGE
        assert list(err) == [LAC_E_SYMBOL_RANGE, 0, 0, LAC_E_SYMBOL_RANGE, 0] and step[0] == step[3] == 1
        ck = c.checkpoint()
        seen.append((ck["state"].tobytes(), _written(ck).tobytes(), err.tobytes(), step.tobytes()))
        c.close()
    assert seen[0] == seen[1]


def test_capacity_error_at_the_same_step():
    from lac_amd._lib import LAC_E_CAPACITY
    V, B, steps, prec, dtype = SHAPES[1]
    k = _case(V, B, steps, prec, dtype)
    # uniform symbols, not the tables' likely ones: ~10 bits and more per step
    dsym = torch.randint(0, V, (steps, B), dtype=torch.int32, device=DEV,
                         generator=torch.Generator(device=DEV).manual_seed(8))
    seen = []
    for c in _both(V, B, prec, steps, cap=64):                     # two plane words per stream
        c.reset()
        hist = []
        for t in range(steps):
            c.encode_logits_step(k.dl[t], dsym[t])
            rc, err, step = c.status()
            hist.append((rc, err.tobytes(), step.tobytes()))
        rc, err, step = c.status()
        assert rc == LAC_E_CAPACITY and (err == LAC_E_CAPACITY).all() and (step < steps).all()
        ck = c.checkpoint()
        seen.append((hist, ck["state"].tobytes(), _written(ck).tobytes()))
        c.close()
    assert seen[0] == seen[1]


@pytest.mark.parametrize("mode", ["fused", "split", "auto"])
def test_refusals_before_anything_is_launched(mode):
    from lac_amd._lib import LAC_E_ARG, LAC_E_STATE, LacError
    V, B, steps, prec, dtype = SHAPES[1]
    k = _case(V, B, steps, prec, dtype)
    c = _coder(V, B, prec, steps, mode)
    with pytest.raises(LacError) as e:                             # no open decode
        c.decode_logits_step(k.dl[0])
    assert e.value.code == LAC_E_STATE
    flat = torch.zeros(B * V + 8, dtype=k.dl.dtype, device=DEV)
    off = flat[1:1 + B * V].view(B, V)                             # a base 2 bytes off 16
    off.copy_(k.dl[1])
    c.reset()
    c.encode_logits_step(k.dl[0], k.dsym[0])
    before = c.checkpoint()
    with pytest.raises(LacError) as e:
        c.encode_logits_step(off, k.dsym[1])
    assert e.value.code == LAC_E_ARG
    n = _launches(c, lambda: pytest.raises(LacError, c.encode_logits_step, off, k.dsym[1]))
    assert not any(n)
    assert _same_ckpt(before, c.checkpoint())
    for t in range(1, steps):
        c.encode_logits_step(k.dl[t], k.dsym[t])
    c.finish()
    assert c.to_bytes()[0] == k.want
    c.decode_open()
    c.decode_logits_step(k.dl[0])
    st = _dec_state(c)
    with pytest.raises(LacError) as e:
        c.decode_logits_step(off)
    assert e.value.code == LAC_E_ARG
    assert _dec_state(c).tobytes() == st.tobytes()
    assert torch.equal(c.decode_logits_step(k.dl[1])[0], k.dsym[1])
    c.close()


# ------------------------------------------------------------------ shapes the fused step does not take
@pytest.mark.parametrize("V,B,dtype", [(1000, None, "bf16"), (151936, 1, "bf16")], ids=["cap+1", "V151936"])
def test_fallback_to_two_launches(V, B, dtype):
    from lac_amd._lib import LAC_E_ARG, LacError
    B = B or _stream_cap() + 1
    steps, prec = 3, 48
    k = _case(V, B, steps, prec, dtype)
    c = _coder(V, B, prec, steps, "auto")
    c.reset()
    n = _launches(c, lambda: [c.encode_logits_step(k.dl[t], k.dsym[t]) for t in range(steps)])
    assert (n[6], n[1]) == (steps, steps), n
    c.finish()
    assert c.to_bytes()[0] == k.want
    c.decode_open()
    n = _launches(c, lambda: _decode_steps(c, k.dl, steps))
    assert (n[6], n[7]) == (steps, steps), n
    c.decode_open()
    assert torch.equal(_decode_steps(c, k.dl, steps), k.dsym)
    c.raise_on_error()
    # mode 1 on the same job: refused, nothing launched, no state changed
    c.set_q1_step("fused")
    st = _dec_state(c)
    with pytest.raises(LacError) as e:
        c.decode_logits_step(k.dl[0])
    assert e.value.code == LAC_E_ARG and _dec_state(c).tobytes() == st.tobytes()
    c.reset()
    before = c.checkpoint()
    with pytest.raises(LacError) as e:
        c.encode_logits_step(k.dl[0], k.dsym[0])
    assert e.value.code == LAC_E_ARG and _same_ckpt(before, c.checkpoint())
    c.close()


def test_logits_compressor_takes_the_step_calls():
    """LogitsCompressor's incremental loops are the serving loop: they call the step methods."""
    from lac_amd.llm import LogitsCompressor, TinyCausalLM
    V, B, T = 1000, 3, 12
    model = TinyCausalLM(vocab=V, max_len=16, seed=5, d=32, layers=1, heads=2).to(DEV).eval()
    tokens = torch.randint(0, V, (B, T), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    outs = []
    for mode in ("fused", "split"):
        lc = LogitsCompressor(model, V, prec=40, logits_dtype=torch.bfloat16, device=DEV, q1_step=mode)
        assert lc.incremental
        data, nbits = lc.compress(tokens)
        assert torch.equal(lc.decompress(data, nbits, T), tokens)
        outs.append((data, [int(v) for v in nbits]))
    assert outs[0] == outs[1]
