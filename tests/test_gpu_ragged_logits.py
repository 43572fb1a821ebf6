"""Per-stream symbol counts (lac_set_stream_lengths) on the logits path and in
LogitsCompressor.  The expected bits of stream b are the C oracle's over its first len[b]
rows, quantised by the oracle's q1; dead logits rows are NaN and dead symbols -1, so a
coder kernel consuming either cannot pass (the q1 statistics kernels may read a dead row:
nothing they compute from it is consumed, and nothing it holds raises anything)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COUNTS = [0, 1, 63, 64, 65, 128, 130, 1000]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _host_bits(t):
    """The exact logits the GPU sees, for the oracle (bf16 as uint16 patterns)."""
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def _sample(pmf, rng):
    c = np.cumsum(pmf.astype(np.uint64))
    return min(int(np.searchsorted(c, np.uint64(rng.random() * float(c[-1])), side="right")), len(pmf) - 1)


@functools.lru_cache(maxsize=None)
def _case(dtype, V, B, T, prec, counts):
    """-> (device logits [T, B, V] with NaN dead rows, sym [T, B] with -1 where dead, live
    lengths, expected bytes, expected bit counts); symbols drawn from the tables."""
    from oracle import oracle
    rng = np.random.default_rng(V * 131 + B)
    x = (rng.standard_normal((T, B, V)) * 3).astype(np.float32)
    t = torch.from_numpy(x)
    t = t.to(torch.bfloat16) if dtype == "bf16" else t
    host = _host_bits(t)
    cnt = np.array([counts[b % len(counts)] for b in range(B)], dtype=np.int64)
    live = np.minimum(cnt, T)
    sym = np.full((T, B), -1, dtype=np.int32)
    want, wbits = [], []
    for b in range(B):
        n = int(live[b])
        pmf = oracle.q1_quantize(host[:max(n, 1), b], prec)
        for i in range(n):
            sym[i, b] = _sample(pmf[i], rng)
        data, L, _ = oracle.encode(pmf, sym[:n, b], prec)
        want.append(data)
        wbits.append(L)
        t[n:, b, :] = float("nan")                              # poison
    return t.to(DEV), sym, cnt, live, want, np.array(wbits, dtype=np.uint64)


def _coder(V, B, T, prec):
    from lac_amd.batch import BatchCoder
    return BatchCoder(V, B, prec=prec, capacity_bits=T * (prec + 2) + 256, device=DEV)


def _clean(c):
    rc, err, _ = c.status()
    assert rc == 0 and not err.any(), (rc, err)


@pytest.mark.parametrize("dtype,V", [("bf16", 1008), ("f32", 1004)])
@pytest.mark.parametrize("B", [5, 70])
def test_ragged_logits_job_matches_oracle(dtype, V, B):
    T, prec = 130, 40
    dl, sym, cnt, live, want, wbits = _case(dtype, V, B, T, prec, tuple(COUNTS))
    ds = torch.from_numpy(sym).to(DEV)
    c = _coder(V, B, T, prec)
    c.set_stream_lengths(cnt)
    c.encode_logits_job(dl, ds)
    _clean(c)
    got, gbits = c.to_bytes()
    assert (gbits == wbits).all() and got == want
    c.decode_open()
    out = c.decode_logits(dl).cpu().numpy()
    _clean(c)
    assert np.array_equal(out, sym)
    # incremental: 50 + 80 steps equal the job; decode in two calls equals one
    c.reset()
    c.encode_logits(dl[:50], ds[:50])
    c.encode_logits(dl[50:], ds[50:])
    c.finish()
    _clean(c)
    got, gbits = c.to_bytes()
    assert (gbits == wbits).all() and got == want
    c.decode_open()
    out = torch.cat([c.decode_logits(dl[:50]), c.decode_logits(dl[50:])]).cpu().numpy()
    _clean(c)
    assert np.array_equal(out, sym)
    c.close()


# Forced row-statistics shapes (LAC_OPT_Q1_SHAPE), each of which must accept the row and run:
# 1 / 6 k_q1_stats (one wave per row; a whole block per row with the rolling prefetch),
# 8 its tiled form, 17 k_q1_stats_rl, 22 k_q1_stats_wide, 19 a row group (segments that
# exchange the row's maximum) -- at V = 1008 / 1004 the smallest row it accepts, two
# segments of 64 vectors and the rest; 0 = AUTO (row groups / the wide form for the long rows).
@pytest.mark.parametrize("dtype,V,shapes", [("bf16", 1008, (0, 1, 6, 8, 17, 22, 19)),
                                            ("f32", 1004, (0, 1, 6, 8, 17, 22, 19)),
                                            ("f32", 65540, (0, 22, 19)),
                                            ("bf16", 131080, (0, 22, 19))])
def test_ragged_logits_forced_q1_shapes(dtype, V, shapes):
    """T = 3 and counts [0, 1, 3] through every named shape: the oracle's bits, a clean
    decode, NaN dead rows raising nothing (these kernels read a dead row, nothing consumes
    what they make of it)."""
    T, B, prec = 3, 3, 48
    dl, sym, cnt, live, want, wbits = _case(dtype, V, B, T, prec, (0, 1, 3))
    ds = torch.from_numpy(sym).to(DEV)
    c = _coder(V, B, T, prec)
    c.set_stream_lengths(cnt)
    for sh in shapes:
        c.set_q1_shape(sh)
        c.encode_logits_job(dl, ds)
        _clean(c)
        got, gbits = c.to_bytes()
        assert (gbits == wbits).all() and got == want, sh
        c.decode_open()
        out = c.decode_logits(dl).cpu().numpy()
        _clean(c)
        assert np.array_equal(out, sym), sh
    c.close()


class _NoCache(torch.nn.Module):
    """A module with forward only: LogitsCompressor's teacher-forced route."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        return self.inner(x)


@pytest.mark.parametrize("incremental", [True, False])
def test_logits_compressor_with_lengths(incremental):
    from lac_amd.llm import LogitsCompressor, TinyCausalLM
    from oracle import oracle
    V, B, T, prec = 1000, 4, 24, 48
    lengths = [24, 1, 0, 17]
    model = TinyCausalLM(vocab=V, d=32, layers=1, heads=2, max_len=T + 1, seed=3)
    comp = LogitsCompressor(model if incremental else _NoCache(model), V, prec=prec, device=DEV)
    assert comp.incremental == incremental
    rng = np.random.default_rng(1)
    tokens = torch.from_numpy(rng.integers(0, V, size=(B, T))).to(DEV)
    data, nbits = comp.compress(tokens, lengths=lengths)
    # the reference: the oracle over the logits the compressor codes (padding fed as BOS)
    padded = tokens.clone()
    for b, n in enumerate(lengths):
        padded[b, n:] = comp.bos
    host = _host_bits(comp.logits(padded))                      # [B, T, V]
    for b, n in enumerate(lengths):
        pmf = oracle.q1_quantize(host[b, :max(n, 1)], prec)
        want, L, _ = oracle.encode(pmf, tokens[b, :n].cpu().numpy().astype(np.int32), prec)
        assert int(nbits[b]) == L and data[b] == want, b
    out = comp.decompress(data, nbits, T, lengths=lengths).cpu().numpy()
    tk = tokens.cpu().numpy()
    for b, n in enumerate(lengths):
        assert np.array_equal(out[b, :n], tk[b, :n]) and (out[b, n:] == -1).all(), b
    # the signatures without lengths keep working
    d2, n2 = comp.compress(tokens)
    assert torch.equal(comp.decompress(d2, n2, T), tokens)
