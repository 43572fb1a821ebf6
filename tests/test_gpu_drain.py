"""Draining settled output mid-job (include/lac.h lac_encode_drain, BatchCoder.drain,
lac_amd.batch.DrainSink): the bytes drained over all calls followed by the finished tail are the
bytes of the same symbols coded with no drain, in a coder whose capacity holds only the bits
between two drains.  Every comparison is against the one-shot job in a large-capacity context and
the C oracle, never against the drained coder itself."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAC_E_ARG, LAC_E_SYMBOL_RANGE, LAC_E_CAPACITY, LAC_E_STATE = -1, -3, -7, -9
ONES = (1 << 64) - 1
SENTINEL = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _dev(pmf):
    it = np.int32 if pmf.dtype == np.uint32 else np.int64
    return torch.from_numpy(np.ascontiguousarray(pmf).view(it)).to(DEV)


def _oracle(pmf, sym, prec):
    from oracle import oracle
    out, nb, status, rc = oracle.encode_batch(pmf, sym, prec, nthreads=16)
    assert rc == 0 and not status.any()
    return [out[b, :(int(nb[b]) + 7) // 8].tobytes() for b in range(pmf.shape[1])], nb


def _job(V, B, prec, bits, cap, dp, ds, lengths=None):
    """The one-shot job in a context that holds the whole stream -> (bytes, bit counts)."""
    from lac_amd.batch import BatchCoder
    with BatchCoder(V, B, prec=prec, pmf_bits=bits, capacity_bits=cap, device=DEV) as c:
        if lengths is not None:
            c.set_stream_lengths(lengths)
        c.encode_job(dp, ds)
        return c.to_bytes()


def _same_stream(ck_a, ck_b, b):
    """Stream b's registers, counters and planes are the same in two checkpoints."""
    return (ck_a["state"][b:b + 1].tobytes() == ck_b["state"][b:b + 1].tobytes()
            and np.array_equal(ck_a["planes"][:, b], ck_b["planes"][:, b]))


def _drive(coder, T, every, step, sink=None, chunk=1):
    """reset, code T steps in calls of `chunk`, pull every `every` steps -> the sink (not finished)."""
    from lac_amd.batch import DrainSink
    sink = sink or DrainSink(coder)
    coder.reset()
    for t in range(0, T, chunk):
        step(t, min(t + chunk, T))
        if (t + chunk) % every == 0:
            sink.pull()
    return sink


# ------------------------------------------------------------------ 1. integer tables, bounded capacity
V1, B1, T1, PREC1 = 256, 70, 600, 48
CAP1 = 100 * (PREC1 + 2) + 256                                  # a coder sized for 100 steps


@functools.lru_cache(maxsize=None)
def _int_case(bits):
    """Skewed tables (entries 2^0 .. 2^19 / 2^39, symbols uniform: ~12 / ~22 bits per symbol, so
    the 600 steps need far more than CAP1) -> tables, symbols, oracle bytes, job bytes."""
    rng = np.random.default_rng(bits)
    ex = rng.integers(0, 20 if bits == 32 else 40, size=(T1, B1, V1))
    pmf = (np.uint64(1) << ex.astype(np.uint64)).astype(np.uint32 if bits == 32 else np.uint64)
    sym = rng.integers(0, V1, size=(T1, B1)).astype(np.int32)
    want, wbits = _oracle(pmf, sym, PREC1)
    assert int(wbits.min()) > CAP1 + 64 * 8                     # no stream fits the bounded coder undrained
    dp, ds = _dev(pmf), torch.from_numpy(sym).to(DEV)
    job, jbits = _job(V1, B1, PREC1, bits, T1 * (PREC1 + 2) + 256, dp, ds)
    assert job == want and (jbits == wbits).all()
    return dp, ds, want, wbits


@pytest.mark.parametrize("every", [1, 7, 64])
@pytest.mark.parametrize("path", ["split", "fused"])
@pytest.mark.parametrize("bits", [32, 64])
def test_bounded_coder_with_drains_equals_job_and_oracle(bits, path, every):
    from lac_amd.batch import BatchCoder
    dp, ds, want, wbits = _int_case(bits)
    with BatchCoder(V1, B1, prec=PREC1, pmf_bits=bits, capacity_bits=CAP1, device=DEV) as c:
        c.set_path(path)
        sink = _drive(c, T1, every, lambda a, b: c.encode(dp[a:b], ds[a:b]))
        got, gbits = sink.finish()
        assert (gbits == wbits).all()
        assert got == want
        assert min(len(p) for p in sink.parts) > CAP1 // 8      # more than a capacity went through the drains


@pytest.mark.parametrize("bits", [32, 64])
def test_bounded_coder_without_drains_runs_out_of_capacity(bits):
    from lac_amd.batch import BatchCoder
    dp, ds, _, _ = _int_case(bits)
    with BatchCoder(V1, B1, prec=PREC1, pmf_bits=bits, capacity_bits=CAP1, device=DEV) as c:
        c.reset()
        for t in range(0, T1, 50):
            c.encode(dp[t:t + 50], ds[t:t + 50])
        rc, err, _ = c.status()
        assert rc == LAC_E_CAPACITY and (err == LAC_E_CAPACITY).all()


# ------------------------------------------------------------------ 2. the logits step calls
@functools.lru_cache(maxsize=None)
def _logits_case():
    V, B, T, prec = 512, 3, 300, 48
    g = torch.Generator().manual_seed(11)
    lg = (torch.randn((T, B, V), generator=g) * 4).to(torch.bfloat16).to(DEV)
    sym = torch.randint(0, V, (T, B), generator=g, dtype=torch.int32).to(DEV)
    from lac_amd.batch import BatchCoder
    with BatchCoder(V, B, prec=prec, capacity_bits=T * (prec + 2) + 256, device=DEV) as c:
        c.encode_logits_job(lg, sym)
        want, wbits = c.to_bytes()
    return V, B, T, prec, lg, sym, want, wbits


@pytest.mark.parametrize("mode", ["fused", "split"])
def test_logits_step_with_drains_equals_logits_job(mode):
    from lac_amd.batch import BatchCoder
    V, B, T, prec, lg, sym, want, wbits = _logits_case()
    cap = 5 * (prec + 2) + 256 + 8 * 64                         # five positions and the kept words
    assert int(wbits.min()) > 4 * cap
    with BatchCoder(V, B, prec=prec, capacity_bits=cap, device=DEV) as c:
        c.set_q1_step(mode)
        sink = _drive(c, T, 5, lambda a, b: c.encode_logits_step(lg[a], sym[a:b]))
        got, gbits = sink.finish()
        assert (gbits == wbits).all() and got == want


# ------------------------------------------------------------------ 3. crafted planes planted with restore()
def _flush_digits(l, h, prec):
    """A_to_bin.flush (arith_code.py:193-202) on given registers."""
    D, Hd = 1 << prec, 1 << (prec - 1)
    out = []
    while l > 0 or h + 1 < D:
        d = l // Hd
        if max(0, min((d + 1) * Hd, h) - max(l, d * Hd) + 1) < max(0, min((d + 2) * Hd, h) - max(l, (d + 1) * Hd) + 1):
            d += 1
        l, h = l * 2 - d * D, h * 2 + 1 - d * D
        out.append(d)
    return out


def _negative_flush_registers(prec):
    """The search of tests/test_drain_host.py: open registers whose flush has a -1 digit."""
    rng = np.random.default_rng(0)
    D, Hd = 1 << prec, 1 << (prec - 1)
    for _ in range(20000):
        l = int(rng.integers(0, D))
        h = l + Hd + int(rng.integers(0, Hd))
        if h >= D and -1 in _flush_digits(l, h, prec):
            return l, h
    raise AssertionError("no registers with a -1 flush digit found")


def test_crafted_planes_drain_where_the_rule_says():
    from lac_amd.batch import ENC_STATE, BatchCoder, DrainSink
    prec, V = 48, 16
    D = 1 << prec
    open_regs = (D - 10, D - 10 + (D >> 1) + 5)                 # h >= 2^prec: not certain
    certain = (5, (D >> 1) + 100)
    neg = _negative_flush_registers(prec)
    assert -1 in _flush_digits(*neg, prec)
    pend = (4 * 64 + 20, 0xFFFFF << 44, 1 << 44)                # 20 ones in the active word, a pending C bit on the last
    # (registers, (L, wa, wc), plane A words below the active one, plane C words, words drained)
    cases = [
        (open_regs, pend, [5, 0x1234, ONES, ONES], [0, 0, 0, 0], 1),          # all-ones between guard and carry
        (open_regs, pend, [5, ONES - 0xF, ONES, ONES], [0, 0x20, 0, 0], 1),   # the guard itself wraps
        (certain, pend, [5, 0x1234, ONES, ONES], [0, 0, 0, 0], 4),            # certain: all but the active word
        (neg, (4 * 64 + 63, 0x5 << 61, 0), [0x77, 0x10, 0, 0], [0, 0, 0, 0], 1),   # zero words, flush straddles a word
        (neg, (5 * 64, 0x5 << 61, 0), [0x77, 0x10, 0, 0], [0, 0, 0, 0], 1),        # and starts one
        (open_regs, (3 * 64 + 9, 0x1FF << 55, 1 << 55), [0x99, ONES, ONES - 3], [0, 0, 3], 0),   # guard at word 0
        (open_regs, (3 * 64, ONES - 1, 1), [7, 0x42], [0, 0], 1),             # L a multiple of 64
        (certain, (3 * 64, ONES - 1, 1), [7, 0x42], [0, 0], 2),
        (certain, (37, (ONES << 27) & ONES, 0), [], [], 0),                   # L <= 64
    ]
    B = len(cases)
    with BatchCoder(V, B, prec=prec, capacity_bits=8 * 64, device=DEV) as c:
        words = c.bits_stride() // 8
        st = np.zeros(B, dtype=ENC_STATE)
        planes = np.zeros((2, B, words), dtype=np.uint64)
        for b, ((l, h), (L, wa, wc), pa, pc, _) in enumerate(cases):
            st[b] = (l, h, L, wa, wc, 7, 0, -1, -1, [0] * 8)
            planes[0, b, :len(pa)], planes[1, b, :len(pc)] = pa, pc
            planes[0, b, (L - 1) >> 6], planes[1, b, (L - 1) >> 6] = wa, wc
        ck = {"state": st, "planes": planes, "prec": prec, "vocab": V}
        c.restore(ck)
        c.finish()
        want, wbits = c.to_bytes()
        assert any(-1 in d for d in c.flush_digits())
        c.reset()
        c.restore(ck)
        sink = DrainSink(c)
        n = sink.pull()
        assert n.tolist() == [8 * g for *_, g in cases]
        after = c.checkpoint()["state"]
        assert after["L"].tolist() == [case[1][0] - 64 * case[4] for case in cases]
        got, gbits = sink.finish()
        assert (gbits == wbits).all() and got == want


# ------------------------------------------------------------------ 4. constant symbols
@pytest.mark.parametrize("V,last", [(2, False), (2, True), (4, False), (4, True)])
def test_constant_symbol_streams_drain_in_16_words(V, last):
    from lac_amd.batch import BatchCoder
    B, T, prec = 4, 3000, 48
    rng = np.random.default_rng(V + last)
    main = V - 1 if last else 0
    sym = np.where(rng.random((T, B)) < 0.97, main, rng.integers(0, V, (T, B))).astype(np.int32)
    sym[:, 0] = main                                            # one stream of nothing else: all 0s / all 1s
    pmf = np.ones((T, B, V), dtype=np.uint32)
    want, wbits = _oracle(pmf, sym, prec)
    assert int(wbits.min()) > 2 * 16 * 64
    row, ds = _dev(pmf[0, 0]), torch.from_numpy(sym).to(DEV)
    with BatchCoder(V, B, prec=prec, capacity_bits=16 * 64, device=DEV) as c:
        sink = _drive(c, T, 64, lambda a, b: c.encode(row, ds[a:b]), chunk=64)
        got, gbits = sink.finish()
        assert (gbits == wbits).all() and got == want


# ------------------------------------------------------------------ 5. ragged and failing streams
def test_ended_streams_drain_and_a_failed_stream_does_not():
    from lac_amd.batch import BatchCoder, DrainSink
    V, B, T, prec = 64, 6, 200, 40
    rng = np.random.default_rng(21)
    pmf = rng.integers(1, 1000, size=(T, B, V)).astype(np.uint32)
    sym = rng.integers(0, V, size=(T, B)).astype(np.int32)
    counts = np.array([0, 30, 100, 1000, 1000, 150], dtype=np.int64)
    bad, bad_step = 4, 120
    ok = [b for b in range(B) if b != bad]
    dp = _dev(pmf)
    big = T * (prec + 2) + 256
    want, wbits = _job(V, B, prec, 32, big, dp, torch.from_numpy(sym).to(DEV), lengths=counts)
    from oracle import oracle
    for b in ok:                                                # the job's streams are the oracle's
        n = int(min(counts[b], T))
        data, L, _ = oracle.encode(pmf[:max(n, 1), b], sym[:n, b], prec)
        assert want[b] == data and int(wbits[b]) == L
    sym[bad_step, bad] = V                                      # out of range: a sticky LAC_E_SYMBOL_RANGE
    ds = torch.from_numpy(sym).to(DEV)
    with BatchCoder(V, B, prec=prec, capacity_bits=20 * (prec + 2) + 256 + 8 * 64, device=DEV) as c:
        c.set_stream_lengths(counts)
        sink = DrainSink(c)
        c.reset()
        frozen = None
        for t in range(0, T, 10):
            c.encode(dp[t:t + 10], ds[t:t + 10])
            sink.pull()
            if t == bad_step + 10:                              # the failed stream, two drains after its error
                frozen = (len(sink.parts[bad]), c.checkpoint())
        assert len(sink.parts[bad]) == frozen[0]
        ck = c.checkpoint()
        assert _same_stream(ck, frozen[1], bad)
        rc, err, step = c.status()
        assert rc == LAC_E_SYMBOL_RANGE and err[bad] == LAC_E_SYMBOL_RANGE and step[bad] == bad_step
        assert not err[ok].any()
        sink.pull()
        c.finish()
        nb = c.nbits_tensor().cpu().numpy().astype(np.uint64)
        tail = c.bits_tensor().cpu().numpy()
        for b in ok:
            got = bytes(sink.parts[b]) + tail[b, :(int(nb[b]) + 7) // 8].tobytes()
            assert got == want[b] and 8 * len(sink.parts[b]) + int(nb[b]) == int(wbits[b]), b
        assert len(sink.parts[2]) > 0 and len(sink.parts[0]) == 0   # an ended stream drained; an empty one had nothing


# ------------------------------------------------------------------ 6. short slots
def test_short_slot_is_all_or_nothing_per_stream():
    from lac_amd.batch import BatchCoder
    V, B, T, prec = 64, 5, 60, 48
    rng = np.random.default_rng(6)
    pmf = rng.integers(1, 1000, size=(T, B, V)).astype(np.uint32)
    sym = rng.integers(0, V, size=(T, B)).astype(np.int32)
    dp, ds = _dev(pmf), torch.from_numpy(sym).to(DEV)
    with BatchCoder(V, B, prec=prec, capacity_bits=T * (prec + 2) + 256, device=DEV) as c:
        c.reset()
        c.encode(dp, ds)
        ck = c.checkpoint()
        wide = torch.zeros((B, c.bits_stride()), dtype=torch.uint8, device=DEV)
        fill = torch.zeros(B, dtype=torch.int64, device=DEV)
        c.drain(wide, fill)                                     # what every stream drains with room
        need = fill.cpu().numpy()
        assert (need >= 16).all() and (need % 8 == 0).all()
        wide = wide.cpu().numpy()
        c.restore(ck)
        stride = int(need.max()) + 16
        buf = torch.full((16 + B * stride + 16,), SENTINEL, dtype=torch.uint8, device=DEV)
        slots = buf[16:16 + B * stride].view(B, stride)
        start = stride - need                                   # every stream's bytes fit exactly ...
        start[1] += 8                                           # ... but stream 1's slot is 8 bytes short
        fill = torch.from_numpy(start.astype(np.int64)).to(DEV)
        c.drain(slots, fill)
        got, f = buf.cpu().numpy(), fill.cpu().numpy()
        body = got[16:16 + B * stride].reshape(B, stride)
        assert (got[:16] == SENTINEL).all() and (got[16 + B * stride:] == SENTINEL).all()
        for b in range(B):
            assert (body[b, :start[b]] == SENTINEL).all()
            if b == 1:
                assert f[b] == start[b] and (body[b] == SENTINEL).all()
            else:
                assert f[b] == stride and np.array_equal(body[b, start[b]:], wide[b, :need[b]])
        now = c.checkpoint()
        assert _same_stream(now, ck, 1)
        assert now["state"]["L"][0] == ck["state"]["L"][0] - 8 * need[0]
        fill[1] = start[1] - 8                                  # the next call, with room, takes it
        c.drain(slots, fill)
        got = buf.cpu().numpy()[16:16 + B * stride].reshape(B, stride)
        assert int(fill[1]) == stride and np.array_equal(got[1, start[1] - 8:], wide[1, :need[1]])
        assert c.checkpoint()["state"]["L"][1] == ck["state"]["L"][1] - 8 * need[1]


# ------------------------------------------------------------------ 7. checkpoint and set_output
@pytest.mark.parametrize("redirect", [False, True])
def test_checkpoint_after_a_drain_continues_in_a_fresh_context(redirect):
    from lac_amd.batch import BatchCoder, DrainSink
    V, B, T, prec, cut = 300, 9, 60, 48, 35
    rng = np.random.default_rng(70)
    pmf = rng.integers(1, 1000, size=(T, B, V)).astype(np.uint32)
    sym = rng.integers(0, V, size=(T, B)).astype(np.int32)
    want, wbits = _oracle(pmf, sym, prec)
    dp, ds = _dev(pmf), torch.from_numpy(sym).to(DEV)
    cap = 40 * (prec + 2) + 256

    def coder():
        c = BatchCoder(V, B, prec=prec, capacity_bits=cap, device=DEV)
        if redirect:
            c.set_output(torch.zeros(c.output_words(), dtype=torch.int64, device=DEV),
                         torch.zeros(B, dtype=torch.int64, device=DEV))
        return c

    with coder() as a:
        sink = _drive(a, cut, 7, lambda s, e: a.encode(dp[s:e], ds[s:e]))
        ck = a.checkpoint()
        parts = [bytes(p) for p in sink.parts]
        assert min(len(p) for p in parts) > 0
    with coder() as b:
        b.restore(ck)
        sink = DrainSink(b)
        for t in range(cut, T):
            b.encode(dp[t:t + 1], ds[t:t + 1])
            if t % 7 == 0:
                sink.pull()
        tail, tbits = sink.finish()
        assert [p + t for p, t in zip(parts, tail)] == want
        assert (tbits + 8 * np.array([len(p) for p in parts], dtype=np.uint64) == wbits).all()


# ------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_state_unchanged():
    from lac_amd.batch import BatchCoder
    V, B, T, prec = 100, 4, 30, 48
    rng = np.random.default_rng(8)
    pmf = rng.integers(1, 1000, size=(T, B, V)).astype(np.uint32)
    sym = rng.integers(0, V, size=(T, B)).astype(np.int32)
    dp, ds = _dev(pmf), torch.from_numpy(sym).to(DEV)
    with BatchCoder(V, B, prec=prec, capacity_bits=T * (prec + 2) + 256, device=DEV) as c:
        out = torch.full((B, c.bits_stride() + 8), SENTINEL, dtype=torch.uint8, device=DEV)
        fill = torch.zeros(B, dtype=torch.int64, device=DEV)
        drain = lambda dst, stride, f: c.lib.lac_encode_drain(c.ctx, dst, stride, f, c._stream)   # noqa: E731
        po, pf, stride = out.data_ptr(), fill.data_ptr(), out.shape[1]
        c.reset()
        c.encode(dp, ds)
        ck = c.checkpoint()

        def same():
            now = c.checkpoint()
            torch.cuda.synchronize()
            return (np.array_equal(now["state"], ck["state"]) and np.array_equal(now["planes"], ck["planes"])
                    and not fill.any() and bool((out == SENTINEL).all()))

        assert drain(None, stride, C.c_void_p(pf)) == LAC_E_ARG and same()
        assert drain(C.c_void_p(po), stride, None) == LAC_E_ARG and same()
        assert drain(C.c_void_p(po + 4), stride, C.c_void_p(pf)) == LAC_E_ARG and same()
        assert drain(C.c_void_p(po), stride - 4, C.c_void_p(pf)) == LAC_E_ARG and same()
        with pytest.raises(ValueError):
            c.drain(out[:, :-4], fill)
        with pytest.raises(TypeError):
            c.drain(out, fill.to(torch.int32))
        with pytest.raises(ValueError):
            c.drain(out[:-1], fill)
        assert same()
        # after a finish with no reset since: plane A holds packed bytes
        c.finish()
        ck = c.checkpoint()
        assert drain(C.c_void_p(po), stride, C.c_void_p(pf)) == LAC_E_STATE and same()
        bits, nb = c.bits_tensor(), c.nbits_tensor()
        # while a decode is open
        c.decode_open()
        assert drain(C.c_void_p(po), stride, C.c_void_p(pf)) == LAC_E_STATE
        torch.cuda.synchronize()
        assert not fill.any() and bool((out == SENTINEL).all())
        assert torch.equal(c.bits_tensor(), bits) and torch.equal(c.nbits_tensor(), nb)
        # a reset, and the drain is taken again
        c.reset()
        c.encode(dp, ds)
        assert drain(C.c_void_p(po), stride, C.c_void_p(pf)) == 0
        assert bool(fill.any())


# ------------------------------------------------------------------ 9. LogitsCompressor
def test_logits_compressor_with_drains():
    from lac_amd.llm import LogitsCompressor, TinyCausalLM
    V, B, T = 512, 2, 40
    model = TinyCausalLM(vocab=V, max_len=64, seed=3, d=32, layers=1, heads=2).to(DEV).eval()
    tokens = torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(4))
    plain = LogitsCompressor(model, V, prec=48, device=DEV)
    want, wbits = plain.compress(tokens)
    lc = LogitsCompressor(model, V, prec=48, device=DEV, drain_every=8)
    got, gbits = lc.compress(tokens)
    assert got == want and (np.asarray(gbits) == np.asarray(wbits)).all()
    assert int(np.asarray(wbits).min()) > 64                    # more than a word each: the drains had work
    assert torch.equal(lc.decompress(got, gbits, T).cpu(), tokens)
