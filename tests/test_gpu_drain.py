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


# ------------------------------------------------------------------ 10. more than one block of 64 words
# k_enc_drain works in blocks of 64 plane words (guard search, block_carries with a scalar carry
# between blocks, the move loop); the cases above hold a few words per stream.  Here the planes
# hold 60..200 words, planted with restore(); the reference is Python integers.
WORDS = 208                                                     # the planted coder's capacity
PREC_P = 48
OPEN_P = ((1 << PREC_P) - 10, (1 << PREC_P) - 10 + (1 << (PREC_P - 1)) + 5)   # h >= 2^prec: not certain
CERTAIN_P = (5, (1 << (PREC_P - 1)) + 100)


def _top_bits(L, pattern=ONES):
    """An active word: `pattern` cut to the bits the word holds when the stream is L bits long."""
    used = ((L - 1) & 63) + 1
    return (pattern >> (64 - used)) << (64 - used) & ONES


def _last_bit(L):
    return 1 << (63 - ((L - 1) & 63))


def _reference(regs, L, A, C, prec=PREC_P):
    """R = A + C + flush * 2^pad in Python integers -> (bytes, bit count), finish_stream's result."""
    digits = _flush_digits(*regs, prec)
    F = 0
    for d in digits:
        F = 2 * F + d
    Lf = L + len(digits)
    nwords = (Lf + 63) // 64
    val = lambda ws: sum(int(w) << (64 * (nwords - 1 - i)) for i, w in enumerate(ws))   # noqa: E731
    R = val(A) + val(C) + (F << (nwords * 64 - Lf))
    assert 0 <= R < 1 << (64 * nwords) and len(A) == len(C) == ((L - 1) >> 6) + 1 <= nwords
    return R.to_bytes(8 * nwords, "big")[:(Lf + 7) // 8], Lf


def _settled(regs, L, A, C, prec=PREC_P):
    """The two rules of lac_drain.h restated: the words a drain emits."""
    wlast = (L - 1) >> 6
    if L <= 64:
        return 0
    if regs[0] >= 0 and regs[1] < 1 << prec:
        return wlast
    for i in range(wlast - 1, -1, -1):
        if (int(A[i]) + int(C[i])) & ONES not in (0, ONES):
            return i
    return 0


def _planted(cases, words):
    """cases: [(registers, L, A words 0..wlast, C words 0..wlast)] -> a checkpoint of a coder of `words`
    words holding one per stream."""
    from lac_amd.batch import ENC_STATE
    st = np.zeros(len(cases), dtype=ENC_STATE)
    planes = np.zeros((2, len(cases), words), dtype=np.uint64)
    for b, ((l, h), L, A, C) in enumerate(cases):
        st[b] = (l, h, L, A[-1], C[-1], 7, 0, -1, -1, [0] * 8)
        planes[0, b, :len(A)], planes[1, b, :len(C)] = A, C
    return {"state": st, "planes": planes, "prec": PREC_P, "vocab": 16}


def _planted_coder(n):
    from lac_amd.batch import BatchCoder
    c = BatchCoder(16, n, prec=PREC_P, capacity_bits=WORDS * 64, device=DEV)
    assert c.bits_stride() // 8 >= WORDS
    return c


def _drain_planted(cases):
    """Plant, finish with no drain; plant again, drain once, finish: both are the reference's bytes,
    and the drain emitted the words the rules name.  -> g per stream."""
    from lac_amd.batch import DrainSink
    want = [_reference(*case) for case in cases]
    gs = [_settled(*case) for case in cases]
    with _planted_coder(len(cases)) as c:
        ck = _planted(cases, c.bits_stride() // 8)
        c.restore(ck)
        c.finish()
        plain, pbits = c.to_bytes()
        assert [int(v) for v in pbits] == [w[1] for w in want] and plain == [w[0] for w in want]
        c.reset()
        c.restore(ck)
        sink = DrainSink(c)
        n = sink.pull()
        assert n.tolist() == [8 * g for g in gs]
        assert c.checkpoint()["state"]["L"].tolist() == [case[1] - 64 * g for case, g in zip(cases, gs)]
        for b, (g, (data, _)) in enumerate(zip(gs, want)):      # the drained words are already final
            assert bytes(sink.parts[b]) == data[:8 * g], b
        got, gbits = sink.finish()
        assert [int(v) for v in gbits] == [w[1] for w in want]
        bad = [b for b in range(len(cases)) if got[b] != want[b][0]]
        assert not bad, bad
    return gs


def _random_words(rng, n):
    return [int(v) for v in rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * 2 + rng.integers(0, 2, size=n,
                                                                                                  dtype=np.uint64)]


def test_drain_guard_far_below_the_active_word():
    """Open registers, L = 150 * 64 + 20: words 4..149 all ones, the guard at word 3, a pending C
    bit on the active word.  The guard search crosses two whole blocks without a hit, the move
    loop moves three blocks of kept words, and the finish ripples the carry through them."""
    L = 150 * 64 + 20
    A = [5, 0x77, 9, 0x1234] + [ONES] * 146 + [_top_bits(L)]
    C = [0] * 150 + [_last_bit(L)]
    assert _drain_planted([(OPEN_P, L, A, C)]) == [3]


def test_drain_certain_carry_through_149_words():
    """Certain registers: word 148 generates (A all ones, C = 1: its low word is 0, no guard), words
    1..147 are all ones, word 0 = 5.  g = wlast = 149: three blocks resolved, the scalar carry
    crossing both block edges into word 0."""
    L = 149 * 64 + 20
    A = [5] + [ONES] * 148 + [_top_bits(L, 0xABCDE << 44)]
    C = [0] * 148 + [1, 0]
    assert _drain_planted([(CERTAIN_P, L, A, C), (OPEN_P, L, A, C)]) == [149, 0]
    want, _ = _reference(CERTAIN_P, L, A, C)
    assert want[:8] == (6).to_bytes(8, "big") and want[8:149 * 8] == bytes(148 * 8)


def test_drain_chains_on_block_edges():
    """With g words drained, block k of the resolve loop holds words g - 64 k - 1 (lane 0) down to
    g - 64 k - 64 (lane 63).  A generate in the last lane of a block with the propagate run ending
    in the first lane of the next; the mirror image (generate in a block's first lane, the run
    ending in that block); runs that cover a whole block or two.  Each in both register kinds: open,
    the guard is word g above the chain and g words drain; certain, g + 1 words drain, which moves
    every chain one lane on, so each edge is met from both sides."""
    cases = []
    for g in (140, 129):
        for gen, run, tail in ((g - 64, 1, 0), (g - 63, 1, 0), (g - 65, 1, 0), (g - 65, 63, 0), (g - 1, 64, 0),
                               (g - 64, 64, 0), (g - 1, 127, 0), (g - 63, 1, 1)):
            rng = np.random.default_rng(gen * 1000 + run)
            L = (g + 1) * 64 + 9
            A = [w | 2 for w in _random_words(rng, g)] + [0x42, _top_bits(L, 0x5A5A << 48)]   # (no chance all-ones)
            C = [0] * (g + 2)
            A[0] = 3
            A[gen], C[gen] = ONES - 6, 7 + tail                 # wraps: generates, low word 0 or 1
            for i in range(gen - run, gen):
                A[i] = ONES                                     # the propagate run; the word below it absorbs
            cases.append((CERTAIN_P, L, A, C))
            # open: word g (0x42) is the guard, the same chain below it
            cases.append((OPEN_P, L, A, C))
    gs = _drain_planted(cases)
    assert gs[::2] == [141] * 8 + [130] * 8                     # certain: all but the active word
    assert gs[1::2] == [140] * 8 + [129] * 8                    # open: up to the guard


@pytest.mark.parametrize("g", [63, 64, 65, 128, 129])
def test_drain_exactly_g_words(g):
    """g on either side of one and two blocks: by rule 2 (certain, g = wlast) and by rule 1 (the
    guard at word g under all-ones / all-zero words up to the active one)."""
    rng = np.random.default_rng(g)
    L = g * 64 + 33
    A = _random_words(rng, g) + [_top_bits(L, 0x123456789 << 28)]
    A[0] = 1
    certain = (CERTAIN_P, L, A, [0] * (g + 1))
    cases = [certain]
    for above, fillw in ((1, ONES), (3, 0), (64, ONES), (65, ONES), (70, 0)):
        wl = g + above                                          # the guard is `above` words below the active word
        L2 = wl * 64 + 20
        A2 = _random_words(rng, g) + [0x1234] + [fillw] * (above - 1) + [_top_bits(L2)]
        A2[0] = 1
        C2 = [0] * wl + [_last_bit(L2)]
        cases.append((OPEN_P, L2, A2, C2))
    assert _drain_planted(cases) == [g] * 6


def test_drain_guard_in_the_last_lane_of_block_one_and_the_first_of_block_two():
    """The guard search's lane j of its first block is word wlast - 1 - j: a guard 64 words below the
    active word sits in the block's last lane, one 65 below in the next block's first; everything
    above it is all ones.  wlast = 64 / 65 / 66 put those guards at words 0, 1 and 2."""
    cases = []
    for wl in (100, 64, 65, 66, 129):
        for below in (64, 65):
            if wl - below < 0:
                continue
            L = wl * 64 + 1
            A = [ONES] * wl + [_top_bits(L)]
            A[0] = 2
            A[wl - below] = 0x99 if wl - below else 2
            cases.append((OPEN_P, L, A, [0] * wl + [_last_bit(L)]))
    gs = _drain_planted(cases)
    assert gs == [36, 35, 0, 1, 0, 2, 1, 65, 64]


def test_drain_slot_fits_more_than_a_block_exactly_or_not_at_all():
    """g = 100 words behind a non-zero fill: a slot with exactly 800 bytes of room takes them, one
    with 792 takes nothing and the stream stays as it was; the bytes around the slots stay."""
    rng = np.random.default_rng(100)
    g, B = 100, 4
    L = g * 64 + 40
    cases = []
    for b in range(B):
        A = _random_words(rng, g) + [_top_bits(L, 0xF0F0F0F0F0 << 24)]
        A[0] = 7
        cases.append((CERTAIN_P, L, A, [1 if i % 5 == 0 else 0 for i in range(g)] + [0]))
    want = [_reference(*case)[0] for case in cases]
    with _planted_coder(B) as c:
        ck = _planted(cases, c.bits_stride() // 8)
        c.restore(ck)
        stride = 8 * g + 48
        buf = torch.full((16 + B * stride + 16,), SENTINEL, dtype=torch.uint8, device=DEV)
        slots = buf[16:16 + B * stride].view(B, stride)
        start = np.array([48, 56, 40, 48], dtype=np.int64)      # exact, one word short, a word to spare, exact
        fill = torch.from_numpy(start.copy()).to(DEV)
        c.drain(slots, fill)
        got, f = buf.cpu().numpy(), fill.cpu().numpy()
        body = got[16:16 + B * stride].reshape(B, stride)
        assert (got[:16] == SENTINEL).all() and (got[16 + B * stride:] == SENTINEL).all()
        assert f.tolist() == [stride, 56, 40 + 8 * g, stride]
        now = c.checkpoint()
        for b in range(B):
            assert (body[b, :start[b]] == SENTINEL).all() and (body[b, f[b]:] == SENTINEL).all()
            if b == 1:
                assert (body[b] == SENTINEL).all() and _same_stream(now, ck, b)
            else:
                assert body[b, start[b]:f[b]].tobytes() == want[b][:8 * g], b
                assert now["state"]["L"][b] == L - 64 * g
        fill[1] = 48                                            # the next call, with room, takes it
        c.drain(slots, fill)
        assert int(fill[1]) == stride
        assert buf.cpu().numpy()[16 + stride:16 + 2 * stride][48:].tobytes() == want[1][:8 * g]
        c.finish()
        tail, _ = c.to_bytes()
        assert [want[b][:8 * g] + tail[b] for b in range(B)] == want


def test_drain_random_planes_of_200_words():
    """20 seeded streams of 200 words: random A, sparse C bits, planted runs of all-ones and
    all-zero words (some right below the active word, some across block edges); both rules."""
    rng = np.random.default_rng(2026)
    cases = []
    for s in range(20):
        wl = 199 + int(rng.integers(0, 5))
        L = wl * 64 + int(rng.integers(1, 65))
        A = _random_words(rng, wl) + [_top_bits(L, int(rng.integers(0, 1 << 63)) * 2 + 1)]
        C = [(1 << int(rng.integers(0, 64))) if rng.random() < 0.1 else 0 for _ in range(wl)] + [
            _last_bit(L) if rng.random() < 0.5 else 0]
        for _ in range(int(rng.integers(1, 5))):                # runs of propagating / empty words
            a = int(rng.integers(1, wl))
            n = int(rng.integers(1, 90))
            fillw = ONES if rng.random() < 0.7 else 0
            for i in range(a, min(a + n, wl)):
                A[i], C[i] = fillw, 0
            if rng.random() < 0.5 and a + n < wl:               # a generate feeding the run
                A[min(a + n, wl - 1)], C[min(a + n, wl - 1)] = ONES, 1 << int(rng.integers(0, 8))
        if s % 4 < 2:                                           # nothing but a run up to the active word
            top = int(rng.integers(1, 140))
            for i in range(wl - top, wl):
                A[i], C[i] = ONES, 0
        A[0], C[0] = int(rng.integers(1, 1 << 32)), 0           # room for the last carry
        cases.append((OPEN_P if s % 2 else CERTAIN_P, L, A, C))
    gs = _drain_planted(cases)
    assert len({g // 64 for g in gs}) >= 3 and min(gs[1::2]) < 128 < max(gs), gs


def test_bounded_coder_drains_a_hundred_words_at_a_time():
    """The u64 tables of _int_case (~22 bits per symbol) in a coder sized for 300 steps, drained every
    300 steps: every drain moves more than one block of words per stream."""
    from lac_amd.batch import BatchCoder, DrainSink
    dp, ds, want, wbits = _int_case(64)
    cap = 300 * (PREC1 + 2) + 256
    with BatchCoder(V1, B1, prec=PREC1, pmf_bits=64, capacity_bits=cap, device=DEV) as c:
        sink = DrainSink(c)
        c.reset()
        moved = []
        for t in range(0, T1, 300):
            c.encode(dp[t:t + 300], ds[t:t + 300])
            moved.append(sink.pull())
        got, gbits = sink.finish()
        assert (gbits == wbits).all()
        assert got == want
        assert len(moved) == 2 and all(int(n.min()) > 64 * 8 for n in moved), [int(n.min()) for n in moved]
