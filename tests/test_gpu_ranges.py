"""Range-level coding on the device (include/lac.h lac_encode_ranges / lac_decode_ranges_step,
BatchCoder.encode_ranges / encode_ranges_job / decode_ranges_step, lac_amd.ranges).

Expected values come only from the reference's fixtures (tests/golden/range_cases.json and the
existing table fixtures whose every total is at most 2^(prec-1)), the C oracle, and this library's
pmf path on the V = 4 tables [lo, hi - lo, T - hi, 0] with symbol 1 -- the table a triple stands
for (lac_amd/csrc/lac_ranges.h).  Integer work: everything is compared bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import ranges as R
from errors import dec_state, set_dec_state, stream_bytes, written
from oracle import oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LAC_E_ARG, LAC_E_ZERO_WIDTH, LAC_E_TABLE, LAC_E_DECODE_RANGE, LAC_E_CAPACITY, LAC_E_STATE = -1, -4, -5, -6, -7, -9
LAC_E_UNDETERMINED = -12
ENC_FIELDS = ("l", "h", "L", "wa", "wc", "nsym", "nflush")
DEC_FIELDS = ("l", "h", "x", "pos", "nsym")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _coder(B, prec, cap=None, steps=130):
    from lac_amd.batch import BatchCoder
    return BatchCoder(4, B, prec=prec, pmf_bits=64, capacity_bits=cap or steps * (prec + 2) + 256, device=DEV)


def _dev(a):
    """Non-negative integers (numpy uint64 or Python ints) -> int64 device tensor, the same bits."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.uint64))
    return torch.from_numpy(a.view(np.int64)).to(DEV)


def _tables(lo, hi, tot):
    """[T, B] uint64 triples -> the V = 4 tables as a device tensor [T, B, 4] and the symbols (all 1)."""
    z = np.zeros_like(lo)
    rows = np.stack([lo, hi - lo, tot - hi, z], axis=-1)
    return _dev(rows), torch.ones(lo.shape, dtype=torch.int32, device=DEV)


def _digits(tr, b, n):
    from lac_amd.batch import digits_of
    return [digits_of(int(E), int(k)) for E, k in tr[:n, b, :].cpu().numpy()]


class Replay:
    """decode_loop's model for a job whose triples are known: every target names symbol 1."""

    def __init__(self, lo, hi, tot):
        self.lo, self.hi, self.tot = lo, hi, tot

    def total(self, t):
        return self.tot[t]

    def lookup(self, t, targets):
        return torch.ones_like(targets), self.lo[t], self.hi[t]


def _same_enc(a, b, fields=None, planes=True):
    """Two checkpoints: the state's fields and the planes' written words.  (planes=False after a
    finish: plane A then holds the bytes, compared as such, and the words of plane C that the
    flush digits reach were never written.)"""
    sa, sb = a["state"], b["state"]
    for f in fields or sa.dtype.names:
        assert np.array_equal(sa[f], sb[f]), (f, sa[f], sb[f])
    if planes:
        assert np.array_equal(written(a), written(b))


def mixed_triples(rng, T, B, prec):
    """Lanes in mixed states: T = 1 streams (zero bits per symbol) beside prec-1 bits per symbol,
    small totals and wide ranges; lo = 0 and hi = T occur."""
    half = 1 << (prec - 1)
    lo, hi, tot = (np.zeros((T, B), np.uint64), np.ones((T, B), np.uint64), np.ones((T, B), np.uint64))
    for b in range(B):
        k = b % 4
        if k == 0:
            continue
        if k == 1:
            t = np.full(T, half, np.uint64)
            l = rng.integers(0, half, T, dtype=np.uint64)
            h = l + np.uint64(1)
        else:
            t = rng.integers(1, 1 << 20 if k == 2 else half + 1, T, dtype=np.uint64)
            h = np.uint64(1) + rng.integers(0, t, dtype=np.uint64)
            l = rng.integers(0, h, dtype=np.uint64)
            l[0], h[-1] = 0, t[-1]
        lo[:, b], hi[:, b], tot[:, b] = l, h, t
    return lo, hi, tot


# ------------------------------------------------------------------ 1. the reference's fixtures
@pytest.mark.parametrize("case", R.RANGE_CASES, ids=[c["name"] for c in R.RANGE_CASES])
def test_formula_fixture(case):
    """encode_ranges_job gives the reference's bytes and L (and the oracle's digits on the
    three-entry rows); decode_loop returns the symbols; with set_decode_stop the stream stops at
    the reference's decoded_count."""
    from lac_amd.ranges import decode_loop
    n, prec = len(case["syms"]), case["prec"]
    lo, hi, T = R.case_triples(case)
    c = _coder(1, prec, steps=n + 8)
    tr = torch.zeros((n, 1, 2), dtype=torch.int64, device=DEV)
    c.encode_ranges_job(_dev(lo).view(n, 1), _dev(hi).view(n, 1), T[0], trace=tr)
    data, nb = c.to_bytes()
    assert int(nb[0]) == case["L"] and data[0].hex() == case["bytes"]
    _, _, digits = oracle.encode(R.three_rows(lo, hi, T), [1] * n, prec)
    flush = c.flush_digits()[0]
    assert sum(_digits(tr, 0, n), []) + flush == digits
    model = R.FormulaModel(case, 1, DEV)
    c.decode_open()
    assert decode_loop(c, n, model)[:, 0].tolist() == case["syms"]
    assert c.status()[0] == 0 and c.determined()[0] == n
    if case["L"]:                   # (a stream of no bits: the reference decides only when a bit arrives)
        dc = case["decoded_count"]
        c.set_decode_stop(True)
        c.decode_open()
        out = decode_loop(c, dc + 3, model)[:, 0].tolist()
        assert out[:n] == case["syms"] and all(s >= 0 for s in out[:dc]) and out[dc:] == [-1] * 3
        rc, err, step = c.status()
        assert (rc, int(step[0]), int(dec_state(c)["nsym"][0])) == (LAC_E_UNDETERMINED, dc, dc)
    c.close()


class TableModel:
    """decode_loop's model of a table job: cdf [T, B, V] on the device."""

    def __init__(self, cdf):
        self.cdf = cdf

    def total(self, t):
        return self.cdf[t, :, -1].contiguous()

    def lookup(self, t, targets):
        c = self.cdf[t]
        s = (c <= targets.clamp(min=0).unsqueeze(1)).sum(1).clamp(max=c.shape[1] - 1)
        hi = c.gather(1, s.unsqueeze(1)).squeeze(1)
        lo = torch.where(s > 0, c.gather(1, (s - 1).clamp(min=0).unsqueeze(1)).squeeze(1), torch.zeros_like(hi))
        return s, lo, hi


def _table_batch(cases, prec):
    """Fixtures of one prec as one ragged batch: stream b codes case b's symbols (its count), the
    steps past them a dummy row.  -> (pmf [T, B, V] int64 on the host, sym [T, B], counts)."""
    B, T = len(cases), max(len(c["syms"]) for c, _ in cases)
    V = max(r.shape[1] for _, r in cases)
    pmf = np.zeros((T, B, V), dtype=np.int64)
    pmf[:, :, 0] = 1
    sym = np.zeros((T, B), dtype=np.int64)
    for b, (c, rows) in enumerate(cases):
        n = len(c["syms"])
        r = rows if rows.shape[0] >= n else np.repeat(rows[:1], n, axis=0)
        pmf[:n, b, :] = 0
        pmf[:n, b, :r.shape[1]] = r[:n].astype(np.int64)
        sym[:n, b] = c["syms"]
    return torch.from_numpy(pmf), torch.from_numpy(sym), [len(c["syms"]) for c, _ in cases]


def _check_table_batch(cases, prec):
    from lac_amd.ranges import decode_loop, table_ranges
    pmf, sym, counts = _table_batch(cases, prec)
    T, B = sym.shape
    lo, hi, tot = (x.to(DEV) for x in table_ranges(pmf, sym))        # cumsum + gather on the host
    c = _coder(B, prec, steps=T)
    c.set_stream_lengths(counts)
    tr = torch.zeros((T, B, 2), dtype=torch.int64, device=DEV)
    c.encode_ranges_job(lo, hi, tot, trace=tr)
    data, nb = c.to_bytes()
    flush = c.flush_digits()
    for b, (case, _) in enumerate(cases):
        assert int(nb[b]) == case["L"] and data[b].hex() == case["bytes"], case.get("name", b)
        assert _digits(tr, b, counts[b]) == case["trace"] and flush[b] == case["flush"], case.get("name", b)
    c.decode_open()
    out = decode_loop(c, T, TableModel(torch.cumsum(pmf.to(DEV), dim=-1))).cpu().numpy()
    for b, (case, _) in enumerate(cases):
        assert out[:counts[b], b].tolist() == case["syms"] and (out[counts[b]:, b] == -1).all()
    assert c.status()[0] == 0
    c.close()


def test_small_fixtures_that_never_fudge():
    """The static and per-step cases of small_cases.json with every total <= 2^(prec-1) (the
    host census holds their number), one ragged batch per prec: bytes, L, traces, flush digits,
    decoded symbols."""
    small = R.small_qualifying()
    assert len(small["static"]) >= 90 and len(small["perstep"]) >= 40
    cases = [(c, np.array(c["rows"], dtype=np.int64)) for c in small["static"] + small["perstep"]]
    for prec in sorted({c["prec"] for c, _ in cases}):
        _check_table_batch([x for x in cases if x[0]["prec"] == prec], prec)


def test_generated_fixtures_that_never_fudge():
    gen = R.gen_qualifying()
    assert len(gen) == 7
    for case, rows in gen:
        _check_table_batch([(case, rows)], case["prec"])


# ------------------------------------------------------------------ 2. batch boundaries
def _counts(rng, T, B):
    n = rng.integers(0, T + 6, B)                                    # ends at different steps, beyond T included
    n[0], n[-1] = T + 5, 0 if B > 1 else T + 5
    if B > 2:
        n[1] = T
    return n.tolist()


@pytest.mark.parametrize("steps", (1, 63, 64, 65, 130))
@pytest.mark.parametrize("B,prec", ((1, 48), (63, 48), (64, 48), (65, 61), (255, 48), (256, 34), (257, 48)))
def test_batch_boundaries_equal_the_pmf_path(B, prec, steps):
    """Bytes, lac_enc_state and planes equal the pmf path's on the V = 4 tables, with per-stream
    counts that end lanes at different steps; and the decode's symbols, registers, status and
    determined counts equal lac_decode_steps'."""
    from lac_amd.ranges import decode_loop
    rng = np.random.default_rng(1000 * B + steps)
    lo, hi, tot = mixed_triples(rng, steps, B, prec)
    counts = _counts(rng, steps, B)
    dlo, dhi, dtot = _dev(lo), _dev(hi), _dev(tot)
    pmf, ones = _tables(lo, hi, tot)
    a, p = _coder(B, prec, steps=steps), _coder(B, prec, steps=steps)
    for c in (a, p):
        c.set_stream_lengths(counts)
        c.reset()
    a.encode_ranges(dlo, dhi, dtot)
    p.encode(pmf, ones)
    _same_enc(a.checkpoint(), p.checkpoint())
    a.finish()
    p.finish()
    da, na = a.to_bytes()
    dp, np_ = p.to_bytes()
    assert da == dp and np.array_equal(na, np_)
    _same_enc(a.checkpoint(), p.checkpoint(), planes=False)
    a.decode_open()
    p.decode_open()
    out = decode_loop(a, steps, Replay(dlo, dhi, dtot)).cpu().numpy()
    want = p.decode(pmf).cpu().numpy()
    assert np.array_equal(out, want)
    sa, sp = dec_state(a), dec_state(p)
    for f in sa.dtype.names:
        assert np.array_equal(sa[f], sp[f]), f
    assert a.status()[0] == p.status()[0] == 0 and np.array_equal(a.determined(), p.determined())
    a.close()
    p.close()


def test_total_strides():
    """tot as [steps, streams], as [streams] and as a Python int are the zero strides of the C call."""
    steps, B, prec = 65, 70, 48
    rng = np.random.default_rng(3)
    per = rng.integers(1, 1 << 30, B, dtype=np.uint64)
    hi = np.uint64(1) + rng.integers(0, np.broadcast_to(per, (steps, B)), dtype=np.uint64)
    lo = rng.integers(0, hi, dtype=np.uint64)
    c = _coder(B, prec, steps=steps)
    c.encode_ranges_job(_dev(lo), _dev(hi), _dev(np.broadcast_to(per, (steps, B))))
    full = c.to_bytes()[0]
    c.encode_ranges_job(_dev(lo), _dev(hi), _dev(per))
    assert c.to_bytes()[0] == full
    one = 1 << 30
    hi1 = np.uint64(1) + rng.integers(0, one, (steps, B), dtype=np.uint64)
    lo1 = rng.integers(0, hi1, dtype=np.uint64)
    c.encode_ranges_job(_dev(lo1), _dev(hi1), _dev(np.full((steps, B), one, np.uint64)))
    full = c.to_bytes()[0]
    c.encode_ranges_job(_dev(lo1), _dev(hi1), one)
    assert c.to_bytes()[0] == full
    c.close()


# ------------------------------------------------------------------ 3. cut jobs
def test_cut_jobs():
    """Calls of 50 + 80 steps equal one call of 130: plain, mixed with lac_encode steps, with a
    drain in between, and across checkpoint / restore."""
    from lac_amd.batch import DrainSink
    steps, B, prec, cut = 130, 70, 48, 50
    rng = np.random.default_rng(5)
    lo, hi, tot = mixed_triples(rng, steps, B, prec)
    dlo, dhi, dtot = _dev(lo), _dev(hi), _dev(tot)
    pmf, ones = _tables(lo, hi, tot)
    whole = _coder(B, prec)
    whole.encode_ranges_job(dlo, dhi, dtot)
    data, nb = whole.to_bytes()
    head = (dlo[:cut], dhi[:cut], dtot[:cut])
    tail = (dlo[cut:], dhi[cut:], dtot[cut:])
    c = _coder(B, prec)
    for kind in ("plain", "pmf_tail", "pmf_head", "drain", "restore"):
        c.reset()
        sink = DrainSink(c) if kind == "drain" else None
        if kind == "pmf_head":
            c.encode(pmf[:cut], ones[:cut])
        else:
            c.encode_ranges(*head)
        if kind == "drain":
            assert sink.pull().any()
        if kind == "restore":
            ck = c.checkpoint()
            c.reset()
            c.encode_ranges(*tail)                                   # something else in between
            c.restore(ck)
        if kind == "pmf_tail":
            c.encode(pmf[cut:], ones[cut:])
        else:
            c.encode_ranges(*tail)
        if kind == "drain":
            got, n = sink.finish()
        else:
            c.finish()
            got, n = c.to_bytes()
        assert got == data and np.array_equal(np.asarray(n, dtype=np.uint64), np.asarray(nb, dtype=np.uint64)), kind
    c.close()
    whole.close()


# ------------------------------------------------------------------ 4. errors
POSITIONS = (0, 62, 63, 64, 126, 127)                                # first, next-to-last, last step of a 64-step block


def _defect(cause, lo, hi, tot, half):
    if cause == "T0":
        return lo, hi, 0
    if cause == "Tbig":
        return lo, hi, half + 1
    if cause == "hi>T":
        return lo, tot + 1, tot
    if cause == "lo>hi":
        return hi, lo, tot
    return lo, lo, tot                                               # "lo==hi"


def test_encode_errors_beside_clean_lanes():
    """One defect per failing stream at the first, last and next-to-last step of a 64-step block,
    beside clean lanes of the same wave: status, err_step, and the frozen state -- which is the
    state of a stream whose count ends at that step -- with the neighbours unaffected."""
    steps, B, prec = 130, 64, 48
    half = 1 << (prec - 1)
    rng = np.random.default_rng(9)
    lo, hi, tot = mixed_triples(rng, steps, B, prec)
    good = (lo.copy(), hi.copy(), tot.copy())
    causes = ("T0", "Tbig", "hi>T", "lo>hi", "lo==hi")
    want_err, want_step = np.zeros(B, np.int32), np.full(B, -1, np.int64)
    b = 1
    for cause in causes:
        for pos in POSITIONS:
            l, h, t = _defect(cause, int(lo[pos, b]), int(hi[pos, b]), int(tot[pos, b]), half)
            lo[pos, b], hi[pos, b], tot[pos, b] = l, h, t
            want_err[b] = LAC_E_ZERO_WIDTH if cause == "lo==hi" else LAC_E_TABLE
            want_step[b] = pos
            b += 2                                                   # every other lane stays clean
    assert b <= B + 1 and (want_err != 0).sum() == 30
    a, p = _coder(B, prec), _coder(B, prec)
    a.reset()
    a.encode_ranges(_dev(lo), _dev(hi), _dev(tot))
    rc, err, step = a.status()
    assert rc == int(want_err[np.flatnonzero(want_err)[0]]) or rc in (LAC_E_TABLE, LAC_E_ZERO_WIDTH)
    assert np.array_equal(err, want_err) and np.array_equal(step, want_step)
    # the yardstick: the pmf path on the clean tables, the failing streams' counts ending at the defect
    pmf, ones = _tables(*good)
    p.set_stream_lengths(np.where(want_err != 0, want_step, steps).tolist())
    p.reset()
    p.encode(pmf, ones)
    _same_enc(a.checkpoint(), p.checkpoint(), fields=ENC_FIELDS)
    # a failed stream stays frozen under more steps; its neighbours go on
    a.encode_ranges(*(x[:3].contiguous() for x in (_dev(good[0]), _dev(good[1]), _dev(good[2]))))
    p.set_stream_lengths(np.where(want_err != 0, want_step, steps + 3).tolist())
    p.encode(pmf[:3].contiguous(), ones[:3].contiguous())
    _same_enc(a.checkpoint(), p.checkpoint(), fields=ENC_FIELDS)
    assert np.array_equal(a.status()[1], want_err) and np.array_equal(a.status()[2], want_step)
    a.close()
    p.close()


def test_precedence_of_a_triple_with_two_defects():
    prec = 16
    half = 1 << 15
    c = _coder(4, prec, steps=2)
    c.reset()
    #            T = 0 and lo == hi   hi > T and lo == hi   lo == hi alone    clean
    lo, hi, tot = [0, half + 1, 7, 3], [0, half + 1, 7, 9], [0, half, 20, 20]
    c.encode_ranges(_dev(lo), _dev(hi), _dev(tot))
    assert c.status()[1].tolist() == [LAC_E_TABLE, LAC_E_TABLE, LAC_E_ZERO_WIDTH, 0]
    assert c.status()[2].tolist() == [0, 0, 0, -1]
    c.close()


def test_capacity_failures_equal_the_pmf_path():
    """A capacity of four words; stream b codes 6 (b mod 8) bits per symbol, so seven kinds of
    stream fail at seven different steps and the zero-bit streams never: status, err_step,
    registers and planes are lac_encode's on the tables."""
    steps, B, prec = 130, 64, 48
    half = 1 << (prec - 1)
    rng = np.random.default_rng(11)
    width = np.array([half >> (6 * (b % 8)) for b in range(B)], dtype=np.uint64)
    tot = np.full((steps, B), half, np.uint64)
    lo = rng.integers(0, np.broadcast_to(np.uint64(half) - width + np.uint64(1), (steps, B)), dtype=np.uint64)
    hi = lo + width
    pmf, ones = _tables(lo, hi, tot)
    a, p = _coder(B, prec, cap=256), _coder(B, prec, cap=256)
    a.reset()
    p.reset()
    a.encode_ranges(_dev(lo), _dev(hi), _dev(tot))
    p.encode(pmf, ones)
    sa, sp = a.status(), p.status()
    assert sa[0] == sp[0] == LAC_E_CAPACITY and np.array_equal(sa[1], sp[1]) and np.array_equal(sa[2], sp[2])
    assert (sa[1] == LAC_E_CAPACITY).sum() == B - B // 8 and (sa[1][::8] == 0).all()
    assert len(set(sa[2][sa[1] != 0].tolist())) >= 7
    _same_enc(a.checkpoint(), p.checkpoint())
    a.finish()
    p.finish()
    assert stream_bytes(a)[0] == stream_bytes(p)[0]
    a.close()
    p.close()


def _encoded(steps, B, prec, seed):
    rng = np.random.default_rng(seed)
    lo, hi, tot = mixed_triples(rng, steps, B, prec)
    c = _coder(B, prec, steps=steps)
    d = (_dev(lo), _dev(hi), _dev(tot))
    c.encode_ranges_job(*d)
    return c, (lo, hi, tot), d


def _step_through(c, d, steps, probe=None):
    """The serving loop by hand: -> targets [steps, B] as numpy int64.  probe(t) runs before call t
    (t = steps: the last symbol's advance)."""
    out, prev = [], None
    for t in range(steps):
        if probe:
            probe(t)
        out.append(c.decode_ranges_step(prev, d[2][t]).cpu().numpy())
        prev = (d[0][t], d[1][t], d[2][t])
    if probe:
        probe(steps)
    c.decode_ranges_step(prev, None)
    return np.stack(out)


def test_decode_errors():
    """Corrupt bits, a range that misses the target, an invalid total at the peek, and x outside
    [l, h]: the code, err_step, and the stream frozen as before the step; neighbours unaffected."""
    steps, B, prec = 40, 66, 48
    half = 1 << (prec - 1)
    c, (lo, hi, tot), d = _encoded(steps, B, prec, 13)
    bits, nbits = c.bits_tensor(), c.nbits_tensor().clone()
    # the clean decode, with every stream's state before each step
    c.decode_open(bits, nbits)
    snaps = []
    clean = _step_through(c, d, steps, probe=lambda t: snaps.append(dec_state(c)))
    final = dec_state(c)
    assert c.status()[0] == 0 and (final["nsym"] == steps).all()
    # (call t advances symbol t - 1 and peeks position t: the state before symbol k is the one call k + 1 met)
    before = snaps[1:] + [final]
    assert all((before[k]["nsym"] == k).all() for k in range(steps + 1))
    assert ((clean >= lo.astype(np.int64)) & (clean < hi.astype(np.int64))).all()

    # (a) corrupt bits in stream 5 (47 bits per symbol: b % 4 == 1): its 3rd symbol's bits flipped
    bad = bits.clone()
    bad[5, 12:16] ^= 0xFF
    c.decode_open(bad, nbits)
    got = _step_through(c, d, steps)
    st, (rc, err, step) = dec_state(c), c.status()
    k = int(step[5])
    assert rc == LAC_E_DECODE_RANGE and err[5] == LAC_E_DECODE_RANGE and 1 <= k <= 3 and (np.delete(err, 5) == 0).all()
    assert st["nsym"][5] == k and not lo[k, 5] <= got[k, 5] < hi[k, 5] and (got[k + 1:, 5] == -1).all()
    assert np.array_equal(np.delete(got, 5, axis=1), np.delete(clean, 5, axis=1))
    for f in DEC_FIELDS:
        assert np.array_equal(np.delete(st[f], 5), np.delete(final[f], 5)), f

    # (b) a range that misses the target at step 7 (stream 6), (c) an empty range (stream 7),
    # (d) an invalid triple at step 9 (stream 10): hi > T
    l2, h2 = lo.copy(), hi.copy()
    l2[7, 6], h2[7, 6] = hi[7, 6], hi[7, 6] + np.uint64(1)           # the next symbol's range
    h2[7, 7] = l2[7, 7]
    h2[9, 10] = tot[9, 10] + np.uint64(1)
    assert hi[7, 6] < tot[7, 6]
    d2 = (_dev(l2), _dev(h2), d[2])
    c.decode_open(bits, nbits)
    _step_through(c, d2, steps)
    st, (rc, err, step) = dec_state(c), c.status()
    want = {6: (LAC_E_DECODE_RANGE, 7), 7: (LAC_E_DECODE_RANGE, 7), 10: (LAC_E_TABLE, 9)}
    for b in range(B):
        code, k = want.get(b, (0, -1))
        assert (err[b], step[b]) == (code, k), b
        ref = final if k < 0 else before[k]
        for f in DEC_FIELDS:
            assert st[f][b] == ref[f][b], (b, f)

    # (e) an invalid total at the peek: UINT64_MAX and no error yet; the advance that uses it raises it
    c.decode_open(bits, nbits)
    t0 = d[2][0].clone()
    t0[3], t0[4] = 0, half + 1
    tg = c.decode_ranges_step(None, t0).cpu().numpy()
    assert tg[3] == tg[4] == -1 and np.array_equal(np.delete(tg, (3, 4)), np.delete(clean[0], (3, 4)))
    assert c.status()[0] == 0
    c.decode_ranges_step((d[0][0], d[1][0], t0), d[2][1])
    rc, err, step = c.status()
    assert err[3] == err[4] == LAC_E_TABLE and step[3] == step[4] == 0 and (np.delete(err, (3, 4)) == 0).all()
    st = dec_state(c)
    for f in DEC_FIELDS:
        assert st[f][3] == before[0][f][3] and st[f][5] == before[1][f][5], f

    # (f) x outside [l, h] via set_state: no target, LAC_E_DECODE_RANGE at the advance
    c.decode_open(bits, nbits)
    st = dec_state(c)
    st["x"][2] = st["h"][2] + 1
    set_dec_state(c, st)
    tg = c.decode_ranges_step(None, d[2][0]).cpu().numpy()
    assert tg[2] == -1 and tg[1] == clean[0, 1] and c.status()[0] == 0
    c.decode_ranges_step((d[0][0], d[1][0], d[2][0]), None)
    rc, err, step = c.status()
    assert err[2] == LAC_E_DECODE_RANGE and step[2] == 0 and (np.delete(err, 2) == 0).all()
    after = dec_state(c)
    for f in DEC_FIELDS:
        assert after[f][2] == st[f][2], f
    c.close()


# ------------------------------------------------------------------ 5. decode details
def test_peek_is_idempotent_and_equals_python_integers():
    steps, B, prec = 20, 65, 61
    c, (lo, hi, tot), d = _encoded(steps, B, prec, 17)
    c.decode_open()
    prev = None
    for t in range(steps):
        if prev is not None:
            c.decode_ranges_step(prev, None)                         # the advance half alone
        before = dec_state(c)
        tg1 = c.decode_ranges_step(None, d[2][t]).cpu().numpy()      # the peek half alone, twice
        tg2 = c.decode_ranges_step(None, d[2][t]).cpu().numpy()
        after = dec_state(c)
        assert np.array_equal(tg1, tg2)
        for f in before.dtype.names:
            assert np.array_equal(before[f], after[f]), f
        want = [((int(s["x"]) - int(s["l"])) * int(T)) // (int(s["h"]) - int(s["l"]) + 1) for s, T in zip(after, tot[t])]
        assert tg1.tolist() == want
        prev = (d[0][t], d[1][t], d[2][t])
    c.close()


def test_windowed_decode_with_refills():
    """A coder whose capacity holds 8 steps of bits, a refill every 8 steps: the whole-stream
    decode's targets, registers (pos + 64 base), status and determined counts."""
    from lac_amd.batch import BatchCoder
    steps, B, prec, N = 130, 66, 48, 8
    c, (lo, hi, tot), d = _encoded(steps, B, prec, 19)
    bits, nbits = c.bits_tensor(), c.nbits_tensor().clone()
    c.decode_open(bits, nbits)
    clean = _step_through(c, d, steps)
    want, ndet = dec_state(c), c.determined()
    with BatchCoder(4, B, prec=prec, pmf_bits=64, capacity_bits=N * (prec + 2) + 256, device=DEV) as w:
        w.decode_open_window(bits, nbits)
        got = _step_through(w, d, steps, probe=lambda t: w.refill() if t and t % N == 0 else None)
        w.refill()
        assert w.status()[0] == 0 and np.array_equal(got, clean)
        st = dec_state(w)
        st["pos"] += np.uint64(64) * w.window_base().astype(np.uint64)
        for f in st.dtype.names:
            assert np.array_equal(st[f], want[f]), f
        assert np.array_equal(w.determined(), ndet)
    c.close()


def test_decode_of_a_packed_job():
    """lac_decode_open_packed in front of the range-level decode."""
    steps, B, prec = 30, 65, 48
    c, (lo, hi, tot), d = _encoded(steps, B, prec, 21)
    payload = torch.zeros(B * c.bits_stride() + 4 * B + 64, dtype=torch.uint8, device=DEV)
    length = torch.zeros(1, dtype=torch.int64, device=DEV)
    c.pack_bits(payload, 4, length)
    c.decode_open()
    clean = _step_through(c, d, steps)
    c.decode_open_packed(payload, 4)
    assert np.array_equal(_step_through(c, d, steps), clean) and c.status()[0] == 0
    c.close()


# ------------------------------------------------------------------ 6. refusals and launches
def test_refusals_launch_nothing_and_change_nothing():
    from lac_amd._lib import LacError
    steps, B, prec = 5, 3, 48
    rng = np.random.default_rng(23)
    lo, hi, tot = (_dev(x) for x in mixed_triples(rng, steps, B, prec))
    c = _coder(B, prec)
    c.reset()
    c.encode_ranges(lo, hi, tot)
    ck = c.checkpoint()
    prof = (C.c_double * 8)()
    cnt = (C.c_int64 * 8)()
    c.lib.lac_profile_enable(c.ctx, 1)

    def refused(code, f, *a):
        with pytest.raises(LacError) as e:
            f(*a)
        assert e.value.code == code
        c.lib.lac_profile_read(c.ctx, prof, cnt, 1)
        assert list(cnt) == [0] * 8                                  # nothing was launched

    c.set_mapping("floor")
    refused(LAC_E_STATE, c.encode_ranges, lo, hi, tot)
    refused(LAC_E_STATE, c.encode_ranges_job, lo, hi, tot)
    c.set_mapping("ceil")
    c.set_termination("acsampler")
    refused(LAC_E_STATE, c.encode_ranges, lo, hi, tot)
    refused(LAC_E_STATE, c.encode_ranges_job, lo, hi, tot)
    c.set_termination("flush")
    refused(LAC_E_STATE, c.decode_ranges_step, (lo[0], hi[0], tot[0]), tot[1])   # encoding: the wrong mode
    _same_enc(c.checkpoint(), ck)
    # the C call's own argument checks
    st = c._stream
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    assert c.lib.lac_encode_ranges(c.ctx, None, p(hi), p(tot), B, 1, steps, None, st) == LAC_E_ARG
    assert c.lib.lac_encode_ranges(c.ctx, p(lo), p(hi), None, B, 1, steps, None, st) == LAC_E_ARG
    assert c.lib.lac_encode_ranges(c.ctx, p(lo), p(hi), p(tot), -1, 1, steps, None, st) == LAC_E_ARG
    assert c.lib.lac_encode_ranges(c.ctx, p(lo), p(hi), p(tot), B, 1, -1, None, st) == LAC_E_ARG
    c.lib.lac_profile_read(c.ctx, prof, cnt, 1)
    assert list(cnt) == [0] * 8
    _same_enc(c.checkpoint(), ck)
    # one coder launch per call whatever the steps, in profile slot 1; the job adds the finish
    c.encode_ranges(lo, hi, tot)
    c.lib.lac_profile_read(c.ctx, prof, cnt, 1)
    assert list(cnt) == [0, 1, 0, 0, 0, 0, 0, 0]
    c.encode_ranges_job(lo, hi, tot)
    c.lib.lac_profile_read(c.ctx, prof, cnt, 1)
    assert list(cnt) == [0, 1, 1, 0, 0, 0, 0, 0]
    # decoding
    c.decode_open()
    c.lib.lac_profile_read(c.ctx, prof, cnt, 1)
    before = dec_state(c)
    refused(LAC_E_STATE, c.encode_ranges, lo, hi, tot)               # decoding: the wrong mode
    refused(LAC_E_ARG, c.decode_ranges_step, None, None)             # both halves NULL
    c.set_mapping("floor")
    refused(LAC_E_STATE, c.decode_ranges_step, None, tot[0])
    c.set_mapping("ceil")
    c.set_termination("acsampler")
    refused(LAC_E_STATE, c.decode_ranges_step, None, tot[0])
    c.set_termination("flush")
    after = dec_state(c)
    for f in before.dtype.names:
        assert np.array_equal(before[f], after[f]), f
    c.decode_ranges_step((lo[0], hi[0], tot[0]), tot[1])             # advance + peek: one launch, slot 3
    c.lib.lac_profile_read(c.ctx, prof, cnt, 1)
    assert list(cnt) == [0, 0, 0, 1, 0, 0, 0, 0]
    c.close()
