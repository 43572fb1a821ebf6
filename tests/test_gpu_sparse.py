"""Sparse rows on the device (include/lac.h lac_encode_sparse / lac_decode_sparse_steps,
BatchCoder.encode_sparse / encode_sparse_job / decode_sparse, lac_amd.sparse).

Expected values come only from the reference's fixtures (tests/golden/sparse_cases.json and the
existing table fixtures that are sparse rows with every symbol a pair), and from this library's
older paths on what a sparse row stands for: the pmf path of a ``pmf_bits = 64`` coder on
``dense_rows`` (small vocabularies) and ``encode_ranges`` on the rows' triples (V = 2^18).  Integer
work: everything is compared bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import sparse as S
from errors import dec_state, stream_bytes, written

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LAC_E_ARG, LAC_E_SYMBOL_RANGE, LAC_E_TABLE, LAC_E_CAPACITY, LAC_E_STATE, LAC_E_UNDETERMINED = -1, -3, -5, -7, -9, -12
ENC_FIELDS = ("l", "h", "L", "wa", "wc", "nsym", "nflush")
BIG = 1 << 18


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _coder(V, B, prec, steps=130, cap=None, pmf_bits=64):
    from lac_amd.batch import BatchCoder
    return BatchCoder(V, B, prec=prec, pmf_bits=pmf_bits, capacity_bits=cap or steps * (prec + 2) + 256, device=DEV)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _u64dev(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint64)).view(np.int64)).to(DEV)


def _same_enc(a, b, fields=None, planes=True):
    sa, sb = a["state"], b["state"]
    for f in fields or sa.dtype.names:
        assert np.array_equal(sa[f], sb[f]), (f, sa[f], sb[f])
    if planes:
        assert np.array_equal(written(a), written(b))


def _same_dec(a, b):
    sa, sb = dec_state(a), dec_state(b)
    for f in sa.dtype.names:
        assert np.array_equal(sa[f], sb[f]), f


def np_rows(rng, T, B, V, K, n, prec, base):
    """Random valid rows [T, B, K] (idx int32, wt uint32 held in int64) with n pairs each (n None:
    a random count per row), and symbols [T, B] at, around and between the pairs."""
    idx = np.full((T, B, K), -1, dtype=np.int32)
    wt = rng.integers(0, 1 << 32, size=(T, B, K), dtype=np.int64)      # a pad's weight is ignored
    nmax = min(K, V) if n is None else min(n, K, V)
    sym = rng.integers(0, V, size=(T, B))
    if nmax:
        if V <= 1024:
            perm = rng.permuted(np.broadcast_to(np.arange(V, dtype=np.int32), (T * B, V)), axis=1)[:, :nmax]
            ids = np.sort(perm, axis=1).reshape(T, B, nmax).astype(np.int64)
        else:
            ids = np.cumsum(rng.integers(1, V // nmax + 1, size=(T, B, nmax)), axis=-1) - 1
            ids[::3, :, 0] = 0                                         # a pair at symbol 0 ...
            last = ids[1::3, :, -1] if nmax == 1 else np.where(ids[1::3, :, -2] < V - 1, V - 1, ids[1::3, :, -1])
            ids[1::3, :, -1] = last                                    # ... and at V - 1
        room = (1 << (prec - 1)) - base * V
        cap = min((1 << 32) - 1, room // nmax)
        w = rng.integers(0, cap + 1, size=(T, B, nmax), dtype=np.int64)
        kind = rng.integers(0, 4, size=(T, B, nmax))
        w = np.where(kind == 0, 0, np.where(kind == 1, cap, w))
        idx[..., :nmax] = ids
        wt[..., :nmax] = w
        if n is None:                                                  # cut every row to its own count
            cnt = rng.integers(0, nmax + 1, size=(T, B, 1))
            idx = np.where(np.arange(K)[None, None, :] < cnt, idx, -1).astype(np.int32)
        j = rng.integers(0, nmax, size=(T, B))
        at = np.take_along_axis(ids, j[..., None], -1)[..., 0]
        kind = rng.integers(0, 5, size=(T, B))
        sym = np.where(kind == 0, sym, np.clip(at + (kind - 2), 0, V - 1))   # at a pair, before it, after it
    return idx, wt, sym.astype(np.int32)


def np_triples(idx, wt, sym, base, V):
    """lo, hi, T of every (row, symbol) as uint64 arrays (every value below 2^63: exact)."""
    live = idx >= 0
    w = np.where(live, wt, 0).astype(np.uint64)
    s = sym[..., None].astype(np.int64)
    lo = np.uint64(base) * sym.astype(np.uint64) + np.where(live & (idx < s), w, np.uint64(0)).sum(-1, dtype=np.uint64)
    hi = lo + np.uint64(base) + np.where(live & (idx == s), w, np.uint64(0)).sum(-1, dtype=np.uint64)
    return lo, hi, np.uint64(base * V) + w.sum(-1, dtype=np.uint64)


class Replay:
    """lac_amd.ranges.decode_loop's model for a job whose triples are known."""

    def __init__(self, lo, hi, tot):
        self.lo, self.hi, self.tot = lo, hi, tot

    def total(self, t):
        return self.tot[t]

    def lookup(self, t, targets):
        return torch.ones_like(targets), self.lo[t], self.hi[t]


def _against_dense(a, p, idx, wt, base, sym, V, lengths=None):
    """One job on the sparse coder `a` and on the pmf coder `p` over dense_rows: planes, registers
    and trace after the encode, bytes after the finish, symbols / registers / status / determined
    counts after the decode."""
    from lac_amd.sparse import dense_rows
    T, B = sym.shape
    di, dw, ds = _dev(idx), _dev(wt), _dev(sym)
    dense = dense_rows(di, dw, base, V)
    ta, tp = (torch.zeros((T, B, 2), dtype=torch.int64, device=DEV) for _ in range(2))
    for c in (a, p):
        c.set_stream_lengths(lengths)
        c.reset()
    a.encode_sparse(di, dw, base, ds, trace=ta)
    p.encode(dense, ds, trace=tp)
    _same_enc(a.checkpoint(), p.checkpoint())
    if lengths is None:
        assert torch.equal(ta, tp)
    else:
        live = (torch.arange(T, device=DEV)[:, None] < _dev(np.asarray(lengths))[None, :])[..., None]
        assert torch.equal(torch.where(live, ta, 0), torch.where(live, tp, 0))
    a.finish()
    p.finish()
    da, na = a.to_bytes()
    dp, np_ = p.to_bytes()
    assert da == dp and np.array_equal(na, np_)
    _same_enc(a.checkpoint(), p.checkpoint(), planes=False)
    assert a.flush_digits() == p.flush_digits()
    a.decode_open()
    p.decode_open()
    out, want = a.decode_sparse(di, dw, base).cpu().numpy(), p.decode(dense).cpu().numpy()
    assert np.array_equal(out, want)
    if lengths is None:
        assert np.array_equal(out, sym)
    _same_dec(a, p)
    assert a.status()[0] == p.status()[0] == 0 and np.array_equal(a.determined(), p.determined())
    return da, na


# ------------------------------------------------------------------ 1. fixtures and census
@pytest.mark.parametrize("case", S.SPARSE_CASES, ids=[c["name"] for c in S.SPARSE_CASES])
def test_reference_fixture_both_directions(case):
    n, prec, V, K, base = len(case["syms"]), case["prec"], case["V"], case["K"], case["base"]
    idx, wt = S.case_slots(case)
    di, dw = _dev(idx).view(n, 1, K), _dev(wt.astype(np.int64)).view(n, 1, K)
    ds = _dev(np.array(case["syms"], dtype=np.int32)).view(n, 1)
    c = _coder(V, 1, prec, steps=n + 8, pmf_bits=32)
    c.encode_sparse_job(di, dw, base, ds)
    data, nb = c.to_bytes()
    assert int(nb[0]) == case["L"] and data[0].hex() == case["bytes"]
    c.decode_open()
    assert c.decode_sparse(di, dw, base)[:, 0].tolist() == case["syms"]
    assert c.status()[0] == 0 and c.determined()[0] == n
    c.close()


def test_census_fixtures_both_directions():
    """Every existing fixture that is a sparse row job with every symbol a pair (base 1,
    wt = entry - 1, K = V rounded up to a multiple of 4): none may be skipped."""
    cen = S.census()
    assert len(cen["static"]) >= 40 and len(cen["perstep"]) >= 8
    done = 0
    for c in cen["static"] + cen["perstep"]:
        idx, wt, base, K = S.census_slots(c)
        V, n = len(c["rows"][0]), len(c["syms"])
        di, dw = _dev(idx)[:, None, :], _dev(wt.astype(np.int64))[:, None, :]
        if di.shape[0] == 1:                                           # a static row: step stride 0
            di, dw = di.expand(n, 1, K), dw.expand(n, 1, K)
        ds = _dev(np.array(c["syms"], dtype=np.int32)).view(n, 1)
        k = _coder(V, 1, c["prec"], steps=n + 8, pmf_bits=32)
        k.encode_sparse_job(di, dw, base, ds)
        data, nb = k.to_bytes()
        assert int(nb[0]) == c["L"] and data[0].hex() == c["bytes"], c
        k.decode_open()
        assert k.decode_sparse(di, dw, base)[:, 0].tolist() == c["syms"]
        assert k.status()[0] == 0
        k.close()
        done += 1
    assert done == len(cen["static"]) + len(cen["perstep"]) >= 48


# ------------------------------------------------------------------ 2. boundaries
@pytest.mark.parametrize("B", (1, 2, 65))
@pytest.mark.parametrize("K", (4, 8, 64, 252, 256))
def test_boundaries_equal_the_pmf_path_on_dense_rows(K, B):
    """V = 300; K puts pairs in slots 3 | 4 and 251 | 255; n in {0, 1, K}; steps around the 64-symbol
    groups: bytes, nbits, registers, planes and trace are the pmf path's on dense_rows."""
    V, prec = 300, 48
    a, p = _coder(V, B, prec, pmf_bits=32), _coder(V, B, prec)
    for n in (0, 1, K):
        for steps in (1, 64, 65, 130):
            rng = np.random.default_rng(1000 * K + 10 * B + steps + n)
            base = (1, 3, 70001)[(n + steps) % 3]
            idx, wt, sym = np_rows(rng, steps, B, V, K, n, prec, base)
            _against_dense(a, p, idx, wt, base, sym, V)
    a.close()
    p.close()


@pytest.mark.parametrize("B", (1, 2, 65))
@pytest.mark.parametrize("K", (4, 8, 64, 252, 256))
def test_boundaries_equal_encode_ranges_on_the_triples(K, B):
    """V = 2^18: bytes, nbits, registers and trace are encode_ranges_job's on the rows' triples; the
    decode returns the symbols with the range decoder's registers."""
    from lac_amd.ranges import decode_loop
    V = BIG
    a, r = None, None
    for n in (0, 1, K):
        for steps, prec in ((1, 34), (64, 48), (65, 61), (130, 48)):
            rng = np.random.default_rng(7000 * K + 10 * B + steps + n)
            base = (1, 3, 70001)[(n + steps) % 3] if prec > 34 else 1
            idx, wt, sym = np_rows(rng, steps, B, V, K, n, prec, base)
            lo, hi, tot = (_u64dev(x) for x in np_triples(idx, wt, sym, base, V))
            a, r = _coder(V, B, prec, steps=steps, pmf_bits=32), _coder(4, B, prec, steps=steps)
            di, dw, ds = _dev(idx), _dev(wt), _dev(sym)
            ta, tr = (torch.zeros((steps, B, 2), dtype=torch.int64, device=DEV) for _ in range(2))
            a.encode_sparse_job(di, dw, base, ds, trace=ta)
            r.encode_ranges_job(lo, hi, tot, trace=tr)
            assert a.to_bytes()[0] == r.to_bytes()[0] and np.array_equal(a.to_bytes()[1], r.to_bytes()[1])
            assert torch.equal(ta, tr)
            _same_enc(a.checkpoint(), r.checkpoint(), planes=False)
            a.decode_open()
            r.decode_open()
            assert np.array_equal(a.decode_sparse(di, dw, base).cpu().numpy(), sym)
            decode_loop(r, steps, Replay(lo, hi, tot))
            _same_dec(a, r)
            assert a.status()[0] == 0 and np.array_equal(a.determined(), r.determined())
            a.close()
            r.close()


# ------------------------------------------------------------------ 3. layouts, cuts, sessions, counts
def test_static_shared_and_padded_rows():
    from lac_amd.sparse import dense_rows
    V, prec, K, B, T = 300, 48, 8, 5, 70
    rng = np.random.default_rng(3)
    a, p = _coder(V, B, prec, pmf_bits=32), _coder(V, B, prec)
    for shape in ((1, B), (T, 1), (1, 1)):                             # static rows, a shared row, both
        idx, wt, _ = np_rows(rng, shape[0], shape[1], V, K, None, prec, 3)
        sym = _dev(rng.integers(0, V, size=(T, B)).astype(np.int32))
        di, dw = _dev(idx).expand(T, B, K), _dev(wt).expand(T, B, K)
        a.encode_sparse_job(di, dw, 3, sym)
        p.encode_job(dense_rows(_dev(idx), _dev(wt), 3, V).expand(T, B, V), sym)
        assert a.to_bytes()[0] == p.to_bytes()[0]
        a.decode_open()
        assert torch.equal(a.decode_sparse(di, dw, 3), sym)
        if shape[0] == 1:                                              # [streams or 1, K]: one step
            a.reset()
            a.encode_sparse(di[0], dw[0], 3, sym[:1])
            p.reset()
            p.encode(dense_rows(di[0], dw[0], 3, V), sym[:1])
            _same_enc(a.checkpoint(), p.checkpoint())
    # padded strides: rows of K = 8 slots at a pitch of 12, streams at a pitch of 2 rows
    idx, wt, sym = np_rows(rng, T, B, V, K, None, prec, 1)
    big_i = torch.full((T, 2 * B, K + 4), 77, dtype=torch.int32, device=DEV)
    big_w = torch.full((T, 2 * B, K + 4), 77, dtype=torch.int32, device=DEV)
    vi, vw = big_i[:, ::2, :K], big_w[:, ::2, :K]
    vi.copy_(_dev(idx))
    vw.copy_(_dev(np.where(wt >= 1 << 31, wt - (1 << 32), wt).astype(np.int32)))
    assert vi.stride() == (2 * B * (K + 4), 2 * (K + 4), 1)
    a.encode_sparse_job(vi, vw, 1, _dev(sym))                          # int32 weights, idx's layout: no copy
    p.encode_job(dense_rows(_dev(idx), _dev(wt), 1, V), _dev(sym))
    assert a.to_bytes()[0] == p.to_bytes()[0]
    a.encode_sparse_job(vi, _dev(wt), 1, _dev(sym))                    # int64 weights: brought to idx's layout
    assert a.to_bytes()[0] == p.to_bytes()[0]
    a.decode_open()
    assert np.array_equal(a.decode_sparse(vi, vw, 1).cpu().numpy(), sym)
    a.close()
    p.close()


def test_cut_job_and_mixed_session():
    """50 + 80 steps equal one call of 130; and one session that mixes encode, encode_ranges and
    encode_sparse equals the pmf path on the dense rows throughout."""
    from lac_amd.ranges import table_ranges
    from lac_amd.sparse import dense_rows
    V, prec, K, B, T, cut = 300, 48, 64, 66, 130, 50
    rng = np.random.default_rng(5)
    idx, wt, sym = np_rows(rng, T, B, V, K, None, prec, 3)
    di, dw, ds = _dev(idx), _dev(wt), _dev(sym)
    dense = dense_rows(di, dw, 3, V)
    a, p = _coder(V, B, prec), _coder(V, B, prec)
    p.encode_job(dense, ds)
    want = p.to_bytes()
    a.encode_sparse_job(di, dw, 3, ds)
    assert a.to_bytes()[0] == want[0]
    a.reset()
    a.encode_sparse(di[:cut], dw[:cut], 3, ds[:cut])
    ck = a.checkpoint()
    a.reset()
    a.encode_sparse(di[cut:], dw[cut:], 3, ds[cut:])                   # something else in between
    a.restore(ck)
    a.encode_sparse(di[cut:], dw[cut:], 3, ds[cut:])
    a.finish()
    assert a.to_bytes()[0] == want[0] and np.array_equal(a.to_bytes()[1], want[1])
    lo, hi, tot = (x.to(DEV) for x in table_ranges(dense[40:90].cpu(), ds[40:90].cpu().to(torch.int64)))
    a.reset()
    a.encode(dense[:20], ds[:20])
    a.encode_sparse(di[20:40], dw[20:40], 3, ds[20:40])
    a.encode_ranges(lo, hi, tot)
    a.encode_sparse(di[90:], dw[90:], 3, ds[90:])
    a.finish()
    assert a.to_bytes()[0] == want[0] and np.array_equal(a.to_bytes()[1], want[1])
    a.close()
    p.close()


def test_per_stream_counts():
    V, prec, K, B, T = 300, 48, 8, 67, 130
    rng = np.random.default_rng(7)
    idx, wt, sym = np_rows(rng, T, B, V, K, None, prec, 1)
    n = rng.integers(0, T + 6, B)
    n[0], n[1], n[-1] = T + 5, T, 0
    a, p = _coder(V, B, prec, pmf_bits=32), _coder(V, B, prec)
    _against_dense(a, p, idx, wt, 1, sym, V, lengths=n.tolist())
    a.decode_open()
    out = a.decode_sparse(_dev(idx), _dev(wt), 1).cpu().numpy()
    for b in range(B):
        assert np.array_equal(out[:min(n[b], T), b], sym[:min(n[b], T), b]) and (out[n[b]:, b] == -1).all()
    a.close()
    p.close()


# ------------------------------------------------------------------ 4. decode around the opened buffer
def _encoded(V, B, prec, K, T, seed, base=3):
    rng = np.random.default_rng(seed)
    idx, wt, sym = np_rows(rng, T, B, V, K, None, prec, base)
    c = _coder(V, B, prec, steps=T, pmf_bits=32)
    d = (_dev(idx), _dev(wt), base)
    c.encode_sparse_job(*d, _dev(sym))
    return c, d, sym


def test_windowed_decode_with_refills():
    from lac_amd.batch import BatchCoder
    V, B, prec, K, T, N = 300, 66, 48, 8, 130, 8
    c, d, sym = _encoded(V, B, prec, K, T, 19)
    bits, nbits = c.bits_tensor(), c.nbits_tensor().clone()
    c.decode_open(bits, nbits)
    assert np.array_equal(c.decode_sparse(*d).cpu().numpy(), sym)
    want, ndet = dec_state(c), c.determined()
    with BatchCoder(V, B, prec=prec, pmf_bits=32, capacity_bits=N * (prec + 2) + 256, device=DEV) as w:
        w.decode_open_window(bits, nbits)
        got = []
        for t in range(0, T, N):
            got.append(w.decode_sparse(d[0][t:t + N], d[1][t:t + N], d[2]).cpu().numpy())
            w.refill()
        assert w.status()[0] == 0 and np.array_equal(np.concatenate(got), sym)
        st = dec_state(w)
        st["pos"] += np.uint64(64) * w.window_base().astype(np.uint64)
        for f in st.dtype.names:
            assert np.array_equal(st[f], want[f]), f
        assert np.array_equal(w.determined(), ndet)
    c.close()


def test_decode_of_a_packed_job():
    V, B, prec, K, T = 300, 65, 48, 8, 30
    c, d, sym = _encoded(V, B, prec, K, T, 21)
    payload = torch.zeros(B * c.bits_stride() + 4 * B + 64, dtype=torch.uint8, device=DEV)
    length = torch.zeros(1, dtype=torch.int64, device=DEV)
    c.pack_bits(payload, 4, length)
    c.decode_open_packed(payload, 4)
    assert np.array_equal(c.decode_sparse(*d).cpu().numpy(), sym) and c.status()[0] == 0
    c.close()


def test_decode_stop_with_streams_stopping_at_different_steps():
    """Streams cut short by different amounts, LAC_OPT_DECODE_STOP on: the symbols, the verdicts,
    err_step and the registers are the pmf path's on the dense rows."""
    from lac_amd.sparse import dense_rows
    V, B, prec, K, T = 300, 66, 48, 8, 70
    c, d, sym = _encoded(V, B, prec, K, T, 23)
    p = _coder(V, B, prec, steps=T)
    bits, nbits = c.bits_tensor(), c.nbits_tensor().clone()
    cut = torch.clamp(nbits - _dev(np.arange(B) * 37 % 900), min=0)
    cut[0] = nbits[0]
    dense = dense_rows(d[0], d[1], d[2], V)
    for k in (c, p):
        k.set_decode_stop(True)
        k.decode_open(bits, cut)
    out, want = c.decode_sparse(*d).cpu().numpy(), p.decode(dense).cpu().numpy()
    assert np.array_equal(out, want)
    sc, sp = c.status(), p.status()
    assert sc[0] == sp[0] == LAC_E_UNDETERMINED and np.array_equal(sc[1], sp[1]) and np.array_equal(sc[2], sp[2])
    assert len(set(sc[2][sc[1] != 0].tolist())) >= 8 and sc[1][0] == 0
    _same_dec(c, p)
    c.close()
    p.close()


# ------------------------------------------------------------------ 5. errors
POSITIONS = (0, 62, 63, 64, 126, 127)                                # first, next-to-last, last step of a 64-step block
ROW_DEFECTS = ("pair_after_pad", "equal", "descending", "below_minus_one", "at_V", "total")


def _break_row(kind, idx, wt, V, base, prec):
    """One row [K] (n = 5 pairs of K = 8) made malformed one way."""
    idx, wt = idx.copy(), wt.copy()
    if kind == "pair_after_pad":
        idx[6] = V - 1
    elif kind == "equal":
        idx[4] = idx[3]                                              # across the lanes' seam 3 | 4
    elif kind == "descending":
        idx[1], idx[2] = idx[2], idx[1]
    elif kind == "below_minus_one":
        idx[7] = -2
    elif kind == "at_V":
        idx[4] = V
    else:                                                            # the total one above 2^(prec-1)
        wt[:5] = 0
        room = (1 << (prec - 1)) - base * V + 1
        assert room <= 5 * ((1 << 32) - 1)
        for j in range(5):
            wt[j] = min(room, (1 << 32) - 1)
            room -= int(wt[j])
    return idx, wt


def _error_job(prec=34):
    V, K, T, base = 300, 8, 130, 3
    kinds = ROW_DEFECTS + ("symbol_high", "symbol_negative")
    B = 2 * len(kinds) * len(POSITIONS) + 1
    rng = np.random.default_rng(9)
    idx, wt, sym = np_rows(rng, T, B, V, K, 5, prec, base)
    good = (idx.copy(), wt.copy(), sym.copy())
    want_err, want_step = np.zeros(B, np.int32), np.full(B, -1, np.int64)
    b = 1
    for kind in kinds:
        for pos in POSITIONS:
            if kind == "symbol_high":
                sym[pos, b] = V
            elif kind == "symbol_negative":
                sym[pos, b] = -1
            else:
                idx[pos, b], wt[pos, b] = _break_row(kind, idx[pos, b], wt[pos, b], V, base, prec)
                assert not S.row_valid(idx[pos, b], wt[pos, b], base, V, prec)
            want_err[b] = LAC_E_SYMBOL_RANGE if kind.startswith("symbol") else LAC_E_TABLE
            want_step[b] = pos
            b += 2                                                   # every other stream stays clean
    assert b == B
    return V, K, T, base, B, prec, (idx, wt, sym), good, want_err, want_step


def test_encode_errors_beside_clean_streams():
    """Each malformed-row kind and an out-of-range symbol at the first, last and next-to-last step
    of a 64-step block, beside clean streams: the verdict, err_step and the frozen state -- the
    pmf path's state for a stream whose count ends at that step -- with the neighbours unaffected."""
    from lac_amd.sparse import dense_rows
    V, K, T, base, B, prec, (idx, wt, sym), good, want_err, want_step = _error_job()
    a, p = _coder(V, B, prec, pmf_bits=32), _coder(V, B, prec)
    a.reset()
    a.encode_sparse(_dev(idx), _dev(wt), base, _dev(sym))
    rc, err, step = a.status()
    assert rc in (LAC_E_TABLE, LAC_E_SYMBOL_RANGE)
    assert np.array_equal(err, want_err) and np.array_equal(step, want_step)
    dense = dense_rows(_dev(good[0]), _dev(good[1]), base, V)
    p.set_stream_lengths(np.where(want_err != 0, want_step, T).tolist())
    p.reset()
    p.encode(dense, _dev(good[2]))
    _same_enc(a.checkpoint(), p.checkpoint(), fields=ENC_FIELDS)
    # the pmf path's own verdict on the symbols (its rows are the clean dense ones)
    q = _coder(V, B, prec)
    q.reset()
    q.encode(dense, _dev(sym))
    sym_streams = want_err == LAC_E_SYMBOL_RANGE
    assert np.array_equal(q.status()[1][sym_streams], err[sym_streams])
    assert np.array_equal(q.status()[2][sym_streams], step[sym_streams])
    q.close()
    # a failed stream stays frozen under more steps; its neighbours go on
    a.encode_sparse(_dev(good[0][:3]), _dev(good[1][:3]), base, _dev(good[2][:3]))
    p.set_stream_lengths(np.where(want_err != 0, want_step, T + 3).tolist())
    p.encode(dense[:3], _dev(good[2][:3]))
    _same_enc(a.checkpoint(), p.checkpoint(), fields=ENC_FIELDS)
    assert np.array_equal(a.status()[1], want_err) and np.array_equal(a.status()[2], want_step)
    a.finish()
    p.finish()
    clean = np.flatnonzero(want_err == 0)
    ba, bp = stream_bytes(a)[0], stream_bytes(p)[0]
    assert all(ba[b] == bp[b] for b in clean)
    a.close()
    p.close()


def test_symbol_range_comes_before_the_row():
    V, K, prec = 300, 8, 34
    rng = np.random.default_rng(2)
    idx, wt, sym = np_rows(rng, 1, 3, V, K, 5, prec, 1)
    idx[0, 0], wt[0, 0] = _break_row("equal", idx[0, 0], wt[0, 0], V, 1, prec)
    idx[0, 1], wt[0, 1] = _break_row("at_V", idx[0, 1], wt[0, 1], V, 1, prec)
    sym[0, 0] = V
    a = _coder(V, 3, prec, pmf_bits=32)
    a.reset()
    a.encode_sparse(_dev(idx), _dev(wt), 1, _dev(sym))
    assert a.status()[1].tolist() == [LAC_E_SYMBOL_RANGE, LAC_E_TABLE, 0] and a.status()[2].tolist() == [0, 0, -1]
    a.close()


def test_order_test_across_every_lane_seam():
    """K = 256, n = K: an equal index across slots 4 j + 3 | 4 j + 4 for lanes inside a 16-lane row
    and across the rows (slots 63 | 64, 127 | 128, 191 | 192), a descending one at 251 | 252; the
    clean streams beside them code as the pmf path does (test_boundaries)."""
    V, K, prec = 300, 256, 48
    seams = (3, 31, 63, 127, 191, 251)
    B = 2 * len(seams) + 1
    rng = np.random.default_rng(4)
    idx, wt, sym = np_rows(rng, 2, B, V, K, K, prec, 1)
    want = np.zeros(B, np.int32)
    for j, m in enumerate(seams):
        b = 2 * j + 1
        if m == 251:
            idx[1, b, m], idx[1, b, m + 1] = idx[1, b, m + 1], idx[1, b, m]
        else:
            idx[1, b, m + 1] = idx[1, b, m]
        want[b] = LAC_E_TABLE
    a = _coder(V, B, prec, pmf_bits=32)
    a.reset()
    a.encode_sparse(_dev(idx), _dev(wt), 1, _dev(sym))
    assert np.array_equal(a.status()[1], want) and np.array_equal(a.status()[2], np.where(want != 0, 1, -1))
    a.close()


def test_capacity_failures_equal_the_pmf_path():
    """A capacity of four words: streams fail at different steps, after the narrowing: status,
    err_step, registers, planes and the trace of the failing step are lac_encode's on the dense rows."""
    from lac_amd.sparse import dense_rows
    V, K, T, B, prec = 300, 8, 130, 66, 48
    rng = np.random.default_rng(11)
    idx, wt, sym = np_rows(rng, T, B, V, K, None, prec, 1)
    di, dw, ds = _dev(idx), _dev(wt), _dev(sym)
    dense = dense_rows(di, dw, 1, V)
    a, p = _coder(V, B, prec, cap=256, pmf_bits=32), _coder(V, B, prec, cap=256)
    ta, tp = (torch.zeros((T, B, 2), dtype=torch.int64, device=DEV) for _ in range(2))
    a.reset()
    p.reset()
    a.encode_sparse(di, dw, 1, ds, trace=ta)
    p.encode(dense, ds, trace=tp)
    sa, sp = a.status(), p.status()
    assert sa[0] == sp[0] == LAC_E_CAPACITY and np.array_equal(sa[1], sp[1]) and np.array_equal(sa[2], sp[2])
    assert (sa[1] == LAC_E_CAPACITY).all() and len(set(sa[2].tolist())) >= 5
    _same_enc(a.checkpoint(), p.checkpoint())
    for b in range(B):
        k = int(sa[2][b])
        assert torch.equal(ta[:k + 1, b], tp[:k + 1, b])
    a.close()
    p.close()


def test_capacity_failures_at_block_positions_beside_clean_streams():
    """A capacity failure steered to the first, last and next-to-last step of a 64-step block of a
    call, beside clean streams.  Two row kinds over V = 256 fix the bits of a step exactly, whatever
    came before (the registers return to l = 0, w = 2^prec after each): the uniform row (n = 0)
    costs 8 bits, the row {0: 254} with symbol 0 costs 1 (255 of 510).  A first call of 40 steps
    fills the streams; stream b then fails at step POSITIONS[..] of the second call, where its bits
    first pass the capacity of (256 + 63) / 64 + 1 words.  Verdicts, err_step, registers, planes and
    the trace up to the failing step are lac_encode's on the dense rows; clean streams go on."""
    from lac_amd.sparse import dense_rows
    V, K, prec, P, T, cap = 256, 4, 48, 40, 130, 256
    room = ((cap + 63) // 64 + 1) * 64                               # lac_open's words, in bits
    B = 2 * len(POSITIONS) + 1
    rng = np.random.default_rng(31)
    idx = np.full((P + T, B, K), -1, dtype=np.int32)
    wt = np.zeros((P + T, B, K), dtype=np.int64)
    sym = np.zeros((P + T, B), dtype=np.int32)
    idx[:, :, 0], wt[:, :, 0] = 0, 254                               # every step 1 bit ...
    want_err, want_step = np.zeros(B, np.int32), np.full(B, -1, np.int64)
    for j, pos in enumerate(POSITIONS):
        b, g = 2 * j + 1, P + pos                                    # ... but for 8-bit steps: m first, and step g
        m = (room - g) // 7
        assert 0 <= m <= g and 7 * m + g <= room < 7 * m + g + 8
        for t in [*range(m), g]:
            idx[t, b, 0], wt[t, b, 0] = -1, 0
            sym[t, b] = rng.integers(0, V)
        want_err[b], want_step[b] = LAC_E_CAPACITY, g
    sym[P + 5, 0] = 77                                               # a clean stream with an 8-bit step of its own
    idx[P + 5, 0, 0], wt[P + 5, 0, 0] = -1, 0
    di, dw, ds = _dev(idx), _dev(wt), _dev(sym)
    dense = dense_rows(di, dw, 1, V)
    a, p = _coder(V, B, prec, cap=cap, pmf_bits=32), _coder(V, B, prec, cap=cap)
    ta, tp = (torch.zeros((T, B, 2), dtype=torch.int64, device=DEV) for _ in range(2))
    a.reset()
    p.reset()
    a.encode_sparse(di[:P], dw[:P], 1, ds[:P])
    p.encode(dense[:P], ds[:P])
    assert a.status()[0] == p.status()[0] == 0
    a.encode_sparse(di[P:], dw[P:], 1, ds[P:], trace=ta)
    p.encode(dense[P:], ds[P:], trace=tp)
    sa, sp = a.status(), p.status()
    assert np.array_equal(sa[1], want_err) and np.array_equal(sa[2], want_step)
    assert np.array_equal(sp[1], want_err) and np.array_equal(sp[2], want_step)
    _same_enc(a.checkpoint(), p.checkpoint())
    for b in range(B):
        k = T if want_err[b] == 0 else int(want_step[b]) - P + 1     # the failing step's digits are traced
        assert torch.equal(ta[:k, b], tp[:k, b]), b
    # more steps: the failed streams stay frozen, the clean ones go on
    a.encode_sparse(di[:3], dw[:3], 1, ds[:3])
    p.encode(dense[:3], ds[:3])
    _same_enc(a.checkpoint(), p.checkpoint())
    assert np.array_equal(a.status()[1], want_err) and np.array_equal(a.status()[2], want_step)
    a.finish()
    p.finish()
    ba, bp = stream_bytes(a)[0], stream_bytes(p)[0]
    assert all(ba[b] == bp[b] for b in np.flatnonzero(want_err == 0))
    a.close()
    p.close()


def test_decode_errors_beside_clean_streams():
    """Malformed rows met by the decoder: LAC_E_TABLE at that step, the stream frozen as before it
    (the pmf decoder's state for a count ending there), -1 from there on, neighbours unaffected."""
    from lac_amd.sparse import dense_rows
    V, K, T, base, B, prec, (idx, wt, sym), good, want_err, want_step = _error_job()
    rows_only = want_err == LAC_E_TABLE
    a, p = _coder(V, B, prec, pmf_bits=32), _coder(V, B, prec)
    a.encode_sparse_job(_dev(good[0]), _dev(good[1]), base, _dev(good[2]))
    bits, nbits = a.bits_tensor(), a.nbits_tensor().clone()
    a.decode_open(bits, nbits)
    out = a.decode_sparse(_dev(idx), _dev(wt), base).cpu().numpy()
    rc, err, step = a.status()
    assert rc == LAC_E_TABLE
    assert np.array_equal(err, np.where(rows_only, LAC_E_TABLE, 0)) and np.array_equal(step, np.where(rows_only, want_step, -1))
    stop = np.where(rows_only, want_step, T)
    for b in range(B):
        assert np.array_equal(out[:stop[b], b], good[2][:stop[b], b]) and (out[stop[b]:, b] == -1).all()
    p.set_stream_lengths(stop.tolist())
    p.decode_open(bits, nbits)
    p.decode(dense_rows(_dev(good[0]), _dev(good[1]), base, V))
    sa, sp = dec_state(a), dec_state(p)
    for f in ("l", "h", "x", "pos", "nsym", "det", "ndet"):
        assert np.array_equal(sa[f], sp[f]), f
    # frozen under more steps
    a.decode_sparse(_dev(good[0][:2]), _dev(good[1][:2]), base)
    assert np.array_equal(dec_state(a)["nsym"][rows_only], want_step[rows_only])
    a.close()
    p.close()


# ------------------------------------------------------------------ 6. refusals and launches
def test_refusals_launch_nothing_and_change_nothing():
    from lac_amd._lib import LacError
    V, K, T, B, prec = 300, 8, 5, 3, 48
    rng = np.random.default_rng(23)
    idx, wt, sym = np_rows(rng, T, B, V, K, None, prec, 1)
    di, dw, ds = _dev(idx), _dev(wt), _dev(sym)
    w32 = _dev(np.where(wt >= 1 << 31, wt - (1 << 32), wt).astype(np.int32))
    c = _coder(V, B, prec, pmf_bits=32)
    c.reset()
    c.encode_sparse(di, dw, 1, ds)
    ck = c.checkpoint()
    prof, cnt = (C.c_double * 8)(), (C.c_int64 * 8)()
    c.lib.lac_profile_enable(c.ctx, 1)

    def nothing_launched():
        c.lib.lac_profile_read(c.ctx, prof, cnt, 1)
        assert list(cnt) == [0] * 8

    def refused(code, f, *a):
        with pytest.raises(LacError) as e:
            f(*a)
        assert e.value.code == code
        nothing_launched()

    c.set_mapping("floor")
    refused(LAC_E_STATE, c.encode_sparse, di, dw, 1, ds)
    refused(LAC_E_STATE, c.encode_sparse_job, di, dw, 1, ds)
    c.set_mapping("ceil")
    c.set_termination("acsampler")
    refused(LAC_E_STATE, c.encode_sparse, di, dw, 1, ds)
    refused(LAC_E_STATE, c.encode_sparse_job, di, dw, 1, ds)
    c.set_termination("flush")
    refused(LAC_E_STATE, c.decode_sparse, di, dw, 1)                   # encoding: the wrong mode
    refused(LAC_E_ARG, c.encode_sparse, di, dw, 0, ds)                 # base = 0
    for bad_w in (-1, 1 << 32):                                        # an int64 weight that is no uint32
        bw = dw.clone()
        bw[2, 1, 0] = bad_w
        with pytest.raises(ValueError):
            c.encode_sparse(di, bw, 1, ds)
        nothing_launched()
    refused(LAC_E_ARG, c.encode_sparse, di[..., :6], dw[..., :6], 1, ds)   # K = 6, and a stride of 8 is fine
    refused(LAC_E_ARG, c.encode_sparse, di[..., 1:5], dw[..., 1:5], 1, ds)   # rows not 16-byte aligned
    _same_enc(c.checkpoint(), ck)
    # the C call's own argument checks
    st = c._stream
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    enc = lambda *a: c.lib.lac_encode_sparse(c.ctx, *a, st)  # noqa: E731
    assert enc(None, p(w32), K, B * K, K, 1, p(ds), T, None) == LAC_E_ARG
    assert enc(p(di), None, K, B * K, K, 1, p(ds), T, None) == LAC_E_ARG
    assert enc(p(di), p(w32), K, B * K, K, 1, None, T, None) == LAC_E_ARG
    for bad_k in (0, 2, 6, 260, -4):
        assert enc(p(di), p(w32), bad_k, B * K, K, 1, p(ds), T, None) == LAC_E_ARG
    assert enc(p(di), p(w32), K, B * K + 2, K, 1, p(ds), T, None) == LAC_E_ARG
    assert enc(p(di), p(w32), K, B * K, K + 1, 1, p(ds), T, None) == LAC_E_ARG
    assert enc(p(di), p(w32), K, -4, K, 1, p(ds), T, None) == LAC_E_ARG
    assert enc(p(di), p(w32), K, B * K, K, 1, p(ds), -1, None) == LAC_E_ARG
    assert enc(C.c_void_p(di.data_ptr() + 4), p(w32), 4, B * K, K, 1, p(ds), T, None) == LAC_E_ARG
    assert enc(p(di), C.c_void_p(w32.data_ptr() + 8), 4, B * K, K, 1, p(ds), T, None) == LAC_E_ARG
    nothing_launched()
    _same_enc(c.checkpoint(), ck)
    # one coder launch per call whatever the steps, in profile slot 1; the job adds the finish
    c.encode_sparse(di, dw, 1, ds)
    c.lib.lac_profile_read(c.ctx, prof, cnt, 1)
    assert list(cnt) == [0, 1, 0, 0, 0, 0, 0, 0]
    c.encode_sparse_job(di, dw, 1, ds)
    c.lib.lac_profile_read(c.ctx, prof, cnt, 1)
    assert list(cnt) == [0, 1, 1, 0, 0, 0, 0, 0]
    # decoding
    c.decode_open()
    c.lib.lac_profile_read(c.ctx, prof, cnt, 1)
    before = dec_state(c)
    refused(LAC_E_STATE, c.encode_sparse, di, dw, 1, ds)               # decoding: the wrong mode
    refused(LAC_E_ARG, c.decode_sparse, di, dw, 0)
    c.set_mapping("floor")
    refused(LAC_E_STATE, c.decode_sparse, di, dw, 1)
    c.set_mapping("ceil")
    c.set_termination("acsampler")
    refused(LAC_E_STATE, c.decode_sparse, di, dw, 1)
    c.set_termination("flush")
    dec = lambda *a: c.lib.lac_decode_sparse_steps(c.ctx, *a, st)  # noqa: E731
    out = torch.zeros((T, B), dtype=torch.int32, device=DEV)
    assert dec(p(di), p(w32), K, B * K, K, 1, T, None) == LAC_E_ARG
    assert dec(p(di), p(w32), 12, B * K, K + 2, 1, T, p(out)) == LAC_E_ARG
    nothing_launched()
    after = dec_state(c)
    for f in before.dtype.names:
        assert np.array_equal(before[f], after[f]), f
    assert np.array_equal(c.decode_sparse(di, dw, 1).cpu().numpy(), sym)   # all the steps: one launch, slot 3
    c.lib.lac_profile_read(c.ctx, prof, cnt, 1)
    assert list(cnt) == [0, 0, 0, 1, 0, 0, 0, 0]
    c.close()


# ------------------------------------------------------------------ 7. top-k rows of a model
def test_topk_rows():
    from lac_amd.sparse import dense_rows, topk_rows
    g = torch.Generator().manual_seed(1)
    lg = (torch.randn((3, 5, 1000), generator=g) * 4).to(DEV)
    idx, wt, base = topk_rows(lg, 20)
    assert idx.shape == (3, 5, 20) and idx.dtype == torch.int32 and wt.dtype == torch.int64 and base == 1
    assert (idx[..., 1:] > idx[..., :-1]).all() and int(wt.max()) == 1 << 24 and int(wt.min()) >= 0
    top = torch.topk(lg, 20, dim=-1).indices.sort(-1).values
    assert torch.equal(idx.to(torch.int64), top)
    idx, wt, _ = topk_rows(lg, 18, weight_bits=16, base=3)
    assert idx.shape[-1] == 20 and (idx[..., 18:] == -1).all() and (wt[..., 18:] == 0).all()
    d = dense_rows(idx, wt, 3, 1000)
    assert torch.equal(d.sum(-1), 3000 + wt.sum(-1)) and int(d.min()) == 3
    with pytest.raises(ValueError):
        topk_rows(lg, 20, weight_bits=24, prec=16)


def test_topk_compressor_round_trip():
    """TinyCausalLM, vocab 1000, k = 20, B = 3, T = 40: the round trip, and bytes equal to encode_job
    on the dense rows of the same top-k rows."""
    from lac_amd.llm import TinyCausalLM
    from lac_amd.sparse import TopKCompressor, dense_rows
    V, k, B, T = 1000, 20, 3, 40
    comp = TopKCompressor(TinyCausalLM(vocab=V, d=32, layers=1, heads=2, max_len=64, seed=3), V, k, device=DEV)
    g = torch.Generator().manual_seed(5)
    tokens = torch.randint(0, V, (B, T), generator=g)
    data, nbits = comp.compress(tokens)
    assert torch.equal(comp.decompress(data, nbits, T).cpu(), tokens)
    idx, wt, base = comp.rows(tokens)
    assert idx.shape == (T, B, k)
    p = _coder(V, B, comp.prec, steps=T)
    p.encode_job(dense_rows(idx, wt, base, V), tokens.t().contiguous().to(torch.int32).to(DEV))
    want, nb = p.to_bytes()
    assert data == want and np.array_equal(np.asarray(nbits, dtype=np.uint64), np.asarray(nb, dtype=np.uint64))
    p.close()
