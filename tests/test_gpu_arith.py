"""The coder's float-assisted divisions on the device itself (tests/native/dev_arith.hip, compiled
with the product's flags), against exact Python integers.

Every quotient the decoders and k_encode take is one float64 estimate plus a fixed correction that
is exact only while the estimate lands within a fixed distance of the quotient (mask form
[-2, +3], div_near / div_mid +-1, div_floor_inv two fix-ups), and that distance depends on the
device's own 1/d: v_rcp_f64 plus Newton steps, or an IEEE divide in a kernel.  The reciprocal sweep
measures those on the device and keeps the divisors at which they are furthest off; the quotient
tests run every primitive over tests/dev_arith.py's cases, those divisors included.  Each test
prints its measured extremes as a line ``DEVARITH {json}`` (profiles/devarith/README.md).
"""
import json

import numpy as np
import pytest

import dev_arith as da

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


@pytest.fixture(scope="module")
def lib():
    return da.load()


@pytest.fixture(scope="module")
def sweep(lib):
    return da.run_sweep(lib)


@pytest.fixture(scope="module")
def worst(sweep):
    return sweep[1]


def report(**kw):
    print("DEVARITH " + json.dumps(kw, sort_keys=True))


def obj(a):
    return [int(x) for x in a]


def expect_equal(name, got, want, cs, est=None):
    """got (uint64 array) == want ([int]); the failure names the first offending case and its estimate."""
    bad = np.nonzero(got != da.u64(want))[0]
    if len(bad):
        i = int(bad[0])
        raise AssertionError(f"{name}: {len(bad)} of {len(want)} wrong; first {dict(zip(cs.names, cs.rows[i]))} "
                             f"labels {sorted(cs.labels[i])}: got {int(got[i])}, exact {want[i]}"
                             + (f", estimate {int(est[i])}" if est is not None else ""))


def expect_distance(name, est, want, lo, hi, cs):
    """lo <= estimate - quotient <= hi on every case -> the observed (min, max)."""
    dist = est.view(np.int64) - da.u64(want).view(np.int64)
    bad = np.nonzero((dist < lo) | (dist > hi))[0]
    if len(bad):
        i = int(bad[0])
        raise AssertionError(f"{name}: estimate outside [{lo}, {hi}] of the quotient on {len(bad)} of {len(want)}; "
                             f"first {dict(zip(cs.names, cs.rows[i]))} labels {sorted(cs.labels[i])}: "
                             f"estimate {int(est[i])}, exact {want[i]}")
    return int(dist.min()), int(dist.max())


# ------------------------------------------------------------------ reciprocals and conversions
def test_reciprocal_sweep(sweep):
    """v_rcp_f64 + Newton (recip, recip_small), two steps (recip2_small), the device's IEEE divide and
    the integer -> double conversions over 2^20 evenly spaced divisors of each length, the 1024 at
    each end and rcp_probe's random family: within what the consumers' host tests simulate
    (tests/test_core_host.py: 16 ulps for div_near's targets, 11 ulps for div_floor_inv,
    11 * 2^-52 relative for div_small -- 2^-49 before this sweep measured 10 * 2^-52 --, 1 ulp for
    recip2_small; the IEEE divide and the conversions exact)."""
    stats, worst = sweep
    for (fn, L), s in sorted(stats.items()):
        report(sweep=fn, L=L, **s)
    for (fn, L), s in sorted(stats.items()):
        if fn in ("u64_to_f64", "small_to_f64"):
            assert s["mismatches"] == 0, (fn, L, s)
        elif fn == "ieee_div":
            assert s["ulp_min"] == 0 and s["ulp_max"] == 0, (fn, L, s)
        elif fn == "recip2_small":
            assert -1 <= s["ulp_min"] and s["ulp_max"] <= 1, (fn, L, s)
        else:
            assert -11 <= s["ulp_min"] and s["ulp_max"] <= 11, (fn, L, s)
            assert -11.0 <= s["rel_min"] and s["rel_max"] <= 11.0, (fn, L, s)    # in units of 2^-52
    for L in da.SWEEP_L + (64,):
        assert 64 <= len(worst[L]) <= 256 and all(d.bit_length() == L for d in worst[L])


def test_conversions_by_the_2_52_magic(lib):
    """small_to_f64 / f64_to_small: exact both ways below 2^52; f64_to_small rounds to nearest, ties to
    even, as the estimates rely on."""
    rng = np.random.default_rng(3)
    n = np.concatenate([np.arange(0, 4096), (1 << 52) - 1 - np.arange(0, 4096),
                        rng.integers(0, 1 << 52, size=100000), (1 << rng.integers(0, 52, size=4096))]).astype(np.uint64)
    conv = da.thread(lib, da.T_RECIP_SMALL, [np.maximum(n, 1)], 3)[2]
    assert np.array_equal(conv, np.maximum(n, 1).astype(np.float64).view(np.uint64))
    e = np.concatenate([n.astype(np.float64), rng.integers(0, 1 << 51, size=100000) + 0.5,
                        rng.integers(0, 1 << 50, size=100000) + rng.choice([0.25, 0.75], size=100000),
                        rng.random(100000) * 2.0 ** rng.integers(0, 52, size=100000)])
    e = e[e < 2.0 ** 52 - 1]
    got = da.thread(lib, da.T_F64_SMALL, [e.view(np.uint64)], 1)[0]
    assert np.array_equal(got, np.rint(e).astype(np.uint64))


# ------------------------------------------------------------------ quotients
def _pairs(cs):
    """Partner numerators for the two-quotient wrappers: T - c for ranges, w - 1 - v for targets."""
    n1 = [(d - n) if s == "range" else (d - 1 - n) for (n, m, add, d, _), s in zip(cs.rows, cs.shape)]
    want1 = [(a * r[1] + r[2]) // r[3] for a, r in zip(n1, cs.rows)]
    return n1, want1


def test_div_small_mask_and_loop_forms(lib, worst):
    """div_small_est with its two corrections, each with the reciprocals its callers pass.

    The sign-mask form (k_decode_seq's chain: div_small_u<true>, div_small_u2<true>) with
    recip2_small: exact at every quotient up to 2^50, the estimate at most 3 above the quotient and
    2 below.  With one Newton step (recip, recip_small) the estimate of a quotient near 2^50 is 3
    below it at the worst divisors -- measured here, the figure printed -- so the mask form takes
    those reciprocals only below 2^49, where it is asserted in the same way; the loop form
    (k_q1_decode: div_small_u<false>, div_small_u2<false>) is exact with them everywhere."""
    cs = da.decoder_cases("small", worst)
    want = da.quotients(cs)
    n, m, add, d, _ = cs.cols()
    n1, want1 = _pairs(cs)
    mask, est, _ = da.thread(lib, da.T_DIV_SMALL, [n, m, add, d], 3, da.INV_RECIP2_SMALL)
    lo, hi = expect_distance("div_small_est[recip2_small]", est, want, -2, 3, cs)
    expect_equal("div_small_fix_mask[recip2_small]", mask, want, cs, est)
    wmask, west, _ = da.wave(lib, da.W_SMALL_U, [n, m, add, d], 3, da.INV_RECIP2_SMALL)
    assert np.array_equal(west, est)
    expect_equal("div_small_u<true>[recip2_small]", wmask, want, cs, west)
    q0, q1, _, _ = da.wave(lib, da.W_SMALL_U2, [n, n1, m, add, d], 4, da.INV_RECIP2_SMALL)
    expect_equal("div_small_u2<true>.0[recip2_small]", q0, want, cs)
    expect_equal("div_small_u2<true>.1[recip2_small]", q1, want1, cs)
    report(primitive="div_small_fix_mask", inv="recip2_small", cases=len(cs), est_minus_q=[lo, hi], allowed=[-2, 3])
    sub = cs.select(lambda r, ls, s: (r[0] * r[1] + r[2]) // r[3] < 1 << 49)
    wsub = da.quotients(sub)
    assert len(sub) > len(cs) // 2 and max(wsub) == (1 << 49) - 1
    for inv, iname in ((da.INV_RECIP, "recip"), (da.INV_RECIP_SMALL, "recip_small")):
        mask, est, loop = da.thread(lib, da.T_DIV_SMALL, [n, m, add, d], 3, inv)
        dist = est.view(np.int64) - da.u64(want).view(np.int64)
        expect_equal(f"div_small_fix[{iname}]", loop, want, cs, est)
        _, west, wloop = da.wave(lib, da.W_SMALL_U, [n, m, add, d], 3, inv)
        assert np.array_equal(west, est)
        expect_equal(f"div_small_u<false>[{iname}]", wloop, want, cs, west)
        _, _, l0, l1 = da.wave(lib, da.W_SMALL_U2, [n, n1, m, add, d], 4, inv)
        expect_equal(f"div_small_u2<false>.0[{iname}]", l0, want, cs)
        expect_equal(f"div_small_u2<false>.1[{iname}]", l1, want1, cs)
        report(primitive="div_small_fix (loops)", inv=iname, cases=len(cs), est_minus_q=[int(dist.min()), int(dist.max())],
               mask_form_wrong=int((mask != da.u64(want)).sum()))
        sn, sm, sadd, sd, _ = sub.cols()
        mask, est, _ = da.thread(lib, da.T_DIV_SMALL, [sn, sm, sadd, sd], 3, inv)
        lo, hi = expect_distance(f"div_small_est[{iname}], quotients below 2^49", est, wsub, -2, 3, sub)
        expect_equal(f"div_small_fix_mask[{iname}], quotients below 2^49", mask, wsub, sub, est)
        report(primitive="div_small_fix_mask", inv=iname, quotients="< 2^49", cases=len(sub), est_minus_q=[lo, hi],
               allowed=[-2, 3])


def test_corrections_over_their_whole_range(lib, worst):
    """Each branch-free correction given every estimate its range admits, whatever reciprocal would
    have produced it: div_small_fix_mask (and div_small_fix_u<true>) from 2 below the quotient to
    3 above, div_near_fix<N32> and div_mid_fix from 1 below to 1 above."""
    for form, span in (("small", range(-2, 4)), ("near32", range(-1, 2)), ("near64", range(-1, 2)),
                       ("mid", range(-1, 2))):
        cs = da.decoder_cases(form, worst)
        cs = cs.select(lambda r, ls, s: "random" not in ls)
        want = da.quotients(cs)
        n, m, add, d, _ = cs.cols()
        for k in span:
            est = [max(q + k, 0) for q in want]
            mask, near, near32, mid = da.thread(lib, da.T_FIX, [n, m, add, d, est], 4)
            if form == "small":
                expect_equal(f"div_small_fix_mask(q{k:+d})", mask, want, cs, da.u64(est))
                wmask, wloop = da.wave(lib, da.W_FIX, [n, m, add, d, est], 2)
                expect_equal(f"div_small_fix_u<true>(q{k:+d})", wmask, want, cs, da.u64(est))
                expect_equal(f"div_small_fix_u<false>(q{k:+d})", wloop, want, cs, da.u64(est))
            elif form == "mid":
                expect_equal(f"div_mid_fix(q{k:+d})", mid, want, cs, da.u64(est))
            else:
                expect_equal(f"div_near_fix<false>(q{k:+d}) {form}", near, want, cs, da.u64(est))
                if form == "near32":
                    r32 = cs.select(lambda r, ls, s: s == "range")
                    keep = np.array([s == "range" for s in cs.shape])
                    expect_equal(f"div_near_fix<true>(q{k:+d})", near32[keep], da.quotients(r32), r32, da.u64(est)[keep])


@pytest.mark.parametrize("form", ["near32", "near64"])
def test_div_near(lib, worst, form):
    """div_near as the lean step takes it: targets floor(v*T/w) with recip_small(w) on u32 rows and
    recip2_small(w) on u64 rows below 2^50, ranges with the device's IEEE 1/T (N32 on u32 rows):
    exact, every estimate within one of the quotient."""
    cs = da.decoder_cases(form, worst)
    tg = cs.select(lambda r, ls, s: s == "target")
    rg = cs.select(lambda r, ls, s: s == "range")
    inv, iname = (da.INV_RECIP_SMALL, "recip_small") if form == "near32" else (da.INV_RECIP2_SMALL, "recip2_small")
    want = da.quotients(tg)
    n, m, add, d, _ = tg.cols()
    q, est, _ = da.thread(lib, da.T_DIV_NEAR, [n, m, add, d], 3, inv)
    lo, hi = expect_distance(f"{form} target estimate[{iname}]", est, want, -1, 1, tg)
    expect_equal(f"div_near_fix target[{iname}]", q, want, tg, est)
    wq, west = da.wave(lib, da.W_NEAR_U, [n, m, add, d], 2, inv)
    assert np.array_equal(west, est)
    expect_equal(f"div_near_u[{iname}]", wq, want, tg, west)
    report(primitive="div_near", form=form, shape="target", inv=iname, cases=len(tg), est_minus_q=[lo, hi],
           allowed=[-1, 1])
    want = da.quotients(rg)
    n, m, add, d, _ = rg.cols()
    n1, want1 = _pairs(rg)
    q, est, q32 = da.thread(lib, da.T_DIV_NEAR, [n, m, add, d], 3, da.INV_IEEE)
    lo, hi = expect_distance(f"{form} range estimate[ieee]", est, want, -1, 1, rg)
    expect_equal("div_near_fix<false> range[ieee]", q, want, rg, est)
    q0, q1, p0, p1 = da.wave(lib, da.W_NEAR_U2, [n, n1, m, add, d], 4, da.INV_IEEE)
    expect_equal("div_near_u2<false>.0[ieee]", q0, want, rg)
    expect_equal("div_near_u2<false>.1[ieee]", q1, want1, rg)
    if form == "near32":                                          # n below 2^32: the 32 x 64-bit product
        expect_equal("div_near_fix<true> range[ieee]", q32, want, rg, est)
        expect_equal("div_near_u2<true>.0[ieee]", p0, want, rg)
        expect_equal("div_near_u2<true>.1[ieee]", p1, want1, rg)
    report(primitive="div_near", form=form, shape="range", inv="ieee", cases=len(rg), est_minus_q=[lo, hi],
           allowed=[-1, 1])


def test_div_mid(lib, worst):
    """div_mid on u64 rows of 2^50 and more, 1/T the device's IEEE divide: div_mid_est_w with the
    addend as (double)T or 0.0 (div_mid_u2) and div_mid_est, both within one of the quotient,
    div_mid_fix exact."""
    cs = da.decoder_cases("mid", worst)
    want = da.quotients(cs)
    n, m, add, d, addd = cs.cols()
    n1, want1 = _pairs(cs)
    q, est, q2, est2 = da.thread(lib, da.T_DIV_MID, [n, m, add, d, addd], 4, da.INV_IEEE)
    lo, hi = expect_distance("div_mid_est_w", est, want, -1, 1, cs)
    lo2, hi2 = expect_distance("div_mid_est", est2, want, -1, 1, cs)
    expect_equal("div_mid_fix(div_mid_est_w)", q, want, cs, est)
    expect_equal("div_mid_fix(div_mid_est)", q2, want, cs, est2)
    q0, q1, e0, e1 = da.wave(lib, da.W_MID_U2, [n, n1, m, add, d, addd], 4, da.INV_IEEE)
    assert np.array_equal(e0, est)
    expect_equal("div_mid_u2.0", q0, want, cs, e0)
    expect_equal("div_mid_u2.1", q1, want1, cs, e1)
    report(primitive="div_mid", inv="ieee", cases=len(cs), est_w_minus_q=[lo, hi], est_minus_q=[lo2, hi2],
           allowed=[-1, 1])


def test_div_floor_and_pairs(lib, worst):
    """div_floor on its device path and div_floor_inv_n with recip(d): exact for quotients up to
    2^64 - 1 (kTopQ and its neighbours), at most two final fix-ups; div_pair, unfudged_range_inv
    and floor_range (the general path past the small forms' thresholds) exact."""
    cs = da.floor_cases(worst)
    nh, nl, d = cs.cols()
    want = [((h << 64) | l) // dd for h, l, dd in cs.rows]
    q, qi, fix = da.thread(lib, da.T_DIV_FLOOR, [nh, nl, d], 3)
    expect_equal("div_floor", q, want, cs)
    expect_equal("div_floor_inv_n", qi, want, cs)
    i = int(fix.argmax())
    assert int(fix[i]) <= 2, f"div_floor_inv_n: {int(fix[i])} fix-ups at {dict(zip(cs.names, cs.rows[i]))}"
    report(primitive="div_floor_inv", inv="recip", cases=len(cs), fixups_max=int(fix.max()), allowed=2)
    rs = da.range_cases(worst)
    lo, hi, T, w = rs.cols()
    ceil = [[-(-(c * ww) // t) for c, ww, t in zip(col, w, T)] for col in (lo, hi)]
    flo = [[c * ww // t for c, ww, t in zip(col, w, T)] for col in (lo, hi)]
    a, b, fa, fb = da.thread(lib, da.T_RANGES, [lo, hi, T, w], 4, da.INV_RECIP)
    for name, got, exact in (("unfudged_range_inv.a", a, ceil[0]), ("unfudged_range_inv.b", b, ceil[1]),
                             ("floor_range.a", fa, flo[0]), ("floor_range.b", fb, flo[1])):
        expect_equal(name, got, exact, rs)
    a, b, _, _ = da.thread(lib, da.T_RANGES, [lo, hi, T, w], 4, da.INV_IEEE)
    expect_equal("unfudged_range_inv.a[ieee]", a, ceil[0], rs)
    expect_equal("unfudged_range_inv.b[ieee]", b, ceil[1], rs)
    for add, exact in (([t - 1 for t in T], ceil), ([0] * len(rs), flo)):
        for inv in (da.INV_RECIP, da.INV_IEEE):
            q0, q1 = da.wave(lib, da.W_DIV_PAIR, [lo, hi, w, add, T], 2, inv)
            expect_equal("div_pair.0", q0, exact[0], rs)
            expect_equal("div_pair.1", q1, exact[1], rs)


def test_row_fractions(lib, worst):
    """row_frac (2^63 at c = T, kNoFrac from T = 2^63) and the products that replace the division:
    frac_mul_div<false>, frac_mul_div<true> below T = 2^62 (thread and wave-uniform), frac_mul_div32
    below 2^32, frac_pair."""
    cs = da.frac_cases(worst)
    c, w, T, ceil = cs.cols()
    want = list(zip(*[da.frac_want(*r) for r in cs.rows]))
    outs = da.thread(lib, da.T_FRAC, [c, w, T, ceil], 4)
    for name, got, exact in zip(("row_frac", "frac_mul_div<false>", "frac_mul_div<true>", "frac_mul_div32"), outs, want):
        expect_equal(name, got, list(exact), cs)
    f, qu = da.wave(lib, da.W_FRAC_UNI, [c, w, T, ceil], 2)
    expect_equal("row_frac (wave)", f, list(want[0]), cs)
    expect_equal("frac_mul_div<true> (wave-uniform)", qu, list(want[2]), cs)
    c1 = [t - x for x, t in zip(c, T)]
    want1 = [da.frac_want(x, ww, t, ce)[1] for x, ww, t, ce in zip(c1, w, T, ceil)]
    q0, q1 = da.wave(lib, da.W_FRAC_PAIR, [c, c1, w, T, ceil], 2)
    expect_equal("frac_pair.0", q0, list(want[1]), cs)
    expect_equal("frac_pair.1", q1, want1, cs)
    report(primitive="row_frac / frac_mul_div", cases=len(cs), q_max=max(x for x in want[0] if x != da.NOFRAC))


def test_fudge_and_ratio(lib, worst):
    """fudge_x / fudge_f (the fudged ranges' closed form), is_fudged, and cr_ratio == CPython's a / b."""
    cs = da.fudge_cases(worst)
    want = list(zip(*[da.fudge_want(*r) for r in cs.rows]))
    i, c, j, T, w, V, minp = cs.cols()
    f, xl, xh = da.thread(lib, da.T_FUDGE, [i, c, j, T, w, V], 3)
    expect_equal("fudge_f", f, list(want[0]), cs)
    expect_equal("fudge_x (low word)", xl, list(want[1]), cs)
    expect_equal("fudge_x (high word)", xh, list(want[2]), cs)
    expect_equal("is_fudged", da.thread(lib, da.T_IS_FUDGED, [T, w, minp], 1)[0], list(want[3]), cs)
    rs = da.ratio_cases(worst)
    a, b = rs.cols()
    expect_equal("cr_ratio", da.thread(lib, da.T_CR_RATIO, [a, b], 1)[0], [da.f64_bits(x / y) for x, y in rs.rows], rs)


# ------------------------------------------------------------------ end to end
def _table(total, V, dtype, rng):
    """V entries of at least 4 summing to `total`, the last two small (symbols V - 2, V - 1: the top of the CDF)."""
    row = rng.integers(total // (2 * V), total // V, size=V).astype(object)
    row[V - 2], row[V - 1] = 5, 4
    row[0] += total - int(row.sum())
    assert int(row.sum()) == total and min(row) >= 4
    return row.astype(dtype)


@pytest.mark.parametrize("B", [2, 64, 2048])
@pytest.mark.parametrize("bits_,prec", [(32, 49), (32, 50), (64, 49), (64, 50)])
def test_tables_with_worst_reciprocal_totals_end_to_end(worst, bits_, prec, B):
    """Static u32 / u64 tables whose totals are the sweep's worst-reciprocal divisors (below 2^32, and
    of 40, 49 and 50 bits), at prec 49 and 50, the symbols weighted to V - 1 and V - 2 so ranges
    reach the top of w: 200 steps encoded and decoded at 2 streams (the lean step), 64
    (k_decode_seq) and 2048 (the wave path), bytes and symbols against the C oracle."""
    import ctypes as C
    from lac_amd.batch import BatchCoder
    from oracle import oracle as coracle
    rng = np.random.default_rng(1000 * bits_ + prec)
    V, T = 32, 200
    dt = np.uint32 if bits_ == 32 else np.uint64
    pool = [d for L in ((32, 24) if bits_ == 32 else (50, 49, 40)) for d in worst[L]]
    rows = np.stack([_table(pool[(b * 7) % len(pool)], V, dt, rng) for b in range(B)])
    sym = rng.choice(V, size=(T, B), p=[0.2 / (V - 2)] * (V - 2) + [0.4, 0.4]).astype(np.int32)
    cap = (T * (prec + 2) + 64) // 8 + 16
    out = np.zeros((B, cap), dtype=np.uint8)
    onb = np.zeros(B, dtype=np.uint64)
    status = np.zeros(B, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = coracle.lib().lacref_encode_batch(p(rows), rows.itemsize, V, T, B, 0, V, p(sym), prec, p(out), cap, p(onb),
                                           p(status), 8)
    assert rc == 0 and not status.any()
    dp = torch.from_numpy(rows.view(np.int32 if bits_ == 32 else np.int64)).to(DEV).view(1, B, V).expand(T, B, V)
    c = BatchCoder(V, B, prec=prec, pmf_bits=bits_, capacity_bits=T * (prec + 2) + 256, device=DEV)
    c.encode_job(dp, torch.from_numpy(sym).to(DEV))
    c.raise_on_error()
    data, nb = c.to_bytes()
    for b in range(B):
        assert int(nb[b]) == int(onb[b]) and data[b] == out[b, :(int(onb[b]) + 7) // 8].tobytes(), b
    for path in ("stats", "fused"):
        c.set_decode_path(path)
        c.decode_open()
        got = c.decode(dp).cpu().numpy()
        assert np.array_equal(got, sym), (path, np.argwhere(got != sym)[:4])
    c.close()
