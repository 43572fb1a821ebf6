"""Host checks of sparse-row coding (include/lac.h lac_encode_sparse / lac_decode_sparse_steps), no
GPU needed.

* lac_amd/csrc/lac_sparse.h, the plain rules the kernels share (tests/native/sparse_check.cpp), in
  both of their forms -- the literal whole-row rule and the per-lane partials over 64 emulated
  lanes: validation and its precedence at every edge, 1 000 random rows against Python integers on
  the dense row (the encode triple of every symbol of interest; the decode search at t = 0, T - 1
  and every A_j - 1, A_j, B_j - 1, B_j), whole jobs of 130 steps against the C oracle on the dense
  rows (V <= 300) and on the three-entry rows of the triples (V = 2^18).  The sweep also runs as a
  stand-alone ASan + UBSan program.
* The fixtures of tests/golden/sparse_cases.json (tools/gen_golden_sparse.py: the reference's
  ``AC(CDFPredictor(lazy), prec)`` on the dense rows) against the C oracle: this pins the yardstick
  the GPU tests use.
* The census of the existing fixtures that are sparse rows with every symbol a pair: the GPU test
  codes them and cannot quietly skip them.
"""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import ranges as R
import sparse as S
from conftest import REPO
from oracle import oracle

NATIVE = os.path.join(REPO, "tests", "native")
SO = os.path.join(NATIVE, "libsparsecheck.so")
SRC = os.path.join(NATIVE, "sparse_check.cpp")
HDRS = [os.path.join(REPO, "lac_amd", "csrc", h) for h in ("lac_sparse.h", "lac_ranges.h", "lac_core.h")] + [
    os.path.join(REPO, "include", "lac.h")]
INCS = ["-I", os.path.join(REPO, "lac_amd", "csrc"), "-I", os.path.join(REPO, "include")]

LAC_OK, LAC_E_SYMBOL_RANGE, LAC_E_TABLE, LAC_E_DECODE_RANGE, LAC_E_CAPACITY, LAC_E_UNDETERMINED = 0, -3, -5, -6, -7, -12
U64, I64, U32 = C.c_uint64, C.c_int64, C.c_uint32
FORMS = (0, 1)                                               # the literal rule, the lanes


def _stale(target, *deps):
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(d) for d in deps)


@pytest.fixture(scope="module")
def sc():
    if _stale(SO, SRC, *HDRS):
        subprocess.run(["hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", *INCS, SRC, "-o", SO], check=True)
    lib = C.CDLL(SO)
    vp = C.c_void_p
    lib.sc_args_ok.argtypes = [U64, U64, I64, I64, I64, U32]
    lib.sc_base_v.argtypes = [U32, I64]
    lib.sc_base_v.restype = U64
    lib.sc_row_check.argtypes = [C.c_int, vp, vp, C.c_int, U32, I64, C.c_int, vp]
    lib.sc_range.argtypes = [C.c_int, vp, vp, C.c_int, U32, I64, C.c_int, I64, vp, vp]
    lib.sc_search.argtypes = [C.c_int, vp, vp, C.c_int, U32, I64, C.c_int, I64, vp, vp, vp, vp]
    lib.sc_encode.argtypes = [C.c_int, I64, vp, vp, C.c_int, U32, I64, vp, C.c_int, U64, vp, vp, vp, vp]
    lib.sc_flush.argtypes = [I64, I64, C.c_int, vp]
    lib.sc_decode.argtypes = [C.c_int, I64, vp, vp, C.c_int, U32, I64, C.c_int, vp, U64, C.c_int, vp, vp]
    lib.sc_sweep.argtypes = [U64, vp]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _check(sc, form, idx, wt, base, V, prec):
    T = U64()
    idx, wt = np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(wt, dtype=np.uint32)
    rc = sc.sc_row_check(form, _p(idx), _p(wt), len(idx), base, V, prec, C.byref(T))
    return rc, T.value


# ------------------------------------------------------------------ the call's arguments
def test_argument_rules(sc):
    ok = lambda idx=64, wt=128, K=8, ss=8, bs=8, base=1: sc.sc_args_ok(idx, wt, K, ss, bs, base)  # noqa: E731
    assert ok() and ok(K=4) and ok(K=256) and ok(ss=0, bs=0) and ok(base=(1 << 32) - 1) and ok(ss=12, bs=1 << 40)
    for K in (0, 1, 2, 3, 5, 6, 7, 254, 255, 257, 260, 512, -4):
        assert not ok(K=K), K
    assert not ok(base=0)
    for s in (1, 2, 3, 5, 7, -4, -1):
        assert not ok(ss=s) and not ok(bs=s), s
    for a in (0, 4, 8, 12, 65, 72):
        assert not ok(idx=a) and not ok(wt=a), a
    assert sc.sc_base_v(3, 300) == 900 and sc.sc_base_v((1 << 32) - 1, 1 << 31) == 1 << 62


# ------------------------------------------------------------------ validity and precedence
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("prec", (2, 16, 48, 61))
def test_validation_at_every_edge(sc, form, prec):
    half = 1 << (prec - 1)
    V = 2 if prec == 2 else 300
    chk = lambda idx, wt, base=1, V=V: _check(sc, form, idx, wt, base, V, prec)  # noqa: E731
    pad8 = [-1] * 8
    assert chk(pad8, [0] * 8) == (LAC_OK, V)                           # n = 0: the uniform row
    assert chk(pad8, [7] * 8) == (LAC_OK, V)                           # a pad's weight is ignored
    room = half - V
    w1 = min(room, (1 << 32) - 1)
    assert chk([0] + [-1] * 7, [w1] + [0] * 7) == (LAC_OK, V + w1)     # a pair at symbol 0
    assert chk([V - 1] + [-1] * 7, [0] + [5] * 7) == (LAC_OK, V)       # a pair at V - 1 with wt = 0
    assert chk([0, 1, -1, -1], [0, w1, 9, 9]) == (LAC_OK, V + w1)      # adjacent pairs
    if room <= (1 << 32) - 1:                                          # T = 2^(prec-1) exactly, and one more
        assert chk([1] + [-1] * 3, [room] + [0] * 3) == (LAC_OK, half)
        if room + 1 <= (1 << 32) - 1:
            assert chk([1] + [-1] * 3, [room + 1] + [0] * 3) == (LAC_E_TABLE, 0)
        assert chk([0, 1, -1, -1], [room, 1, 0, 0]) == (LAC_E_TABLE, 0)
    assert chk([V] + [-1] * 3, [0] * 4) == (LAC_E_TABLE, 0)            # idx >= V
    assert chk([1 << 30] + [-1] * 3, [0] * 4) == (LAC_E_TABLE, 0)
    assert chk([-2] + [-1] * 3, [0] * 4) == (LAC_E_TABLE, 0)           # idx < -1, first slot
    assert chk([0, -1, -1, -2], [0] * 4) == (LAC_E_TABLE, 0)           # idx < -1 among the pads
    assert chk([0, -(1 << 31), -1, -1], [0] * 4) == (LAC_E_TABLE, 0)
    assert chk([-1, 0, -1, -1], [0] * 4) == (LAC_E_TABLE, 0)           # a pair after a pad
    assert chk([0, -1, -1, -1, -1, -1, -1, 1], [0] * 8) == (LAC_E_TABLE, 0)
    assert chk([1, 1, -1, -1], [0] * 4) == (LAC_E_TABLE, 0)            # equal
    assert chk([1, 0, -1, -1], [0] * 4) == (LAC_E_TABLE, 0)            # descending
    if V >= 8:
        # the lanes' seam: slots 3 | 4 and 251 | 255
        assert chk([0, 1, 2, 3, 4, -1, -1, -1], [0] * 8)[0] == LAC_OK
        assert chk([0, 1, 2, 4, 4, -1, -1, -1], [0] * 8)[0] == LAC_E_TABLE      # equal across the seam
        assert chk([0, 1, 2, 5, 4, -1, -1, -1], [0] * 8)[0] == LAC_E_TABLE      # descending across it
        assert chk([0, 1, 2, -1, 4, -1, -1, -1], [0] * 8)[0] == LAC_E_TABLE     # a pad, then a pair in the next lane
        full = list(range(256))
        assert chk(full, [0] * 256)[0] == LAC_OK                       # n = K = 256
        assert chk(full[:252] + [-1] * 4, [0] * 256)[0] == LAC_OK
        assert chk(full[:251] + [251, 251, 253, 254, 255][:5], [0] * 256)[0] == LAC_E_TABLE
        assert chk(full[:255] + [254], [0] * 256)[0] == LAC_E_TABLE    # slot 255 equals slot 254
        assert chk(full[:251] + [-1] + full[252:], [0] * 256)[0] == LAC_E_TABLE
    # base: base V alone above 2^(prec-1)
    if half // V + 1 < 1 << 32:
        assert chk(pad8, [0] * 8, base=half // V)[0] == LAC_OK
        assert chk(pad8, [0] * 8, base=half // V + 1)[0] == LAC_E_TABLE
    assert chk(pad8, [0] * 8, base=(1 << 32) - 1, V=1 << 31)[0] == LAC_E_TABLE


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("prec", (2, 16, 48, 61))
def test_step_precedence_and_what_errors_freeze(sc, form, prec):
    """Encode: symbol range, then the row, then capacity after the narrowing.  Decode: the row, then
    the registers, then undetermined.  A failed step leaves everything as before it."""
    V, K, base = (2, 4, 1) if prec == 2 else (300, 8, 3)
    rows, syms = S.random_job(11, V, base, K, prec, 6)
    idx, wt = S.job_slots(rows, K)

    def enc(idx, wt, syms, cap_words=8, V=V, base=base):
        ek = np.zeros(2 * len(syms), dtype=np.uint64)
        planes = np.zeros(2 * cap_words, dtype=np.uint64)
        regs, es = np.zeros(4, dtype=np.int64), I64(-1)
        st = sc.sc_encode(form, len(syms), _p(np.ascontiguousarray(idx)), _p(np.ascontiguousarray(wt)), K, base, V,
                          _p(np.array(syms, dtype=np.int32)), prec, cap_words, _p(ek), _p(planes), _p(regs), C.byref(es))
        return st, es.value, ek.reshape(-1, 2), planes, regs

    ref3 = enc(idx[:3], wt[:3], syms[:3])
    assert ref3[0] == LAC_OK
    bad_row = idx.copy()
    bad_row[3, 1] = bad_row[3, 0] if bad_row[3, 0] >= 0 else -2        # malformed whatever n is
    for ii, ss, code in ((bad_row, syms, LAC_E_TABLE), (idx, syms[:3] + [V] + syms[4:], LAC_E_SYMBOL_RANGE),
                         (idx, syms[:3] + [-1] + syms[4:], LAC_E_SYMBOL_RANGE),
                         (bad_row, syms[:3] + [V] + syms[4:], LAC_E_SYMBOL_RANGE)):        # the symbol before the row
        st, es, ek, planes, regs = enc(ii, wt, ss)
        assert (st, es, regs[3]) == (code, 3, 3) and regs.tolist() == ref3[4].tolist()
        assert np.int64(ek[3, 1]) == -1 and (planes == ref3[3]).all()
    # capacity, after the narrowing.  Uniform rows (n = 0) over Vu = 2^bits symbols cost exactly `bits`
    # bits a step and bring the registers back to l = 0, w = 2^prec, so a capacity of one word holds
    # 64 / bits steps and the next one fails: its digits are in the trace, its registers the narrowed ones
    bits = min(8, prec - 1)
    Vu, ok_steps = 1 << bits, 64 // bits
    n = ok_steps + 2
    ui, uw = np.full((n, K), -1, dtype=np.int32), np.zeros((n, K), dtype=np.uint32)
    usyms = [(5 * t + 1) % Vu for t in range(n)]
    st, es, ek, planes, regs = enc(ui, uw, usyms, cap_words=1, V=Vu, base=1)
    full = enc(ui, uw, usyms, V=Vu, base=1)
    assert full[0] == LAC_OK and int(full[4][2]) == n * bits
    assert (st, es, int(regs[3])) == (LAC_E_CAPACITY, ok_steps, ok_steps)
    assert int(np.int64(ek[es, 1])) == bits and (ek[:es + 1] == full[2][:es + 1]).all()
    assert (int(regs[0]), int(regs[1]), int(regs[2])) == (0, (1 << prec) - 1, (ok_steps + 1) * bits)
    # a symbol out of range on a full stream is the symbol's error, a malformed row the row's: both before capacity
    st, es, ek, planes, regs = enc(ui, uw, usyms[:ok_steps] + [Vu] + usyms[ok_steps + 1:], cap_words=1, V=Vu, base=1)
    assert (st, es) == (LAC_E_SYMBOL_RANGE, ok_steps)
    ub = ui.copy()
    ub[ok_steps, 1] = 0
    st, es, ek, planes, regs = enc(ub, uw, usyms, cap_words=1, V=Vu, base=1)
    assert (st, es) == (LAC_E_TABLE, ok_steps)
    # decode
    data, nbits, _ = oracle.encode(S.dense_job(rows, base, V), syms, prec)
    buf = np.frombuffer(data + b"\0" * 8, dtype=np.uint8).copy()

    def dec(idx, wt, n, stop=0, nb=nbits):
        out, regs = np.zeros(n, dtype=np.int32), np.zeros(7, dtype=np.int64)
        st = sc.sc_decode(form, n, _p(np.ascontiguousarray(idx)), _p(np.ascontiguousarray(wt)), K, base, V, prec, _p(buf),
                          nb, stop, _p(out), _p(regs))
        return st, out.tolist(), regs.tolist()

    st, out, regs = dec(idx, wt, 6)
    assert (st, out) == (LAC_OK, syms)
    st3, out3, regs3 = dec(idx, wt, 3)
    st, out, regs = dec(bad_row, wt, 6)
    assert (st, out, regs) == (LAC_E_TABLE, syms[:3] + [-1] * 3, regs3)
    # a truncated stream: with the stop the decoder halts before the first undetermined symbol
    st, out, regs = dec(idx, wt, 6, stop=1, nb=max(nbits - 20, 0))
    assert st == LAC_E_UNDETERMINED and out == syms[:regs[4]] + [-1] * (6 - regs[4]) and regs[4] == regs[6] < 6


# ------------------------------------------------------------------ both forms against Python integers
def test_thousand_random_rows_against_python_integers_on_the_dense_row(sc):
    """Per row: both forms' verdict and total; the triple of every symbol of interest; the search
    at t = 0, T - 1 and every A_j - 1, A_j, B_j - 1, B_j -- equal to each other and to the dense row."""
    rng = random.Random(20)
    for i in range(1000):
        prec = rng.choice((16, 34, 48, 61))
        K = rng.choice((4, 8, 12, 64, 252, 256))
        V = rng.choice((5, 7, 64, 300, rng.randrange(1, 301)))
        base = rng.choice((1, 3, 70001))
        if base * V > 1 << (prec - 1):
            base = 1
        n = rng.choice((0, 1, K, None))
        pairs = S.random_pairs(rng, V, base, K, prec, n=n, full=(i % 6 == 0))
        idx, wt = S.slots(pairs, K)
        wt[len(pairs[0]):] = rng.randrange(1 << 32)                  # a pad's weight is ignored
        row, T = S.dense(pairs, base, V), S.total(pairs, base, V)
        assert sum(row) == T
        for form in FORMS:
            assert _check(sc, form, idx, wt, base, V, prec) == (LAC_OK, T), (i, form)
        ss = sorted({0, V - 1, rng.randrange(V), *(x for j in pairs[0] for x in (j - 1, j, j + 1) if 0 <= x < V)})
        lo, hi = U64(), U64()
        for s in ss:
            want = (sum(row[:s]), sum(row[:s + 1]))
            assert want == S.triple(pairs, base, s)
            for form in FORMS:
                sc.sc_range(form, _p(idx), _p(wt), K, base, V, prec, s, C.byref(lo), C.byref(hi))
                assert (lo.value, hi.value) == want, (i, form, s)
        ts = S.search_targets(pairs, base, V)
        tarr = np.array(ts, dtype=np.uint64)
        want = [S.dense_search(row, t) for t in ts]
        for form in FORMS:
            so, lo_, hi_ = np.zeros(len(ts), dtype=np.int64), np.zeros(len(ts), dtype=np.uint64), np.zeros(len(ts), dtype=np.uint64)
            sc.sc_search(form, _p(idx), _p(wt), K, base, V, prec, len(ts), _p(tarr), _p(so), _p(lo_), _p(hi_))
            got = list(zip(so.tolist(), (int(x) for x in lo_), (int(x) for x in hi_)))
            assert got == want, (i, form)


# ------------------------------------------------------------------ whole jobs against the oracle
def _encode_native(sc, form, idx, wt, K, base, V, syms, prec):
    n = len(syms)
    cap_words = (n * (prec + 2) + 64 + 63) // 64
    ek, planes = np.zeros(2 * n, dtype=np.uint64), np.zeros(2 * cap_words, dtype=np.uint64)
    regs, es = np.zeros(4, dtype=np.int64), I64(-1)
    st = sc.sc_encode(form, n, _p(np.ascontiguousarray(idx)), _p(np.ascontiguousarray(wt)), K, base, V,
                      _p(np.array(syms, dtype=np.int32)), prec, cap_words, _p(ek), _p(planes), _p(regs), C.byref(es))
    return st, ek.reshape(-1, 2), regs


def _digits(sc, ek, regs, prec):
    from lac_amd.batch import digits_of
    out = []
    for E, k in ek.tolist():
        out += digits_of(int(E), int(np.int64(np.uint64(k))))
    fd = np.zeros(8, dtype=np.int8)
    m = sc.sc_flush(int(regs[0]), int(regs[1]), prec, _p(fd))
    return out + fd[:m].tolist()


def _decode_native(sc, form, idx, wt, K, base, V, prec, data, nbits, n):
    buf = np.frombuffer(data + b"\0" * 8, dtype=np.uint8).copy()
    out, regs = np.zeros(n, dtype=np.int32), np.zeros(7, dtype=np.int64)
    st = sc.sc_decode(form, n, _p(np.ascontiguousarray(idx)), _p(np.ascontiguousarray(wt)), K, base, V, prec, _p(buf),
                      nbits, 0, _p(out), _p(regs))
    return st, out.tolist(), regs


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("prec,V,base,K", ((16, 300, 3, 8), (34, 5, 70001, 4), (48, 300, 1, 64), (61, 257, 1, 256),
                                           (48, 300, 1, 252)))
def test_whole_jobs_against_the_oracle_on_the_dense_rows(sc, form, prec, V, base, K):
    n = 130
    rows, syms = S.random_job(prec + K, V, base, K, prec, n)
    idx, wt = S.job_slots(rows, K)
    drows = S.dense_job(rows, base, V)
    data, nbits, digits = oracle.encode(drows, syms, prec)
    st, ek, regs = _encode_native(sc, form, idx, wt, K, base, V, syms, prec)
    assert st == LAC_OK and regs[3] == n and _digits(sc, ek, regs, prec) == digits
    assert oracle.decode(drows, data, nbits, n, prec) == syms
    st, out, dregs = _decode_native(sc, form, idx, wt, K, base, V, prec, data, nbits, n)
    assert (st, out, int(dregs[4])) == (LAC_OK, syms, n)
    # the registers and ndet are the range decoder's on the triples, in Python integers
    lo, hi, T = S.triples(rows, base, V, syms)
    _, ndet, states = R.py_decode(lo, hi, T, prec, data, nbits)
    assert tuple(dregs[:4].tolist()) == states[-1] and dregs[6] == ndet


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("prec,base,K", ((34, 1, 8), (48, (1 << 29) - 1, 64), (61, 3, 256)))
def test_whole_jobs_at_a_large_vocabulary_on_three_entry_rows(sc, form, prec, base, K):
    V, n = 1 << 18, 130
    rows, syms = S.random_job(prec, V, base, K, prec, n)
    idx, wt = S.job_slots(rows, K)
    lo, hi, T = S.triples(rows, base, V, syms)
    three = R.three_rows(lo, hi, T)
    data, nbits, digits = oracle.encode(three, [1] * n, prec)
    st, ek, regs = _encode_native(sc, form, idx, wt, K, base, V, syms, prec)
    assert st == LAC_OK and _digits(sc, ek, regs, prec) == digits
    st, out, dregs = _decode_native(sc, form, idx, wt, K, base, V, prec, data, nbits, n)
    assert (st, out) == (LAC_OK, syms)
    _, ndet, states = R.py_decode(lo, hi, T, prec, data, nbits)
    assert tuple(dregs[:4].tolist()) == states[-1] and dregs[6] == ndet


def test_sanitized_sweep_program(sc):
    """The sweep (the lanes against the literal rule and a dense row walked entry by entry, malformed
    rows included) in the library, and with whole-job round trips as a stand-alone program under
    AddressSanitizer + UndefinedBehaviorSanitizer (host code only)."""
    n = I64(0)
    assert sc.sc_sweep(12345, C.byref(n)) == 0 and n.value > 20000
    outdir = os.path.join(NATIVE, "_asan")
    os.makedirs(outdir, exist_ok=True)
    exe = os.path.join(outdir, "sparse_check_main")
    if _stale(exe, SRC, *HDRS):
        # host code only: the sanitizers are given to the host compilation alone
        subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-DSPARSE_CHECK_MAIN",
                        "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", *INCS, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    report = r.stdout + r.stderr
    assert r.returncode == 0, report[-3000:]
    assert "sparse_check: ok" in report and "ERROR" not in report and "runtime error" not in report


# ------------------------------------------------------------------ the fixtures pin the yardstick
def test_fixture_set_covers_the_issue():
    cases = S.SPARSE_CASES
    assert len(cases) >= 12
    assert {c["V"] for c in cases} >= {5, 300, 1 << 18} and {c["prec"] for c in cases} >= {16, 34, 48, 61}
    bases = {c["base"] for c in cases}
    assert {1, 3} <= bases and any(b > 1 << 16 for b in bases)
    rows = [(c, r, s) for c in cases for r, s in zip(c["rows"], c["syms"])]
    assert any(S.total(r, c["base"], c["V"]) == 1 << (c["prec"] - 1) for c, r, _ in rows)
    assert {0, 1} <= {len(r[0]) for _, r, _ in rows} and any(len(r[0]) == c["K"] for c, r, _ in rows)
    assert any(b == a + 1 for _, r, _ in rows for a, b in zip(r[0], r[0][1:]))           # adjacent pairs
    assert any(r[0] and r[0][0] == 0 for _, r, _ in rows) and any(r[0] and r[0][-1] == c["V"] - 1 for c, r, _ in rows)
    at = lambda f: any(f(c, r[0], s) for c, r, s in rows)  # noqa: E731
    assert at(lambda c, i, s: s in i)                                                      # at a pair
    assert at(lambda c, i, s: s not in i and s + 1 in i)                                   # directly before one
    assert at(lambda c, i, s: s not in i and s - 1 in i)                                   # directly after one
    assert at(lambda c, i, s: s not in i and (s == 0 or s - 1 in i) and s + 1 not in i and s + 1 < c["V"])   # first in a gap
    assert at(lambda c, i, s: s not in i and (s == c["V"] - 1 or s + 1 in i) and s - 1 not in i and s > 0)   # last in a gap
    for c in cases:
        assert c["K"] % 4 == 0 and 4 <= c["K"] <= 256 and len(c["rows"]) == len(c["syms"])
        for r in c["rows"]:
            idx, wt = S.slots(r, c["K"])
            assert S.row_valid(idx, wt, c["base"], c["V"], c["prec"]), c["name"]
        assert c["decoded_count"] >= len(c["syms"])
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "sparse_cases.json")) < 64 << 10


@pytest.mark.parametrize("case", S.SPARSE_CASES, ids=[c["name"] for c in S.SPARSE_CASES])
def test_reference_bits_are_the_oracle_and_both_forms(sc, case):
    V, base, K, prec, syms = case["V"], case["base"], case["K"], case["prec"], case["syms"]
    n = len(syms)
    lo, hi, T = S.triples(case["rows"], base, V, syms)
    if V <= 300:
        rows, osyms = S.dense_job(case["rows"], base, V), syms
    else:
        rows, osyms = R.three_rows(lo, hi, T), [1] * n
    data, nbits, digits = oracle.encode(rows, osyms, prec)
    assert nbits == case["L"] and data.hex() == case["bytes"]
    assert oracle.decode(rows, data, nbits, n, prec) == osyms
    idx, wt = S.case_slots(case)
    for form in FORMS:
        st, ek, regs = _encode_native(sc, form, idx, wt, K, base, V, syms, prec)
        assert st == LAC_OK and _digits(sc, ek, regs, prec) == digits
        st, out, dregs = _decode_native(sc, form, idx, wt, K, base, V, prec, data, nbits, n)
        assert (st, out) == (LAC_OK, syms)
        assert dregs[6] == n <= case["decoded_count"]        # the bits determine every symbol of the job


# ------------------------------------------------------------------ census of the existing fixtures
def test_census_of_fixtures_that_are_sparse_rows(sc):
    cen = S.census()
    assert len(cen["static"]) >= 40 and len(cen["perstep"]) >= 8
    # their slots code to the reference's bits
    for c in cen["static"][:10] + cen["perstep"][:10]:
        idx, wt, base, K = S.census_slots(c)
        V, n = len(c["rows"][0]), len(c["syms"])
        if len(idx) == 1:
            idx, wt = np.repeat(idx, n, 0), np.repeat(wt, n, 0)
        for form in FORMS:
            st, ek, regs = _encode_native(sc, form, idx, wt, K, base, V, c["syms"], c["prec"])
            assert st == LAC_OK
            data, nbits, digits = oracle.encode(c["rows"], c["syms"], c["prec"], static=False) if len(c["rows"]) > 1 else \
                oracle.encode(c["rows"][0], c["syms"], c["prec"], static=True)
            assert nbits == c["L"] and data.hex() == c["bytes"] and _digits(sc, ek, regs, c["prec"]) == digits
