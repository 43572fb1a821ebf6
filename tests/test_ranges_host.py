"""Host checks of range-level coding (include/lac.h lac_encode_ranges / lac_decode_ranges_step),
no GPU needed.

* lac_amd/csrc/lac_ranges.h, the plain rules the kernels share (tests/native/ranges_check.cpp):
  validation and its precedence at the edges of validity, the launch geometry, the mapping of
  1 000 random valid triples (totals to 2^60, widths to 2^61) against Python integers, and whole
  jobs -- the same step function the kernels' lanes run -- against the C oracle on the
  three-entry rows [lo, hi - lo, T - hi] with symbol 1.  The sweep also runs as a stand-alone
  ASan + UBSan program.
* The fixtures of tests/golden/range_cases.json (tools/gen_golden_ranges.py: the reference's
  ``AC(CDFPredictor(lazy), prec)`` on implicit CDFs) against the C oracle on three-entry rows: this
  pins the yardstick the GPU tests use.
* The census of the existing fixtures whose every row total is at most 2^(prec-1): the GPU test
  codes their triples and cannot quietly skip them.
"""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import ranges as R
from conftest import REPO
from oracle import oracle

NATIVE = os.path.join(REPO, "tests", "native")
SO = os.path.join(NATIVE, "librangescheck.so")
SRC = os.path.join(NATIVE, "ranges_check.cpp")
HDRS = [os.path.join(REPO, "lac_amd", "csrc", h) for h in ("lac_ranges.h", "lac_core.h")] + [
    os.path.join(REPO, "include", "lac.h")]
INCS = ["-I", os.path.join(REPO, "lac_amd", "csrc"), "-I", os.path.join(REPO, "include")]

LAC_OK, LAC_E_ZERO_WIDTH, LAC_E_TABLE, LAC_E_DECODE_RANGE, LAC_E_CAPACITY, LAC_E_UNDETERMINED = 0, -4, -5, -6, -7, -12
U64 = C.c_uint64


def _stale(target, *deps):
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(d) for d in deps)


@pytest.fixture(scope="module")
def rc():
    if _stale(SO, SRC, *HDRS):
        subprocess.run(["hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", *INCS, SRC, "-o", SO], check=True)
    lib = C.CDLL(SO)
    lib.rc_check.argtypes = [U64, U64, U64, C.c_int]
    lib.rc_blocks.argtypes = [C.c_int64]
    lib.rc_blocks.restype = C.c_uint
    lib.rc_table.argtypes = [U64, U64, U64, C.c_void_p]
    lib.rc_map.argtypes = [U64, U64, U64, U64, C.c_void_p, C.c_void_p]
    lib.rc_target.argtypes = [U64, U64, U64]
    lib.rc_target.restype = U64
    lib.rc_encode.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, U64, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p]
    lib.rc_flush.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_void_p]
    lib.rc_decode.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, U64, C.c_int,
                              C.c_void_p, C.c_void_p]
    lib.rc_sweep.argtypes = [U64, C.c_void_p]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _u64(xs):
    return np.array([int(x) for x in xs], dtype=np.uint64)


# ------------------------------------------------------------------ lac_ranges.h: validity, geometry
@pytest.mark.parametrize("prec", (2, 16, 34, 48, 61))
def test_validation_and_precedence(rc, prec):
    half = 1 << (prec - 1)
    ok = rc.rc_check
    assert ok(0, 1, 1, prec) == LAC_OK                               # T = 1
    assert ok(0, half, half, prec) == LAC_OK                         # T = 2^(prec-1), hi = T
    assert ok(half - 1, half, half, prec) == LAC_OK
    assert ok(0, 0, 0, prec) == LAC_E_TABLE                          # T = 0, before the zero width
    assert ok(0, 1, 0, prec) == LAC_E_TABLE
    assert ok(0, 1, half + 1, prec) == LAC_E_TABLE                   # T = 2^(prec-1) + 1
    assert ok(0, half + 1, half + 1, prec) == LAC_E_TABLE
    assert ok(0, half + 1, half, prec) == LAC_E_TABLE                # hi = T + 1
    assert ok(half + 1, half + 1, half, prec) == LAC_E_TABLE         # hi > T before lo == hi
    assert ok(1, 0, half, prec) == LAC_E_TABLE                       # lo > hi
    assert ok(half, half - 1, half, prec) == LAC_E_TABLE if half > 1 else True
    assert ok(0, 0, half, prec) == LAC_E_ZERO_WIDTH                  # lo = hi
    assert ok(half, half, half, prec) == LAC_E_ZERO_WIDTH
    assert ok((1 << 64) - 1, (1 << 64) - 1, (1 << 64) - 1, prec) == LAC_E_TABLE


def test_launch_geometry(rc):
    assert rc.rc_threads() == 256
    assert [rc.rc_blocks(B) for B in (1, 64, 65, 256, 257)] == [1, 1, 1, 1, 2]
    assert rc.rc_blocks(1 << 20) == 4096 and rc.rc_blocks(65536) == 256


def test_three_entry_table(rc):
    row = np.zeros(3, dtype=np.uint64)
    rc.rc_table(5, 9, 20, _p(row))
    assert row.tolist() == [5, 4, 11] == R.three_rows([5], [9], [20])[0].tolist()


def _random_triple(rng, prec, i):
    half = 1 << (prec - 1)
    T = half if i % 7 == 0 else rng.randrange(1, half + 1)
    hi = T if i % 5 == 0 else rng.randrange(1, T + 1)
    lo = 0 if i % 3 == 0 else rng.randrange(0, hi)
    return lo, hi, T


def test_mapping_against_python_integers(rc):
    """1 000 random valid triples, totals to 2^60 and widths to 2^61."""
    rng = random.Random(7)
    a, b = U64(), U64()
    for i in range(1000):
        prec = rng.choice((2, 3, 16, 34, 48, 60, 61))
        lo, hi, T = _random_triple(rng, prec, i)
        half = 1 << (prec - 1)
        w = 2 * half if i % 11 == 0 else rng.randrange(half + 1, 2 * half + 1)
        assert rc.rc_check(lo, hi, T, prec) == LAC_OK
        rc.rc_map(lo, hi, T, w, C.byref(a), C.byref(b))
        assert (a.value, b.value) == (-(-(lo * w) // T), -(-(hi * w) // T)), (lo, hi, T, w)
        assert a.value < b.value <= w
        v = rng.randrange(a.value, b.value)
        assert lo <= rc.rc_target(v, T, w) == (v * T) // w < hi


def _encode_native(rc, lo, hi, T, prec, cap_words=None):
    n = len(lo)
    cap_words = cap_words or (n * (prec + 2) + 64 + 63) // 64
    ek = np.zeros(2 * max(n, 1), dtype=np.uint64)
    planes = np.zeros(2 * cap_words, dtype=np.uint64)
    regs = np.zeros(4, dtype=np.int64)
    es = C.c_int64(-1)
    st = rc.rc_encode(n, _p(_u64(lo)), _p(_u64(hi)), _p(_u64(T)), prec, cap_words, _p(ek), _p(planes), _p(regs),
                      C.byref(es))
    return st, es.value, ek.reshape(-1, 2)[:n], planes.reshape(2, cap_words), regs


def _digits(ek):
    from lac_amd.batch import digits_of
    out = []
    for E, k in ek.tolist():
        out += digits_of(int(E), int(np.int64(np.uint64(k))))
    return out


def _flush(rc, regs, prec):
    fd = np.zeros(8, dtype=np.int8)
    m = rc.rc_flush(int(regs[0]), int(regs[1]), prec, _p(fd))
    return fd[:m].tolist()


@pytest.mark.parametrize("prec", (16, 34, 40, 48, 61))
def test_whole_jobs_against_the_oracle_on_three_entry_rows(rc, prec):
    """The step the kernels' lanes run, 130 symbols: digits, flush and plane bits are the oracle's
    on [lo, hi - lo, T - hi] with symbol 1; the oracle decodes all 1s; the native decoder's targets
    lie in [lo, hi), equal the Python-integer decoder's, and so do its registers and ndet."""
    rng = random.Random(prec)
    n = 130
    tri = [_random_triple(rng, prec, i + 1) for i in range(n)]
    tri[0], tri[1] = (0, 1, 1), (0, tri[1][2], tri[1][2])            # T = 1 and lo = 0, hi = T: zero bits
    lo, hi, T = (list(x) for x in zip(*tri))
    rows = R.three_rows(lo, hi, T)
    data, nbits, digits = oracle.encode(rows, [1] * n, prec)
    st, _, ek, planes, regs = _encode_native(rc, lo, hi, T, prec)
    assert st == LAC_OK and regs[3] == n
    assert _digits(ek) + _flush(rc, regs, prec) == digits
    # planes: A + C (big integers of L bits) are the digits before the flush
    L = int(regs[2])
    val = lambda p: int.from_bytes(p.astype(">u8").tobytes(), "big") >> (64 * len(p) - L) if L else 0  # noqa: E731
    body = 0
    for d in _digits(ek):
        body = 2 * body + d
    assert val(planes[0]) + val(planes[1]) == body and L == len(_digits(ek))
    assert oracle.decode(rows, data, nbits, n, prec) == [1] * n
    tg = np.zeros(n, dtype=np.uint64)
    dregs = np.zeros(7, dtype=np.int64)
    buf = np.frombuffer(data + b"\0" * 8, dtype=np.uint8).copy()
    assert rc.rc_decode(n, _p(_u64(lo)), _p(_u64(hi)), _p(_u64(T)), prec, _p(buf), nbits, 0, _p(tg), _p(dregs)) == LAC_OK
    want, ndet, states = R.py_decode(lo, hi, T, prec, data, nbits)
    assert tg.tolist() == want and all(a <= t < b for a, t, b in zip(lo, want, hi))
    assert tuple(dregs[:4].tolist()) == states[-1] and dregs[4] == n and dregs[6] == ndet
    # with the stop the stream halts before the first undetermined symbol, registers as before it
    rcode = rc.rc_decode(n, _p(_u64(lo)), _p(_u64(hi)), _p(_u64(T)), prec, _p(buf), nbits, 1, _p(tg), _p(dregs))
    assert (rcode, int(dregs[4])) == ((LAC_OK, n) if ndet == n else (LAC_E_UNDETERMINED, ndet))
    assert tuple(dregs[:4].tolist()) == states[int(dregs[4])]


def test_step_errors_and_what_they_freeze(rc):
    prec, half = 16, 1 << 15
    good = [(3, 9, 20)] * 5
    for bad, code in (((0, 1, 0), LAC_E_TABLE), ((0, 1, half + 1), LAC_E_TABLE), ((0, 21, 20), LAC_E_TABLE),
                      ((9, 3, 20), LAC_E_TABLE), ((9, 9, 20), LAC_E_ZERO_WIDTH), ((0, 0, 0), LAC_E_TABLE)):
        lo, hi, T = (list(x) for x in zip(*(good[:3] + [bad] + good[3:])))
        st, es, ek, planes, regs = _encode_native(rc, lo, hi, T, prec, cap_words=4)
        ref = _encode_native(rc, lo[:3], hi[:3], T[:3], prec, cap_words=4)
        assert (st, es, regs[3]) == (code, 3, 3) and regs.tolist() == ref[4].tolist()
        assert np.int64(np.uint64(ek[3, 1])) == -1 and (planes == ref[3]).all()
    # capacity: one word holds the first symbols' digits; the failing step's registers are the narrowed ones
    lo, hi, T = [1] * 40, [2] * 40, [half] * 40                      # 15 bits per symbol
    st, es, ek, planes, regs = _encode_native(rc, lo, hi, T, prec, cap_words=1)
    assert (st, es, regs[3]) == (LAC_E_CAPACITY, 4, 4) and regs[2] == 75
    rows = R.three_rows(lo, hi, T)
    # decode: a range that misses the target, an invalid triple, and an empty range
    data, nbits, _ = oracle.encode(rows[:5], [1] * 5, prec)
    buf = np.frombuffer(data + b"\0" * 8, dtype=np.uint8).copy()
    tg, dregs = np.zeros(5, dtype=np.uint64), np.zeros(7, dtype=np.int64)
    for bad, code in (((2, 3, half), LAC_E_DECODE_RANGE), ((1, 2, half + 1), LAC_E_TABLE), ((1, 1, half), LAC_E_DECODE_RANGE),
                      ((0, 1, half), LAC_E_DECODE_RANGE), ((2, 1, half), LAC_E_TABLE)):
        l2, h2, t2 = lo[:5], hi[:5], T[:5]
        l2[2], h2[2], t2[2] = bad
        assert rc.rc_decode(5, _p(_u64(l2)), _p(_u64(h2)), _p(_u64(t2)), prec, _p(buf), nbits, 0, _p(tg), _p(dregs)) == code
        want = R.py_decode(lo[:2], hi[:2], T[:2], prec, data, nbits)[2][-1]
        assert dregs[4] == 2 and tuple(dregs[:4].tolist()) == want
        assert tg[2] == ((1 << 64) - 1 if t2[2] > half else (want[2] - want[0]) * t2[2] // (want[1] - want[0] + 1))


def test_sanitized_sweep_program(rc):
    """The sweep (mapping against 128-bit division, range_append against plane_append, whole-job
    round trips) in the library, and as a stand-alone program under AddressSanitizer +
    UndefinedBehaviorSanitizer (host code only)."""
    n = C.c_int64(0)
    assert rc.rc_sweep(12345, C.byref(n)) == 0 and n.value > 3000
    outdir = os.path.join(NATIVE, "_asan")
    os.makedirs(outdir, exist_ok=True)
    exe = os.path.join(outdir, "ranges_check_main")
    if _stale(exe, SRC, *HDRS):
        # host code only: the sanitizers are given to the host compilation alone
        subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-DRANGES_CHECK_MAIN",
                        "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", *INCS, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    report = r.stdout + r.stderr
    assert r.returncode == 0, report[-3000:]
    assert "ranges_check: ok" in report and "ERROR" not in report and "runtime error" not in report


# ------------------------------------------------------------------ the fixtures pin the yardstick
def test_fixture_set_covers_the_issue():
    cases = R.RANGE_CASES
    assert len(cases) >= 10
    assert {(c["kind"], c["V"]) for c in cases} >= {("quad", 1 << 16), ("quad", 1 << 20), ("uniform", 1)}
    for prec in (16, 48):
        assert any(c["kind"] == "uniform" and R.total_of(c) == 1 << (prec - 1) and c["prec"] == prec for c in cases)
    assert {c["prec"] for c in cases} >= {16, 34, 48, 61} and {len(c["syms"]) for c in cases} >= {1, 64, 65, 130}
    for c in cases:
        assert 0 < R.total_of(c) <= 1 << (c["prec"] - 1), c["name"]
        if len(c["syms"]) > 1:
            assert 0 in c["syms"] and c["V"] - 1 in c["syms"], c["name"]
        if c["V"] == 1:                                    # every symbol is zero bits; L is the flush alone
            assert c["L"] == 0 and c["bytes"] == "" and c["decoded_count"] == 0
        else:
            assert c["decoded_count"] >= len(c["syms"])
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "range_cases.json")) < 64 << 10


@pytest.mark.parametrize("case", R.RANGE_CASES, ids=[c["name"] for c in R.RANGE_CASES])
def test_reference_bits_are_the_oracle_on_three_entry_rows(case):
    lo, hi, T = R.case_triples(case)
    rows, n = R.three_rows(lo, hi, T), len(case["syms"])
    data, nbits, _ = oracle.encode(rows, [1] * n, case["prec"])
    assert nbits == case["L"] and data.hex() == case["bytes"]
    assert oracle.decode(rows, data, nbits, n, case["prec"]) == [1] * n
    targets, ndet, _ = R.py_decode(lo, hi, T, case["prec"], data, nbits)
    assert [R.symbol_of(case, t) for t in targets] == case["syms"]
    if case["L"]:                                          # (no bits: the reference decides only when one arrives)
        assert ndet == n <= case["decoded_count"]          # the bits determine every symbol of the job


# ------------------------------------------------------------------ census of the existing fixtures
def test_census_of_fixtures_that_never_fudge():
    small = R.small_qualifying()
    assert len(small["static"]) >= 90 and len(small["perstep"]) >= 40
    gen = R.gen_qualifying()
    assert [c["name"] for c, _ in gen] == list(R.GEN_NAMES)
    for c, rows in gen:
        assert R.qualifies(rows, c["prec"]), c["name"]
    assert {c["steps"] for c, _ in gen} >= {150, 70}
    # their triples code to the reference's bits on three-entry rows
    for c, rows in [(c, np.array(c["rows"])) for c in small["static"][:10] + small["perstep"][:10]] + gen[:2]:
        n = len(c["syms"])
        lo, hi, T = R.table_triples(rows, c["syms"])
        data, nbits, _ = oracle.encode(R.three_rows(lo, hi, T), [1] * n, c["prec"])
        assert nbits == c["L"] and data.hex() == c["bytes"], c.get("name", c)
