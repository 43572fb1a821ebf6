"""The device arithmetic tests' inputs, checked without a GPU: tests/native/dev_arith.hip
cross-compiles for gfx950 with the product's flags, every generated case (tests/dev_arith.py) meets
its primitive's documented precondition, every class of input is present for every primitive, and
the same cases give exact results through the host build of the same headers
(tests/native/core_check.cpp) with the exact reciprocal.  tests/test_gpu_arith.py runs them on the
device, with the device's own reciprocals and the divisors at which those are furthest off in place
of the seeded stand-ins used here."""
import ctypes as C
import os
import subprocess

import pytest

import dev_arith as da
from conftest import REPO

SO = os.path.join(REPO, "tests", "native", "libcorecheck.so")
SRC = os.path.join(REPO, "tests", "native", "core_check.cpp")
U = C.c_uint64


@pytest.fixture(scope="module")
def core():
    deps = [SRC] + [os.path.join(REPO, "lac_amd", "csrc", h) for h in ("lac_core.h", "lac_hc.h")] + [
        os.path.join(REPO, "include", "lac.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(REPO, "lac_amd", "csrc"),
                        "-I", os.path.join(REPO, "include"), SRC, "-o", SO], check=True)
    lib = C.CDLL(SO)
    for name, args in (("cc_div_floor", [U, U, U]), ("cc_div_floor_inv", [U, U, U]),
                       ("cc_div_small", [U, U, U, U, C.c_double]), ("cc_div_small_mask", [U, U, U, U, C.c_double]),
                       ("cc_div_mid", [U, U, U, U]), ("cc_div_mid_w", [U, U, U, C.c_double, U]),
                       ("cc_div_near", [U, U, U, U, C.c_int, C.c_int]), ("cc_frac_mul_div", [U, U, U, C.c_int]),
                       ("cc_frac_mul_div_uni", [U, U, U, C.c_int]), ("cc_frac_mul_div32", [U, U, U, C.c_int]),
                       ("cc_cr_ratio", [U, U])):
        getattr(lib, name).restype = U
        getattr(lib, name).argtypes = args
    return lib


def test_harness_cross_compiles_with_the_products_flags():
    from lac_amd import build as lbuild
    cmd = da.compile_command()
    assert all(f in cmd for f in lbuild.FLAGS) and "--offload-arch=gfx950" in " ".join(cmd)
    assert os.path.exists(da.build(force=True))


def test_sweep_divisors_cover_each_length():
    for L in da.SWEEP_L + (64,):
        d = da.sweep_divisors(L, n_even=1 << 12, n_rand=1 << 10)
        lo, hi = 1 << (L - 1), 1 << L
        assert int(d.min()) == lo and int(d.max()) == hi - 1 and len(d) >= min(hi - lo, 1 << 12)
        assert set(range(lo, min(hi, lo + 1024))) <= set(d.tolist()) and set(range(max(lo, hi - 1024), hi)) <= set(d.tolist())
    # tools/rcp_probe.hip's mix
    assert int(da.splitmix(da.u64([0]))[0]) == 0xE220A8397B1DCDAF


@pytest.mark.parametrize("form", list(da.FORMS))
def test_decoder_cases_meet_their_preconditions(core, form):
    """Census and documented bounds of one form's cases (quotient at most 2^50 -- reached: c = T at
    w = 2^50 --, operand sizes, add < d), and the host build exact on all of them."""
    cs = da.decoder_cases(form)
    census = cs.census()
    assert len(cs) >= 200000 and set(da.CLASSES[form]) <= set(census), set(da.CLASSES[form]) - set(census)
    assert all(census[c] >= 100 for c in da.CLASSES[form]), census
    assert da.check_decoder_preconditions(form, cs) == 1 << 50
    shapes = set(cs.shape)
    assert shapes == ({"range"} if form == "mid" else {"range", "target"})
    for (n, m, add, d, addd), shape in zip(cs.rows, cs.shape):
        q = (n * m + add) // d
        if form == "small":
            assert core.cc_div_small(n, m, add, d, 0.0) == q and core.cc_div_small_mask(n, m, add, d, 0.0) == q, (n, m, add, d)
        elif form == "mid":
            assert core.cc_div_mid(n, m, add, d) == q, (n, m, add, d)
            assert core.cc_div_mid_w(n, m, add, float(d) if addd else 0.0, d) == q, (n, m, add, d)
        else:
            assert core.cc_div_near(n, m, add, d, 0, int(form == "near32" and shape == "range")) == q, (n, m, add, d)


def test_general_division_cases(core):
    cs = da.floor_cases()
    census = cs.census()
    assert len(cs) >= 200000 and all(census.get(c, 0) >= 100 for c in da.CLASSES["floor"]), census
    top = 0
    for nh, nl, d in cs.rows:
        N = (nh << 64) | nl
        q = N // d
        assert d > 0 and q < 1 << 64
        top = max(top, q)
        assert core.cc_div_floor(nh, nl, d) == q and core.cc_div_floor_inv(nh, nl, d) == q, (N, d)
    assert top == (1 << 64) - 1
    rs = da.range_cases()
    census = rs.census()
    assert len(rs) >= 150000 and all(census.get(c, 0) >= 100 for c in da.CLASSES["ranges"]), census
    for lo, hi, T, w in rs.rows:
        assert 0 <= lo <= hi <= T < 1 << 64 and 2 < w <= 1 << 61
    assert {(1 << 50) + 1, 1 << 51} <= {r[3] for r in rs.rows}                 # prec 51: past the small forms
    assert {1 << 50, 1 << 32} <= {r[2] for r in rs.rows}


def test_row_fraction_cases(core):
    cs = da.frac_cases()
    census = cs.census()
    assert len(cs) >= 200000 and all(census.get(c, 0) >= 100 for c in da.CLASSES["frac"]), census
    seen_top = False
    for c, w, T, ceil in cs.rows:
        assert 0 <= c <= T < 1 << 64 and T > 0 and 2 < w <= 1 << 61 and ceil in (0, 1)
        f, q, qu, q32 = da.frac_want(c, w, T, ceil)
        seen_top |= f == 1 << 63
        assert core.cc_frac_mul_div(c, w, T, ceil) == q, (c, w, T, ceil)
        assert core.cc_frac_mul_div_uni(c, w, T, ceil) == qu, (c, w, T, ceil)
        assert core.cc_frac_mul_div32(c, w, T, ceil) == q32, (c, w, T, ceil)
    assert seen_top
    Ts = {r[2] for r in cs.rows}
    assert {(1 << 62) - 1, 1 << 62, (1 << 63) - 1, 1 << 63, (1 << 32) - 1, 1 << 32} <= Ts


def test_fudge_and_ratio_cases(core):
    cs = da.fudge_cases()
    census = cs.census()
    assert len(cs) >= 100000 and all(census.get(c, 0) >= 100 for c in da.CLASSES["fudge"]), census
    for i, c, j, T, w, V, minp in cs.rows:
        prec = (w - 1).bit_length()
        assert 0 <= c <= T < 1 << 64 and 2 <= V <= 1 << (prec - 1) and 0 <= i < V and 0 <= j < V and minp >= 1
        assert (1 << (prec - 1)) < w <= (1 << prec) and prec <= 61
    rs = da.ratio_cases()
    census = rs.census()
    assert len(rs) >= 100000 and all(census.get(c, 0) >= 100 for c in da.CLASSES["ratio"]), census
    for a, b in rs.rows:
        assert 0 <= a <= b and 0 < b < 1 << 63
        assert core.cc_cr_ratio(a, b) == da.f64_bits(a / b), (a, b)
