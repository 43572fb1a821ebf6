"""Host check of q1_step_plan (lac_amd/csrc/lac_select.h): when the one-position logits calls
(lac_decode_logits_step / lac_encode_logits_step) take the fused one-launch step, and in which
block shape.

Compiles tests/native/step_select_check.cpp (plain C++ over the header, nothing else linked);
no GPU needed.
"""
import ctypes as C
import os
import subprocess

import pytest

from conftest import REPO

SO = os.path.join(REPO, "tests", "native", "libstepselectcheck.so")
SRC = os.path.join(REPO, "tests", "native", "step_select_check.cpp")

LAC_OK, LAC_E_ARG = 0, -1
AUTO, FUSED, SPLIT = 0, 1, 2
CUS = 256


@pytest.fixture(scope="module")
def sel():
    hdr = os.path.join(REPO, "lac_amd", "csrc", "lac_select.h")
    deps = [SRC, hdr, os.path.join(REPO, "include", "lac.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(REPO, "lac_amd", "csrc"),
                        "-I", os.path.join(REPO, "include"), SRC, "-o", SO], check=True)
    lib = C.CDLL(SO)
    i64p = C.POINTER(C.c_int64)
    lib.ssc_step_plan.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_int, i64p]
    lib.ssc_step_plan.restype = None
    lib.ssc_consts.argtypes = [i64p]
    lib.ssc_consts.restype = None
    k = (C.c_int64 * 4)()
    lib.ssc_consts(k)
    lib.max_vec, lib.max_streams, lib.max_threads, lib.max_r = (int(v) for v in k)
    return lib


def plan(sel, V, bf16, streams, mode=AUTO, cus=CUS):
    """(fused, rc, threads, R)"""
    o = (C.c_int64 * 4)()
    sel.ssc_step_plan(cus, V, 2 if bf16 else 4, streams, mode, o)
    return tuple(int(v) for v in o)


def test_capacity_constants(sel):
    assert sel.max_vec >= 16384 and sel.max_vec == sel.max_threads * sel.max_r
    assert sel.max_threads == 1024 and sel.max_threads % 64 == 0
    assert 1 <= sel.max_streams <= CUS


def test_serving_shape_is_fused(sel):
    assert plan(sel, 32000, True, 1) == (1, LAC_OK, 1024, 4)            # 4000 vectors over 16 waves
    assert plan(sel, 32000, False, 1) == (1, LAC_OK, 1024, 8)           # 8000 vectors
    assert plan(sel, 128256, True, 1) == (1, LAC_OK, 1024, 16)          # 16032 vectors
    assert plan(sel, 24, False, 1) == (1, LAC_OK, 64, 4)                # 6 vectors: one wave
    assert plan(sel, 1000, True, 1) == (1, LAC_OK, 64, 4)               # 125 vectors: 32 threads' worth


def test_stream_cap(sel):
    cap = sel.max_streams
    assert plan(sel, 32000, True, cap)[:2] == (1, LAC_OK)
    assert plan(sel, 32000, True, cap, FUSED)[:2] == (1, LAC_OK)
    assert plan(sel, 32000, True, cap + 1) == (0, LAC_OK, 0, 0)
    assert plan(sel, 32000, True, cap + 1, FUSED) == (0, LAC_E_ARG, 0, 0)
    # never more workgroups than compute units, whatever the constant
    small = max(1, cap // 2)
    assert plan(sel, 32000, True, small, cus=small)[0] == 1
    assert plan(sel, 32000, True, small + 1, cus=small)[0] == 0


@pytest.mark.parametrize("bf16", [True, False])
def test_row_cap(sel, bf16):
    n = 8 if bf16 else 4
    assert plan(sel, sel.max_vec * n, bf16, 1)[:2] == (1, LAC_OK)
    assert plan(sel, (sel.max_vec + 1) * n, bf16, 1) == (0, LAC_OK, 0, 0)
    assert plan(sel, (sel.max_vec + 1) * n, bf16, 1, FUSED) == (0, LAC_E_ARG, 0, 0)


def test_f32_65536_is_the_cap(sel):
    assert sel.max_vec == 16384
    assert plan(sel, 65536, False, 1) == (1, LAC_OK, 1024, 16)
    assert plan(sel, 65540, False, 1) == (0, LAC_OK, 0, 0)
    assert plan(sel, 131072, True, 1) == (1, LAC_OK, 1024, 16)
    assert plan(sel, 131080, True, 1) == (0, LAC_OK, 0, 0)
    assert plan(sel, 151936, True, 1, FUSED) == (0, LAC_E_ARG, 0, 0)


def test_modes(sel):
    for V, bf16, streams in ((32000, True, 1), (24, False, 3), (65540, False, 1), (32000, True, 100000)):
        assert plan(sel, V, bf16, streams, SPLIT) == (0, LAC_OK, 0, 0)   # mode 2: never fused, never refused
        fused, rc, _, _ = plan(sel, V, bf16, streams, FUSED)             # mode 1: fused or the refusal
        assert (fused, rc) in ((1, LAC_OK), (0, LAC_E_ARG))
        assert fused == plan(sel, V, bf16, streams, AUTO)[0]
        assert plan(sel, V, bf16, streams, AUTO)[1] == LAC_OK            # auto never refuses


@pytest.mark.parametrize("bf16", [True, False])
def test_every_fused_plan_holds_its_row(sel, bf16):
    n = 8 if bf16 else 4
    vecs = set(range(1, sel.max_vec + 200, 37)) | {1, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, sel.max_vec - 1,
                                                  sel.max_vec, sel.max_vec + 1}
    for nvec in sorted(vecs):
        fused, rc, threads, r = plan(sel, nvec * n, bf16, 1)
        assert rc == LAC_OK and fused == int(nvec <= sel.max_vec), nvec
        if not fused:
            continue
        assert r in (4, 8, 16) and 64 <= threads <= sel.max_threads and threads % 64 == 0, (nvec, threads, r)
        assert threads * r >= nvec, (nvec, threads, r)
        # no idle wave: the last wave's first vector lies in the row
        assert (threads // 64 - 1) * 64 * r < nvec, (nvec, threads, r)
        # the fewest vectors per thread whose full block holds the row
        assert r == 4 or nvec > sel.max_threads * (r // 2), (nvec, r)
