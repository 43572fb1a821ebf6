"""Shared by test_topk_host.py and test_gpu_topk.py: the yardstick of lac_topk_logits -- Python
integers on the C oracle's q1 tables -- the native library of lac_amd/csrc/lac_topk.h
(tests/native/topk_check.cpp), and the rows both tests use: random rows, rows built to tie, and rows
whose tie class straddles a seam of the kernels' layout."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import REPO
from oracle import oracle

NATIVE = os.path.join(REPO, "tests", "native")
SO = os.path.join(NATIVE, "libtopkcheck.so")
SRC = os.path.join(NATIVE, "topk_check.cpp")
HDRS = [os.path.join(REPO, "lac_amd", "csrc", "lac_topk.h"), os.path.join(REPO, "include", "lac.h"),
        os.path.join(REPO, "include", "lac_q1_table.h")]
INCS = ["-I", os.path.join(REPO, "lac_amd", "csrc"), "-I", os.path.join(REPO, "include")]
U64, I64, U32 = C.c_uint64, C.c_int64, C.c_uint32
BF16, F32 = 1, 2                                              # LAC_LOGITS_*
FORM_AUTO, FORM_REGS, FORM_STREAM = 0, 1, 2
TIE_A, TIE_B, LOW = -15.8, -16.1, -16.9                       # nats below a maximum of 0: two levels of the
                                                              # class TAB = 2 (exact in bf16), and the class TAB = 1


def stale(target, *deps):
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(d) for d in deps)


_lib = None


def native():
    global _lib
    if _lib is None:
        if stale(SO, SRC, *HDRS):
            subprocess.run(["hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", *INCS, SRC, "-o", SO], check=True)
        lib = C.CDLL(SO)
        vp = C.c_void_p
        lib.tk_args_ok.argtypes = [U64, C.c_int, I64, I64, I64, I64, I64, I64, U64, U64]
        lib.tk_plan.argtypes = [I64, C.c_int, C.c_int, vp]
        lib.tk_seams.argtypes = [I64, C.c_int, C.c_int, vp]
        lib.tk_class.argtypes = [C.c_int, vp, vp]
        lib.tk_level.argtypes = [C.c_float, C.c_float]
        lib.tk_level.restype = U32
        lib.tk_threshold.argtypes = [C.c_int, vp, C.c_int, vp]
        lib.tk_row.argtypes = [C.c_int, vp, C.c_int, I64, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
        lib.tk_sweep.argtypes = [U64, vp]
        _lib = lib
    return _lib


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def plan(V, type_bytes, forced=FORM_AUTO):
    """-> (rc, form, R, threads, tiles)"""
    out = np.zeros(4, dtype=np.int32)
    rc = native().tk_plan(V, type_bytes, forced, ptr(out))
    return (rc, *out.tolist())


def seams(V, type_bytes, forced):
    """the first symbol after a thread, register-round, wave and tile seam (those inside the row)"""
    out = np.zeros(4, dtype=np.int64)
    assert native().tk_seams(V, type_bytes, forced, ptr(out)) == 0
    return sorted({int(s) for s in out if 0 < s < V})


# ------------------------------------------------------------------ rows
def as_type(x, type_bytes):
    """float rows -> the bytes a call reads: uint16 bit patterns of bf16 (round to nearest even;
    NaN and the infinities survive) or float32"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if type_bytes == 4:
        return x
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r)


def random_rows(rng, n, V, spread=30.0):
    top = rng.integers(-20, 21, size=(n, 1)).astype(np.float32)
    return top - spread * rng.random((n, V), dtype=np.float32)


def special_rows(rng, V, k):
    """Rows built to tie, by name"""
    out = {}
    out["flat"] = np.full(V, 3.25, dtype=np.float32)
    out["all_neg_inf"] = np.full(V, -np.inf, dtype=np.float32)
    x = random_rows(rng, 1, V)[0]
    x[rng.integers(0, V)] = np.inf
    out["pos_inf"] = x
    x = random_rows(rng, 1, V)[0]
    x[rng.integers(0, V, size=max(1, V // 7))] = np.nan
    x[rng.integers(0, V, size=max(1, V // 9))] = -np.inf
    out["nan_and_neg_inf"] = x
    out["all_nan"] = np.full(V, np.nan, dtype=np.float32)
    # the threshold inside a multi-level tie class: everything 13.3 .. 17 nats below one maximum
    x = (-13.3 - 3.7 * rng.random(V)).astype(np.float32)
    x[rng.integers(0, V)] = 0.0
    out["deep_classes"] = x
    # more than k ties at the maximum
    x = random_rows(rng, 1, V, 12.0)[0]
    x[rng.permutation(V)[:min(V, k + 1 + V // 3)]] = x.max()
    out["ties_at_max"] = x
    return out


def seam_rows(V, seam, k_max=256):
    """Rows whose tie class (TAB = 2, two of its levels) has members on both sides of `seam`, with a
    few heavier entries, everything else one class lower: -> [(row, k)] with k chosen so the cut --
    the last tie taken -- is the tie just before the seam, the one before that, and the first after."""
    ties = sorted({s for s in (1, seam - 9, seam - 2, seam - 1, seam, seam + 1, seam + 8, V - 1) if 0 <= s < V})
    heavy = sorted({s for s in (0, seam - 3, seam + 2) if 0 <= s < V and s not in ties})
    row = np.full(V, LOW, dtype=np.float32)
    for n, s in enumerate(ties):
        row[s] = TIE_A if n % 2 else TIE_B
    row[heavy] = -1.0
    row[heavy[0]] = 0.0
    below = sum(1 for s in ties if s < seam)
    return [(row, len(heavy) + r) for r in (below - 1, below, below + 1)
            if 1 <= r <= len(ties) and len(heavy) + r <= min(V, k_max)]


def last_vector_row(V, type_bytes, k):
    """Survivors only in the row's last 16 bytes"""
    n = 16 // type_bytes
    row = np.full(V, LOW, dtype=np.float32)
    row[V - n:] = np.linspace(-3.0, 0.0, n, dtype=np.float32)
    return row, min(k, n)


# ------------------------------------------------------------------ the yardstick
def yardstick(rows, k, weight_bits, K):
    """rows [..., V] (uint16 bf16 bit patterns or float32) -> (idx int32 [..., K], wt uint32 [..., K]):
    Python integers on oracle.q1_quantize(row, 61): lexsort by (-g, symbol), take k, sort by symbol,
    shift; pads idx -1, wt 0."""
    g = oracle.q1_quantize(rows, 61).astype(np.int64)
    V = g.shape[-1]
    flat = g.reshape(-1, V)
    idx = np.full((flat.shape[0], K), -1, dtype=np.int32)
    wt = np.zeros((flat.shape[0], K), dtype=np.uint32)
    sym = np.arange(V)
    for i, row in enumerate(flat):
        keep = np.sort(np.lexsort((sym, -row))[:k])
        idx[i, :k] = keep
        wt[i, :k] = [int(row[s]) >> (24 - weight_bits) for s in keep]
    return idx.reshape(*g.shape[:-1], K), wt.reshape(*g.shape[:-1], K)


def native_row(which, row, k, weight_bits, K, forced=FORM_AUTO, fill=-7):
    row = np.ascontiguousarray(row)
    tb = row.dtype.itemsize
    idx, wt = np.full(K, fill, dtype=np.int32), np.full(K, 0xDEADBEEF, dtype=np.uint32)
    rc = native().tk_row(which, ptr(row), tb, row.shape[-1], k, weight_bits, K, forced, ptr(idx), ptr(wt))
    assert rc == 0, rc
    return idx, wt
