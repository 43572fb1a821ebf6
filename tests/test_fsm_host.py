"""Host checks of the finite-state models (include/lac.h lac_fsm_*), no GPU needed.

* The fixtures of tests/golden/nfa_cases.json (tools/gen_golden_nfa.py: the reference's
  ``AC(NFA(...), prec)``) against the C oracle on the gathered rows pmf[q_t]: this pins the
  yardstick the GPU tests use -- a finite-state job IS the pmf job on its gathered tables.
* lac_amd/csrc/lac_fsm.h, the plain host rules the kernels share (tests/native/fsm_check.cpp):
  model limits, prepared-layout offsets, and the prepared row's O(1) {lo, hi, T, ceil(T / minp)}
  and search against a plain scan of 1 000 random rows, totals at 2^32 - 1, 2^50 +- 1, near 2^60 and
  in [2^63, 2^64) among them, and of sparse rows -- at most 8 positive entries at chunk and vector
  bounds, zero runs of whole chunks -- searched at every c_i - 1, c_i and T - 1; the sweep also
  runs as a stand-alone ASan + UBSan program.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO, load_golden
from oracle import oracle

NATIVE = os.path.join(REPO, "tests", "native")
SO = os.path.join(NATIVE, "libfsmcheck.so")
SRC = os.path.join(NATIVE, "fsm_check.cpp")
HDR = os.path.join(REPO, "lac_amd", "csrc", "lac_fsm.h")
INCS = ["-I", os.path.join(REPO, "lac_amd", "csrc")]

CASES = load_golden("nfa_cases.json")
IDS = [c["name"] for c in CASES]


def next_table(case):
    if case["next"] == "symbol":                                  # an order-1 model: the state is the last symbol
        return np.tile(np.arange(case["V"], dtype=np.int32), (case["K"], 1))
    return np.array(case["next"], dtype=np.int32)


def state_walk(case, syms=None, state=None):
    """q_0 .. q_n for the symbols: the host walk of ``next``."""
    nxt = next_table(case)
    q = [case["state"] if state is None else state]
    for s in (case["syms"] if syms is None else syms):
        q.append(int(nxt[q[-1], s]))
    return q


def gathered_rows(case, states):
    dt = np.uint32 if case["pmf_bits"] == 32 else np.uint64
    return np.array(case["tables"], dtype=dt)[np.asarray(states, dtype=np.int64)]


# ------------------------------------------------------------------ the fixtures pin the yardstick
def test_fixture_set_covers_the_issue():
    assert len(CASES) >= 12
    assert {c["prec"] for c in CASES} >= {16, 24, 48}
    assert min(c["V"] for c in CASES) == 2 and max(c["V"] for c in CASES) == 256
    assert min(c["K"] for c in CASES) == 1 and max(c["K"] for c in CASES) == 256
    assert any(c["K"] == 256 and c["V"] == 256 and c["next"] == "symbol" for c in CASES)

    def fudged_share(c):
        w, q = 1 << (c["prec"] - 1), state_walk(c)[:-1]           # the narrowest width a coder has: > 2^(prec-1)
        f = [sum(c["tables"][s]) > 2 * w * min(p for p in c["tables"][s] if p) for s in q]
        return sum(f) / len(f)
    shares = {c["name"]: fudged_share(c) for c in CASES if c["prec"] == 16}
    assert sum(1 for v in shares.values() if v > 0.5) >= 2, shares          # rows that fudge at every width
    assert any(0.1 < v < 0.9 for v in shares.values()), shares              # fudging and plain rows mixed


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_bits_are_the_oracle_on_gathered_rows(case):
    q = state_walk(case)
    assert q[-1] == case["end_state"]
    data, nbits, _ = oracle.encode(gathered_rows(case, q[:-1]), case["syms"], case["prec"])
    assert nbits == case["L"] and data.hex() == case["bytes"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_decoded_counts_are_the_bitserial_oracle(case):
    data = bytes.fromhex(case["bytes"])
    q = state_walk(case, case["decoded"])                             # the decoder's own walk, extras included
    rows = gathered_rows(case, q)                                     # (one row past the last symbol: the step that stops)
    assert oracle.decode_bitserial(rows, data, case["L"], case["prec"]) == case["decoded"]
    assert len(case["decoded"]) == case["decoded_count"] >= len(case["syms"])
    pre = oracle.decode_bitserial(rows, data, case["prefix_bits"], case["prec"])
    assert pre == case["decoded"][:case["prefix_decoded_count"]]


# ------------------------------------------------------------------ lac_fsm.h
def _stale(target, *deps):
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(d) for d in deps)


@pytest.fixture(scope="module")
def fc():
    if _stale(SO, SRC, HDR):
        subprocess.run(["hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", *INCS, SRC, "-o", SO], check=True)
    lib = C.CDLL(SO)
    lib.fc_limits_ok.argtypes = [C.c_int64, C.c_int64]
    lib.fc_layout.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p]
    lib.fc_sweep.argtypes = [C.c_int, C.c_uint64]
    return lib


def test_model_limits(fc):
    ok = fc.fc_limits_ok
    assert ok(1, 1) and ok(65536, 256) and ok(256, 65536) and ok(1 << 24, 1)       # an order-2 byte model fits
    assert not ok(65537, 256) and not ok(257, 65536) and not ok((1 << 24) + 1, 1)  # K * V > 2^24
    assert ok(1, 65536) and not ok(1, 65537)                                       # V > 65536
    assert not ok(0, 4) and not ok(4, 0) and not ok(-1, 4)
    assert not ok(1 << 62, 1 << 10)                                                # (no overflow of K * V)


def _layout(fc, K, V, bits, has_next):
    out = np.zeros(11, dtype=np.uint64)
    fc.fc_layout(K, V, bits, int(has_next), out.ctypes.data_as(C.c_void_p))
    names = ("Vp", "nvec", "long", "G", "meta", "cdf", "pmf", "bounds", "next", "bytes", "meta_size")
    return dict(zip(names, (int(v) for v in out)))


@pytest.mark.parametrize("bits", (32, 64))
def test_prepared_layout(fc, bits):
    vec, esize = 128 // bits, bits // 8
    for K, V in ((1, 1), (3, 5), (256, 256), (2, 260), (7, 64 * vec), (7, 64 * vec + 1), (2, 65536), (65536, 256)):
        for has_next in (False, True):
            y = _layout(fc, K, V, bits, has_next)
            assert y["meta_size"] == 32
            assert y["Vp"] == -(-V // vec) * vec and y["nvec"] == y["Vp"] // vec     # rows padded to 16 B
            assert y["long"] == (y["nvec"] > 64) and y["G"] == -(-y["nvec"] // 64)  # one round of 64 vectors, or chunks
            # the sections in order, 256-B aligned, none overlapping the next
            sizes = (("meta", 32 * K), ("cdf", K * y["Vp"] * esize), ("pmf", K * y["Vp"] * esize),
                     ("bounds", K * 64 * esize if y["long"] else 0), ("next", 4 * K * V if has_next else 0))
            end = 0
            for name, size in sizes:
                assert y[name] % 256 == 0 and y[name] >= end, (K, V, name)
                end = y[name] + size
            assert y["bytes"] >= end and y["bytes"] - end < 256
    assert _layout(fc, 1 << 16, 256, 32, True)["bytes"] < 200 << 20                 # an order-2 byte model: < 200 MiB


def test_prepared_rows_against_a_plain_scan(fc):
    assert fc.fc_sweep(1000, 12345) == 0


def test_sanitized_sweep_program():
    """The same sweep as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer
    (host code only; every buffer a heap block of exactly the layout's size)."""
    outdir = os.path.join(NATIVE, "_asan")
    os.makedirs(outdir, exist_ok=True)
    exe = os.path.join(outdir, "fsm_check_main")
    if _stale(exe, SRC, HDR):
        # host code only: the sanitizers are given to the host compilation alone
        subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-DFSM_CHECK_MAIN",
                        "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", *INCS, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    report = r.stdout + r.stderr
    assert r.returncode == 0, report[-3000:]
    assert "fsm_check: ok" in report and "ERROR" not in report and "runtime error" not in report
