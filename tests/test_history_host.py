"""Host checks of the match-history models (include/lac.h lac_hist_*), no GPU needed.

* The fixtures of tests/golden/history_cases.json (tools/gen_golden_history.py: the reference's
  ``AC(History(V, P, lfunc), prec)``) against the C oracle on the rows of the literal host
  restatement (tests/history.py): this pins the yardstick the GPU tests use -- a history-model job
  IS the pmf job on the rows the ring produces.
* The census of the fixtures: one case mixes fudged with plain rows, one has none.
* lac_amd/csrc/lac_history.h, the plain host rules the kernels share
  (tests/native/history_check.cpp): the incremental rule against the literal loops over
  P in {1, 2, 3, 5, 64, 256} x V in {2, 3, 256}, phases of random, period-3 and constant symbols of
  more than 3 P steps each, with the state set in mid-sequence; the limits and the refusals of
  set_state; the sweep also runs as a stand-alone ASan + UBSan program.
* coder.History and coder.MatchWeights against the restatement, and on the per-token path's
  yardstick with a lambda ``lfunc``.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import history as H
from conftest import REPO, load_golden
from oracle import oracle

NATIVE = os.path.join(REPO, "tests", "native")
SO = os.path.join(NATIVE, "libhistorycheck.so")
SRC = os.path.join(NATIVE, "history_check.cpp")
HDR = os.path.join(REPO, "lac_amd", "csrc", "lac_history.h")
INCS = ["-I", os.path.join(REPO, "lac_amd", "csrc")]

ALL = load_golden("history_cases.json")
CASES = [c for c in ALL if c["lfunc"] is None]                    # tables: the device's family
IDS = [c["name"] for c in CASES]
LAMBDAS = [c for c in ALL if c["lfunc"] is not None]


def weights_of(case):
    if case["lfunc"] is not None:
        return H.table_of(H.LFUNCS[case["lfunc"]], case["V"], case["P"])
    return H.default_weights(case["V"], case["P"]) if case["weights"] == "default" else case["weights"]


def case_rows(case, syms=None, extra_row=False):
    return H.walk(case["V"], case["P"], weights_of(case), case["syms"] if syms is None else syms,
                  case["pmf_bits"], extra_row=extra_row)


# ------------------------------------------------------------------ the fixtures pin the yardstick
def test_fixture_set_covers_the_issue():
    shapes = {(c["V"], c["P"], c["prec"], len(c["syms"])) for c in ALL}
    assert shapes >= {(3, 5, 16, 60), (2, 1, 12, 30), (5, 8, 16, 80), (17, 16, 24, 80), (256, 64, 20, 60),
                      (256, 64, 48, 60), (256, 256, 48, 40)}
    for c in ALL:                                                  # prec 48: bytes, bit count and ring only
        assert (c["decoded"] is None) == (c["prec"] == 48), c["name"]
    assert any(isinstance(c["weights"], list) for c in CASES) and len(LAMBDAS) >= 1
    assert any(c.get("fudged_band") == [0.1, 0.9] for c in CASES) and any(c.get("fudged_band") == [0.0, 0.0] for c in CASES)
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "history_cases.json")) < 64 << 10


def test_census_of_fudged_rows():
    """minp is 1 and 2^(prec-1) < w <= 2^prec: a step surely fudges when T > 2^prec and surely does
    not when T <= 2^(prec-1)."""
    for c in CASES:
        if "fudged_band" not in c:
            continue
        rows, _ = case_rows(c)
        T = rows.sum(axis=1, dtype=np.uint64)
        sure, maybe = float((T > 1 << c["prec"]).mean()), float((T > 1 << (c["prec"] - 1)).mean())
        assert c["fudged_band"][0] <= sure and maybe <= c["fudged_band"][1], (c["name"], sure, maybe)
    assert H.fudged_share(5, 8, H.default_weights(5, 8), 11, [4] * 30) > 0.5


@pytest.mark.parametrize("case", ALL, ids=[c["name"] for c in ALL])
def test_reference_bits_are_the_oracle_on_restated_rows(case):
    rows, st = case_rows(case)
    assert st.ring == case["ring"] and st.pasti == case["pasti"]
    data, nbits, _ = oracle.encode(rows, case["syms"], case["prec"])
    assert nbits == case["L"] and data.hex() == case["bytes"]


@pytest.mark.parametrize("case", [c for c in ALL if c["decoded"] is not None],
                         ids=[c["name"] for c in ALL if c["decoded"] is not None])
def test_reference_decoded_counts_are_the_bitserial_oracle(case):
    data = bytes.fromhex(case["bytes"])
    rows, _ = case_rows(case, case["decoded"], extra_row=True)        # the decoder's own walk, extras included
    assert oracle.decode_bitserial(rows, data, case["L"], case["prec"]) == case["decoded"]
    assert len(case["decoded"]) == case["decoded_count"] >= len(case["syms"])
    assert case["decoded"][:len(case["syms"])] == case["syms"]


@pytest.mark.parametrize("P,V", ((1, 2), (2, 3), (5, 4), (17, 3), (64, 256)))
def test_the_array_form_of_the_restatement_is_its_loops(P, V):
    rng = np.random.default_rng(P)
    st = H.Stream(V, P, H.default_weights(V, P))
    for s in H.draw(rng, V, 3 * P + 5, 3).T.reshape(-1).tolist():
        assert st.runs_np() == list(st.runs())
        assert st.row(fast=True) == st.row(fast=False) and st.row()[0] == 1
        st.accept(s)


# ------------------------------------------------------------------ lac_history.h
def _stale(target, *deps):
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(d) for d in deps)


@pytest.fixture(scope="module")
def hc():
    if _stale(SO, SRC, HDR):
        subprocess.run(["hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", *INCS, SRC, "-o", SO], check=True)
    lib = C.CDLL(SO)
    lib.hc_limits_ok.argtypes = [C.c_int64, C.c_int64]
    lib.hc_weights_ok.argtypes = [C.c_void_p, C.c_int]
    lib.hc_state_ok.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int]
    lib.hc_walk.argtypes = [C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                            C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hc_sweep.argtypes = [C.c_uint64, C.c_void_p]
    return lib


def test_incremental_rule_is_the_literal_rule(hc):
    """Every lag's run at every step: 6 ring lengths x 3 vocabularies x 6 phases of 3 P + 4 steps."""
    steps = C.c_int64(0)
    assert hc.hc_sweep(12345, C.byref(steps)) == 0
    assert steps.value == 3 * 6 * sum(3 * P + 4 for P in (1, 2, 3, 5, 64, 256))


def test_model_limits(hc):
    ok = hc.hc_limits_ok
    assert ok(1, 1) and ok(4096, 256) and ok(2, 256) and ok(4096, 1)
    assert not ok(4097, 1) and not ok(0, 1) and not ok(-1, 4)            # V in [1, 4096]
    assert not ok(4, 0) and not ok(4, 257) and not ok(4, -1) and not ok(4, 1 << 32)   # P in [1, 256]
    w = np.array([0, (1 << 48) - 1, 5, 1 << 48], dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert hc.hc_weights_ok(p(w), 1) and not hc.hc_weights_ok(p(w), 2)
    w[3] = (1 << 64) - 1
    assert not hc.hc_weights_ok(p(w), 2)
    w[3] = 7
    assert hc.hc_weights_ok(p(w), 2)
    # T stays below 2^57: the widest row the limits allow
    assert 4096 + 256 * ((1 << 48) - 1) < 1 << 57


def test_states_set_state_refuses(hc):
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    V, P = 7, 4
    ring = np.array([-1, 0, 6, 3], dtype=np.int32)
    assert hc.hc_state_ok(p(ring), 0, V, P) and hc.hc_state_ok(p(ring), 3, V, P)
    assert not hc.hc_state_ok(p(ring), 4, V, P) and not hc.hc_state_ok(p(ring), -1, V, P)   # pasti in [0, P)
    for bad in (7, -2, 2 ** 31 - 1, -2 ** 31):                           # entries in [-1, V)
        r = ring.copy()
        r[2] = bad
        assert not hc.hc_state_ok(p(r), 1, V, P), bad


def _c_walk(hc, V, P, L, bits, syms, ring=None, pasti=0):
    rg = np.full(P, -1, dtype=np.int32) if ring is None else np.array(ring, dtype=np.int32)
    pi = C.c_int32(pasti)
    w = np.array(L, dtype=np.uint64)
    s = np.array(syms, dtype=np.int32)
    rows = np.zeros((len(s), V), dtype=np.uint64)
    ok, acc = np.zeros(len(s), dtype=np.int32), np.zeros(len(s), dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    hc.hc_walk(V, P, p(w), bits, p(s), len(s), p(rg), C.byref(pi), p(rows), p(ok), p(acc))
    return rows, ok, acc, rg, pi.value


@pytest.mark.parametrize("V,P,bits", ((2, 1, 32), (3, 2, 32), (5, 5, 32), (17, 16, 64), (256, 64, 32), (260, 65, 64)))
def test_row_and_accept_against_the_python_restatement(hc, V, P, bits):
    rng = np.random.default_rng(V * 10 + P)
    L = rng.integers(0, 1000, size=(P, P)).tolist()
    T = 3 * P + 5
    syms = H.draw(rng, V, T, 3).T.reshape(-1)                        # constant, period-3 and random phases
    rows, ok, acc, ring, pasti = _c_walk(hc, V, P, L, bits, syms)
    st = H.Stream(V, P, L)
    for t, s in enumerate(syms):
        assert rows[t].tolist() == st.row() and ok[t] == 1 and acc[t] == 1, t
        st.accept(s)
    assert ring.tolist() == st.ring and pasti == st.pasti
    # continued from a stored state, on both sides of a ring wrap: the same as the unbroken walk
    for k in (P - 1, P, P + 1, 2 * P + 3):
        a = _c_walk(hc, V, P, L, bits, syms[:k])
        b = _c_walk(hc, V, P, L, bits, syms[k:], a[3], a[4])
        assert np.array_equal(b[0], rows[k:]) and b[3].tolist() == st.ring and b[4] == st.pasti, k


def test_bad_rows_and_symbols_stop_the_walk(hc):
    # u32 entries: a constant run's weights at symbol 3 pass 2^32 at the step the restatement predicts
    V, P = 4, 4
    L = [[1 << 30] * P for _ in range(P)]
    syms = [3] * 8
    rows, ok, acc, ring, pasti = _c_walk(hc, V, P, L, 32, syms)
    want, st = H.walk(V, P, L, syms, 32)
    first_bad = int(np.flatnonzero(want.sum(axis=1) == 0)[0])
    assert first_bad == 4 and ok.tolist() == [1] * 4 + [0] * 4 and acc.tolist() == [1] * 4 + [0] * 4
    assert ring.tolist() == st.ring == [3, 3, 3, 3] and pasti == st.pasti == 0
    rows64, ok64, acc64, _, _ = _c_walk(hc, V, P, L, 64, syms)
    assert ok64.all() and acc64.all()
    # a symbol out of range: nothing moves from there on
    _, _, acc, ring, pasti = _c_walk(hc, 5, 3, H.default_weights(5, 3), 32, [0, 1, 5, 2])
    assert acc.tolist() == [1, 1, 0, 0] and ring.tolist() == [0, 1, -1] and pasti == 2


def test_sanitized_sweep_program():
    """The same sweep as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer
    (host code only; every buffer a heap block of exactly the model's size)."""
    outdir = os.path.join(NATIVE, "_asan")
    os.makedirs(outdir, exist_ok=True)
    exe = os.path.join(outdir, "history_check_main")
    if _stale(exe, SRC, HDR):
        # host code only: the sanitizers are given to the host compilation alone
        subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-DHISTORY_CHECK_MAIN",
                        "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", *INCS, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    report = r.stdout + r.stderr
    assert r.returncode == 0, report[-3000:]
    assert "history_check: ok" in report and "ERROR" not in report and "runtime error" not in report


# ------------------------------------------------------------------ coder.History on the host
def _host_bits(predictor, prec, syms):
    """The host restatement's coder over a predictor's own rows: the per-token path's yardstick."""
    rows = []
    for s in syms:
        cdf = list(predictor.calc_dist())
        rows.append([cdf[0]] + [cdf[k] - cdf[k - 1] for k in range(1, len(cdf))])
        predictor.accept(s)
    return oracle.encode(np.array(rows, dtype=np.uint64), syms, prec)


@pytest.mark.parametrize("case", LAMBDAS, ids=[c["name"] for c in LAMBDAS])
def test_history_class_with_a_lambda_lfunc(case):
    from lac_amd.coder import History
    p = History(case["V"], case["P"], H.LFUNCS[case["lfunc"]])
    data, nbits, _ = _host_bits(p, case["prec"], case["syms"])
    assert nbits == case["L"] and data.hex() == case["bytes"]
    assert p.past == case["ring"] and p.pasti == case["pasti"] and isinstance(p.past, list)


def test_history_class_is_the_issues_model():
    from lac_amd.coder import History, MatchWeights, _history_model
    case = next(c for c in CASES if c["name"] == "v5_p8_p16")
    V, P = case["V"], case["P"]
    p = History(V, P)                                               # lfunc=None: n r^3 + 1
    assert isinstance(p.lfunc, MatchWeights) and [list(r) for r in p.lfunc.table] == H.default_weights(V, P)
    assert p.lfunc(3, 2, V, P) == V * 27 + 1 and p.n == V and p.pasti == 0 and p.past == [-1] * P
    st = H.Stream(V, P, H.default_weights(V, P))
    q = p.copy()
    for s in case["syms"]:
        assert list(p.runs()) == list(st.runs())
        assert p.dist == list(np.cumsum(st.row())) and p.dist[0] == 1
        p.accept(s)
        st.accept(s)
    assert p.past == st.ring == case["ring"] and p.pasti == st.pasti == case["pasti"]
    assert q.past == [-1] * P and q.pasti == 0 and q.lfunc is p.lfunc and type(q) is History   # the copy did not move
    r = p.copy()
    assert r.past == p.past and r.past is not p.past and r.pasti == p.pasti
    # what the device path takes, and what keeps the per-token path
    m = _history_model(p)
    assert m is not None and m[:2] == (V, P) and m[2] is p.lfunc
    assert _history_model(History(V, P, lambda r, i, n, k: 1)) is None              # a callable without its table
    assert _history_model(History(V, P, MatchWeights([[1 << 48] * P] * P))) is None  # a weight >= 2^48
    assert _history_model(History(V, 257)) is None and _history_model(History(4097, 4)) is None
    assert _history_model(History(V, P, MatchWeights([[1] * (P - 1)] * P))) is None   # a table too small

    class Sub(History):
        def runs(self):
            return super().runs()

    class Minp(History):
        minp = 1

    assert _history_model(Sub(V, P)) is None and _history_model(Minp(V, P)) is None
    bad = History(V, P)
    bad.past[1] = V
    assert _history_model(bad) is None                                              # a ring entry outside [-1, V)
