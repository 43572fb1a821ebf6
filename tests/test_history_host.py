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
* The jobs of tests/test_gpu_history_limits.py (builders in tests/history.py): each reaches, on
  the restatement and the C oracle, what it is built to reach -- the weight limit and its totals,
  the shares of fudged steps, totals next to 2^50, u32 entries of 2^32 - 1 and 2^32, weights that
  tell the lags on two sides of a lane seam apart, every seam position of the decoder's search
  coded, and probes that sit exactly on a symbol's range bounds.
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


# ------------------------------------------------------------------ the jobs of test_gpu_history_limits.py
# Each job reaches, on the host restatement and the C oracle, what it is built to reach.
WIDE_SHAPES = ((300, 4), (300, 256), (4096, 65))
WIDE_PRECS = (61, 57, 50, 48, 16)
SEAM_P = (127, 128, 129, 191, 192, 193, 255)
STEER_V = {32: (255, 256, 513, 4093, 4096), 64: (127, 128, 257, 4096)}
PROBES = ((32, 513, 48), (32, 513, 16), (64, 257, 60), (64, 257, 16))   # (entry bits, V, prec): prec 16 fudges


def test_wide_weights_are_the_issues_table():
    for P in (4, 65, 256):
        L = H.wide_weights(P)
        assert all(L[i][P - i - 1] == H.W48 for i in range(P)) and max(map(max, L)) == H.W48
        assert {0, 1, (1 << 32) - 1, 1 << 32} <= {x for r in L for x in r}
        pick = lambda i, r: (0, 1, (1 << 32) - 1, 1 << 32, (1 << 47) + i, H.W48 - r)[(7 * i + 3 * r) % 6]  # noqa: E731
        assert all(L[i][r] == pick(i, r) for i in range(P) for r in range(P) if r != P - i - 1)


@pytest.mark.parametrize("V,P", WIDE_SHAPES)
def test_wide_jobs_code_cleanly_and_reach_the_weight_limit(V, P):
    _, _, L, bits, sym, rows, _ = H.job("wide", V, P)
    assert sym.shape == (2 * P + 9, 5) and bits == 64
    for prec in WIDE_PRECS + (51,):
        assert not H.job_verdict(prec, "wide", V, P)["code"].any(), prec
    tot = H.totals(rows)
    assert int(tot.max()) == V + P * H.W48                          # the constant streams reach the documented maximum
    if (V, P) == (300, 256):
        assert int(tot.max()) == (1 << 56) + 44


def test_wide_job_fudge_classes():
    tot = H.totals(H.job("wide", 300, 256)[5])
    always, some, never = H.fudge_classes(tot, 61)
    assert never == 1.0
    always, some, never = H.fudge_classes(tot, 57)                  # measured: 0 / 10.3 % / 89.7 %
    assert always == 0 and some >= 0.05
    for prec in (48, 16):                                           # measured at 48: 79.2 % / 0.2 % / 20.6 %
        always, some, never = H.fudge_classes(tot, prec)
        assert always >= 0.5 and never >= 0.1, prec


def test_wide_job_totals_near_2_50():
    """(300, 4): at prec 50 a total <= 2^49 never fudges and takes the decoder's small division
    form with a large T; prec 51 takes the general form on the same rows.  Measured: 24 and 13 of
    85 steps."""
    tot = [int(x) for x in H.totals(H.job("wide", 300, 4)[5]).reshape(-1)]
    assert len(tot) == 85
    assert sum((1 << 47) <= x <= (1 << 49) for x in tot) >= 10
    assert sum((1 << 49) < x < (1 << 50) for x in tot) >= 10


def test_u32_edge_job_sits_on_the_last_entry_that_fits():
    V, P, L, _, sym, rows, sts = H.job("edge32", 32, 0, 64, 128)
    r64 = H.job("edge32", 64, 0, 64, 128)[5]
    top = r64.max(axis=2)
    assert [int(top[t, 0]) for t in (63, 64, 65, 128, 129)] == [1 << 31, 1 << 31, (1 << 32) - 1, (1 << 32) - 1, 1 << 32]
    assert (top[65:129, 0] == (1 << 32) - 1).all() and not rows[129:, 0].any() and rows[128, 0].any()
    coded = r64[np.arange(140), 1, sym[:, 1]]
    assert int((coded == (1 << 32) - 1).sum()) == 35 and int(top[:, 1].max()) == (1 << 32) - 1
    for prec in (48, 16):
        v = H.job_verdict(prec, "edge32", 32, 0, 64, 128)
        assert v["code"].tolist() == [-5, 0, -5, 0] and v["step"].tolist() == [129, -1, 129, -1]    # LAC_E_TABLE
        assert not H.job_verdict(prec, "edge32_clean", 64, 0, 64, 128)["code"].any()
    assert sts[0].pasti == sts[2].pasti == 129 and sts[0].ring == [5] * 129 + [-1] * 63
    # the same entries from the lags of three lanes
    rows2 = H.job("edge32_lanes", 32)[5]
    v = H.job_verdict(48, "edge32_lanes", 32)
    assert v["code"].tolist() == [-5, 0] and v["step"].tolist() == [3, -1]
    assert [int(rows2[t, 0].max()) for t in range(4)] == [1, 1 << 31, (1 << 32) - 1, 0]


def _bytes_change(P, L):
    V, _, _, _, sym, _, _ = H.job("seam", P)
    rows, _ = H.walk_batch(V, P, L, sym, 32)
    import errors
    import types
    v = errors.verdict(types.SimpleNamespace(B=3, prec=48), rows, sym)
    return [b for b in range(3) if v["data"][b] != H.job_verdict(48, "seam", P)["data"][b]]


@pytest.mark.parametrize("P", SEAM_P)
def test_lag_seam_jobs_tell_the_lags_apart(P):
    """The oracle's bytes change when the weight rows on two sides of a lane seam change places,
    and when the last lag loses its weights (measured: streams 1 and 2, for every P)."""
    L = H.job("seam", P)[2]
    assert not H.job_verdict(48, "seam", P)["code"].any()
    for a in (63, 127, 191):
        if a + 1 < P:
            M = [r[:] for r in L]
            M[a], M[a + 1] = M[a + 1], M[a]
            assert _bytes_change(P, M), a
    M = [r[:] for r in L]
    M[P - 1] = [0] * P
    assert _bytes_change(P, M)


@pytest.mark.parametrize("bits,V", [(b, V) for b in (32, 64) for V in STEER_V[b]])
def test_steered_jobs_code_every_seam_position(bits, V):
    """Every seam position is coded with the entry 1 (P = 4: never in the ring) and -- but for
    symbol 0, whose entry is 1 by the model's rule -- with an entry above 1 (P = 64)."""
    S = H.seam_positions(V, bits)
    assert len(S) > 4 and {0, 1, V - 2, V - 1} <= set(S)
    seen = {}
    for P in (4, 64):
        _, _, _, _, sym, rows, _ = H.job("steered", V, bits, P)
        assert sym[:len(S), 0].tolist() == S and sym[:len(S), 1].tolist() == S[::-1]
        e = rows[np.arange(len(sym))[:, None], np.arange(2)[None, :], sym]
        seen[P] = ({int(s) for s in sym[e == 1]}, {int(s) for s in sym[e > 1]})
        assert not H.job_verdict(48, "steered", V, bits, P)["code"].any()
        assert H.fudge_classes(H.totals(rows), 48)[2] == 1.0          # prec 48: never fudged
    assert seen[4] == (set(S), set()) and seen[64][1] == set(S) - {0}
    if V == 4096:
        assert not H.job_verdict(16, "steered", V, bits, 64)["code"].any()
        assert H.fudge_classes(H.totals(H.job("steered", V, bits, 64)[5]), 16)[0] > 0.5


def probe_model(bits, V, prec):
    """The exact-bounds probes' weights, ring, row and (s, x) pairs."""
    L = H.seam_weights(16, (1 << 20) if prec == 16 else 0)
    ring, pasti = H.probe_ring(V, bits)
    row = H.Stream(V, 16, L, ring, pasti).row()
    return L, ring, pasti, row, H.bound_probes(row, V, bits, prec)


@pytest.mark.parametrize("bits,V,prec", PROBES)
def test_bound_probes_sit_on_the_cdf_bounds(bits, V, prec):
    from oracle import restate
    L, ring, pasti, row, probes = probe_model(bits, V, prec)
    cdf, w = restate.cdf_of(row), 1 << prec
    assert len(probes) == {(32, 48): 24, (32, 16): 19, (64, 60): 20, (64, 16): 16}[bits, prec]
    assert (cdf[-1] > w) == (prec == 16)                             # fudged at prec 16 alone
    assert {s for s, _ in probes} >= set(H.seam_positions(V, bits))
    for s, x in probes:
        a, b = restate.symbol_to_range(cdf, 1, s, w)
        assert x in (a, b - 1) and restate.val_to_symbol(cdf, 1, x, w) == s
        if s > 0:
            assert restate.val_to_symbol(cdf, 1, a - 1, w) == s - 1
        if s + 1 < V:
            assert restate.val_to_symbol(cdf, 1, b, w) == s + 1
        if prec != 16:                                              # w >= T: the targets are c_{s-1} and c_s - 1
            assert a * cdf[-1] // w == (cdf[s - 1] if s else 0) and (b - 1) * cdf[-1] // w == cdf[s] - 1
