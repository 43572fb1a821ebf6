"""Host checks of the adaptive n-gram count models (include/lac.h lac_count_*), no GPU needed.

* The fixtures of tests/golden/markov_cases.json (tools/gen_golden_markov.py: the reference's
  ``AC(Markov_up_to_n(V, order, lfunc), prec)`` with ``lfunc`` linear in the count) against the C
  oracle on the rows of the dense host restatement (tests/counts.py): this pins the yardstick the
  GPU tests use -- a count-model job IS the pmf job on the rows the counts produce.
* The census of the fixtures: rows that fudge at every width, and cases that mix them with plain
  rows.
* lac_amd/csrc/lac_count.h, the plain host rules the kernels share (tests/native/count_check.cpp):
  the limits at their edges, the layout, the row and accept against the Python restatement on
  random histories and against a sparse n-gram map; the sweep also runs as a stand-alone
  ASan + UBSan program.
* coder.Markov_up_to_n on the per-token path of the host coder with a non-linear ``lfunc``.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import counts as K
from conftest import REPO, load_golden
from oracle import oracle

NATIVE = os.path.join(REPO, "tests", "native")
SO = os.path.join(NATIVE, "libcountcheck.so")
SRC = os.path.join(NATIVE, "count_check.cpp")
HDR = os.path.join(REPO, "lac_amd", "csrc", "lac_count.h")
INCS = ["-I", os.path.join(REPO, "lac_amd", "csrc")]

ALL = load_golden("markov_cases.json")
CASES = [c for c in ALL if c["weights"] is not None]              # the linear ones: the device's family
IDS = [c["name"] for c in CASES]
NONLINEAR = [c for c in ALL if c["weights"] is None]


def case_rows(case, syms=None, extra_row=False):
    return K.walk(case["V"], case["order"], case["weights"], case["syms"] if syms is None else syms,
                  case["pmf_bits"], extra_row=extra_row)


# ------------------------------------------------------------------ the fixtures pin the yardstick
def test_fixture_set_covers_the_issue():
    shapes = {(c["V"], c["order"], tuple(c["weights"]), c["prec"], len(c["syms"])) for c in CASES}
    assert shapes >= {(2, 1, (1,), 16, 64), (4, 2, (1, 9), 16, 200), (17, 2, (3, 7000), 16, 300),
                      (40, 2, (900, 1), 16, 200), (64, 1, (5000,), 16, 150), (12, 3, (0, 12, 96), 16, 200),
                      (100, 2, (1, 30000), 16, 120), (300, 2, (2000, 1), 16, 90), (256, 2, (1, 300), 48, 130),
                      (256, 1, (1,), 24, 70), (5, 3, (1, 40, 5000), 16, 260),
                      (31, 3, (1, 1 << 20, 1 << 29), 48, 100)}
    assert any(c["order"] == 4 and c["V"] == 3 for c in CASES)
    assert any(c["pmf_bits"] == 64 and c["V"] == 129 for c in CASES)
    assert any(c.get("default_lfunc") for c in CASES) and len(NONLINEAR) >= 1
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "markov_cases.json")) < 64 << 10


def test_census_of_fudged_rows():
    """With w0 = 2^(prec-1) a step always fudges when T > 2 w0 minp."""
    shares = {c["name"]: K.always_fudged_share(c) for c in CASES if c["prec"] == 16}
    assert sum(1 for v in shares.values() if v > 0.5) >= 2, shares
    assert any(0.05 < v < 0.5 for v in shares.values()), shares


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_bits_are_the_oracle_on_restated_rows(case):
    rows, st = case_rows(case)
    assert list(st.past) == case["past"]
    data, nbits, _ = oracle.encode(rows, case["syms"], case["prec"])
    assert nbits == case["L"] and data.hex() == case["bytes"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_decoded_counts_are_the_bitserial_oracle(case):
    data = bytes.fromhex(case["bytes"])
    rows, _ = case_rows(case, case["decoded"], extra_row=True)        # the decoder's own walk, extras included
    assert oracle.decode_bitserial(rows, data, case["L"], case["prec"]) == case["decoded"]
    assert len(case["decoded"]) == case["decoded_count"] >= len(case["syms"])
    assert case["decoded"][:len(case["syms"])] == case["syms"]
    pre = oracle.decode_bitserial(rows, data, case["prefix_bits"], case["prec"])
    assert pre == case["decoded"][:case["prefix_decoded_count"]]


def test_restated_table_is_the_reference_dict():
    """Stream.table(): the dense counts as n-gram tuples, against a plain dict walk."""
    case = next(c for c in CASES if c["order"] == 3)
    _, st = case_rows(case)
    want, past = {}, ()
    for s in case["syms"]:
        g = past + (s,)
        for i in range(len(past)):
            want[g[-i - 1:]] = want.get(g[-i - 1:], 0) + 1
        past = g[-case["order"]:]
    assert st.table() == want


# ------------------------------------------------------------------ lac_count.h
def _stale(target, *deps):
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(d) for d in deps)


@pytest.fixture(scope="module")
def cc():
    if _stale(SO, SRC, HDR):
        subprocess.run(["hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", *INCS, SRC, "-o", SO], check=True)
    lib = C.CDLL(SO)
    lib.cc_limits_ok.argtypes = [C.c_int64, C.c_int]
    lib.cc_weights_ok.argtypes = [C.c_void_p, C.c_int]
    lib.cc_ngrams.argtypes = [C.c_int64, C.c_int]
    lib.cc_ngrams.restype = C.c_int64
    lib.cc_layout.argtypes = [C.c_int64, C.c_int, C.c_void_p]
    lib.cc_walk.argtypes = [C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                            C.c_void_p, C.c_void_p, C.c_void_p]
    lib.cc_sweep.argtypes = [C.c_int, C.c_uint64]
    return lib


def test_model_limits(cc):
    ok = cc.cc_limits_ok
    assert ok(1, 1) and ok(2, 4) and ok(4096, 1) and ok(4096, 2) and not ok(4097, 1)   # V <= 4096
    assert ok(256, 3) and not ok(256, 4)                        # an order-3 byte model fits: 16.8 M counts
    assert cc.cc_ngrams(256, 3) == 256 + 256 ** 2 + 256 ** 3 <= 1 << 25
    assert ok(75, 4) and not ok(76, 4)                          # 75 + .. + 75^4 = 32 068 200 <= 2^25 < 76 + .. + 76^4
    assert K.ngrams(75, 4) <= 1 << 25 < K.ngrams(76, 4) and cc.cc_ngrams(76, 4) == -1
    assert ok(322, 3) and not ok(323, 3)
    assert K.ngrams(322, 3) <= 1 << 25 < K.ngrams(323, 3)
    assert not ok(4096, 3)                                      # (no overflow of V^i)
    assert not ok(4, 0) and not ok(4, 5) and not ok(4, -1) and not ok(0, 1) and not ok(-3, 2)
    w = np.array([0, (1 << 30) - 1, 5, 1 << 30], dtype=np.uint32)
    p = w.ctypes.data_as(C.c_void_p)
    assert cc.cc_weights_ok(p, 3) and not cc.cc_weights_ok(p, 4)


def _layout(cc, V, order):
    out = np.zeros(7, dtype=np.int64)
    cc.cc_layout(V, order, out.ctypes.data_as(C.c_void_p))
    return {"Vc": int(out[0]), "stride": int(out[1]), "words": int(out[2]), "off": [int(x) for x in out[3:3 + order]]}


def test_layout(cc):
    for V, order in ((1, 1), (2, 4), (3, 4), (5, 3), (17, 2), (255, 2), (256, 3), (257, 2), (4096, 2), (300, 2)):
        y, want = _layout(cc, V, order), K.layout(V, order)
        assert y["Vc"] == -(-V // 4) * 4 and y["Vc"] % 4 == 0                     # every row starts on a 16-B vector
        assert y["stride"] % 64 == 0 and 0 <= y["stride"] - y["words"] < 64      # a multiple of 256 B
        assert y["off"] == want["off"] and y["words"] == want["words"] and y["stride"] == want["stride"]
        assert y["off"][0] == 0
        for i in range(1, order):
            assert y["off"][i] == y["off"][i - 1] + V ** (i - 1) * y["Vc"]       # sections back to back


def _c_walk(cc, V, order, W, bits, syms, counts=None, past=None):
    y = K.layout(V, order)
    cs = np.zeros(y["stride"], dtype=np.uint32) if counts is None else counts.copy()
    ps = np.full(order, -1, dtype=np.int32) if past is None else np.array(past, dtype=np.int32)
    w = np.array(W, dtype=np.uint32)
    s = np.array(syms, dtype=np.int32)
    rows = np.zeros((len(s), V), dtype=np.uint64)
    ok, acc = np.zeros(len(s), dtype=np.int32), np.zeros(len(s), dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    cc.cc_walk(V, order, p(w), bits, p(s), len(s), p(cs), p(ps), p(rows), p(ok), p(acc))
    return rows, ok, acc, cs, ps


@pytest.mark.parametrize("V,order,W,bits", ((2, 4, [1, 2, 3, 4], 32), (5, 3, [1, 40, 5000], 32), (17, 2, [0, 9], 64),
                                            (256, 2, [1, 300], 32), (257, 1, [7], 32),
                                            (31, 3, [1, 1 << 20, (1 << 30) - 1], 64)))
def test_row_and_accept_against_the_python_restatement(cc, V, order, W, bits):
    rng = np.random.default_rng(V * 10 + order)
    syms = K.draw(rng, V, 150)[:, 0]
    rows, ok, acc, cs, ps = _c_walk(cc, V, order, W, bits, syms)
    st = K.Stream(V, order, W)
    for t, s in enumerate(syms):
        assert rows[t].tolist() == st.row() and ok[t] == 1 and acc[t] == 1, t
        st.accept(s)
    assert np.array_equal(cs, st.counts) and ps.tolist() == st.past_row()
    # continued from a stored state: the same as the unbroken walk
    a = _c_walk(cc, V, order, W, bits, syms[:70])
    b = _c_walk(cc, V, order, W, bits, syms[70:], a[3], a[4])
    assert np.array_equal(b[0], rows[70:]) and np.array_equal(b[3], cs) and np.array_equal(b[4], ps)


def test_bad_rows_and_symbols_stop_the_walk(cc):
    # u32 entries: 1 + 2^29 * 8 does not fit -> the row's status is bad at the step the restatement predicts
    V, order, W = 4, 1, [1 << 29]
    syms = [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]
    rows, ok, acc, cs, ps = _c_walk(cc, V, order, W, 32, syms)
    want, _ = K.walk(V, order, W, syms, 32)
    first_bad = int(np.flatnonzero(want.sum(axis=1) == 0)[0])
    assert first_bad == 9 and ok.tolist() == [1] * 9 + [0, 0] and acc.tolist() == [1] * 9 + [0, 0]
    assert int(cs[1]) == 8 and int(cs.sum()) == 8                 # (the first step has no history to count under)
    rows64, ok64, acc64, _, _ = _c_walk(cc, V, order, W, 64, syms)
    assert ok64.all() and acc64.all()
    # a symbol out of range: nothing moves from there on
    _, _, acc, cs, ps = _c_walk(cc, 5, 2, [1, 2], 32, [0, 1, 5, 2])
    assert acc.tolist() == [1, 1, 0, 0] and ps.tolist() == [0, 1] and int(cs.sum()) == 1


def _slot(V, order, sec, ctx, s):
    y = K.layout(V, order)
    return y["off"][sec] + K.row_index(ctx, V) * y["Vc"] + s


@pytest.mark.parametrize("order,sec", ((1, 0), (4, 0), (4, 3)))
def test_a_full_count_refuses_the_step(cc, order, sec):
    """Preset counts of 0xfffffffe and 0xffffffff in section `sec`: the first takes one more accept
    and is then full, the second refuses at once; a refused step changes nothing and ends the walk.
    ok / acc, the counts and the past of lac_count.h against the restatement's."""
    V, W, bits = 5, [1, 2, 3, 4][:order], 64
    a, x, b = 0, 2, 1
    for past, syms, what in (((3, 1, 4, 2)[-order:], [a, x, b, 3, 3], "a second slot"),
                             ((a,) * order, [a, a, 4, a], "the same slot")):
        counts = np.zeros(K.layout(V, order)["stride"], dtype=np.uint32)
        counts[_slot(V, order, sec, past[order - sec:], a)] = 0xfffffffe
        if what == "a second slot":
            after = (tuple(past) + (a, x))[-order:]
            counts[_slot(V, order, sec, after[order - sec:], b)] = 0xffffffff
        rows, ok, acc, cs, ps = _c_walk(cc, V, order, W, bits, syms, counts, past)
        st, want_ok, want_acc, dead = K.Stream(V, order, W, counts, past), [], [], False
        for t, s in enumerate(syms):
            r = st.row()
            assert rows[t].tolist() == r, (what, t)
            want_ok.append(int(max(r) < 1 << bits and sum(r) < 1 << 64))
            go = not dead and bool(want_ok[-1]) and st.accept(s)
            want_acc.append(int(go))
            dead = dead or not go
        stop = 2 if what == "a second slot" else 1                # (the restatement itself stops where it was built to)
        assert want_acc == [1] * stop + [0] * (len(syms) - stop) and all(want_ok), (what, want_acc)
        assert ok.tolist() == want_ok and acc.tolist() == want_acc, (what, ok, acc)
        assert np.array_equal(cs, st.counts) and ps.tolist() == st.past_row(), what
        assert int(cs.max()) == 0xffffffff and int(cs[_slot(V, order, sec, past[order - sec:], a)]) == 0xffffffff
        # walk(): the refused step's row is the empty row, and the walk is dead from there on
        wrows, wst = K.walk(V, order, W, syms, bits, counts, past)
        assert not wrows[stop:].any() and wrows[:stop].all() and np.array_equal(wst.counts, st.counts)
        assert wst.past == st.past
        with pytest.raises(oracle.OracleError) as e:
            oracle.encode(wrows, syms, 24)
        assert (e.value.code, e.value.step) == (-5, stop)         # LAC_E_TABLE at that step


def test_rules_against_a_sparse_map(cc):
    assert cc.cc_sweep(150, 12345) == 0


def test_sanitized_sweep_program():
    """The same sweep as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer
    (host code only; every buffer a heap block of exactly the layout's size)."""
    outdir = os.path.join(NATIVE, "_asan")
    os.makedirs(outdir, exist_ok=True)
    exe = os.path.join(outdir, "count_check_main")
    if _stale(exe, SRC, HDR):
        # host code only: the sanitizers are given to the host compilation alone
        subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-DCOUNT_CHECK_MAIN",
                        "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", *INCS, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    report = r.stdout + r.stderr
    assert r.returncode == 0, report[-3000:]
    assert "count_check: ok" in report and "ERROR" not in report and "runtime error" not in report


# ------------------------------------------------------------------ coder.Markov_up_to_n on the host
def _host_bits(predictor, prec, syms):
    """The host restatement's coder over a predictor's own rows: the per-token path's yardstick."""
    rows = []
    for s in syms:
        rows.append([predictor.prob(x) for x in range(predictor.n)])
        predictor.accept(s)
    return oracle.encode(np.array(rows, dtype=np.uint64), syms, prec)


@pytest.mark.parametrize("case", NONLINEAR, ids=[c["name"] for c in NONLINEAR])
def test_markov_class_with_a_nonlinear_lfunc(case):
    from lac_amd.coder import Markov_up_to_n
    p = Markov_up_to_n(case["V"], case["order"], K.LFUNCS[case["lfunc"]])
    data, nbits, _ = _host_bits(p, case["prec"], case["syms"])
    assert nbits == case["L"] and data.hex() == case["bytes"]
    assert list(p.past) == case["past"] and isinstance(p.past, tuple) and isinstance(p.table, dict)


def test_markov_class_is_the_issues_model():
    from lac_amd.coder import CountWeights, Markov_up_to_n
    case = next(c for c in CASES if c.get("default_lfunc"))
    V, order = case["V"], case["order"]
    p = Markov_up_to_n(V, order)                                    # lfunc=None: W[o] = n o^3
    assert isinstance(p.lfunc, CountWeights) and list(p.lfunc.weights) == case["weights"]
    assert p.lfunc(3, 2, V, order) == 3 * case["weights"][2]
    st = K.Stream(V, order, case["weights"])
    q = p.copy()
    for s in case["syms"][:80]:
        assert [p.prob(x) for x in range(V)] == st.row()
        assert p.dist[-1] == sum(st.row())
        p.accept(s)
        st.accept(s)
    assert p.table == st.table() and p.past == st.past
    assert all(p[k] == v for k, v in st.table().items()) and p[st.past + (0,)] == 0   # item access; absent: 0
    assert q.table == {} and q.past == ()                            # the copy did not move
    r = Markov_up_to_n(V, order, past=p.past, table=dict(p.table))   # handed over with a table
    assert [r.prob(x) for x in range(V)] == st.row()
