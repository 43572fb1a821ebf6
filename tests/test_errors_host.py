"""The error fixtures of tests/errors.py, checked on the host: every input the GPU error tests use
is built here and its verdict computed by the C oracle, so what those tests assume of their inputs
-- which stream fails, with which code, at which step; which streams are clean; which capacity
class a stream falls in -- is shown without a GPU."""
import numpy as np
import pytest

import errors as E
from straight_forms import forms_reached


@pytest.mark.parametrize("bits", [32, 64])
def test_verdicts_are_the_planted_defects(bits):
    """oracle.encode's (code, step) per stream is the defect make_case planted, and
    lacref_encode_batch's status agrees with it."""
    for case, v in zip(E.encode_cases(bits), E.encode_verdicts(bits)):
        for b, (kind, _, pos) in enumerate(case.streams):
            assert int(v["code"][b]) == E.EXPECT_CODE[kind], (case.prec, b, kind, v["code"][b])
            assert int(v["step"][b]) == pos, (case.prec, b, kind, v["step"][b])
        assert np.array_equal(v["batch_status"], v["code"])
        assert v["batch_rc"] == E.first_code(v["code"])
        assert len(case.clean) >= 2
        assert case.T == E.T_STEPS and case.V <= 512 and case.B <= 12
    for case, v in zip(E.encode_cases(bits), E.clean_verdicts(bits)):
        assert not v["code"].any()


def test_census():
    """Every defect kind occurs at every listed position; no (stream, step) carries two defects."""
    seen = set()
    for bits in (32, 64):
        for case in E.encode_cases(bits):
            for b, (kind, _, pos) in enumerate(case.streams):
                if kind == "none":
                    assert np.array_equal(case.pmf[:, b], case.clean_pmf[:, b])
                    assert np.array_equal(case.sym[:, b], case.clean_sym[:, b])
                    continue
                seen.add((bits, kind, pos))
                dsym = np.flatnonzero(case.sym[:, b] != case.clean_sym[:, b])
                dpmf = np.flatnonzero((case.pmf[:, b] != case.clean_pmf[:, b]).any(axis=1))
                assert len(dsym) + len(dpmf) == 1 and list(dsym) + list(dpmf) == [pos], (bits, b, kind)
    for bits, kinds in ((32, E.KINDS32), (64, E.KINDS64)):
        for kind in kinds:
            for pos in E.POSITIONS:
                assert (bits, kind, pos) in seen, (bits, kind, pos)


@pytest.mark.parametrize("bits", [32, 64])
def test_fudge_controls_take_zero_probability_symbols(bits):
    """The prec-21 case's clean streams take a symbol of probability 0 on a row that fudges at
    that step -- legal, width 1 -- and the oracle codes them."""
    case, v = E.encode_cases(bits)[-1], E.encode_verdicts(bits)[-1]
    assert case.prec == 21
    for b in case.clean:
        assert len(case.fudged_zero[b]) >= 3, (b, case.fudged_zero[b])
        for t in case.fudged_zero[b]:
            assert case.pmf[t, b, case.sym[t, b]] == 0
        assert v["code"][b] == 0 and v["nbits"][b] > 0


def test_clean_streams_reach_every_straight_form():
    """The clean streams of the split-path cases reach the u32 kernel's straight form and the u64
    kernel's t32, wide and fudge-testing instances (tests/straight_forms.py)."""
    got = {32: set(), 64: set()}
    for bits in (32, 64):
        for case in E.encode_cases(bits)[:2] + E.encode_cases(bits)[-1:]:
            for b in case.clean:
                got[bits] |= forms_reached(case.pmf[:, b].tolist(), case.sym[:, b].tolist(), case.prec, bits)
    assert "u32" in got[32]
    assert {"t32", "wide", "wide+ft", "wide+ft+exit", "t32+ft", "t32+ft+exit"} <= got[64], got[64]


@pytest.mark.parametrize("bits", [32, 64])
def test_floor_mapping_keeps_the_verdicts(bits):
    """Under the floor mapping no stream of the prec >= 32 cases meets a zero width the ceil
    mapping does not: the symbol and table tests do not depend on the mapping, a zero entry at
    the symbol is a zero width under both, and every other symbol keeps a positive width."""
    for case in E.encode_cases(bits)[:-1]:
        for b in range(case.B):
            kind, _, pos = case.streams[b]
            n = case.T if kind == "none" else pos
            E.floor_encode(case.pmf[:n, b].tolist(), case.sym[:n, b].tolist(), case.prec)
        kind_at = {b: k for b, (k, _, _) in enumerate(case.streams)}
        for b in case.failing:
            if kind_at[b] == "zero_width":
                t = case.streams[b][2]
                with pytest.raises(ZeroDivisionError):
                    E.floor_encode(case.pmf[:t + 1, b].tolist(), case.sym[:t + 1, b].tolist(), case.prec)


def test_precedence_case():
    """The two-defect fixture: each planted step holds both defects, and the oracle -- which
    builds the CDF before it looks at the symbol -- names the step, if not the code."""
    case, code, step = E.precedence_case()
    v = E.verdict(case)
    assert np.array_equal(v["step"], step)
    assert np.array_equal(v["code"] != 0, code != 0)
    assert case.sym[64, 1] == case.V and not case.pmf[64, 1].any()
    assert case.sym[65, 2] == case.V and sum(int(x) for x in case.pmf[65, 2]) == 1 << 64
    assert case.pmf[1, 4, case.sym[1, 4]] == 0 and sum(int(x) for x in case.pmf[1, 4]) == 1 << 65


def test_capacity_case_classes():
    cc = E.capacity_case()
    assert all(cc.cls.count(k) > 0 for k in "abc"), cc.cls
    assert (cc.capacity_bits + 63) // 64 + 1 == cc.words
    for b, k in enumerate(cc.cls):
        if k == "a":
            assert cc.code[b] == 0 and (cc.nbits[b] + 63) // 64 <= cc.words
        elif k == "b":
            assert cc.code[b] == E.LAC_E_CAPACITY and cc.step[b] == cc.T
        else:
            assert cc.code[b] == E.LAC_E_CAPACITY and 0 < cc.step[b] < cc.T
    assert len({int(s) for b, s in enumerate(cc.step) if cc.cls[b] == "c"}) >= 2   # more than one failing step
    out, nbits, status, rc = E.oracle.encode_batch(cc.pmf, cc.sym, cc.prec)     # the tables themselves are clean
    assert rc == 0 and not status.any()


@pytest.mark.parametrize("bits,prec", [(32, 32), (64, 56), (64, 48)])
def test_decode_cases(bits, prec):
    """The decode fixtures: the clean tables code without error, every listed position carries a
    bad row, and at least two streams stay clean."""
    for k in ((0, 1) if bits == 64 else (0,)):
        case = E.decode_case(bits, prec, k)
        assert not E.verdict(case, case.clean_pmf, case.clean_sym)["code"].any()
        assert sorted(p for _, _, p in case.streams if p >= 0) == list(E.POSITIONS)
        assert len(case.clean) >= 2 and np.array_equal(case.sym, case.clean_sym)
        v = E.verdict(case)
        for b, (kind, _, pos) in enumerate(case.streams):
            assert int(v["code"][b]) == E.EXPECT_CODE[kind] and int(v["step"][b]) == pos
    lean = E.decode_case(32, 48, lean=True)
    assert lean.B <= 5 and not E.verdict(lean, lean.clean_pmf, lean.clean_sym)["code"].any()


@pytest.mark.parametrize("bits,prec", [(32, 32), (64, 56)])
def test_windowed_decode_cases_outgrow_their_window(bits, prec):
    """The windowed run's streams ('skew' rows) are longer than the smallest window
    include/lac.h's rule allows for a refill every 32 steps, bad rows and all verdicts as in the
    other decode fixtures."""
    case = E.decode_case(bits, prec, 0, flavour="skew")
    v = E.verdict(case, case.clean_pmf, case.clean_sym)
    assert not v["code"].any()
    W = (33 * prec + 63 + 63) // 64
    assert int(v["nbits"].min()) > 64 * (W + 8), (v["nbits"], W)
    bad = E.verdict(case)
    for b, (kind, _, pos) in enumerate(case.streams):
        assert int(bad["code"][b]) == E.EXPECT_CODE[kind] and int(bad["step"][b]) == pos
