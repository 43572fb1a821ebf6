"""The sticky per-stream error contract of include/lac.h on every encode kernel form: coder_step
(the split path's general chain, taken by every block of a traced encode and by any block with a
bad step), the straight 64-step blocks of k_encode (the u32 form with bits 32; the t32, wide and
fudge-testing instances of straight_steps with bits 64 -- tests/test_errors_host.py shows the
clean streams reach each), k_encode_fused, and finish_stream in k_finish and under the job
kernels' kFinish flag; ceil and floor mapping; one call, a job, and calls cut at 1 and 65.

Every expected status, step and byte comes from the C oracle through tests/errors.py (floor
mapping: its floor restatement of restate.encode_digits).  The two comparisons between GPU runs
are the ones the contract itself is about: a failed stream's registers and planes against a
context that coded only that stream's first err_step symbols (whose bytes the oracle then
confirms), and the capacity error's state across forms."""
import numpy as np
import pytest

import errors as E

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A5A5A5A5A

# encode path, mapping, traced
FORMS = (("split", None, False), ("fused", None, False), ("split", None, True), ("split", "floor", False),
         ("fused", "floor", False))
FORM_IDS = ["split", "fused", "split-traced", "split-floor", "fused-floor"]
WAYS = ("one", "job", "cuts")
REG_FIELDS = ("l", "h", "L", "wa", "wc", "nsym")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _coder(case, path, mapping, cap=None):
    from lac_amd.batch import BatchCoder
    c = BatchCoder(case.V, case.B, prec=case.prec, pmf_bits=case.bits,
                   capacity_bits=cap or case.capacity_bits, device=DEV)
    c.set_path(path)
    if mapping:
        c.set_mapping(mapping)
    return c


def _encode(c, dp, ds, way, traced):
    """-> status before the finish (None for a job), the checkpoint there, the trace."""
    T, B = ds.shape
    tr = torch.full((T, B, 2), SENTINEL, dtype=torch.int64, device=DEV) if traced else None
    if way == "job":
        c.encode_job(dp, ds, trace=tr)
        return None, None, tr
    c.reset()
    for a, b in (((0, T),) if way == "one" else E.CUTS):
        c.encode(dp[a:b], ds[a:b], trace=None if tr is None else tr[a:b])
    before = c.status()
    ck = c.checkpoint()
    c.finish()
    return before, ck, tr


_expect_cache = {}


def _expect(bits, i, mapping):
    """Per stream: code, step, (bytes, nbits) of the stream or of its failing prefix -- the
    oracle's, or for the floor mapping errors.floor_encode's on the oracle's verdict
    (test_errors_host.py::test_floor_mapping_keeps_the_verdicts)."""
    key = (bits, i, mapping)
    if key not in _expect_cache:
        case, v = E.encode_cases(bits)[i], E.encode_verdicts(bits)[i]
        data, nbits = list(v["data"]), v["nbits"].copy()
        if mapping == "floor":
            for b in range(case.B):
                n = case.T if v["code"][b] == 0 else int(v["step"][b])
                data[b], nbits[b] = E.floor_encode(case.pmf[:n, b].tolist(), case.sym[:n, b].tolist(), case.prec)
        _expect_cache[key] = (v["code"], v["step"], data, nbits)
    return _expect_cache[key]


_prefix_cache = {}


def _prefix(bits, i, mapping):
    """The reference states: a split-path context given the same tables, in which per-stream
    counts end every failing stream after its first err_step symbols (the reference verdict's
    step), so it codes exactly the prefix and meets no defect.  Its finish must give the
    expected prefix bytes; its checkpoint before that is what a failed stream must look like."""
    key = (bits, i, mapping)
    if key not in _prefix_cache:
        case = E.encode_cases(bits)[i]
        code, step, data, nbits = _expect(bits, i, mapping)
        c = _coder(case, "split", mapping)
        c.set_stream_lengths(np.where(code == 0, case.T, step))
        c.reset()
        c.encode(E.dev_pmf(case.pmf, DEV), E.dev_sym(case.sym, DEV),
                 trace=torch.zeros((case.T, case.B, 2), dtype=torch.int64, device=DEV))
        ck = c.checkpoint()
        c.finish()
        rc, err, _ = c.status()
        assert rc == 0 and not err.any()
        got, gn = E.stream_bytes(c)
        c.close()
        assert np.array_equal(gn, nbits), (gn, nbits)
        assert got == data
        _prefix_cache[key] = ck
    return _prefix_cache[key]


def _check_status(st, code, step, what):
    rc, err, es = st
    assert np.array_equal(err, code), (what, err, code)
    assert np.array_equal(es, step), (what, es, step)
    assert rc == E.first_code(code), (what, rc)


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("bits", [32, 64])
def test_encode_errors(bits, form, way):
    path, mapping, traced = form
    cases = E.encode_cases(bits)
    for i, case in enumerate(cases):
        if mapping == "floor" and case.prec < 32:
            continue                                              # (rows that fudge: ceil mapping only)
        what = (bits, FORM_IDS[FORMS.index(form)], way, i)
        code, step, data, nbits = _expect(bits, i, mapping)
        dp, ds = E.dev_pmf(case.pmf, DEV), E.dev_sym(case.sym, DEV)
        c = _coder(case, path, mapping)
        before, ck, tr = _encode(c, dp, ds, way, traced)
        _check_status(c.status(), code, step, what)
        got, gn = E.stream_bytes(c)
        for b in range(case.B):
            if code[b] == 0:                                      # clean: the oracle's stream
                assert int(gn[b]) == int(nbits[b]) and got[b] == data[b], (what, b)
            else:
                assert int(gn[b]) == 0, (what, b, gn[b])
        if before is not None:
            _check_status(before, code, step, what)
            ref = _prefix(bits, i, mapping)
            wp, rp = E.written(ck), E.written(ref)
            assert np.array_equal(ck["state"]["err"], code) and np.array_equal(ck["state"]["err_step"], step)
            for b in range(case.B):                               # failed: frozen before the failing step
                for f in REG_FIELDS:
                    assert ck["state"][f][b] == ref["state"][f][b], (what, b, f, ck["state"][b], ref["state"][b])
                assert np.array_equal(wp[:, b], rp[:, b]), (what, b)
        if traced:
            t = tr.cpu().numpy().view(np.uint64)
            for b in range(case.B):
                n = case.T if code[b] == 0 else int(step[b])
                assert (t[n:, b] == np.uint64(SENTINEL)).all(), (what, b)
                assert (t[:n, b, 1] <= 64).all(), (what, b)
                assert int(t[:n, b, 1].sum()) == int(ck["state"]["L"][b]) if ck is not None else True, (what, b)
        c.close()


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("bits", [32, 64])
def test_errors_are_sticky_until_reset(bits, form):
    """One more encode of valid rows leaves a failed stream's state and planes byte for byte and
    moves the clean streams on; reset clears err to 0 and err_step to -1, and the context then
    codes the clean job to the oracle's bytes."""
    path, mapping, traced = form
    cases, cleans = E.encode_cases(bits), E.clean_verdicts(bits)
    for i in (0, len(cases) - 1):
        case = cases[i]
        if mapping == "floor" and case.prec < 32:
            continue
        code, step, _, _ = _expect(bits, i, mapping)
        c = _coder(case, path, mapping)
        c.reset()
        tr = torch.zeros((case.T, case.B, 2), dtype=torch.int64, device=DEV) if traced else None
        c.encode(E.dev_pmf(case.pmf, DEV), E.dev_sym(case.sym, DEV), trace=tr)
        ck1 = c.checkpoint()
        c.encode(E.dev_pmf(case.clean_pmf[:1], DEV), E.dev_sym(case.clean_sym[:1], DEV),
                 trace=None if tr is None else tr[:1])
        ck2 = c.checkpoint()
        _check_status(c.status(), code, step, (bits, form, i))
        w1, w2 = E.written(ck1), E.written(ck2)
        for b in range(case.B):
            if code[b]:
                assert ck1["state"][b].tobytes() == ck2["state"][b].tobytes(), (form, i, b)
                assert np.array_equal(w1[:, b], w2[:, b]), (form, i, b)
            else:
                assert ck2["state"]["nsym"][b] == case.T + 1, (form, i, b)
        c.reset()
        rc, err, es = c.status()
        assert rc == 0 and not err.any() and (es == -1).all(), (form, i, err, es)
        c.encode_job(E.dev_pmf(case.clean_pmf, DEV), E.dev_sym(case.clean_sym, DEV))
        rc, err, es = c.status()
        assert rc == 0 and not err.any() and (es == -1).all(), (form, i, err, es)
        got, gn = E.stream_bytes(c)
        for b in range(case.B):
            if mapping == "floor":
                wd, wn = E.floor_encode(case.clean_pmf[:, b].tolist(), case.clean_sym[:, b].tolist(), case.prec)
            else:
                wd, wn = cleans[i]["data"][b], int(cleans[i]["nbits"][b])
            assert int(gn[b]) == wn and got[b] == wd, (form, i, b)
        c.close()


CAP_FORMS = (("split", False, "one"), ("split", True, "one"), ("fused", False, "one"), ("split", False, "job"),
             ("fused", False, "job"))


def test_capacity_classes():
    """errors.capacity_case on split + finish, fused + finish and the two jobs: (a) streams that
    fit give the oracle's bytes, (b) streams whose flush alone does not fit fail in finish_stream
    with err_step = T, (c) streams that overflow at a step fail there, at the step restate's
    per-step digit counts give under plane_append's rule.  A capacity error comes after the
    narrowing, so its state is compared across the forms: ENC_STATE and the written planes of
    split-straight, split-traced and fused are byte-identical."""
    cc = E.capacity_case()
    dp, ds = E.dev_pmf(cc.pmf, DEV), E.dev_sym(cc.sym, DEV)
    cks = {}
    for path, traced, way in CAP_FORMS:
        what = (path, traced, way)
        c = _coder(cc, path, None, cap=cc.capacity_bits)
        assert c.bits_stride() == 8 * cc.words
        before, ck, _ = _encode(c, dp, ds, way, traced)
        _check_status(c.status(), cc.code, cc.step, what)
        got, gn = E.stream_bytes(c)
        assert np.array_equal(gn, cc.nbits), (what, gn, cc.nbits)
        for b, k in enumerate(cc.cls):
            if k == "a":
                assert got[b] == cc.data[b], (what, b)
        if before is not None:                                    # before the finish: only class (c) has failed
            code = np.where(np.array(cc.cls) == "c", cc.code, 0).astype(np.int32)
            _check_status(before, code, np.where(code != 0, cc.step, -1), what)
            cks[(path, traced)] = ck
        c.close()
    base = cks[("split", False)]
    for key in (("split", True), ("fused", False)):
        assert base["state"].tobytes() == cks[key]["state"].tobytes(), (key, base["state"], cks[key]["state"])
        assert np.array_equal(E.written(base), E.written(cks[key])), key


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_precedence_symbol_then_table_then_zero_width(form, way):
    """Two defects in one step: every encode form reports the code of include/lac.h's order --
    the symbol's range before the table, the table before a zero width -- at the same step."""
    path, mapping, traced = form
    case, code, step = E.precedence_case()
    c = _coder(case, path, mapping)
    before, _, _ = _encode(c, E.dev_pmf(case.pmf, DEV), E.dev_sym(case.sym, DEV), way, traced)
    if before is not None:
        _check_status(before, code, step, (form, way, "before finish"))
    _check_status(c.status(), code, step, (form, way))
    got, gn = E.stream_bytes(c)
    for b in range(case.B):
        if code[b]:
            assert int(gn[b]) == 0
        elif mapping is None:
            wd, wn, _ = E.oracle.encode(case.pmf[:, b], case.sym[:, b], case.prec)
            assert int(gn[b]) == wn and got[b] == wd, (form, way, b)
    c.close()
