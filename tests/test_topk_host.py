"""Host checks of top-k rows from logits (include/lac.h lac_topk_logits), no GPU needed.

lac_amd/csrc/lac_topk.h, the plain rules the kernels share (tests/native/topk_check.cpp), in both of
their forms -- the literal whole-row rule, and the level histogram / threshold by lanes / ordered
rank walked over the kernels' tiles, waves, register rounds and lanes under both forms' plans --
against Python integers on the C oracle's q1 tables (topk.yardstick): 1000 random rows, rows built
to tie, rows whose tie class straddles every seam of the layout, the argument rules at every edge
and the form selection.  The sweep also runs as a stand-alone ASan + UBSan program.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import topk as TK
from oracle import oracle

LAC_E_ARG = -1
FORMS = ((0, TK.FORM_AUTO), (1, TK.FORM_REGS), (1, TK.FORM_STREAM))   # the literal rule; the kernels' form, both plans


@pytest.fixture(scope="module")
def tk():
    return TK.native()


def _same(rows, k, wb, K, what):
    """every form of every row against the yardstick, element for element including pads"""
    want_i, want_w = TK.yardstick(rows, k, wb, K)
    for n, row in enumerate(rows.reshape(-1, rows.shape[-1])):
        for which, forced in FORMS:
            idx, wt = TK.native_row(which, row, k, wb, K, forced)
            assert np.array_equal(idx, want_i.reshape(-1, K)[n]), (what, n, which, forced, k)
            assert np.array_equal(wt, want_w.reshape(-1, K)[n]), (what, n, which, forced, k)


# ------------------------------------------------------------------ the table the rule leans on
def test_weights_are_the_q1_table_at_24_bits_and_classes_are_runs(tk):
    """g = what the oracle's q1 writes at prec 61 (and at 48, for these vocabularies); TAB has 453
    distinct values over 545 levels, the first equal pair at index 423 (value 30)."""
    x = np.linspace(0.0, -17.5, 2048, dtype=np.float32)
    g = oracle.q1_quantize(x, 61)
    assert np.array_equal(g, oracle.q1_quantize(x, 48)) and g[0] == 1 << 24 and g[-1] == 1
    tab = sorted({int(v) for v in g}, reverse=True)
    lo, hi = C.c_int(), C.c_int()
    classes = set()
    for j in range(545):
        tk.tk_class(j, C.byref(lo), C.byref(hi))
        assert lo.value <= j <= hi.value
        classes.add((lo.value, hi.value))
    assert len(classes) == 453 == len(tab)
    multi = sorted(c for c in classes if c[0] != c[1])
    assert multi[-1] == (544 - 424, 544 - 423)                  # the highest levels that tie
    assert (0, 24) in classes                                   # TAB = 1: 25 levels
    # the levels the seam rows use: two levels of one class, and a lower class
    la, lb, ll = (tk.tk_level(np.float32(v), np.float32(0.0)) for v in (TK.TIE_A, TK.TIE_B, TK.LOW))
    tk.tk_class(la, C.byref(lo), C.byref(hi))
    assert la != lb and lo.value <= lb <= hi.value and ll < lo.value


# ------------------------------------------------------------------ the call's arguments
def test_argument_rules_at_every_edge(tk):
    def ok(lg=64, typ=TK.BF16, V=64, ss=64, bs=64, k=8, wb=24, K=8, idx=128, wt=256):
        return bool(tk.tk_args_ok(lg, typ, V, ss, bs, k, wb, K, idx, wt))
    assert ok() and ok(typ=TK.F32, V=4, k=4, K=4) and ok(ss=0, bs=0) and ok(ss=72, bs=1 << 40)
    for typ in (0, 3, -1):
        assert not ok(typ=typ)
    assert not ok(lg=0) and not ok(lg=8) and not ok(lg=65) and not ok(idx=0) and not ok(wt=0)
    for a in (4, 8, 12, 129):
        assert not ok(idx=a) and not ok(wt=a), a
    assert not ok(V=60) and ok(typ=TK.F32, V=60) and not ok(typ=TK.F32, V=62)
    for s in (-8, -1, 4, 63):
        assert not ok(ss=s) and not ok(bs=s), s
    assert ok(typ=TK.F32, ss=4, bs=12) and not ok(typ=TK.F32, bs=2)
    # k in [1, min(V, 256)]
    assert ok(k=1, K=4) and not ok(k=0, K=4) and not ok(k=-1, K=4)
    assert ok(V=8, k=8, K=8) and not ok(V=8, k=9, K=12)
    assert ok(V=512, k=256, K=256) and not ok(V=512, k=257, K=260)
    # K a multiple of 4 in [k, 256]
    assert ok(k=5, K=8) and ok(k=5, K=256) and not ok(k=5, K=4) and not ok(k=5, K=6) and not ok(k=5, K=260)
    assert ok(V=512, k=253, K=256) and not ok(V=512, k=253, K=254)
    # weight_bits in [0, 24]
    assert ok(wb=0) and ok(wb=16) and not ok(wb=-1) and not ok(wb=25)


def test_form_selection():
    """Rows of at most 16384 vectors stay in registers; longer ones stream in about four tiles."""
    for name, V, tb, form in (("qwen2 bf16", 151936, 2, None), ("llama-3 bf16", 128256, 2, TK.FORM_REGS),
                              ("llama-2 bf16", 32000, 2, TK.FORM_REGS), ("llama-3 f32", 128256, 4, TK.FORM_STREAM),
                              ("llama-2 f32", 32000, 4, TK.FORM_REGS), ("tiny", 8, 2, TK.FORM_REGS)):
        rc, f, R, threads, tiles = TK.plan(V, tb)
        nvec = V * tb // 16
        assert rc == 0 and threads % 64 == 0 and 64 <= threads <= 1024 and R in (8, 16), name
        assert f == (TK.FORM_REGS if nvec <= 16384 else TK.FORM_STREAM), name
        assert form is None or f == form, name
        assert threads * R * tiles >= nvec and (f == TK.FORM_STREAM or tiles == 1), name
        if f == TK.FORM_STREAM:
            assert threads * R * (tiles - 1) < nvec
    assert TK.plan(131072, 2)[1] == TK.FORM_REGS and TK.plan(131080, 2)[1] == TK.FORM_STREAM
    assert TK.plan(65536, 4)[1] == TK.FORM_REGS and TK.plan(65540, 4)[1] == TK.FORM_STREAM
    # a forced form: streamed holds any row, registers only its own
    assert TK.plan(128256, 4, TK.FORM_REGS)[0] == LAC_E_ARG and TK.plan(131080, 2, TK.FORM_REGS)[0] == LAC_E_ARG
    assert TK.plan(128256, 2, TK.FORM_STREAM)[:2] == (0, TK.FORM_STREAM) and TK.plan(8, 2, TK.FORM_STREAM)[0] == 0
    assert TK.plan(64, 2, 3)[0] == LAC_E_ARG
    # the small shapes the device tests force have more than one wave, round or tile
    assert TK.plan(4104, 2, TK.FORM_REGS)[2:] == (8, 128, 1) and TK.plan(4104, 2, TK.FORM_STREAM)[4] == 2
    assert TK.plan(4104, 4, TK.FORM_STREAM)[4] >= 3
    assert TK.seams(4104, 2, TK.FORM_REGS) == [8, 512, 4096] and TK.seams(4104, 2, TK.FORM_STREAM) == [8, 512, 4096]
    assert TK.seams(4104, 4, TK.FORM_STREAM) == [4, 256, 2048]


# ------------------------------------------------------------------ rows
def test_thousand_random_rows_against_python_integers_on_the_oracle():
    rng = np.random.default_rng(31)
    done = 0
    for V in (8, 16, 24, 64, 72, 256, 264, 520, 1000, 2048, 4104):
        for tb in (2, 4):
            n = 46 if V < 4104 else 40
            rows = TK.as_type(TK.random_rows(rng, n, V, spread=rng.choice((6.0, 30.0))), tb)
            ks = [k for k in (1, 2, 63, 64, 255, 256) if k <= V] + [min(V, 256)]
            for r0 in range(0, n, len(ks)):                    # each row at one k, every k in turn
                for i, k in enumerate(ks):
                    if r0 + i < n:
                        wb = int(rng.integers(0, 25))
                        K = (k + 3) // 4 * 4 if (r0 + i) % 2 else 256
                        _same(rows[r0 + i:r0 + i + 1], k, wb, K, ("random", V, tb))
                        done += 1
    assert done >= 1000


@pytest.mark.parametrize("tb", (2, 4))
@pytest.mark.parametrize("V", (8, 64, 520, 4104))
def test_rows_built_to_tie(V, tb):
    rng = np.random.default_rng(V + tb)
    for k in sorted({1, 3, min(64, V), min(256, V)}):
        for name, row in TK.special_rows(rng, V, k).items():
            rows = TK.as_type(row[None], tb)
            want_i, _ = TK.yardstick(rows, k, 24, 256)
            if name in ("flat", "all_neg_inf", "pos_inf", "all_nan"):          # all-tie rows: symbols 0 .. k - 1
                assert want_i[0, :k].tolist() == list(range(k)), name
            _same(rows, k, 24, (k + 3) // 4 * 4, name)
            _same(rows, k, 16, 256, name)
    # the deep row's threshold really falls inside a class of several levels
    if V == 520:
        row = TK.as_type(TK.special_rows(rng, V, 256)["deep_classes"][None], tb)
        g = oracle.q1_quantize(row, 61)[0]
        gstar = np.sort(g)[-256]
        f = row[0] if tb == 4 else (row[0].astype(np.uint32) << 16).view(np.float32)
        levels = {TK.native().tk_level(float(v), 0.0) for v in f[g == gstar]}
        assert len(levels) > 1 and (g == gstar).sum() > 1 and (g > gstar).sum() < 256


@pytest.mark.parametrize("tb", (2, 4))
@pytest.mark.parametrize("V", (64, 520, 4104))
def test_tie_classes_across_every_seam(V, tb):
    """The cut -- the last tie taken -- exactly at a thread, register-round, wave or tile seam, one
    entry before it and one after it; and survivors only in the row's last vector."""
    seen = 0
    for forced in (TK.FORM_REGS, TK.FORM_STREAM):
        for seam in TK.seams(V, tb, forced):
            for row, k in TK.seam_rows(V, seam):
                rows = TK.as_type(row[None], tb)
                _same(rows, k, 24, 256, ("seam", seam))
                seen += 1
    assert seen >= 6
    for k in (1, 3, 64):
        row, kk = TK.last_vector_row(V, tb, k)
        _same(TK.as_type(row[None], tb), kk, 24, (kk + 3) // 4 * 4, "last vector")


def test_seam_rows_tie_as_designed():
    """The seam rows' two tie logits weigh the same at different levels, in bf16 and in f32."""
    for tb in (2, 4):
        x = TK.as_type(np.array([0.0, -1.0, TK.TIE_A, TK.TIE_B, TK.LOW, TK.LOW, TK.LOW, TK.LOW], dtype=np.float32), tb)
        g = oracle.q1_quantize(x, 61).tolist()
        assert g[0] == 1 << 24 and g[2] == g[3] == 2 and g[4] == 1 and g[1] > 2


def test_sanitized_sweep_program(tk):
    """The sweep (the literal rule against the kernels' form under both plans, the literal threshold
    against the lanes' at every k) in the library, and as a stand-alone program under
    AddressSanitizer + UndefinedBehaviorSanitizer (host code only)."""
    n = TK.I64(0)
    assert tk.tk_sweep(12345, C.byref(n)) == 0 and n.value > 20000
    outdir = os.path.join(TK.NATIVE, "_asan")
    os.makedirs(outdir, exist_ok=True)
    exe = os.path.join(outdir, "topk_check_main")
    if TK.stale(exe, TK.SRC, *TK.HDRS):
        subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-DTOPK_CHECK_MAIN",
                        "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", *TK.INCS, TK.SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    report = r.stdout + r.stderr
    assert r.returncode == 0, report[-3000:]
    assert "topk_check: ok" in report and "ERROR" not in report and "runtime error" not in report
