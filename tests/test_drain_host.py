"""Host check of the drain rules (lac_amd/csrc/lac_drain.h): which words of an open stream are
settled, drain_stream_host -- lac_encode_drain for one stream in plain loops, the rules
k_enc_drain shares -- and a host copy of finish_stream's add, against oracle/restate.py.

Compiles tests/native/drain_check.cpp (plain C++ over lac_drain.h and lac_core.h); no GPU needed.
The planes are filled by plane_append from restate.encode_digits' per-symbol digits; the drained
bytes followed by the finished tail must be restate.encode_bytes' bytes.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO
from oracle import restate

NATIVE = os.path.join(REPO, "tests", "native")
SO = os.path.join(NATIVE, "libdraincheck.so")
SRC = os.path.join(NATIVE, "drain_check.cpp")
INCS = ["-I", os.path.join(REPO, "lac_amd", "csrc"), "-I", os.path.join(REPO, "include")]
DEPS = [SRC, os.path.join(REPO, "include", "lac.h")] + [os.path.join(REPO, "lac_amd", "csrc", h)
                                                        for h in ("lac_drain.h", "lac_core.h")]

LAC_OK = 0
ONES = (1 << 64) - 1
SENTINEL = 0xA5
PRECS = (16, 24, 36, 48, 61)


def _stale(target):
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(d) for d in DEPS)


@pytest.fixture(scope="module")
def dc():
    if _stale(SO):
        subprocess.run(["hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", *INCS, SRC, "-o", SO], check=True)
    lib = C.CDLL(SO)
    u64, i64, vp, i32 = C.c_uint64, C.c_int64, C.c_void_p, C.c_int32
    lib.dc_is_guard.argtypes = [u64, u64]
    lib.dc_is_certain.argtypes = [i64, i64, C.c_int]
    lib.dc_slot_fits.argtypes = [u64, u64, u64]
    lib.dc_block_carries.argtypes, lib.dc_block_carries.restype = [u64, u64, u64, vp], u64
    lib.dc_flush_digits.argtypes = [i64, i64, C.c_int, vp]
    lib.dc_run.argtypes = [C.c_int, i64, vp, vp, vp, vp, vp, u64, u64, vp, u64, vp, vp, vp]
    lib.dc_drain.argtypes, lib.dc_drain.restype = [i64, i64, C.c_int, i32, i32, vp, vp, vp, vp, u64, vp], u64
    lib.dc_finish.argtypes, lib.dc_finish.restype = [i64, i64, C.c_int, vp, vp, vp, u64, vp, vp, vp], i64
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------ traces from the reference
def trace_stream(rows, symbols, prec):
    """Per symbol (E, k, l, h): the digits restate.encode_digits emits for it as one integer and
    their count, and the registers after it (the reference's own update, arith_code.py:169-186)."""
    tr = []
    restate.encode_digits(rows, symbols, prec, stop=False, trace=tr)
    R = restate._Rows(rows)
    denom = 1 << prec
    l, h = 0, denom - 1
    E, K, Ls, Hs = [], [], [], []
    for i, s in enumerate(symbols):
        cdf, minp = R.get(i)
        lo, hi = restate.symbol_to_range(cdf, minp, s, h - l + 1)
        h = l + hi - 1
        l += lo
        e = 0
        for d in tr[i]:
            l = l * 2 - d * denom
            h = h * 2 + 1 - d * denom
            e = e * 2 + d
        E.append(e), K.append(len(tr[i])), Ls.append(l), Hs.append(h)
    return (np.array(E, dtype=np.uint64), np.array(K, dtype=np.int32), np.array(Ls, dtype=np.int64),
            np.array(Hs, dtype=np.int64))


def make_stream(family, prec, seed):
    rng = np.random.default_rng(seed)
    if family == "random":                                    # a fresh random row per step
        V = int(rng.integers(2, 201))
        n = 300
        rows = rng.integers(1, 1000, (n, V)).tolist()
        syms = rng.integers(0, V, n).tolist()
    elif family == "peaky":                                   # one heavy symbol, coded most of the time
        V = int(rng.integers(2, 201))
        n = 600
        row = [1] * V
        peak = int(rng.integers(0, V))
        row[peak] = 1 << min(20, prec - 9)
        rows = [row]
        syms = [peak if rng.random() < 0.9 else int(rng.integers(0, V)) for _ in range(n)]
    else:                                                     # uniform table, one symbol 97 % of the time
        V = 2 if seed % 2 else 4
        n = 3000
        rows = [[1] * V]
        main = 0 if family == "const_first" else V - 1
        syms = [main if rng.random() < 0.97 else int(rng.integers(0, V)) for _ in range(n)]
    return rows, syms


def run(dc, prec, tr, drains, cap_words, stage_bytes):
    E, K, Ls, Hs = tr
    n = len(E)
    dr = np.ascontiguousarray(drains, dtype=np.uint8)
    out = np.zeros(n * (prec + 2) // 8 + 64 + 8 * cap_words, dtype=np.uint8)
    nbytes, nbits = C.c_uint64(), C.c_uint64()
    stats = np.zeros(4, dtype=np.uint64)
    rc = dc.dc_run(prec, n, _p(E), _p(K), _p(Ls), _p(Hs), _p(dr), cap_words, stage_bytes, _p(out), out.size,
                   C.byref(nbytes), C.byref(nbits), _p(stats))
    return rc, out[:nbytes.value].tobytes(), nbits.value, stats


@pytest.fixture(scope="module")
def streams():
    """The reference side, computed once: (family, prec, trace, reference bytes, bit count)."""
    out = []
    for family in ("random", "peaky", "const_first", "const_last"):
        for prec in PRECS:
            for seed in range(3):
                rows, syms = make_stream(family, prec, 100 * prec + seed)
                want, L = restate.encode_bytes(rows, syms, prec)
                out.append((family, prec, trace_stream(rows, syms, prec), want, L))
    return out


# ------------------------------------------------------------------ the arithmetic
def test_rule_tests_and_block_carries(dc):
    assert not dc.dc_is_guard(0, 0) and not dc.dc_is_guard(ONES, 0) and not dc.dc_is_guard(ONES - 4, 4)
    assert not dc.dc_is_guard(ONES, 1)                        # wraps to 0
    assert dc.dc_is_guard(1, 0) and dc.dc_is_guard(ONES, 2) and dc.dc_is_guard(ONES - 1, 0)
    assert dc.dc_is_certain(0, (1 << 48) - 1, 48) and not dc.dc_is_certain(0, 1 << 48, 48)
    assert not dc.dc_is_certain(-1, 5, 48) and dc.dc_is_certain(7, 9, 16)
    assert dc.dc_slot_fits(2, 0, 16) and not dc.dc_slot_fits(3, 0, 16) and dc.dc_slot_fits(1, 8, 16)
    assert not dc.dc_slot_fits(1, 16, 16) and not dc.dc_slot_fits(1, 24, 16) and not dc.dc_slot_fits(1, 4, 64)
    assert not dc.dc_slot_fits(ONES, 0, 64)
    rng = np.random.default_rng(5)
    for _ in range(2000):
        gen = int(rng.integers(0, 1 << 63)) & int(rng.integers(0, 1 << 63)) | (int(rng.integers(0, 2)) << 63)
        prop = (int(rng.integers(0, 1 << 63)) | (1 << 63)) & ~gen & ONES
        if rng.random() < 0.3:
            prop = ~gen & ONES
        cin = int(rng.integers(0, 2))
        want, c = 0, cin
        for j in range(64):
            want |= c << j
            c = ((gen >> j) & 1) | (((prop >> j) & 1) & c)
        cout = C.c_uint64(9)
        assert dc.dc_block_carries(gen, prop, cin, C.byref(cout)) == want and cout.value == c


# ------------------------------------------------------------------ parity with the reference
@pytest.mark.parametrize("schedule", ["every", "every64", "random"])
def test_drained_streams_equal_the_reference(dc, streams, schedule):
    neg_flush = moved = longer = 0
    kept = {}
    for i, (family, prec, tr, want, L) in enumerate(streams):
        n = len(tr[0])
        if schedule == "every":
            drains, gap = np.ones(n, np.uint8), 1
        elif schedule == "every64":
            drains, gap = (np.arange(1, n + 1) % 64 == 0), 64
        else:
            rng = np.random.default_rng(i)
            drains, gap = (np.arange(1, n + 1) % 50 == 0) | (rng.random(n) < 0.1), 50
        # planes for what `gap` symbols can add plus the words a drain keeps: far below the stream
        cap_words = (gap * (prec + 2) + 256) // 64 + 12
        rc, got, nbits, stats = run(dc, prec, tr, drains, cap_words, 8 * cap_words)
        assert rc == LAC_OK, (family, prec, rc)
        assert got == want and nbits == L, (family, prec, schedule)
        neg_flush += int(stats[2]) < 8
        moved += int(stats[1])
        kept[family] = max(kept.get(family, 0), int(stats[0]))
        longer += L > 64 * cap_words                          # the stream does not fit the planes undrained
    assert moved > 100 and longer >= len(streams) // 3
    assert neg_flush >= 1, "no stream of the set ends in a flush with a -1 digit"
    # with both rules a drain keeps a few words, whatever the stream's length
    assert max(kept.values()) <= 8, kept


def test_undrained_host_planes_equal_the_reference(dc, streams):
    """The checker's own planes and finish (no drain) are the reference's bytes: what the drained
    runs are compared with is not the drain's own output."""
    for family, prec, tr, want, L in streams[::4]:
        n = len(tr[0])
        rc, got, nbits, _ = run(dc, prec, tr, np.zeros(n, np.uint8), n * (prec + 2) // 64 + 8, 8)
        assert rc == LAC_OK and got == want and nbits == L, (family, prec)


# ------------------------------------------------------------------ crafted planes
def find_negative_flush(dc, prec, seed=0):
    """Registers a coder reaches (width in (2^(prec-1), 2^prec], 0 <= l < 2^prec) whose flush has
    a -1 digit and that are not certain."""
    rng = np.random.default_rng(seed)
    D, Hd = 1 << prec, 1 << (prec - 1)
    fd = np.zeros(8, dtype=np.int8)
    for _ in range(20000):
        w = Hd + 1 + int(rng.integers(0, Hd))
        l = int(rng.integers(0, D))
        h = l + w - 1
        m = dc.dc_flush_digits(l, h, prec, _p(fd))
        if m > 0 and -1 in fd[:m].tolist() and h >= D:
            return l, h, fd[:m].tolist()
    raise AssertionError("no registers with a -1 flush digit found")


def drain_and_finish(dc, l, h, prec, L, wa, wc, words_a, words_c, stride=None, fill0=0, err=0, nflush=-1):
    """-> (g, drained bytes + finished tail, bit count, undrained finish bytes, its bit count,
    state after the drain)."""
    cap = len(words_a) + 2
    pa = np.zeros(cap, dtype=np.uint64)
    pc = np.zeros(cap, dtype=np.uint64)
    pa[:len(words_a)] = words_a
    pc[:len(words_c)] = words_c
    wlast = (L - 1) >> 6 if L else 0
    pa[wlast], pc[wlast] = wa, wc
    lw = np.array([L, wa, wc], dtype=np.uint64)
    fd, nfd = np.zeros(8, dtype=np.int8), C.c_int32()
    ref = np.zeros(8 * cap, dtype=np.uint8)
    Lref = dc.dc_finish(l, h, prec, _p(lw), _p(pa), _p(pc), cap, _p(ref), _p(fd), C.byref(nfd))
    assert Lref >= 0
    stride = 8 * cap if stride is None else stride
    buf = np.full(16 + stride + 16, SENTINEL, dtype=np.uint8)
    fill = C.c_uint64(fill0)
    before = (lw.copy(), pa.copy(), pc.copy())
    g = dc.dc_drain(l, h, prec, err, nflush, _p(lw), _p(pa), _p(pc), _p(buf[16:]), stride, C.byref(fill))
    assert fill.value == fill0 + 8 * g
    slot = buf[16:16 + stride]
    assert (buf[:16] == SENTINEL).all() and (buf[16 + stride:] == SENTINEL).all()
    assert (slot[:fill0] == SENTINEL).all() and (slot[fill.value:] == SENTINEL).all()
    if g == 0:
        assert all(np.array_equal(x, y) for x, y in zip(before, (lw, pa, pc)))
    tail = np.zeros(8 * cap, dtype=np.uint8)
    Lt = dc.dc_finish(l, h, prec, _p(lw), _p(pa), _p(pc), cap, _p(tail), _p(fd), C.byref(nfd))
    assert Lt >= 0
    got = slot[fill0:fill.value].tobytes() + tail[:(Lt + 7) // 8].tobytes()
    return g, got, 8 * 8 * g + Lt, ref[:(Lref + 7) // 8].tobytes(), Lref, (lw, pa, pc)


PREC = 48
OPEN = ((1 << PREC) - 10, (1 << PREC) - 10 + (1 << (PREC - 1)) + 5)      # h >= 2^prec: not certain
CERTAIN = (5, (1 << (PREC - 1)) + 100)


def test_all_ones_between_guard_and_pending_carry(dc):
    # active word: 20 bits written, all ones, and a pending C bit on the last of them: the carry
    # runs through the all-ones words into the guard word, and from a wrapping guard into word 0
    L = 4 * 64 + 20
    wa, wc = 0xFFFFF << 44, 1 << 44
    for guard_a, guard_c in ((0x1234, 0), (ONES - 0xF, 0x20)):
        g, got, nb, want, Lref, (lw, pa, pc) = drain_and_finish(
            dc, *OPEN, PREC, L, wa, wc, [5, guard_a, ONES, ONES, 0], [0, guard_c, 0, 0, 0])
        assert g == 1 and got == want and nb == Lref
        assert lw[0] == L - 64 and pa[0] == (guard_a + guard_c) & ONES and pc[0] == 0
        assert pa[1] == ONES and pa[3] == wa and pc[3] == wc and lw[1] == wa and lw[2] == wc
        assert got[:8] == (5 + ((guard_a + guard_c) >> 64)).to_bytes(8, "big")
    # the same planes in a certain state: everything below the active word goes, resolved
    g, got, nb, want, Lref, (lw, pa, pc) = drain_and_finish(
        dc, *CERTAIN, PREC, L, wa, wc, [5, 0x1234, ONES, ONES, 0], [0, 0, 0, 0, 0])
    assert g == 4 and got == want and nb == Lref
    assert got[:32] == (5).to_bytes(8, "big") + (0x1235).to_bytes(8, "big") + bytes(16)
    assert lw[0] == 20 and lw[1] == 0 and lw[2] == 0 and pa[0] == 0 and pc[0] == 0


@pytest.mark.parametrize("off", [63, 64, 20])
def test_zero_words_before_a_negative_flush(dc, off):
    l, h, digits = find_negative_flush(dc, PREC)
    assert -1 in digits
    L = 4 * 64 + off                                          # off 63 / 64: the flush digits straddle / start a word
    wa = 0x5 << 61
    g, got, nb, want, Lref, (lw, pa, pc) = drain_and_finish(
        dc, l, h, PREC, L, wa, 0, [0x77, 0x10, 0, 0, 0], [0, 0, 0, 0, 0])
    assert g == 1 and got == want and nb == Lref              # stops at the guard: the zero words stay
    assert lw[0] == L - 64 and pa[0] == 0x10 and pa[1] == 0 and pa[2] == 0


def test_guard_at_word_zero_drains_nothing(dc):
    L = 3 * 64 + 9
    g, got, nb, want, Lref, _ = drain_and_finish(dc, *OPEN, PREC, L, 0x1FF << 55, 1 << 55,
                                                 [0x99, ONES, ONES - 3, 0], [0, 0, 3, 0])
    assert g == 0 and got == want and nb == Lref
    # no guard at all below the active word
    g, got, nb, want, Lref, _ = drain_and_finish(dc, *OPEN, PREC, L, 0x3 << 55, 0, [0, 0, ONES, 0], [0, 0, 0, 0])
    assert g == 0 and got == want


@pytest.mark.parametrize("regs,want_g", [(OPEN, 1), (CERTAIN, 2)])
def test_length_a_multiple_of_64(dc, regs, want_g):
    L = 3 * 64                                                # the active word is full
    g, got, nb, want, Lref, (lw, pa, pc) = drain_and_finish(dc, *regs, PREC, L, ONES - 1, 1, [7, 0x42, 0], [0, 0, 0])
    assert g == want_g and got == want and nb == Lref and lw[0] == L - 64 * want_g
    if regs is CERTAIN:
        assert lw[1] == ONES and lw[2] == 0 and pa[0] == ONES and pc[0] == 0


@pytest.mark.parametrize("L", [0, 1, 37, 64])
def test_at_most_one_word_drains_nothing(dc, L):
    wa = (ONES << (64 - L)) & ONES if L else 0
    g, got, nb, want, Lref, _ = drain_and_finish(dc, *CERTAIN, PREC, L, wa, 0, [0], [0])
    assert g == 0 and got == want and nb == Lref


def test_failed_and_finished_streams_drain_nothing(dc):
    planes = ([5, 0x1234, 0], [0, 0, 0])
    assert drain_and_finish(dc, *CERTAIN, PREC, 140, 0xABC << 52, 0, *planes)[0] == 2
    assert drain_and_finish(dc, *CERTAIN, PREC, 140, 0xABC << 52, 0, *planes, err=-3)[0] == 0
    assert drain_and_finish(dc, *CERTAIN, PREC, 140, 0xABC << 52, 0, *planes, nflush=0)[0] == 0


def test_short_slot_is_all_or_nothing(dc):
    L, wa = 4 * 64 + 20, 0xABCDE << 44
    planes = ([5, 0x1234, ONES, 0x77, 0], [0, 0, 0, 0, 0])
    # three words settle (the guard is word 3): 24 bytes behind 8 already there need a 32-byte slot
    g, got, nb, want, Lref, _ = drain_and_finish(dc, *OPEN, PREC, L, wa, 0, *planes, stride=24, fill0=8)
    assert g == 0 and got == want                              # (drain_and_finish: state and slot untouched)
    g, got, nb, want, Lref, _ = drain_and_finish(dc, *OPEN, PREC, L, wa, 0, *planes, stride=32, fill0=8)
    assert g == 3 and got == want and nb == Lref
    g = drain_and_finish(dc, *OPEN, PREC, L, wa, 0, *planes, stride=32, fill0=12)[0]      # fill no multiple of 8
    assert g == 0


# ------------------------------------------------------------------ under the sanitizers
def test_drain_rules_under_sanitizers():
    """The same checker as a stand-alone program (its own main: seeded random streams coded with
    and without drains) built with AddressSanitizer + UndefinedBehaviorSanitizer, host code only,
    run as a subprocess."""
    outdir = os.path.join(NATIVE, "_asan")
    os.makedirs(outdir, exist_ok=True)
    exe = os.path.join(outdir, "drain_check")
    if _stale(exe):
        # host code only: the sanitizers are given to the host compilation alone
        subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g",
                        "-Xarch_host", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                        "-DDRAIN_CHECK_MAIN", *INCS, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    report = r.stdout + r.stderr
    assert r.returncode == 0, report[-3000:]
    assert "drain_check: ok" in report and "ERROR" not in report and "runtime error" not in report
