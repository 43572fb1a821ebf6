"""Host check of the decode window's rules (lac_amd/csrc/lac_refill.h): the four predicates at
their edges and refill_stream_host -- lac_decode_refill for one stream in plain loops, the rules
k_dec_refill shares -- under a reader model: a reader that pulls k <= prec bits per step from the
window must read what a Python read_bits of the whole string gives at pos + 64 * base.

Compiles tests/native/refill_check.cpp (plain C++ over lac_refill.h) as a shared library and
tests/native/refill_main.cpp as a stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer; no GPU needed.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

NATIVE = os.path.join(REPO, "tests", "native")
SO = os.path.join(NATIVE, "librefillcheck.so")
SRC = os.path.join(NATIVE, "refill_check.cpp")
MAIN = os.path.join(NATIVE, "refill_main.cpp")
HDR = os.path.join(REPO, "lac_amd", "csrc", "lac_refill.h")
INCS = ["-I", os.path.join(REPO, "lac_amd", "csrc")]

IDLE, MOVED, DRY = 0, 1, 2
PRECS = (16, 24, 36, 48, 61)
EVERY = (1, 7, 64)
SENTINEL = 0xA5A5A5A5A5A5A5A5


def _stale(target, *deps):
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(d) for d in deps)


@pytest.fixture(scope="module")
def rc():
    if _stale(SO, SRC, HDR):
        subprocess.run(["hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", *INCS, SRC, "-o", SO], check=True)
    lib = C.CDLL(SO)
    u64, vp, i32 = C.c_uint64, C.c_void_p, C.c_int32
    lib.rc_stream_words.argtypes, lib.rc_stream_words.restype = [u64], u64
    lib.rc_bad_source.argtypes = [u64, u64, u64]
    lib.rc_held_bits.argtypes, lib.rc_held_bits.restype = [u64, u64, u64], u64
    lib.rc_complete.argtypes = [u64, u64, u64]
    lib.rc_ran_dry.argtypes = [u64, u64, C.c_int]
    lib.rc_drop_words.argtypes, lib.rc_drop_words.restype = [u64, C.c_int], u64
    lib.rc_open.argtypes = [vp, u64, u64, u64, u64, vp, vp]
    lib.rc_refill.argtypes = [vp, u64, u64, C.c_int, i32, u64, vp, vp]
    return lib


def bound_words(N, prec):
    """The smallest W with 64 W >= (N + 1) * prec + 63 (lac_refill.h, Sizing)."""
    return ((N + 1) * prec + 63 + 63) // 64


def read_bits(data: bytes, nbits, pos, k):
    """Bits [pos, pos + k) of a big-endian byte string as an integer, zeros at or past nbits."""
    v = 0
    for q in range(pos, pos + k):
        v = v << 1 | ((data[q >> 3] >> (7 - (q & 7))) & 1 if q < nbits else 0)
    return v


class Window:
    """One stream's source and window in arrays with a sentinel word on each side: the source has
    exactly nw words between its sentinels, the window exactly W."""

    def __init__(self, rc, rng, nw, nbits, W, prec, base=0):
        self.rc, self.nw, self.nbits, self.W, self.prec = rc, nw, nbits, W, prec
        self.src = np.full(nw + 2, SENTINEL, dtype=np.uint64)
        self.src[1:nw + 1] = rng.integers(0, 1 << 64, nw, dtype=np.uint64)
        self.whole = self.src[1:nw + 1].tobytes()
        self.win = np.full(W + 2, SENTINEL, dtype=np.uint64)
        self.st = np.array([base, 0, prec], dtype=np.uint64)      # base, held, pos
        held = C.c_uint64(0)
        self.opened = bool(rc.rc_open(self.src.ctypes.data + 8, 8 * nw, nbits, base, W, self.win.ctypes.data + 8,
                                      C.byref(held)))
        self.st[1] = held.value

    base = property(lambda s: int(s.st[0]))
    held = property(lambda s: int(s.st[1]))
    pos = property(lambda s: int(s.st[2]))

    def read(self, k):
        """k bits at pos from the window -> (value, the whole string's value); advances pos."""
        got = read_bits(self.win[1:self.W + 1].tobytes(), self.held, self.pos, k)
        want = read_bits(self.whole, self.nbits, self.pos + 64 * self.base, k)
        self.st[2] += np.uint64(k)
        return got, want

    def refill(self, err=0):
        r = self.rc.rc_refill(self.src.ctypes.data + 8, 8 * self.nw, self.nbits, self.prec, err, self.W,
                              self.win.ctypes.data + 8, self.st.ctypes.data)
        self.check_sentinels()
        return r

    def check_sentinels(self):
        assert self.win[0] == SENTINEL and self.win[-1] == SENTINEL, "a word outside the window slot was written"
        assert self.src[0] == SENTINEL and self.src[-1] == SENTINEL and self.src[1:self.nw + 1].tobytes() == self.whole


# ------------------------------------------------------------------ the predicates at their edges
def test_drop_words_edges(rc):
    for prec in PRECS:
        for d, g in ((0, 0), (1, 0), (63, 0), (64, 1), (65, 1), (127, 1), (128, 2), (64 * 1000 + 63, 1000)):
            pos = prec + d
            assert rc.rc_drop_words(pos, prec) == g
            assert prec <= pos - 64 * g <= prec + 63


def test_held_and_complete_edges(rc):
    W = 5
    for nbits in (0, 63, 64, 65, 64 * W, 64 * W + 1):
        nw = (nbits + 63) // 64
        assert rc.rc_stream_words(nbits) == nw
        assert rc.rc_held_bits(nbits, 0, W) == min(nbits, 64 * W)
        assert bool(rc.rc_complete(nbits, 0, W)) == (nbits <= 64 * W)
    assert rc.rc_held_bits(64 * W + 1, 1, W) == 64 * (W - 1) + 1      # one word on: the end comes into view
    assert rc.rc_complete(64 * W + 1, 1, W)
    for nw in (W + 3, 40):
        for last in (1, 64):                                          # a last word of 1 bit and a full one
            nbits = 64 * (nw - 1) + last
            assert rc.rc_complete(nbits, nw - W, W) and rc.rc_held_bits(nbits, nw - W, W) == nbits - 64 * (nw - W)
            assert not rc.rc_complete(nbits, nw - W - 1, W) and rc.rc_held_bits(nbits, nw - W - 1, W) == 64 * W
    assert rc.rc_held_bits(128, 2, W) == 0 and rc.rc_complete(128, 2, W)   # 64 * base == nbits: an empty window


def test_ran_dry_edges(rc):
    held = 64 * 5
    assert not rc.rc_ran_dry(held, held, 0)                           # the last bit read was held - 1
    assert rc.rc_ran_dry(held + 1, held, 0)
    assert not rc.rc_ran_dry(held + 1, held, 1) and not rc.rc_ran_dry(held + 10 ** 6, held, 1)
    assert not rc.rc_ran_dry(0, 0, 0) and rc.rc_ran_dry(1, 0, 0)


def test_bad_source(rc):
    assert not rc.rc_bad_source(64, 1, 8) and rc.rc_bad_source(65, 0, 8)      # nbits against 8 * stride
    assert not rc.rc_bad_source(127, 1, 16) and rc.rc_bad_source(127, 2, 16)  # 64 * base against nbits
    assert not rc.rc_bad_source(0, 0, 0) and rc.rc_bad_source(0, 1, 0)
    assert rc.rc_bad_source(1 << 40, 1 << 63, 1 << 40)                        # (no overflow of 64 * base)
    rng = np.random.default_rng(0)
    w = Window(rc, rng, 2, 200, 4, 48)                                        # 200 bits in a 128-bit slot
    assert not w.opened and (w.win[1:-1] == SENTINEL).all() and w.held == 0
    w.check_sentinels()
    assert w.refill() == IDLE and (w.win[1:-1] == SENTINEL).all()


# ------------------------------------------------------------------ the reader model
@pytest.mark.parametrize("N", EVERY)
@pytest.mark.parametrize("prec", PRECS)
def test_reader_reads_the_whole_string(rc, prec, N):
    rng = np.random.default_rng(1000 * prec + N)
    W = bound_words(N, prec)
    assert 64 * W >= (N + 1) * prec + 63 > 64 * (W - 1)
    moved = 0
    for nw in (0, 1, 2, W - 1, W, W + 1, 17, 40, int(rng.integers(0, 41)), int(rng.integers(0, 41))):
        nw = max(nw, 0)
        for nbits in sorted({64 * nw, max(64 * nw - 63, 0), max(64 * nw - int(rng.integers(0, 64)), 0)}):
            w = Window(rc, rng, nw, nbits, W, prec)
            assert w.opened
            assert read_bits(w.win[1:W + 1].tobytes(), w.held, 0, prec) == read_bits(w.whole, nbits, 0, prec)
            steps = 2 * nbits // (prec + 1) + 3 * N + 4                   # well past the stream's end
            for t in range(steps):
                k = prec if rng.integers(0, 4) == 0 else int(rng.integers(0, prec + 1))
                got, want = w.read(k)
                assert got == want, (nw, nbits, t)
                if (t + 1) % N == 0:
                    absolute = w.pos + 64 * w.base
                    r = w.refill()
                    assert r != DRY
                    assert w.pos + 64 * w.base == absolute and w.pos >= prec
                    if r == MOVED:
                        assert w.pos <= prec + 63
                        moved += 1
                    if 64 * nw > 64 * W and w.base + W >= nw:             # the window reached the end: it stays
                        assert w.held == nbits - 64 * w.base
            assert w.refill() != DRY
    assert moved > 0


@pytest.mark.parametrize("N", EVERY)
@pytest.mark.parametrize("prec", PRECS)
def test_one_word_below_the_bound_runs_dry(rc, prec, N):
    """From the worst position after a refill, prec + 63, N steps of k = prec end at
    (N + 1) * prec + 63 > 64 * (W - 1): one word below the bound the window is dry, flagged at the
    refill and left unchanged; at the bound the same steps are safe.  (With 64 bits the window
    cannot even hold position prec + 63, so the lead-in may already flag it.)"""
    rng = np.random.default_rng(7)
    for shrink in (0, 1):
        W = bound_words(N, prec) - shrink
        nw = W + 80
        w = Window(rc, rng, nw, 64 * nw - 5, W, prec)

        def checked_refill():
            before = (w.win.copy(), w.st.copy())
            absolute = w.pos + 64 * w.base
            r = w.refill()
            if r == DRY:
                assert (w.win == before[0]).all() and (w.st == before[1]).all()
            else:
                assert w.pos + 64 * w.base == absolute
            return r

        r, rem = IDLE, 63
        while rem > 0 and r != DRY:                                       # lead-in: (pos - prec) mod 64 = 63
            k = min(rem, prec)
            got, want = w.read(k)
            rem -= k
            r = checked_refill()
            assert r == DRY or got == want
        if r != DRY:
            assert w.pos == prec + 63
            reads = [w.read(prec) for _ in range(N)]
            r = checked_refill()
            if not shrink:
                assert all(g == v for g, v in reads)
        assert r == (DRY if shrink else MOVED)
        before = (w.win.copy(), w.st.copy())
        assert w.refill(err=-7) == IDLE                                   # a failed stream is left alone
        assert (w.win == before[0]).all() and (w.st == before[1]).all()


def test_open_at_a_base_and_past_the_end(rc):
    """A window opened mid-stream holds the words from base on; words at or past nw are zero and
    the word after the source is never read (it is a nonzero sentinel)."""
    rng = np.random.default_rng(3)
    W, prec = 6, 48
    for nw, nbits, base in ((10, 640, 3), (10, 601, 7), (10, 640, 10), (10, 577, 9), (1, 1, 0), (0, 0, 0)):
        w = Window(rc, rng, nw, nbits, W, prec, base=base)
        assert w.opened
        want = [int(w.src[1 + base + j]) if base + j < nw else 0 for j in range(W)]
        assert w.win[1:W + 1].tolist() == want
        assert w.held == min(nbits - 64 * base, 64 * W)
        w.check_sentinels()


def test_sanitized_reader_program(tmp_path):
    """tests/native/refill_main.cpp: the reader model over lac_refill.h as a stand-alone program
    built with AddressSanitizer + UndefinedBehaviorSanitizer (host code only, heap blocks of
    exactly nw and W words), run as a subprocess."""
    outdir = os.path.join(NATIVE, "_asan")
    os.makedirs(outdir, exist_ok=True)
    exe = os.path.join(outdir, "refill_main")
    if _stale(exe, MAIN, HDR):
        # host code only: the sanitizers are given to the host compilation alone
        subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g",
                        "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", *INCS, MAIN, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    report = r.stdout + r.stderr
    assert r.returncode == 0, report[-3000:]
    assert "refill_check: ok" in report and "ERROR" not in report and "runtime error" not in report
