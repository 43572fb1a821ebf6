"""The coder's float-assisted divisions on the device: loader of tests/native/dev_arith.hip and the
seeded case generators of tests/test_gpu_arith.py and tests/test_arith_cases_host.py.

The library evaluates lac_core.h / lac_dec_dev.h primitives on arrays it owns, one case per thread
(``thread``) or one per wave (``wave``), compiled with lac_amd.build.FLAGS.  The generators are pure
Python: every expected value is a Python integer quotient (``cr_ratio``: CPython's ``a / b``).

Every case carries labels, the classes of input at which these routines can be wrong:

    rem_qd, rem_qd_m1, rem_qd_dm1   n*m + add = q*d, q*d - 1, q*d + d - 1
    tgt_edge                        targets at v = ceil(c*w/T) and at that minus 1, integer c
    c_edge                          ranges at c in {0, 1, T - 1, T}
    mod_edge                        ranges at c with c*w mod T in {0, 1, T - 1}
    q_ceil                          the form's largest quotients (2^50 - 1, 2^50, 2^32 - 1, 2^63, 2^64 - 1)
    thr                             a form threshold: prec 50 / 51, T at 2^50, 2^32, 2^62, 2^63,
                                    w at 2^(prec-1) + 1 and 2^prec -- the side the form admits
    pow2                            divisors 2^k and 2^k +- j, j < 1024
    round53                         divisors 2^53 +- 1 and larger odd ones, where (double)d rounds
    worst                           divisors at which the device reciprocal is furthest off (the
                                    sweep of tests/test_gpu_arith.py picks them; without a device,
                                    seeded stand-ins), crossed with q_ceil and the remainder edges
    random

``census`` counts cases per label; CLASSES names what each family must hold.
"""
import ctypes as C
import functools
import math
import os
import random
import struct
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "dev_arith.hip")
SO = os.path.join(REPO, "tests", "native", "libdevarith.so")

INV_RECIP, INV_RECIP_SMALL, INV_RECIP2_SMALL, INV_IEEE = range(4)
(T_RECIP, T_RECIP_SMALL, T_F64_SMALL, T_DIV_FLOOR, T_DIV_SMALL, T_DIV_NEAR, T_DIV_MID, T_FRAC, T_RANGES, T_FUDGE,
 T_IS_FUDGED, T_CR_RATIO, T_FIX) = range(13)
W_SMALL_U, W_SMALL_U2, W_NEAR_U, W_NEAR_U2, W_MID_U2, W_FRAC_UNI, W_DIV_PAIR, W_FRAC_PAIR, W_FIX = range(9)
N_IN, N_OUT = 6, 4
M64 = (1 << 64) - 1
NOFRAC = M64
SWEEP_L = (16, 24, 32, 40, 49, 50)                              # divisor bit lengths of the reciprocal sweep


def compile_command(out=SO):
    """hipcc with exactly the product's flags and include paths (lac_amd.build)."""
    from lac_amd import build as lbuild
    return ["hipcc", *lbuild.FLAGS, *lbuild._incs(), "-shared", SRC, "-o", out]


def build(force=False):
    from lac_amd import build as lbuild
    deps = [SRC, *lbuild.HEADERS]
    if force or not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(compile_command(), check=True)
    return SO


def load():
    """tests/native/dev_arith.hip as a ctypes library (compiled when older than its sources)."""
    lib = C.CDLL(build())
    pp = C.POINTER(C.c_void_p)
    for f in (lib.da_thread, lib.da_wave):
        f.restype = C.c_int
        f.argtypes = [C.c_int, C.c_int, C.c_int64, pp, pp]
    a, b = C.c_int(), C.c_int()
    lib.da_limits(C.byref(a), C.byref(b))
    assert (a.value, b.value) == (N_IN, N_OUT)
    return lib


def u64(xs):
    return np.ascontiguousarray(np.array(xs, dtype=np.uint64))


def _run(fn, fam, inv, ins, nout):
    ins = [u64(x) for x in ins]
    n = len(ins[0])
    assert 0 < len(ins) <= N_IN and nout <= N_OUT and all(len(x) == n for x in ins)
    outs = [np.zeros(n, dtype=np.uint64) for _ in range(nout)]
    pin = (C.c_void_p * N_IN)(*[x.ctypes.data for x in ins])
    pout = (C.c_void_p * N_OUT)(*[x.ctypes.data for x in outs])
    rc = fn(fam, inv, n, pin, pout)
    assert rc == 0, f"HIP status {rc} (family {fam}, inv {inv})"
    return outs


def thread(lib, fam, ins, nout, inv=INV_RECIP):
    """One case per thread -> nout uint64 arrays."""
    return _run(lib.da_thread, fam, inv, ins, nout)


def wave(lib, fam, ins, nout, inv=INV_RECIP):
    """One case per wave (the wave-uniform wrappers) -> nout uint64 arrays."""
    return _run(lib.da_wave, fam, inv, ins, nout)


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


# ------------------------------------------------------------------ the reciprocal sweep's divisors
def splitmix(x):
    """splitmix64 over a uint64 array (tools/rcp_probe.hip's mix)."""
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def sweep_divisors(L, n_even=1 << 20, n_end=1024, n_rand=1 << 18, n_top=1 << 18):
    """Divisors of bit length L: n_even evenly spaced over [2^(L-1), 2^L), n_end at each end, and
    n_rand of tools/rcp_probe.hip's random family cut to L bits (top bit set), n_top more at the top."""
    lo, hi = 1 << (L - 1), 1 << L
    span = hi - lo
    if span <= n_even:
        even = np.arange(lo, hi, dtype=np.uint64)
    else:
        even = (np.uint64(lo) + (np.arange(n_even, dtype=np.uint64) * np.uint64(span // n_even)))
    ends = np.concatenate([np.arange(lo, min(hi, lo + n_end), dtype=np.uint64),
                           np.arange(max(lo, hi - n_end), hi - 1, dtype=np.uint64),
                           np.array([hi - 1], dtype=np.uint64)])
    r = splitmix(splitmix(np.arange(n_rand, dtype=np.uint64) + np.uint64(L << 32)))
    rnd = (r >> np.uint64(64 - L)) | np.uint64(lo)
    # just under the power of two, where one Newton step leaves the largest error: the last
    # 1/4096 of the range again at n_top evenly spaced divisors
    top = np.zeros(0, dtype=np.uint64)
    if span // 4096 > n_top:
        top = np.uint64(hi - span // 4096) + np.arange(n_top, dtype=np.uint64) * np.uint64(span // 4096 // n_top)
    return np.unique(np.concatenate([even, ends, rnd, top]))


def ulps_off(got_bits, want):
    """Signed distance in ulps of positive doubles given as bit patterns from the float64 array `want`."""
    return got_bits.view(np.int64) - want.view(np.int64)


def stand_in_worst(seed=7):
    """{L: divisors} where no device chose them: seeded divisors of each length, the ends included."""
    rng = random.Random(seed)
    out = {}
    for L in SWEEP_L + (64,):
        lo, hi = 1 << (L - 1), 1 << L
        out[L] = sorted({lo + 1, hi - 1, hi - 3, *[rng.randrange(lo + 1, hi) for _ in range(29)]})
    return out


# ------------------------------------------------------------------ cases
class Cases:
    """rows: [tuple of int] in the order of `names`; labels: [frozenset of str]; shape: [str]
    ("target" / "range" for the decoder's forms, else "")."""

    def __init__(self, names):
        self.names = names
        self.rows, self.labels, self.shape = [], [], []

    def add(self, row, labels, shape=""):
        self.rows.append(tuple(row))
        self.labels.append(frozenset(labels))
        self.shape.append(shape)

    def __len__(self):
        return len(self.rows)

    def col(self, k):
        k = self.names.index(k) if isinstance(k, str) else k
        return [r[k] for r in self.rows]

    def cols(self):
        return [self.col(k) for k in range(len(self.names))]

    def census(self):
        n = {}
        for ls in self.labels:
            for c in ls:
                n[c] = n.get(c, 0) + 1
        return dict(sorted(n.items()))

    def select(self, pred):
        out = Cases(self.names)
        for r, ls, s in zip(self.rows, self.labels, self.shape):
            if pred(r, ls, s):
                out.add(r, ls, s)
        return out


CLASSES = {
    "small": "rem_qd rem_qd_m1 rem_qd_dm1 tgt_edge c_edge mod_edge q_ceil thr pow2 worst random".split(),
    "near32": "rem_qd rem_qd_m1 rem_qd_dm1 tgt_edge c_edge mod_edge q_ceil thr pow2 worst random".split(),
    "near64": "rem_qd rem_qd_m1 rem_qd_dm1 tgt_edge c_edge mod_edge q_ceil thr pow2 worst random".split(),
    "mid": "rem_qd rem_qd_m1 rem_qd_dm1 c_edge mod_edge q_ceil thr pow2 round53 worst random".split(),
    "floor": "rem_qd rem_qd_m1 rem_qd_dm1 q_ceil pow2 round53 worst random".split(),
    "frac": "c_edge mod_edge q_ceil thr pow2 worst random".split(),
    "ranges": "c_edge mod_edge q_ceil thr pow2 round53 worst random".split(),
    "fudge": "c_edge q_ceil pow2 worst random".split(),
    "ratio": "c_edge pow2 round53 worst random".split(),
}
# The forms' documented operand bounds (lac_core.h, lac_dec_dev.h): name -> (T range, largest prec)
FORMS = {
    "small": (1, (1 << 50) - 1, 50),        # div_small: T < 2^50, prec <= 50
    "near32": (1, (1 << 32) - 1, 50),       # div_near on u32 rows
    "near64": (1, (1 << 50) - 1, 50),       # div_near on u64 rows below 2^50
    "mid": (1 << 50, M64, 50),              # div_mid: u64 rows of 2^50 and more
}


def _near_pow2(rng, lo, hi, n):
    """n values 2^k + j, |j| < 1024, inside [lo, hi], every admissible k first."""
    ks = [k for k in range(0, 65) if lo <= (1 << k) + 1023 and (1 << k) - 1023 <= hi]
    out = []
    for k in ks:
        for j in (0, 1, -1):
            out.append((1 << k) + j)
    while len(out) < n:
        out.append((1 << rng.choice(ks)) + rng.randint(-1023, 1023))
    return [x for x in out if lo <= x <= hi]


def _w_of(rng, prec):
    return rng.choice([(1 << (prec - 1)) + 1, 1 << prec, (1 << prec) - 1,
                       rng.randint((1 << (prec - 1)) + 1, 1 << prec)])


def _mod_c(c_mod, w, T):
    """c in [0, T] with c*w mod T == c_mod mod T: for 0 the smallest positive one, T / gcd(w, T);
    None where there is none (1 and T - 1 need w invertible mod T)."""
    g = math.gcd(w, T)
    if c_mod % T == 0:
        return T // g
    if g != 1:
        return None
    return (c_mod % T) * pow(w, -1, T) % T


@functools.lru_cache(maxsize=None)
def _decoder_cases(form, worst_key, scale):
    worst = dict(worst_key)
    Tlo, Thi, pmax = FORMS[form]
    rng = random.Random({"small": 1, "near32": 2, "near64": 3, "mid": 4}[form])
    cs = Cases(["n", "m", "add", "d", "addd"])
    targets = form != "mid"

    def rng_T():
        return rng.choice([rng.randint(Tlo, Thi), rng.randint(Tlo, min(Thi, max(Tlo, 1 << 20))), Thi,
                           min(Thi, max(Tlo, (1 << rng.randint(1, 64)) + rng.randint(-3, 3)))])

    def put_range(c, w, T, ceil, *labels):
        assert 0 <= c <= T and Tlo <= T <= Thi
        add = T - 1 if ceil else 0
        cs.add((c, w, add, T, f64_bits(float(T)) if ceil else 0), set(labels), "range")

    def put_target(v, T, w, *labels):
        assert 0 <= v < w and Tlo <= T <= Thi
        cs.add((v, T, 0, w, 0), set(labels), "target")

    def put_rem_edges(T, w, *labels):
        # c = T: n*m + add = w*T (rem 0), w*T + T - 1, and w*T - 1 = (w - 1)*T + T - 1
        put_range(T, w, T, False, "rem_qd", *labels)
        put_range(T, w, T, True, "rem_qd_dm1", *labels)
        put_range(T, w - 1, T, True, "rem_qd_m1", *labels)

    def light(T, w, *labels):
        """The top of one (T, w): the remainder edges at c = T, and c = T - 1."""
        put_rem_edges(T, w, *labels)
        if T > 1:
            put_range(T - 1, w, T, True, "c_edge", *labels)
        if targets:
            put_target(w - 1, T, w, "tgt_edge", *labels)

    def family(T, w, *labels):
        """Every decoder-shape edge of one (T, w)."""
        for ceil in (True, False):
            for c in (0, 1, T - 1, T):
                if 0 <= c <= T:
                    put_range(c, w, T, ceil, "c_edge", *labels)
            for cm in (0, 1, -1):
                c = _mod_c(cm, w, T)
                if c is not None:
                    put_range(c, w, T, ceil, "mod_edge", *labels)
        put_rem_edges(T, w, *labels)
        if targets:
            for c in (1, T // 2, T - 1, T, rng.randint(0, T)):
                v = -(-(c * w) // T)
                for vv in (v, v - 1):
                    if 0 <= vv < w:
                        put_target(vv, T, w, "tgt_edge", *labels)
            put_target(w - 1, T, w, "tgt_edge", *labels)
            put_target(0, T, w, *labels, "tgt_edge")

    n_each = int(250 * scale)
    # T | w*c with factors in common: c*w mod T = 0 away from c = 0 and c = T
    for _ in range(n_each * 4):
        prec = rng.randint(8, pmax)
        t1 = rng.randint(2, 1 << (prec // 2))
        t2lo = max(1, -(-Tlo // t1))
        t2 = rng.randint(t2lo, max(t2lo, min(Thi // t1, t2lo + (1 << 40))))
        T, w = t1 * t2, t1 * rng.randint(((1 << (prec - 1)) // t1) + 1, (1 << prec) // t1)
        if Tlo <= T <= Thi and (1 << (prec - 1)) < w <= (1 << prec):
            for ceil in (True, False):
                put_range(t2 * rng.randint(1, t1), w, T, ceil, "mod_edge")
    # quotient ceilings: c = T so q = w, w at the top of prec 50 (2^50, 2^50 - 1) and at its bottom
    for _ in range(n_each):
        T = rng_T()
        for w in ((1 << 50), (1 << 50) - 1, (1 << 49) + 1):
            family(T, w, "q_ceil", "thr")
    if form == "near32":                                         # u32 targets: quotients at 2^32 - 1 (generic operands)
        for _ in range(n_each * 4):
            w = _w_of(rng, rng.randint(33, 50))
            for q in ((1 << 32) - 1, (1 << 32) - 2):
                cs.add((q, w, 0, w, 0), {"q_ceil", "rem_qd"}, "target")
                cs.add((q, w, w - 1, w, 0), {"q_ceil", "rem_qd_dm1"}, "target")
    # thresholds in T (the side this form admits) and in w at every prec
    for T in {Tlo, Tlo + 1, Thi, Thi - 1, *[t for t in ((1 << 32) - 1, 1 << 32, (1 << 50) - 1, 1 << 50, (1 << 62) - 1,
                                                        1 << 62, (1 << 63) - 1, 1 << 63) if Tlo <= t <= Thi]}:
        for prec in range(2, pmax + 1):
            for w in ((1 << (prec - 1)) + 1, 1 << prec):
                family(T, w, "thr")
    # divisor mantissas: T and w at 2^k +- j
    for T in _near_pow2(rng, Tlo, Thi, n_each):
        family(T, _w_of(rng, rng.randint(2, pmax)), "pow2")
        family(T, _w_of(rng, pmax), "pow2")
    if targets:
        for w in _near_pow2(rng, 3, 1 << pmax, n_each):
            prec = max(2, (w - 1).bit_length())
            if (1 << (prec - 1)) < w <= (1 << prec) and prec <= pmax:
                family(rng_T(), w, "pow2")
    if form == "mid":
        for _ in range(n_each):
            T = rng.choice([(1 << 53) + 1, (1 << 53) - 1, (1 << rng.randint(53, 63)) + 2 * rng.randint(0, 1 << 20) + 1,
                            M64 - 2 * rng.randint(0, 1 << 20), rng.randint(1 << 53, M64) | 1])
            family(T, _w_of(rng, rng.randint(40, pmax)), "round53")
    # worst-reciprocal divisors as T (ranges; the targets' 1/w too) crossed with everything above
    for L, ds in sorted(worst.items()):
        for d in ds:
            if Tlo <= d <= Thi:
                family(d, 1 << 50, "worst", "q_ceil")
                for w in ((1 << 50) - 1, (1 << 49) + 1, _w_of(rng, 50), _w_of(rng, 49), _w_of(rng, rng.randint(2, 48))):
                    light(d, w, "worst", "q_ceil")
                    for k in (2, 3, rng.randint(2, 4096)):
                        if d - k >= 0:
                            put_range(d - k, w, d, True, "worst")
            if targets and 2 <= L <= pmax and (1 << (L - 1)) < d <= (1 << L):
                family(Thi, d, "worst", "q_ceil")
                for T in (Thi - 1, rng_T(), rng_T()):
                    light(T, d, "worst", "q_ceil")
    # random
    while len(cs) < int(200000 * scale):
        T, w = rng_T(), _w_of(rng, rng.randint(2, pmax))
        put_range(rng.randint(0, T), w, T, rng.random() < 0.7, "random")
        if targets:
            put_target(rng.randint(0, w - 1), T, w, "random")
    return cs


def decoder_cases(form, worst=None, scale=1.0):
    """The decode step's quotients floor((n*m + add)/d) of one form (FORMS): shape "target"
    (v, T, 0, w) and "range" (c, w, T - 1 or 0, T), columns n, m, add, d, addd (bits of the
    addend as div_mid_est_w takes it)."""
    worst = stand_in_worst() if worst is None else worst
    return _decoder_cases(form, tuple(sorted((L, tuple(ds)) for L, ds in worst.items())), scale)


def quotients(cs):
    return [(r[0] * r[1] + r[2]) // r[3] for r in cs.rows]


def check_decoder_preconditions(form, cs):
    """The documented bounds of a form's primitive on every case; returns the largest quotient."""
    Tlo, Thi, pmax = FORMS[form]
    top = 0
    for (n, m, add, d, addd), shape in zip(cs.rows, cs.shape):
        q = (n * m + add) // d
        top = max(top, q)
        assert add < d and d > 0
        assert q <= 1 << 50                                     # (2^50 itself: c = T at w = 2^50, the decoder reaches it)
        if form == "mid":
            assert shape == "range" and n < 1 << 64 and m <= 1 << 51 and d < 1 << 64
        else:
            assert n < 1 << 52 and m < 1 << 52 and add < 1 << 52 and d <= 1 << 50
        if shape == "range":
            assert n <= d and Tlo <= d <= Thi and m <= 1 << pmax
            assert addd == f64_bits(float(d)) if add else addd in (0, f64_bits(float(d)))   # (T = 1: add = T - 1 = 0)
        elif form == "near32":
            assert q < 1 << 32
    return top


@functools.lru_cache(maxsize=None)
def _floor_cases(worst_key, scale):
    """div_floor / div_floor_inv: N < 2^128, any d, quotient < 2^64 -> columns nh, nl, d."""
    worst = dict(worst_key)
    rng = random.Random(5)
    cs = Cases(["nh", "nl", "d"])

    def put(q, d, r, *labels):
        N = q * d + r
        assert 0 <= r < d and q <= M64 and N >> 128 == 0
        cs.add((N >> 64, N & M64, d), labels)

    def edges(q, d, *labels):
        put(q, d, 0, "rem_qd", *labels)
        put(q, d, d - 1, "rem_qd_dm1", *labels)
        if q:
            put(q - 1, d, d - 1, "rem_qd_m1", *labels)
        put(q, d, rng.randrange(0, d), *labels)

    tops = [M64, M64 - 1, M64 - 2, 0xFFFFFFFFFFFFF800, 0xFFFFFFFFFFFFF7FF, 0xFFFFFFFFFFFFF801, 1 << 63, (1 << 63) - 1,
            (1 << 50), (1 << 50) - 1, (1 << 32) - 1]

    def rq():
        return rng.choice([rng.randrange(0, 1 << 64), M64 - rng.randrange(0, 1 << 12), rng.randrange(0, 1 << 48),
                           rng.randrange(0, 1 << rng.choice([8, 32, 47, 61, 62, 63, 64]))])

    def rd():
        return rng.choice([1, 3, rng.randrange(1, 1 << 20), rng.randrange(1, 1 << 47), rng.randrange(1, 1 << 64),
                           M64 - rng.randrange(0, 1 << 10), (1 << 63) + rng.randrange(0, 1 << 10)])

    n_each = int(1500 * scale)
    for _ in range(n_each):
        d = rd()
        for q in tops:
            edges(q, d, "q_ceil")
    for d in _near_pow2(rng, 1, M64, n_each * 2):
        edges(rq(), d, "pow2")
        edges(rng.choice(tops), d, "pow2", "q_ceil")
    for _ in range(n_each):
        d = rng.choice([(1 << 53) + 1, (1 << 53) - 1, (1 << rng.randint(53, 63)) + 2 * rng.randint(0, 1 << 20) + 1,
                        M64 - 2 * rng.randint(0, 1 << 20), rng.randint(1 << 53, M64) | 1])
        edges(rq(), d, "round53")
        edges(rng.choice(tops), d, "round53", "q_ceil")
    for L, ds in sorted(worst.items()):
        for d in ds:
            for q in tops + [rq() for _ in range(4)]:
                edges(q, d, "worst", "q_ceil")
    while len(cs) < int(200000 * scale):
        d = rd()
        put(rq(), d, rng.randrange(0, d), "random")
    return cs


def floor_cases(worst=None, scale=1.0):
    worst = stand_in_worst() if worst is None else worst
    return _floor_cases(tuple(sorted((L, tuple(ds)) for L, ds in worst.items())), scale)


@functools.lru_cache(maxsize=None)
def _frac_cases(worst_key, scale):
    """row_frac + frac_mul_div: columns c, w, T, ceil; c <= T, prec <= 61.  T up to 2^64 - 1 (rows of
    2^63 and more have no fraction: kNoFrac)."""
    worst = dict(worst_key)
    rng = random.Random(6)
    cs = Cases(["c", "w", "T", "ceil"])

    def family(T, w, *labels):
        for ceil in (0, 1):
            for c in (0, 1, T - 1, T):
                if 0 <= c <= T:
                    cs.add((c, w, T, ceil), {"c_edge", *labels} | ({"q_ceil"} if c == T else set()))
            for cm in (0, 1, -1):
                c = _mod_c(cm, w, T)
                if c is not None:
                    cs.add((c, w, T, ceil), {"mod_edge", *labels})
            cs.add((rng.randint(0, T), w, T, ceil), set(labels))

    n_each = int(600 * scale)
    thr = [(1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 62) - 1, 1 << 62, (1 << 62) + 1, (1 << 63) - 1, 1 << 63,
           (1 << 63) + 1, M64, (1 << 50) - 1, 1 << 50, 1, 2, 3]
    for T in thr:
        for prec in range(2, 62):
            for w in ((1 << (prec - 1)) + 1, 1 << prec):
                family(T, w, "thr")
    for T in _near_pow2(rng, 1, M64, n_each * 2):
        family(T, _w_of(rng, rng.randint(2, 61)), "pow2")
        family(T, _w_of(rng, 61), "pow2")
    for L, ds in sorted(worst.items()):
        for d in ds:
            for prec in (61, 60, 50, 49, rng.randint(2, 61)):
                for w in ((1 << (prec - 1)) + 1, 1 << prec, _w_of(rng, prec)):
                    family(d, w, "worst")
    while len(cs) < int(200000 * scale):
        T = rng.choice([rng.randrange(1, 1 << 20), rng.randrange(1, 1 << 32), rng.randrange(1, 1 << 40),
                        rng.randrange(1, 1 << 62), rng.randrange(1, 1 << 63), (1 << 63) - rng.randrange(1, 1000),
                        (1 << 62) - rng.randrange(1, 1000), (1 << 32) - rng.randrange(1, 1000)])
        cs.add((rng.randint(0, T), _w_of(rng, rng.randint(2, 61)), T, rng.randint(0, 1)), {"random"})
    return cs


def frac_cases(worst=None, scale=1.0):
    worst = stand_in_worst() if worst is None else worst
    return _frac_cases(tuple(sorted((L, tuple(ds)) for L, ds in worst.items())), scale)


def frac_want(c, w, T, ceil):
    """-> (row_frac, frac_mul_div<false>, frac_mul_div<true>, frac_mul_div32) as the harness reports them."""
    q = -(-(c * w) // T) if ceil else c * w // T
    if T >> 63:
        return NOFRAC, NOFRAC, NOFRAC, NOFRAC
    f = (1 << 63) if c >= T else (c << 63) // T
    return f, q, (NOFRAC if T >> 62 else q), (NOFRAC if (T >> 32 or c > T) else q)


@functools.lru_cache(maxsize=None)
def _range_cases(worst_key, scale):
    """unfudged_range_inv / floor_range / div_pair: lo <= hi <= T < 2^64, any prec <= 61 -> columns
    lo, hi, T, w.  Holds the far side of the small forms' thresholds (prec 51, T = 2^50, T = 2^32)."""
    worst = dict(worst_key)
    rng = random.Random(8)
    cs = Cases(["lo", "hi", "T", "w"])

    def family(T, w, *labels):
        for lo, hi in ((0, 1), (0, T), (T - 1, T), (1, T - 1), (T, T), (0, 0)):
            if 0 <= lo <= hi <= T:
                cs.add((lo, hi, T, w), {"c_edge", *labels} | ({"q_ceil"} if hi == T else set()))
        ms = [c for c in (_mod_c(cm, w, T) for cm in (0, 1, -1)) if c is not None]
        if ms:
            cs.add((min(ms), max(ms), T, w), {"mod_edge", *labels})
            cs.add((ms[0], T, T, w), {"mod_edge", *labels})
        a, b = sorted((rng.randint(0, T), rng.randint(0, T)))
        cs.add((a, b, T, w), set(labels))

    n_each = int(600 * scale)
    for T in [(1 << 32) - 1, 1 << 32, (1 << 50) - 1, 1 << 50, (1 << 62) - 1, 1 << 62, (1 << 63) - 1, 1 << 63, M64, 1, 2]:
        for prec in range(2, 62):
            for w in ((1 << (prec - 1)) + 1, 1 << prec):
                family(T, w, "thr")
    for T in _near_pow2(rng, 1, M64, n_each * 2):
        family(T, _w_of(rng, rng.randint(2, 61)), "pow2")
    for _ in range(n_each):
        T = rng.choice([(1 << 53) + 1, (1 << 53) - 1, (1 << rng.randint(53, 63)) + 2 * rng.randint(0, 1 << 20) + 1,
                        M64 - 2 * rng.randint(0, 1 << 20), rng.randint(1 << 53, M64) | 1])
        family(T, _w_of(rng, rng.randint(40, 61)), "round53")
    for L, ds in sorted(worst.items()):
        for d in ds:
            for prec in (61, 51, 50, 49, rng.randint(2, 61)):
                for w in ((1 << (prec - 1)) + 1, 1 << prec, _w_of(rng, prec)):
                    family(d, w, "worst")
    while len(cs) < int(150000 * scale):
        T = rng.choice([rng.randrange(1, 1 << 20), rng.randrange(1, 1 << 47), rng.randrange(1, 1 << 64),
                        M64 - rng.randrange(0, 1 << 10)])
        a, b = sorted((rng.randint(0, T), rng.randint(0, T)))
        cs.add((a, b, T, _w_of(rng, rng.randint(2, 61))), {"random"})
    return cs


def range_cases(worst=None, scale=1.0):
    worst = stand_in_worst() if worst is None else worst
    return _range_cases(tuple(sorted((L, tuple(ds)) for L, ds in worst.items())), scale)


@functools.lru_cache(maxsize=None)
def _fudge_cases(worst_key, scale):
    """fudge_x + fudge_f: columns i, c, j, T, w, V (X = c*w - j*T; c <= T, j < V <= 2^(prec-1) < w), and
    is_fudged's minp as column minp."""
    worst = dict(worst_key)
    rng = random.Random(9)
    cs = Cases(["i", "c", "j", "T", "w", "V", "minp"])

    def family(T, prec, *labels):
        w = _w_of(rng, prec)
        V = rng.choice([2, 1 << (prec - 1), rng.randint(2, 1 << (prec - 1))])
        for c in (0, 1, T - 1, T, rng.randint(0, T)):
            if not 0 <= c <= T:
                continue
            for j in (0, V - 1, rng.randrange(0, V)):
                ls = {*labels} | ({"c_edge"} if c in (0, 1, T - 1, T) else set()) | ({"q_ceil"} if c == T and j == 0 else set())
                minp = rng.choice([1, max(1, T // w), T // w + 1, rng.randint(1, max(1, T))])
                cs.add((rng.randrange(0, V), c, j, T, w, V, minp), ls)

    n_each = int(800 * scale)
    for T in _near_pow2(rng, 1, M64, n_each * 2):
        family(T, rng.randint(2, 61), "pow2")
    for L, ds in sorted(worst.items()):
        for d in ds:
            for prec in (61, 50, rng.randint(2, 61)):
                family(d, prec, "worst")
    while len(cs) < int(100000 * scale):
        family(rng.choice([rng.randrange(1, 1 << 20), rng.randrange(1, 1 << 47), rng.randrange(1, 1 << 64)]),
               rng.randint(2, 61), "random")
    return cs


def fudge_cases(worst=None, scale=1.0):
    worst = stand_in_worst() if worst is None else worst
    return _fudge_cases(tuple(sorted((L, tuple(ds)) for L, ds in worst.items())), scale)


def fudge_want(i, c, j, T, w, V, minp):
    """-> (fudge_f, X low word, X high word, is_fudged)."""
    X = c * w - j * T
    g = max(1, min(w - V + 1, X // T))
    return i + g, X & M64, (X >> 64) & M64, int(T > w * minp)


@functools.lru_cache(maxsize=None)
def _ratio_cases(worst_key, scale):
    """cr_ratio: 0 <= a <= b, 0 < b < 2^63 -> columns a, b."""
    worst = dict(worst_key)
    rng = random.Random(23)
    cs = Cases(["a", "b"])

    def family(b, *labels):
        for a in (0, b, b - 1, 1, b // 2, b // 3 + 1, rng.randrange(0, b + 1), rng.randrange(0, b + 1)):
            a = max(0, min(a, b))
            cs.add((a, b), {*labels} | ({"c_edge"} if a in (0, 1, b - 1, b) else set()))

    n_each = int(1500 * scale)
    for b in _near_pow2(rng, 1, (1 << 63) - 1, n_each * 2):
        family(b, "pow2")
    for _ in range(n_each):
        family(rng.choice([(1 << 53) + 1, (1 << 53) - 1, (1 << rng.randint(53, 62)) + 2 * rng.randint(0, 1 << 20) + 1,
                           (1 << 63) - 1 - 2 * rng.randint(0, 1 << 20), rng.randint(1 << 53, (1 << 63) - 1) | 1]), "round53")
    for L, ds in sorted(worst.items()):
        for d in ds:
            if d < 1 << 63:
                family(d, "worst")
    while len(cs) < int(100000 * scale):
        family(rng.choice([rng.randrange(1, 1 << 20), rng.randrange(1, 1 << 53), rng.randrange(1 << 53, 1 << 63)]), "random")
    return cs


def ratio_cases(worst=None, scale=1.0):
    worst = stand_in_worst() if worst is None else worst
    return _ratio_cases(tuple(sorted((L, tuple(ds)) for L, ds in worst.items())), scale)


# ------------------------------------------------------------------ the reciprocal sweep
def run_sweep(lib, keep=64):
    """Every reciprocal path over sweep_divisors(L), L in SWEEP_L (and 64 for recip), against numpy's
    correctly rounded 1.0 / float64(d) -> (stats, worst): stats[(function, L)] = {n, ulp_min, ulp_max,
    rel_min, rel_max (relative error in units of 2^-52), at_min, at_max (divisors)}; worst[L] = the
    `keep` divisors furthest off in each direction (by relative error of recip / recip_small)."""
    stats, worst = {}, {}

    def note(name, L, d, got_bits, ref):
        ul = ulps_off(got_bits, ref)
        rel = (got_bits.view(np.float64) - ref) / ref * 2.0 ** 52
        stats[(name, L)] = dict(n=len(d), ulp_min=int(ul.min()), ulp_max=int(ul.max()), rel_min=float(rel.min()),
                                rel_max=float(rel.max()), at_min=int(d[rel.argmin()]), at_max=int(d[rel.argmax()]))
        return rel

    for L in SWEEP_L + (64,):
        d = sweep_divisors(L)
        dd = d.astype(np.float64)
        ref = 1.0 / dd
        r, ieee, conv = thread(lib, T_RECIP, [d], 3)
        rel = note("recip", L, d, r, ref)
        note("ieee_div", L, d, ieee, ref)
        stats[("u64_to_f64", L)] = dict(n=len(d), mismatches=int((conv != dd.view(np.uint64)).sum()))
        order = np.argsort(rel, kind="stable")
        picks = set(d[order[:keep]].tolist()) | set(d[order[-keep:]].tolist())
        if L <= 50:
            rs, r2, sconv = thread(lib, T_RECIP_SMALL, [d], 3)
            rel_s = note("recip_small", L, d, rs, ref)
            note("recip2_small", L, d, r2, ref)
            stats[("small_to_f64", L)] = dict(n=len(d), mismatches=int((sconv != dd.view(np.uint64)).sum()))
            order = np.argsort(rel_s, kind="stable")
            picks |= set(d[order[:keep]].tolist()) | set(d[order[-keep:]].tolist())
        worst[L] = sorted(picks)
    return stats, worst
