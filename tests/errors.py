"""Fixtures and reference verdicts for the sticky per-stream error contract of include/lac.h
(tests/test_errors_host.py, tests/test_gpu_errors_encode.py, tests/test_gpu_errors_decode.py).

Everything here runs on the host.  A case is a batch of T = 130 steps in which some streams carry
exactly one defect -- a bad symbol, a bad table row, a zero-width symbol -- at a step drawn from
POSITIONS: the first, last and next-to-last steps of a 64-step block of k_encode and of a launch
chunk of the stats decode, so a whole block, a partial block and the final step are all covered.
The expected status of every stream comes from the C oracle (oracle.encode's OracleError(code,
step), cross-checked with lacref_encode_batch's status), never from the GPU; the expected bytes of
a clean stream, and of a failed stream's prefix, are the oracle's encode of those symbols.

The oracle builds a row's CDF before it looks at the symbol, coder_step (lac_amd/csrc/lac_dev.h)
tests the symbol first: with one defect per (stream, step) the two orders give the same verdict.
precedence_case() is the one fixture with two defects in a step; its expected codes are the order
include/lac.h documents.
"""
import ctypes as C
import functools

import numpy as np

from oracle import oracle, restate

LAC_E_ARG, LAC_E_SYMBOL_RANGE, LAC_E_ZERO_WIDTH, LAC_E_TABLE = -1, -3, -4, -5
LAC_E_DECODE_RANGE, LAC_E_CAPACITY = -6, -7

T_STEPS = 130
POSITIONS = (0, 1, 63, 64, 65, 127, 128, 129)
CUTS = ((0, 1), (1, 65), (65, 130))
SYM_KINDS = ("sym_neg", "sym_V", "sym_min", "sym_max")
KINDS32 = SYM_KINDS + ("zero_row", "zero_width")
KINDS64 = KINDS32 + ("u64_overflow", "u64_overflow_big")      # high words summing below 2^32, and not
BAD_SYMBOL = {"sym_neg": -1, "sym_min": -2 ** 31, "sym_max": 2 ** 31 - 1}   # sym_V: the vocabulary size
EXPECT_CODE = {"sym_neg": LAC_E_SYMBOL_RANGE, "sym_V": LAC_E_SYMBOL_RANGE, "sym_min": LAC_E_SYMBOL_RANGE,
               "sym_max": LAC_E_SYMBOL_RANGE, "zero_row": LAC_E_TABLE, "zero_width": LAC_E_ZERO_WIDTH,
               "u64_overflow": LAC_E_TABLE, "u64_overflow_big": LAC_E_TABLE, "none": 0}


class Case:
    """pmf [T, B, V] and sym [T, B] with the defects in, clean_pmf / clean_sym without them,
    streams: per stream (kind, flavour, position or -1)."""

    def __init__(self, bits, prec, V, pmf, sym, clean_pmf, clean_sym, streams, fudged_zero):
        self.bits, self.prec, self.V = bits, prec, V
        self.pmf, self.sym, self.clean_pmf, self.clean_sym = pmf, sym, clean_pmf, clean_sym
        self.streams = streams
        self.T, self.B = sym.shape
        self.fudged_zero = fudged_zero          # per stream: steps whose symbol has probability 0 on a fudged row
        self.capacity_bits = self.T * (prec + 2) + 256

    @property
    def failing(self):
        return [b for b, (k, _, _) in enumerate(self.streams) if k != "none"]

    @property
    def clean(self):
        return [b for b, (k, _, _) in enumerate(self.streams) if k == "none"]


# ------------------------------------------------------------------ tables
def _rows(rng, flavour, bits, prec, T, V):
    """T rows of one stream.  Flavours, by what the split-path encoder's block test makes of them
    (tests/straight_forms.py):
      t16    totals <= 2^16: with prec >= 32 no row can fudge (T <= w minp always), so a zero entry
             at the symbol is a true zero width; the u32 kernel's straight form / 't32'
      wide   entries in [2^31, 2^32) (bits 64): totals ~2^40 >= 2^32, never fudged; 'wide'
      ft     totals ~1.5 * 2^(prec-1), entries >= 2 except a lone 1 in every 13th row, which fudges
             that step: '+ft' and '+ft+exit'
      skew   one entry of 2^22 (never the symbol) among entries 1..3: ~21 bits per symbol, so 130
             steps outgrow a decode window sized for 32; T < 2^23 <= w minp at prec >= 32: no fudge
      fudge  prec 21: totals 2^20 + V/2 on even rows (tests/test_gpu_straight.py's shape; at
             V = 256 such a row fudges one step in ~8000) and ~1.5 * 2^20 on odd rows (fudged at
             about every other step), skewed, with zero entries and minp 1"""
    dt = np.uint32 if bits == 32 else np.uint64
    if flavour == "t16":
        return rng.integers(1, 256, size=(T, V)).astype(dt)
    if flavour == "wide":
        assert bits == 64
        return rng.integers(1 << 31, 1 << 32, size=(T, V)).astype(dt)
    if flavour == "skew":
        assert prec >= 32
        rows = rng.integers(1, 4, size=(T, V)).astype(dt)
        rows[:, V - 1] = 1 << 22
        return rows
    if flavour == "ft":
        lo = 1 << (prec - 1)
        e = lo // V
        rows = rng.integers(e, 2 * e, size=(T, V)).astype(dt)
        rows[::13, V - 1] = 1
        return rows
    if flavour == "fudge":
        assert prec == 21
        z = rng.normal(size=(T, V)) * 4.0
        p = np.exp(z - z.max(axis=1, keepdims=True))
        p /= p.sum(axis=1, keepdims=True)
        want = np.where(np.arange(T) % 2 == 0, (1 << 20) + V // 2, 3 << 19)
        q = np.floor(p * want[:, None]).astype(np.int64)          # (tiny probabilities: zero entries)
        ar = np.arange(T)
        big = q.argmax(axis=1)
        small = np.where(q > 0, q, np.iinfo(np.int64).max).argmin(axis=1)
        assert (small != big).all()
        q[ar, small] = 1                                          # minp 1
        q[ar, big] += want - q.sum(axis=1)                        # the total, exactly
        assert (q >= 0).all() and (q.sum(axis=1) == want).all() and (q == 0).any(axis=1).all()
        return q.astype(dt)
    raise ValueError(flavour)


def _walk_symbols(rng, rows, prec, flavour):
    """Symbols of positive probability for one stream; for the 'fudge' flavour a symbol of
    probability 0 wherever a row of the first block fudges at the coder's width there (legal:
    fudged_dist gives it width 1, arith_code.py:83-93; the later blocks keep positive symbols, so
    their fudged steps leave a straight block).  -> (symbols, steps that took such a symbol)."""
    T, V = rows.shape
    if flavour != "fudge":
        s = rng.integers(0, V - 1, size=T)                        # ('ft', 'skew': never the entry at V - 1)
        return s.astype(np.int32), []
    half, denom = 1 << (prec - 1), 1 << prec
    l, h = 0, denom - 1
    syms, zeros = [], []
    for t in range(T):
        row = [int(x) for x in rows[t]]
        cdf = restate.cdf_of(row)
        minp = restate.positive_min(cdf)
        w = h - l + 1
        if cdf[-1] > w * minp and t < 64:                         # fudged (arith_code.py:84)
            s = row.index(0)
            zeros.append(t)
        else:
            pos = [i for i, x in enumerate(row) if x > 0]
            s = pos[int(rng.integers(0, len(pos)))]
        lo, hi = restate.symbol_to_range(cdf, minp, s, w)
        assert hi > lo
        h = l + hi - 1
        l += lo
        while (h - l) < half:
            b = l // half
            l = l * 2 - b * denom
            h = h * 2 + 1 - b * denom
        syms.append(s)
    return np.array(syms, dtype=np.int32), zeros


def make_case(bits, prec, kind_by_stream, T=T_STEPS, V=256, seed=0):
    """kind_by_stream: per stream 'kind', 'kind:flavour' or ('kind[:flavour]', position); kinds
    are KINDS64 or 'none', flavours those of _rows (default t16), a missing position is drawn from
    POSITIONS.  Exactly one defect per failing stream; zero_width only on t16 rows with prec >= 32
    (a row that cannot fudge)."""
    rng = np.random.default_rng(seed)
    B = len(kind_by_stream)
    dt = np.uint32 if bits == 32 else np.uint64
    pmf = np.zeros((T, B, V), dtype=dt)
    sym = np.zeros((T, B), dtype=np.int32)
    streams, fz = [], []
    for b, spec in enumerate(kind_by_stream):
        kind, pos = spec if isinstance(spec, tuple) else (spec, None)
        kind, _, flavour = kind.partition(":")
        flavour = flavour or "t16"
        assert kind == "none" or kind in (KINDS32 if bits == 32 else KINDS64), kind
        rows = _rows(rng, flavour, bits, prec, T, V)
        pmf[:, b, :] = rows
        sym[:, b], zeros = _walk_symbols(rng, rows, prec, flavour)
        fz.append(zeros)
        if kind == "none":
            pos = -1
        elif pos is None:
            pos = POSITIONS[int(rng.integers(0, len(POSITIONS)))]
        streams.append((kind, flavour, pos))
    clean_pmf, clean_sym = pmf.copy(), sym.copy()
    for b, (kind, flavour, t) in enumerate(streams):
        if kind in SYM_KINDS:
            sym[t, b] = V if kind == "sym_V" else BAD_SYMBOL[kind]
        elif kind == "zero_row":
            pmf[t, b, :] = 0
        elif kind == "zero_width":
            assert flavour == "t16" and prec >= 32
            pmf[t, b, sym[t, b]] = 0
        elif kind == "u64_overflow":                              # total 2^64, high words sum 2^32 - 1
            pmf[t, b, :] = 0
            pmf[t, b, 3], pmf[t, b, V - 2] = 0x7FFFFFFFFFFFFFFF, 0x8000000000000001
        elif kind == "u64_overflow_big":                          # total 2^65, high words sum 2^33
            pmf[t, b, :] = 0
            pmf[t, b, ::V // 8] = 1 << 62
    return Case(bits, prec, V, pmf, sym, clean_pmf, clean_sym, streams, fz)


# ------------------------------------------------------------------ the reference verdict
def oracle_prefix(rows, syms, n, prec):
    """The oracle's (bytes, nbits) for the first n symbols of one stream."""
    data, nbits, _ = oracle.encode(rows[:max(n, 1)], syms[:n], prec)
    return data, nbits


def verdict(case, pmf=None, sym=None):
    """Per stream, from the C oracle: code, step (-1 when clean), and the (bytes, nbits) of the
    stream (clean) or of its first `step` symbols (failed); plus lacref_encode_batch's status."""
    pmf = case.pmf if pmf is None else pmf
    sym = case.sym if sym is None else sym
    code, step, data, nbits = [], [], [], []
    for b in range(case.B):
        rows, s = pmf[:, b, :], sym[:, b]
        try:
            d, n, _ = oracle.encode(rows, s, case.prec)
            c, t = 0, -1
        except oracle.OracleError as e:
            c, t = e.code, e.step
            d, n = oracle_prefix(rows, s, t, case.prec)
        code.append(c), step.append(t), data.append(d), nbits.append(n)
    _, _, status, rc = oracle.encode_batch(pmf, sym, case.prec)
    return {"code": np.array(code, dtype=np.int32), "step": np.array(step, dtype=np.int64), "data": data,
            "nbits": np.array(nbits, dtype=np.int64), "batch_status": status, "batch_rc": rc}


def first_code(code):
    """What lac_stream_status returns: the lowest-index failing stream's code."""
    bad = np.flatnonzero(code)
    return int(code[bad[0]]) if len(bad) else 0


def floor_encode(rows, syms, prec):
    """restate.encode_digits with Predictor.symbol_to_range's floor mapping (arith_code.py:69-70,
    a = floor(lo w / T), b = floor(hi w / T), no fudge) on the rows' CDF, then A_to_bin.flush and
    bytes(group_bits(bits())) -- LAC_MAP_FLOOR with LAC_TERM_FLUSH.  Raises on a zero width."""
    half, denom = 1 << (prec - 1), 1 << prec
    l, h = 0, denom - 1
    out = []
    for row, s in zip(rows, syms):
        cdf = restate.cdf_of(row)
        w = h - l + 1
        lo = (cdf[s - 1] * w) // cdf[-1] if s > 0 else 0
        hi = (cdf[s] * w) // cdf[-1]
        if hi <= lo:
            raise ZeroDivisionError("zero width under the floor mapping")
        h = l + hi - 1
        l += lo
        while (h - l) < half:
            b = l // half
            l = l * 2 - b * denom
            h = h * 2 + 1 - b * denom
            out.append(b)
    while l > 0 or h + 1 < denom:                                 # restate.encode_digits' flush, :193-202
        b = l // half
        if restate.region_overlap(l, h, b * half, (b + 1) * half) < \
           restate.region_overlap(l, h, (b + 1) * half, (b + 2) * half):
            b += 1
        l = l * 2 - b * denom
        h = h * 2 + 1 - b * denom
        out.append(b)
    R, L = restate.digits_to_int(out)
    return bytes(restate.group_bits(restate.int_to_bits(R, L))), L


# ------------------------------------------------------------------ the case lists
def _rot(kinds, k, flavours=("t16",)):
    out = []
    for j, kind in enumerate(kinds):
        fl = "t16" if kind == "zero_width" else flavours[(j + k) % len(flavours)]
        out.append((f"{kind}:{fl}", POSITIONS[(j + k) % len(POSITIONS)]))
    return out


@functools.lru_cache(maxsize=None)
def encode_cases(bits):
    """Eight rotations, so that every kind meets every position, plus the prec-21 case whose
    controls take probability-0 symbols on fudged rows.  Clean streams sit first, in the middle
    and last; bits 64 gives them (and the failing streams) the t16 / wide / ft flavours."""
    cases = []
    if bits == 32:
        for k in range(8):
            ks = _rot(KINDS32, k)
            spec = ["none"] + ks[:3] + ["none:ft"] + ks[3:] + ["none"]
            cases.append(make_case(32, 32, spec, seed=3200 + k))
    else:
        for k in range(8):
            ks = _rot(KINDS64, k, ("t16", "wide", "ft"))
            spec = ["none:wide"] + ks[:4] + ["none:ft"] + ks[4:] + ["none"]
            cases.append(make_case(64, 48, spec, seed=6400 + k))
    spec = ["none:fudge", ("sym_V:fudge", 64), "none:fudge", ("zero_row:fudge", 65), ("sym_neg:fudge", 1),
            "none:fudge"]
    cases.append(make_case(bits, 21, spec, seed=2100 + bits))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def encode_verdicts(bits):
    return tuple(verdict(c) for c in encode_cases(bits))


@functools.lru_cache(maxsize=None)
def clean_verdicts(bits):
    """The oracle's bytes of every stream of the cases' defect-free tables."""
    return tuple(verdict(c, c.clean_pmf, c.clean_sym) for c in encode_cases(bits))


@functools.lru_cache(maxsize=None)
def precedence_case():
    """Two defects in one step (bits 64): sym_V on a zero row, sym_V on a row of total 2^64, a
    zero-width symbol on a row of total 2^65.  include/lac.h: symbol range, then table, then zero
    width -> SYMBOL_RANGE, SYMBOL_RANGE, TABLE."""
    c = make_case(64, 48, ["none", ("zero_row", 64), ("u64_overflow", 65), "none:wide", ("u64_overflow_big", 1)],
                  seed=77)
    c.sym[64, 1] = c.V
    c.sym[65, 2] = c.V
    c.sym[1, 4] = 5                                              # a zero entry of that row
    assert c.pmf[1, 4, 5] == 0
    want = np.array([0, LAC_E_SYMBOL_RANGE, LAC_E_SYMBOL_RANGE, 0, LAC_E_TABLE], dtype=np.int32)
    return c, want, np.array([-1, 64, 65, -1, 1], dtype=np.int64)


# ------------------------------------------------------------------ capacity
class CapacityCase:
    pass


@functools.lru_cache(maxsize=None)
def capacity_case(bits=32, prec=32, T=T_STEPS, V=64, B=10, seed=5):
    """Clean tables and symbols whose streams' bit counts differ widely (a dominant symbol taken
    with a per-stream probability, else a uniform one), and a capacity of W words -- a context
    holds ceil(capacity_bits / 64) + 1 per stream (lac_open; BatchCoder.bits_stride() / 8, which
    the GPU test asserts) -- chosen from restate's digit counts so that
      (a) some streams fit, flush included;
      (b) some hold their symbols' digits (L <= 64 W) but not the flush (ceil((L + m) / 64) > W):
          finish_stream's own test (lac_dev.h: `nwords > cap_words`), LAC_E_CAPACITY, err_step T;
      (c) some overflow at a step: the first step whose digits take L past 64 W.  plane_append
          (lac_amd/csrc/lac_core.h) refuses exactly that -- its last line,
          `return ((L - 1) >> 6) < cap_words`, and the store test `if (idx >= cap_words) return
          false` in its loop -- and a step with no digits (`if (k <= 0) return true`) never fails."""
    rng = np.random.default_rng(seed)
    dt = np.uint32 if bits == 32 else np.uint64
    cand = []
    for i in range(400):
        rows = rng.integers(1, 16, size=(T, V)).astype(dt)
        rows[:, 0] = 1 << int(rng.integers(8, 20))
        q = float(rng.uniform(0.0, 1.0))
        s = np.where(rng.uniform(size=T) < q, 0, rng.integers(0, V, size=T)).astype(np.int32)
        trace = []
        dg = restate.encode_digits(rows, s, prec, stop=True, trace=trace)
        per = np.array([len(x) for x in trace], dtype=np.int64)
        L = int(per.sum())
        cand.append((rows, s, per, L, len(dg) - L))
        tight = [c for c in cand if c[3] > 128 and c[4] > 0 and (c[3] % 64 == 0 or (c[3] % 64) + c[4] > 64)]
        if tight and len(cand) >= 60:
            break
    assert tight, "no stream whose flush alone crosses a word"
    W = (tight[0][3] + 63) // 64

    def cls(c):
        L, m = c[3], c[4]
        return "a" if (L + m + 63) // 64 <= W else ("b" if L <= 64 * W else "c")
    by = {k: [c for c in cand if cls(c) == k] for k in "abc"}
    by["a"].sort(key=lambda c: c[3])
    by["c"].sort(key=lambda c: c[3])
    na = min(4, len(by["a"]))
    pick_a = [by["a"][i * (len(by["a"]) - 1) // max(na - 1, 1)] for i in range(na)]
    pick_b = by["b"][:2]
    nc = B - len(pick_a) - len(pick_b)
    pick_c = [by["c"][i * (len(by["c"]) - 1) // max(nc - 1, 1)] for i in range(nc)] if by["c"] else []
    order = []
    for i in range(max(len(pick_a), len(pick_b), len(pick_c))):   # interleaved: the classes as neighbours
        for lst, k in ((pick_c, "c"), (pick_a, "a"), (pick_b, "b")):
            if i < len(lst):
                order.append((lst[i], k))
    cc = CapacityCase()
    cc.bits, cc.prec, cc.V, cc.T, cc.B = bits, prec, V, T, len(order)
    cc.words = W
    cc.capacity_bits = 64 * (W - 1) - 13                          # ceil(capacity_bits / 64) + 1 == W
    cc.pmf = np.stack([c[0] for c, _ in order], axis=1)
    cc.sym = np.stack([c[1] for c, _ in order], axis=1)
    cc.cls = [k for _, k in order]
    code, step, data, nbits = [], [], [], []
    for (rows, s, per, L, m), k in order:
        if k == "a":
            d, n, _ = oracle.encode(rows, s, prec)
            assert n == L + m
            code.append(0), step.append(-1), data.append(d), nbits.append(n)
        else:
            over = np.flatnonzero(np.cumsum(per) > 64 * W)
            code.append(LAC_E_CAPACITY), step.append(T if k == "b" else int(over[0]))
            data.append(b""), nbits.append(0)
    cc.code, cc.step = np.array(code, dtype=np.int32), np.array(step, dtype=np.int64)
    cc.data, cc.nbits = data, np.array(nbits, dtype=np.int64)
    assert all(cc.cls.count(k) > 0 for k in "abc"), cc.cls
    return cc


# ------------------------------------------------------------------ decode fixtures
@functools.lru_cache(maxsize=None)
def decode_case(bits, prec, k=0, V=256, lean=False, flavour="t16"):
    """Clean tables to encode, and the tables to decode against: stream b's row at its position
    made bad -- an all-zero row, with bits 64 alternating with a total of 2^64 / 2^65 (k rotates
    the kinds over the positions).  Streams 0, 5 and 10 of the 11 stay clean, so every clean stream
    has a neighbour whose bad row sits one step ahead of some step it decodes.  flavour: the rows
    of every stream (_rows; 'skew' for the windowed run's long streams).  lean: B = 5 for the
    few-stream lean step; clean stream 1's rows 60..69 and stream 2's rows 60..62 have totals >= 2^32
    (u32 entries of 2^25), which the lean step leaves to k_decode_seq -- a legal hand-over -- before
    stream 2's bad row at 64."""
    if lean:
        spec = ["none", "none", ("zero_row", 64), ("zero_row", 129), ("zero_row", 0)]
    else:
        kinds = ("zero_row",) if bits == 32 else ("zero_row", "u64_overflow", "zero_row", "u64_overflow_big")
        bad = [(f"{kinds[(j + k) % len(kinds)]}:{flavour}", POSITIONS[j]) for j in range(len(POSITIONS))]
        none = f"none:{flavour}"
        spec = [none] + bad[:4] + [none] + bad[4:] + [none]
    c = make_case(bits, prec, spec, V=V, seed=9000 + bits + prec + k)
    if lean:
        for p in (c.pmf, c.clean_pmf):
            p[60:70, 1, :] = 1 << 25
            p[60:63, 2, :] = 1 << 25                              # (and stream 2 itself, just before its bad row)
        assert int(c.pmf[60, 1].astype(np.uint64).sum()) >= 1 << 32
        assert int(c.pmf[62, 2].astype(np.uint64).sum()) >= 1 << 32 and not c.pmf[64, 2].any()
    return c


# ------------------------------------------------------------------ device-side helpers (GPU tests)
def dev_pmf(pmf, dev):
    import torch
    it = np.int32 if pmf.dtype == np.uint32 else np.int64
    return torch.from_numpy(np.ascontiguousarray(pmf).view(it)).to(dev)


def dev_sym(sym, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(sym, dtype=np.int32)).to(dev)


def stream_bytes(c):
    """(per-stream bytes, nbits) of a finished coder, failed streams included (BatchCoder.to_bytes
    raises when any stream failed)."""
    n = c.lengths()
    s = c.bits_stride()
    host = np.zeros((c.streams, s), dtype=np.uint8)
    from lac_amd._lib import check
    check(c.lib.lac_copy_bits(c.ctx, host.ctypes.data_as(C.c_void_p), s, c._stream))
    return [host[b, :(int(n[b]) + 7) // 8].tobytes() for b in range(c.streams)], n.astype(np.int64)


def written(ck):
    """A checkpoint's planes with the words past each stream's L bits (never written: whatever the
    allocation held) zeroed."""
    p = ck["planes"].copy()
    for b, L in enumerate(ck["state"]["L"]):
        p[:, b, (int(L) + 63) // 64:] = 0
    return p


def dec_state(c):
    from lac_amd._lib import check
    from lac_amd.coder import _DEC_STATE
    st = np.zeros(c.streams, dtype=_DEC_STATE)
    check(c.lib.lac_decode_get_state(c.ctx, st.ctypes.data_as(C.c_void_p), c._stream))
    return st


def set_dec_state(c, st):
    from lac_amd._lib import check
    st = np.ascontiguousarray(st)
    check(c.lib.lac_decode_set_state(c.ctx, st.ctypes.data_as(C.c_void_p), c._stream))
