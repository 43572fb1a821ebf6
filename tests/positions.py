"""Where in a row the kernels' arithmetic changes: the element indices a test has to code to
meet every block, segment, slot and word boundary of every kernel form that takes the row.

Host only.  The structure is read from the selection code (lac_amd/csrc/lac_select.h) through
tests/native/select_check.cpp -- the plan of every live row-statistics shape in both directions,
the one-position step's plan, the decode plan and the lean chunk layout -- so a changed form
moves the positions with it; nothing here restates a capacity.

A boundary at element e is exercised by the two entries e - 1 and e: with e a multiple of the
16-byte vector, the last entry of one vector and the first of the next.  ``Positions.pos`` maps
each element index to its labels ``(class, side)``, side "below" (e - 1) or "above" (e); the row
ends 0, 1, V - 2, V - 1 carry the class "row_end".

Logits rows (``logits_positions``), boundaries in 16-byte vectors of the row or, for the forms
that cut a row into segments, of the segment:

    row_end     0, 1, V - 2, V - 1
    group       64-vector groups (decode's totals): every group of rows of <= 4096 vectors; for
                longer rows the three groups around every other boundary and the last two
    mult256     rows of > 4096 vectors: every multiple of 256 vectors
    chunk       decode chunk starts (groups_per_chunk groups)
    run         a thread's next vector: multiples of nt (k_q1_stats_rl), of kQ1WideThreads
                (k_q1_stats_wide)
    slot_step   registers -> LDS slots: kRLRegVec * nt; kQ1WideMaxVec
    last_slot   the trimmed last slot: (kRLRegVec + kRLSlots - 1) * nt and + lastn
    tile        tile starts 64 * RW * R of the tiled forms
    step_wave   64 * R: the fused one-position step's waves
    segment     j * split of the group forms

Integer tables (``pmf_positions``), boundaries in elements:

    row_end, iter (64 * vec), lean_chunk (lean_chunk_layout_n, where decode_plan takes
    k_decode_lean), fine_wave (64 * vec * NR),
    block_wave (64 * vec * NW, NW = 4 / 8 / 16)

A row budget thins classes in a fixed order (``Positions.thinned`` names those it cut): the
first two and last three boundaries of a thinned class always stay, the rest are sampled evenly.
For logits only mult256 may be thinned; rows that do not fit the device budget at once are coded
in successive batches.

``logits_case`` / ``pmf_case`` are the parametrisations of tests/test_gpu_positions_*.py: the
positions, their rows and the [steps, B, V] layout within the tests' memory budget.
tests/test_positions_host.py asserts their census without a GPU.
"""
import ctypes as C
import os
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(REPO, "tests", "native", "libselectcheck.so")
_SRC = os.path.join(REPO, "tests", "native", "select_check.cpp")

LIVE = (1, 2, 3, 4, 6, 8, 10, 14, 15, 17, 18, 19, 20, 21, 22, 23)
TILED, RL, WIDE, RL_GROUP, WIDE_GROUP = range(5)
Q1_FIELDS = ("shape family rw r multi pf nwb rep lastn nt wide_slots k split nrb rep16 repair "
             "groups_per_chunk tiled_shape").split()
LAYOUT_CONSTS = "kRLRegVec kRLSlots kQ1WideThreads kQ1WideMaxVec kQ1WideSlotMaxVec kQ1StepMaxVec".split()
# the one logits class a row budget may thin: the plain multiples of 256 vectors
LOGITS_THIN = ("mult256",)
PMF_THIN = ("iter", "fine_wave", "block_wave", "lean_chunk")
# the kinds of row of tests/test_gpu_positions_logits.py
KINDS = ("plain", "sole_max", "nan_ninf", "pinf_neighbour", "capped_pair", "signed_zero_max")


class Plan(dict):
    __getattr__ = dict.__getitem__


def load_select():
    """tests/native/select_check.cpp as a ctypes library (compiled when stale)."""
    hdr = os.path.join(REPO, "lac_amd", "csrc", "lac_select.h")
    deps = [_SRC, hdr, os.path.join(REPO, "include", "lac.h")]
    if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(REPO, "lac_amd", "csrc"),
                        "-I", os.path.join(REPO, "include"), _SRC, "-o", _SO], check=True)
    lib = C.CDLL(_SO)
    i64p = C.POINTER(C.c_int64)
    lib.sc_q1_plan.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, i64p]
    lib.sc_q1_group.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, i64p]
    lib.sc_q1_slot_cap.restype = C.c_int64
    lib.sc_q1_slot_cap.argtypes = [C.c_int, C.c_int]
    lib.sc_consts.argtypes = [i64p]
    lib.sc_layout_consts.argtypes = [i64p]
    lib.sc_layout_consts.restype = None
    lib.sc_q1_step_plan.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_int, i64p]
    lib.sc_q1_step_plan.restype = None
    lib.sc_lean_chunks.argtypes = [C.c_int64, C.c_int, C.c_int, i64p]
    lib.sc_lean_chunks.restype = None
    lib.sc_decode_plan.argtypes = [i64p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                   C.c_int64, i64p]
    lib.sc_decode_plan.restype = None
    buf = (C.c_int64 * len(LAYOUT_CONSTS))()
    lib.sc_layout_consts(buf)
    lib.L = Plan(zip(LAYOUT_CONSTS, buf))
    return lib


def q1_plan(sel, V, type_bytes, dec, cus, shape=0):
    """The row-statistics plan, or None where q1_plan refuses the shape for the row."""
    o = (C.c_int64 * 18)()
    return Plan(zip(Q1_FIELDS, o)) if sel.sc_q1_plan(cus, V, type_bytes, int(dec), shape, o) == 0 else None


def step_plan(sel, V, type_bytes, cus, streams=1):
    """The fused one-position step's plan (AUTO at `streams` streams), or None where it does not take the row."""
    o = (C.c_int64 * 4)()
    sel.sc_q1_step_plan(cus, V, type_bytes, streams, 0, o)
    return Plan(fused=o[0], rc=o[1], threads=o[2], R=o[3]) if o[0] else None


class Positions:
    """pos: {element: {(class, side)}}; classes: every class the row has; thinned: the classes the
    budget cut; segments: [(first, last)] elements of every group form's segments; shapes: the
    forced shapes that take the row; census(): positions per class."""

    def __init__(self, V):
        self.V = V
        self.pos = {}
        self.classes = set()
        self.thinned = ()
        self.segments = []
        self.shapes = []

    def labels(self, p):
        return {c for c, _ in self.pos[p]}

    def census(self):
        n = {}
        for labs in self.pos.values():
            for c in {c for c, _ in labs}:
                n[c] = n.get(c, 0) + 1
        return dict(sorted(n.items()))

    def sides(self, cls):
        return {s for labs in self.pos.values() for c, s in labs if c == cls}


def _finish(P, bounds, V, budget, thin_order):
    """bounds {element: {classes}} -> P.pos within `budget` positions (row ends included)."""
    bounds = {e: c for e, c in bounds.items() if 0 < e < V}
    P.classes = {c for cs in bounds.values() for c in cs} | {"row_end"}
    room = (budget - 4) // 2                                   # boundaries: two positions each
    thinned = []
    keep = set(bounds)
    for n in range(1, len(thin_order) + 1):
        if len(keep) <= room:
            break
        soft = set(thin_order[:n])
        thinned = list(thin_order[:n])
        hard = {e for e, cs in bounds.items() if not cs <= soft}
        cand = sorted(set(bounds) - hard)
        must = set()
        for c in soft:                                         # the ends of every thinned class stay
            of = [e for e in sorted(bounds) if c in bounds[e]]
            must |= set(of[:2] + of[-3:])
        keep = hard | must
        rest = [e for e in cand if e not in keep]
        take = room - len(keep)
        if take > 0 and rest:
            idx = np.unique(np.linspace(0, len(rest) - 1, min(take, len(rest))).round().astype(int))
            keep |= {rest[i] for i in idx}
    if len(keep) > room:
        raise ValueError(f"V={V}: {len(keep)} boundaries that may not be thinned exceed the budget of {room}")
    P.thinned = tuple(c for c in thinned if any(c in bounds[e] for e in set(bounds) - keep))
    for e in sorted(keep):
        P.pos.setdefault(e - 1, set()).update((c, "below") for c in bounds[e])
        P.pos.setdefault(e, set()).update((c, "above") for c in bounds[e])
    for p, side in ((0, "above"), (1, "above"), (V - 2, "below"), (V - 1, "below")):
        if 0 <= p < V:
            P.pos.setdefault(p, set()).add(("row_end", side))
    return P


def logits_positions(sel, V, dtype, cus=256, budget=1 << 30):
    """The positions of a row of V logits (dtype "bf16" / "f32") on a device of `cus` compute units,
    over AUTO and every forced live shape in both directions, within `budget` positions."""
    tb = 2 if dtype == "bf16" else 4
    N = 16 // tb
    nvec = V // N
    K = sel.L
    vb = {}                                                    # boundary (vectors) -> classes

    def add(v, cls):
        if 0 < v <= nvec:
            vb.setdefault(int(v), set()).add(cls)

    P = Positions(V)
    plans = {}
    for shape in (0,) + LIVE:
        for dec in (False, True):
            p = q1_plan(sel, V, tb, dec, cus, shape)
            if p is None:
                continue
            if shape and shape not in P.shapes:
                P.shapes.append(shape)
            plans[tuple(p.values())] = p
    for p in plans.values():
        segs = [(0, nvec)]
        if p.family in (RL_GROUP, WIDE_GROUP):
            segs = [(j * p.split, min(p.split, nvec - j * p.split)) for j in range(p.k)]
            for s0, n in segs:
                add(s0, "segment")
                P.segments.append((s0 * N, (s0 + n) * N - 1))
        for s0, n in segs:
            if p.family in (RL, RL_GROUP):
                for m in range(1, (n - 1) // p.nt + 1):
                    add(s0 + m * p.nt, "run")
                if n > K.kRLRegVec * p.nt:
                    add(s0 + K.kRLRegVec * p.nt, "slot_step")
                last = (K.kRLRegVec + K.kRLSlots - 1) * p.nt
                if n > last:
                    add(s0 + last, "last_slot")
                    if n >= last + p.lastn:
                        add(s0 + last + p.lastn, "last_slot")
            elif p.family in (WIDE, WIDE_GROUP):
                for m in range(1, (n - 1) // K.kQ1WideThreads + 1):
                    add(s0 + m * K.kQ1WideThreads, "run")
                if n > K.kQ1WideMaxVec:
                    add(s0 + K.kQ1WideMaxVec, "slot_step")
        if p.tiled_shape and p.multi:                          # the tiled forms, a group's repair included
            tile = 64 * p.rw * p.r
            for m in range(1, (nvec - 1) // tile + 1):
                add(m * tile, "tile")
        gpc = p.groups_per_chunk
        for m in range(1, (nvec - 1) // (64 * gpc) + 1):
            add(m * 64 * gpc, "chunk")
    sp = step_plan(sel, V, tb, cus)
    if sp is not None:
        for m in range(1, (nvec - 1) // (64 * sp.R) + 1):
            add(m * 64 * sp.R, "step_wave")
    ngrp = (nvec + 63) // 64
    if nvec <= 4096:
        for g in range(1, ngrp):
            add(64 * g, "group")
    else:
        for v in list(vb):
            for g in (v // 64 - 1, v // 64, v // 64 + 1):
                add(64 * g, "group")
        for g in (ngrp - 2, ngrp - 1):
            add(64 * g, "group")
        for m in range(1, (nvec - 1) // 256 + 1):
            add(256 * m, "mult256")
    return _finish(P, {v * N: cs for v, cs in vb.items()}, V, budget, LOGITS_THIN)


def logits_rows(P, bf16):
    """One row per position, kinds dealt round-robin, then one more row for every (kind, class)
    pair still missing -> [(position, kind index into KINDS, n-th row of that kind)]."""
    nk = 6 if bf16 else 5
    rows, seen, count = [], set(), [0] * nk

    def put(p, k):
        if k == 4 and p == 0:                                  # the pair needs x[p - 1]
            return False
        rows.append((p, k, count[k]))
        count[k] += 1
        seen.update((k, c) for c in P.labels(p))
        return True

    for i, p in enumerate(sorted(P.pos)):
        if not put(p, i % nk):
            put(p, (i + 1) % nk)
    for c in sorted(P.classes):
        of = [p for p in sorted(P.pos) if c in P.labels(p)]
        for k in range(nk):
            if (k, c) not in seen:
                put(next(p for p in of[k % len(of):] + of if not (k == 4 and p == 0)), k)
    return rows


def pmf_vec(V, bits):
    vw = 4 if bits == 32 else 2
    return vw if V % vw == 0 else 1


def lean_plan(sel, V, bits, streams, prec):
    """decode_plan's default path for contiguous rows at `streams` streams -> (k_decode_lean takes it,
    its 64-load iterations per chunk)."""
    kn = (C.c_int64 * 10)(0, 2048, 1536, 160, 256, 0, 1, 0, 0, 64)
    d = (C.c_int64 * 12)()
    sel.sc_decode_plan(kn, streams, V, bits, prec, 1, streams * V, V, 64, d)
    return bool(d[7]), int(d[8])


def pmf_positions(sel, V, bits, budget=1 << 30):
    """The positions of a contiguous integer table row of V entries of `bits` bits (lean chunks:
    where k_decode_lean takes the row at PMF_LEAN_B streams and PMF_LEAN_PREC)."""
    vec = pmf_vec(V, bits)
    it = 64 * vec
    nit = (V // vec + 63) // 64
    eb = {}

    def add(e, cls):
        if 0 < e < V:
            eb.setdefault(int(e), set()).add(cls)

    P = Positions(V)
    for m in range(1, nit + 1):
        add(m * it, "iter")
    if vec > 1:
        lean, ci = lean_plan(sel, V, bits, PMF_LEAN_B, PMF_LEAN_PREC)
        if lean:
            o = (C.c_int64 * 2)()
            sel.sc_lean_chunks(V, vec, bits, o)
            assert int(o[0]) == ci
            for m in range(1, int(o[1])):
                add(m * ci * it, "lean_chunk")
        kn = (C.c_int64 * 10)(2, 2048, 1536, 160, 256, 0, 1, 0, 0, 64)       # the fused (wave) path, fine on
        d = (C.c_int64 * 12)()
        sel.sc_decode_plan(kn, 16, V, bits, 48, 1, 16 * V, V, 64, d)
        if d[3]:                                               # fine_nr
            for m in range(1, (nit - 1) // int(d[3]) + 1):
                add(m * int(d[3]) * it, "fine_wave")
        for nw in (4, 8, 16):
            kn[0], kn[5] = 4, nw                               # the block path at nw waves
            sel.sc_decode_plan(kn, 16, V, bits, 48, 1, 16 * V, V, 64, d)
            if d[1] == 2 and d[4] == nw:
                for m in range(1, (nit - 1) // nw + 1):
                    add(m * nw * it, "block_wave")
    return _finish(P, eb, V, budget, PMF_THIN)


# ------------------------------------------------------------------ the GPU tests' parametrisations
LOGITS_CASES = [("bf16", V) for V in (1000, 32000, 128512, 128520, 163848, 208896, 262144)] + [
    ("f32", V) for V in (24, 32000, 65536, 65540, 151936, 262144)]
STEP_CASES = {("bf16", 1000), ("bf16", 32000), ("bf16", 128512), ("f32", 24), ("f32", 32000), ("f32", 65536)}
LOGITS_BYTES = 256 << 20                                       # logits on the device at a time: one batch of rows
LOGITS_ROWS = 2048                                             # rows of one parametrisation, over all its batches
LOGITS_B = 16
PMF_CASES = [(32000, 32), (32004, 32), (5003, 32), (65540, 32), (131076, 32), (16000, 64), (65538, 64)]
PMF_ENTRIES = 1 << 26                                         # table entries of one parametrisation
PMF_B = 48                                                     # past kLeanMaxStreams: the stats path is k_decode_seq
PMF_LEAN_B, PMF_LEAN_PREC = 16, 40                             # the run that k_decode_lean takes


class Case:
    """rows laid out row-major as [steps, B, V]; batches: [(first row, rows)] coded one after the
    other, each a [steps, B, V] job of its own."""

    def __init__(self, P, rows, B, batches):
        self.P, self.rows, self.B, self.batches = P, rows, B, batches
        self.steps = -(-len(rows) // B)


def logits_case(sel, dtype, V, cus=256):
    """-> Case: rows [(position, kind, n)] in batches of whole steps, each batch's logits within
    LOGITS_BYTES."""
    tb = 2 if dtype == "bf16" else 4
    nk = 6 if dtype == "bf16" else 5
    reserve = nk * 11                                          # at most one more row per (kind, class)
    P = logits_positions(sel, V, dtype, cus, budget=LOGITS_ROWS - reserve)
    rows = logits_rows(P, dtype == "bf16")
    per = LOGITS_BYTES // (V * tb) // LOGITS_B * LOGITS_B
    assert per >= LOGITS_B and len(rows) <= LOGITS_ROWS
    return Case(P, rows, LOGITS_B, [(a, min(per, len(rows) - a)) for a in range(0, len(rows), per)])


def pmf_case(sel, V, bits):
    """-> Case: rows [position] as [steps, B, V]."""
    max_rows = PMF_ENTRIES // V // PMF_B * PMF_B
    P = pmf_positions(sel, V, bits, budget=max_rows)
    rows = sorted(P.pos)
    return Case(P, rows, PMF_B, [(0, len(rows))])
