"""Host check of the kernel selection (lac_amd/csrc/lac_select.h): which row-statistics
shape q1_plan picks for a row of logits, and which decode path decode_plan picks for a call.

Compiles tests/native/select_check.cpp (plain C++ over the header, nothing else linked);
no GPU needed.  The expectations are DESIGN.md sections 1 / 5 / 5b and the comments beside
each rule, restated here by hand: a rule change shows up as a failing line to re-decide.
"""
import ctypes as C

import pytest

import positions

LAC_OK, LAC_E_ARG = 0, -1
TILED, RL, WIDE, RL_GROUP, WIDE_GROUP = range(5)
PER_STEP, WAVE, BLOCK, STATS = range(4)
PATH_AUTO, PATH_SPLIT, PATH_FUSED, PATH_STATS, PATH_BLOCK = range(5)
Q1_FIELDS = ("shape family rw r multi pf nwb rep lastn nt wide_slots k split nrb rep16 repair "
             "groups_per_chunk tiled_shape").split()
DEC_FIELDS = "rc path vec fine_nr block_nw G step_waves lean CI cs help static_rows".split()
CONSTS = ("kRLRep kRLLastTrim kRLTrimMaxVec kQ1WideMaxVec kQ1WideSlotMaxVec kQ1MaxSeg kLeanMaxStreams "
          "kLeanHelpMaxStreams kLeanHelpers kLeanBytes kLeanRounds LeanCW32").split()
LIVE = (1, 2, 3, 4, 6, 8, 10, 14, 15, 17, 18, 19, 20, 21, 22, 23)
RETIRED = (5, 7, 9, 11, 12, 13, 16)
BOUNDARIES = (256, 1024, 2048, 4096, 8192, 16064, 16384, 20480, 26112)     # vectors
# (RW, R, MULTI, PF, NWB) of the tiled shapes
TILED_FORMS = {1: (1, 4, 0, 0, 8), 2: (2, 8, 0, 0, 8), 3: (4, 8, 0, 0, 8), 4: (8, 8, 0, 0, 8), 6: (8, 8, 0, 1, 8),
               8: (8, 8, 1, 0, 8), 10: (16, 16, 1, 0, 16), 14: (16, 8, 1, 1, 16)}


class Plan(dict):
    __getattr__ = dict.__getitem__


@pytest.fixture(scope="module")
def sel():
    lib = positions.load_select()                             # compiled when stale, every sc_* declared there
    buf = (C.c_int64 * 12)()
    lib.sc_consts(buf)
    lib.K = Plan(zip(CONSTS, buf))
    return lib


def q1(sel, V, bf16, dec, cus=256, shape=0):
    """The plan, or None where q1_plan refuses (LAC_E_ARG)."""
    o = (C.c_int64 * 18)()
    rc = sel.sc_q1_plan(cus, V, 2 if bf16 else 4, int(dec), shape, o)
    assert rc in (LAC_OK, LAC_E_ARG)
    return Plan(zip(Q1_FIELDS, o)) if rc == LAC_OK else None


def dplan(sel, B, V=32000, bits=32, prec=48, aligned=True, step_stride=None, stream_stride=None, steps=1000, **knobs):
    k = dict(dpath=PATH_AUTO, wave_decode_min_streams=2048, block_decode_min_streams=1536, block_window_lo=160,
             block_window_hi=256, block_waves=0, fine_decode=1, dec_stop=0, has_len=0, chunk_steps=64)
    assert set(knobs) <= set(k)
    k.update(knobs)
    kn = (C.c_int64 * 10)(*k.values())
    o = (C.c_int64 * 12)()
    sel.sc_decode_plan(kn, B, V, bits, prec, int(aligned), B * V if step_stride is None else step_stride,
                       V if stream_stride is None else stream_stride, steps, o)
    return Plan(zip(DEC_FIELDS, o))


def tiled(p):
    return (p.rw, p.r, p.multi, p.pf, p.nwb)


def rl(p):
    return (p.rep, p.lastn, p.nt)


# ------------------------------------------------------------------ q1_plan: named choices
def test_constants(sel):
    K = sel.K
    assert (K.kRLRep, K.kRLLastTrim, K.kRLTrimMaxVec) == (8, 704, 16064)
    assert (K.kQ1WideMaxVec, K.kQ1WideSlotMaxVec, K.kQ1MaxSeg) == (20480, 26112, 16)
    assert [sel.sc_q1_slot_cap(n, r) for n in (1, 2, 4) for r in (1, 0)] == [16064, 16384, 8000, 8192, 4032, 4096]
    assert (K.kLeanMaxStreams, K.kLeanHelpMaxStreams, K.kLeanHelpers, K.kLeanBytes, K.kLeanRounds) == (
        44, 16, 16, 512 << 20, 3)
    assert [s for s in range(-2, 30) if sel.sc_q1_shape_live(s)] == [0, *LIVE]


@pytest.mark.parametrize("dec", [False, True])
def test_q1_named_auto_choices(sel, dec):
    p = q1(sel, 32000, True, dec)                             # bf16 c3
    assert (p.shape, p.family, tiled(p)) == (6, TILED, (8, 8, 0, 1, 8))
    p = q1(sel, 32000, False, dec)                            # f32 c3: 8000 vectors, exactly 15 * 512 + 320
    assert (p.shape, p.family, rl(p)) == (18, RL, (16, 320, 512))
    p = q1(sel, 16384, False, dec)                            # 4096 vectors > 4032: the 8-copy form (encode only)
    assert (p.shape, p.family, tiled(p)) == (6, TILED, (8, 8, 0, 1, 8)) if dec else (
        p.shape, p.family, rl(p)) == (17, RL, (8, 256, 256))
    p = q1(sel, 128256, True, dec)                            # Llama-3 bf16: 16032 vectors, last slot 704
    assert (p.shape, p.family, rl(p)) == (15, RL, (16, 704, 1024))
    p = q1(sel, 131072, True, dec)
    assert (p.shape, p.family, rl(p)) == (15, RL, (8, 1024, 1024))
    p = q1(sel, 65536, False, dec)
    assert (p.shape, p.family, rl(p)) == (15, RL, (8, 1024, 1024))
    p = q1(sel, 151936, True, dec)                            # Qwen2 bf16: registers only
    assert (p.shape, p.family, p.wide_slots) == (22, WIDE, 0)
    p = q1(sel, 202048, True, dec)                            # Llama-4 bf16
    assert (p.shape, p.family, p.wide_slots) == (22, WIDE, 1)
    p = q1(sel, 100280, False, dec)                           # cl100k f32
    assert (p.shape, p.family, p.wide_slots) == (22, WIDE, 1)
    p = q1(sel, 128256, False, dec)                           # Llama-3 f32: two 16-copy halves
    assert (p.shape, p.family, p.k, p.split, p.nrb, rl(p)) == (19, RL_GROUP, 2, 16064, 1, (16, 704, 1024))
    assert (p.repair, tiled(p)) == ((10, TILED_FORMS[10]) if dec else (14, TILED_FORMS[14]))
    p = q1(sel, 256000, True, dec)                            # Gemma bf16
    assert (p.shape, p.family, p.k, p.split, p.nrb, rl(p)) == (19, RL_GROUP, 2, 16000, 1, (16, 704, 1024))
    assert (p.repair, tiled(p)) == ((10, TILED_FORMS[10]) if dec else (8, TILED_FORMS[8]))


def test_q1_qwen2_f32_encode_goes_to_wide_groups(sel):
    o = (C.c_int64 * 4)()
    assert sel.sc_q1_group(256, 151936 // 4, 0, 0, 0, o) == 1 and o[2] == 2      # the best slot form: two rows per block
    p = q1(sel, 151936, False, False)
    assert (p.shape, p.family, p.k, p.split, p.nrb) == (23, WIDE_GROUP, 2, 19008, 1)
    assert (p.repair, tiled(p)) == (14, TILED_FORMS[14])


# ------------------------------------------------------------------ q1_plan: boundaries
def auto_expect(nvec, bf16, dec):
    """AUTO up to kQ1WideSlotMaxVec vectors as DESIGN.md 5b states it: (shape, family, form)."""
    if nvec <= 2048:
        sh = 1 if nvec <= 256 else 2 if nvec <= 1024 else 3
        return sh, TILED, TILED_FORMS[sh]
    if nvec <= 4096:
        if not bf16 and not dec:                              # four rows per block; 16 copies up to 15 * 256 + 192
            return 17, RL, ((16, 192, 256) if nvec <= 4032 else (8, 256, 256))
        return 6, TILED, TILED_FORMS[6]
    if nvec <= 8192:
        return 18, RL, ((16, 320, 512) if nvec <= 8000 else (8, 512, 512))
    if nvec <= 16384:
        return 15, RL, ((16, 704, 1024) if nvec <= 16064 else (8, 1024, 1024))
    assert nvec <= 26112
    return 22, WIDE, int(nvec > 20480)


def form_of(p):
    return tiled(p) if p.family == TILED else rl(p) if p.family == RL else p.wide_slots


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("dec", [False, True])
def test_q1_boundaries(sel, bf16, dec):
    n = 8 if bf16 else 4
    for b in BOUNDARIES:
        for nvec in (b - 1, b, b + 1):
            p = q1(sel, nvec * n, bf16, dec)
            if nvec > 26112:
                # the first row of the group forms: 7 segments of 3776 vectors in the four-row slots fill
                # 26113 / (7 * 4096) = 91 % of their capacity on 126 of 128 slots (score 0.897, decode's
                # 8-copy form 0.852) against 80 % for two one-row halves or four two-row quarters; wide
                # groups would be two blocks at 64 % < 75 %
                assert (p.shape, p.family, p.k, p.split, p.nrb) == (21, RL_GROUP, 7, 3776, 4)
                assert rl(p) == ((8, 256, 256) if dec else (16, 192, 256))
            else:
                assert (p.shape, p.family, form_of(p)) == auto_expect(nvec, bf16, dec), (nvec, bf16, dec)
    # ... and what flips at each, literally
    sh = lambda nvec: q1(sel, nvec * n, bf16, dec).shape
    f32enc = not bf16 and not dec
    assert [sh(256), sh(257), sh(1024), sh(1025), sh(2048)] == [1, 2, 2, 3, 3]
    assert [sh(2049), sh(4096)] == ([17, 17] if f32enc else [6, 6])
    assert [sh(4097), sh(8192), sh(8193), sh(16384), sh(16385), sh(26112)] == [18, 18, 15, 15, 22, 22]
    assert [rl(q1(sel, v * n, bf16, dec))[0] for v in (16064, 16065)] == [16, 8]
    assert [q1(sel, v * n, bf16, dec).wide_slots for v in (20480, 20481)] == [0, 1]
    if f32enc:
        assert [rl(q1(sel, v * n, bf16, dec)) for v in (4032, 4033)] == [(16, 192, 256), (8, 256, 256)]
    assert [rl(q1(sel, v * n, bf16, dec)) for v in (8000, 8001)] == [(16, 320, 512), (8, 512, 512)]


# ------------------------------------------------------------------ q1_plan: sweeps
def sweep_vs(n):
    vs = set(range(n, 300000 + 1, 331 * n)) | {n, 300000 // n * n}
    for b in BOUNDARIES + (8000, 4032, 32768, 2 * 20480):
        vs |= {(b + d) * n for d in (-1, 0, 1) if (b + d) * n <= 300000}
    return sorted(vs)


def fits(sel, shape, nvec, cus, dec, bf16):
    """Whether a forced live shape holds the row: by the capacities DESIGN.md 5b lists."""
    if shape in (8, 10, 14):
        return True                                           # tiles: any row
    if shape in TILED_FORMS:
        rw, r = TILED_FORMS[shape][:2]
        return nvec <= 64 * rw * r
    if shape in (15, 17, 18):
        return nvec <= {15: 16384, 18: 8192, 17: 4096}[shape]
    if shape == 22:
        return nvec <= 26112
    o = (C.c_int64 * 4)()
    if shape == 23:                                           # 2..16 blocks of an XCD, <= 20480 vectors each
        return any(64 * -(-(-(-nvec // 64)) // k) <= 20480 and 0 < nvec - (k - 1) * 64 * -(-(-(-nvec // 64)) // k)
                   for k in range(max(2, -(-nvec // 20480)), min(16, cus // 8) + 1))
    return bool(sel.sc_q1_group(cus, nvec, int(dec), int(bf16), {19: 1, 20: 2, 21: 4}[shape], o))


@pytest.mark.parametrize("cus", [64, 256, 304])
@pytest.mark.parametrize("bf16", [True, False])
def test_q1_sweep(sel, cus, bf16):
    n = 8 if bf16 else 4
    for dec in (False, True):
        for V in sweep_vs(n):
            nvec = V // n
            p = q1(sel, V, bf16, dec, cus)
            assert p is not None, (V, "AUTO never fails")
            assert p.shape in LIVE and p.groups_per_chunk == max(1, -(-(-(-nvec // 64)) // 64))
            # the tiled form is the plan's own shape, a group's repair, or none
            assert p.tiled_shape == (p.shape if p.family == TILED else p.repair)
            if nvec <= 26112:
                assert (p.shape, p.family, form_of(p)) == auto_expect(nvec, bf16, dec), (V, bf16, dec, cus)
            if p.family in (RL_GROUP, WIDE_GROUP):
                check_group(sel, p, nvec, cus, dec, bf16)
            elif nvec > 26112:                                # no group form takes the row: the tiled fallbacks
                want = 10 if dec else 8 if bf16 else 14
                assert (p.shape, p.family, tiled(p), p.repair) == (want, TILED, TILED_FORMS[want], 0)


def check_group(sel, p, nvec, cus, dec, bf16):
    slots = cus // 8 * p.nrb                                  # row slots per XCD
    cap = 20480 if p.family == WIDE_GROUP else sel.sc_q1_slot_cap(p.nrb, p.rep16)
    last = nvec - (p.k - 1) * p.split
    assert p.split % 64 == 0 and 0 < last <= cap and p.split <= cap, (nvec, dict(p))
    assert 2 <= p.k <= min(16, slots), (nvec, dict(p))
    assert p.repair == (10 if dec else 8 if bf16 else 14) == p.tiled_shape and tiled(p) == TILED_FORMS[p.repair]
    if p.family == RL_GROUP:
        assert p.shape == {1: 19, 2: 20, 4: 21}[p.nrb] and p.nt == 1024 // p.nrb and not (dec and p.nrb == 4 and p.rep16)
        assert rl(p) == ((16, {1: 704, 2: 320, 4: 192}[p.nrb], p.nt) if p.rep16 else (8, p.nt, p.nt))
    else:
        assert p.shape == 23 and p.nrb == 1


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_q1_forced_shapes(sel, cus):
    for bf16 in (True, False):
        n = 8 if bf16 else 4
        for dec in (False, True):
            for V in sweep_vs(n)[::7] + [b * n for b in BOUNDARIES] + [(b + 1) * n for b in BOUNDARIES]:
                nvec = V // n
                for shape in LIVE:
                    p = q1(sel, V, bf16, dec, cus, shape)
                    assert (p is not None) == fits(sel, shape, nvec, cus, dec, bf16), (V, shape, cus, dec, bf16)
                    if p is None:
                        continue
                    assert p.shape == shape
                    if shape in TILED_FORMS:
                        assert (p.family, tiled(p), p.repair) == (TILED, TILED_FORMS[shape], 0)
                    elif shape in (15, 17, 18):
                        nrb = {15: 1, 18: 2, 17: 4}[shape]
                        trim = nvec <= sel.sc_q1_slot_cap(nrb, 1)
                        rep = 16 if trim and not (shape == 17 and dec) else 8
                        assert (p.family, rl(p)) == (RL, (rep, {1: 704, 2: 320, 4: 192}[nrb] if trim else 1024 // nrb,
                                                         1024 // nrb))
                    elif shape == 22:
                        assert (p.family, p.wide_slots) == (WIDE, int(nvec > 20480))
                    else:
                        assert p.family == (WIDE_GROUP if shape == 23 else RL_GROUP)
                        check_group(sel, p, nvec, cus, dec, bf16)
                for shape in RETIRED + (-1, 24, 100):
                    assert q1(sel, V, bf16, dec, cus, shape) is None


# ------------------------------------------------------------------ decode_plan
def test_decode_default_paths_by_streams(sel):
    """V = 32000 u32, prec 48, default knobs: the stream counts lac_host.h's comments name."""
    for B in (1, 8, 16, 44):
        p = dplan(sel, B)
        assert (p.rc, p.path, p.vec, p.lean, p.CI, p.help) == (0, STATS, 4, 1, 2, int(B <= 16)), B
    for B in (45, 64, 128, 159, 257, 300, 512, 1024, 1535):
        p = dplan(sel, B)
        assert (p.path, p.vec, p.lean, p.help, p.cs, p.static_rows) == (STATS, 4, 0, 0, 64, 0), B
    for B, nw in ((160, 16), (256, 16), (1536, 4), (2047, 4)):
        p = dplan(sel, B)
        assert (p.path, p.vec, p.block_nw) == (BLOCK, 4, nw), B
    for B in (2048, 4096):
        p = dplan(sel, B)
        assert (p.path, p.vec, p.fine_nr) == (WAVE, 4, 2), B   # 125 iterations per row


def test_decode_plan_follows_each_input(sel):
    assert dplan(sel, 2048, dec_stop=1).path == STATS          # LAC_OPT_DECODE_STOP: always the stats path,
    assert dplan(sel, 160, dec_stop=1).path == STATS
    assert dplan(sel, 160, dec_stop=1, dpath=PATH_SPLIT).path == STATS
    assert dplan(sel, 8, dec_stop=1).lean == 1                 # ... lean included
    p = dplan(sel, 8, has_len=1)                               # per-stream counts: k_decode_seq alone
    assert (p.path, p.lean, p.help) == (STATS, 0, 0)
    assert dplan(sel, 8, prec=50).lean == 1 and dplan(sel, 8, prec=51).lean == 0
    p = dplan(sel, 8, step_stride=0, steps=777)                # a static model: one launch group, no helpers
    assert (p.path, p.lean, p.help, p.static_rows, p.cs) == (STATS, 1, 0, 1, 777)
    p = dplan(sel, 300, step_stride=0, steps=777)
    assert (p.path, p.lean, p.static_rows, p.cs) == (STATS, 0, 1, 777)
    for kw in (dict(aligned=False), dict(V=32001), dict(stream_stride=32002), dict(step_stride=8 * 32000 + 1)):
        assert (dplan(sel, 8, **kw).vec, dplan(sel, 8, **kw).lean) == (1, 0), kw
        assert dplan(sel, 160, **kw).path == STATS             # not blockable
        assert (dplan(sel, 2048, **kw).path, dplan(sel, 2048, **kw).fine_nr) == (WAVE, 0)
    p = dplan(sel, 8, bits=64)                                 # u64 tables: two entries per load, two bounds per lane
    assert (p.path, p.vec, p.lean, p.CI, p.help) == (STATS, 2, 1, 2, 1)
    assert dplan(sel, 8, bits=64, V=32001).vec == 1 and dplan(sel, 8, bits=64, V=32002).vec == 2
    assert (dplan(sel, 2048, bits=64).path, dplan(sel, 2048, bits=64).fine_nr) == (WAVE, 4)    # 250 iterations
    assert dplan(sel, 2048, V=65536).fine_nr == 4 and dplan(sel, 2048, V=131072).fine_nr == 8
    assert dplan(sel, 2048, V=131076).fine_nr == 0             # 513 iterations: k_decode_wave
    assert dplan(sel, 160, V=131072).path == BLOCK and dplan(sel, 160, V=131076).path == STATS
    assert dplan(sel, 2048, fine_decode=0).fine_nr == 0
    assert [dplan(sel, 160, block_waves=w).block_nw for w in (0, 4, 8, 16, 5)] == [16, 4, 8, 16, 16]
    assert dplan(sel, 600).path == STATS and dplan(sel, 600, dpath=PATH_BLOCK).block_nw == 8
    assert dplan(sel, 8, V=65536).lean == 1 and dplan(sel, 8, V=65540).lean == 0      # CI 4 / 5
    assert dplan(sel, 8, bits=64, V=65536).CI == 4 and dplan(sel, 8, bits=64, V=65538).lean == 0
    # the window and thresholds are knobs
    assert dplan(sel, 300, block_window_hi=304).path == BLOCK and dplan(sel, 1536, block_decode_min_streams=1537).path == STATS
    assert dplan(sel, 1024, wave_decode_min_streams=1024).path == WAVE


def test_decode_forced_paths(sel):
    assert dplan(sel, 8, dpath=PATH_FUSED).path == WAVE
    assert dplan(sel, 4096, dpath=PATH_STATS).path == STATS
    assert dplan(sel, 8, dpath=PATH_BLOCK).path == BLOCK
    assert dplan(sel, 8, dpath=PATH_BLOCK, aligned=False).path == STATS        # not blockable: the stats path
    for B, bits, vec, G, waves in ((8, 32, 4, 8, 16), (256, 32, 4, 8, 16), (257, 32, 4, 2, 4), (4096, 64, 2, 4, 4),
                                   (8, 64, 2, 8, 16)):
        p = dplan(sel, B, bits=bits, dpath=PATH_SPLIT)
        assert (p.rc, p.path, p.vec, p.G, p.step_waves) == (0, PER_STEP, vec, G, waves), B
    p = dplan(sel, 300, dpath=PATH_SPLIT, aligned=False)
    assert (p.path, p.vec, p.G, p.step_waves) == (PER_STEP, 1, 8, 4)
    # the chunk table (8 bytes per chunk of 64 * vec * G entries) must fit 64 KiB of LDS
    assert dplan(sel, 8, V=2048 * 8192, dpath=PATH_SPLIT).rc == LAC_OK
    assert dplan(sel, 8, V=2048 * 8192 + 4, dpath=PATH_SPLIT).rc == LAC_E_ARG
    assert dplan(sel, 300, V=512 * 8192 + 4, dpath=PATH_SPLIT).rc == LAC_E_ARG
    assert dplan(sel, 8, V=2048 * 8192 + 4).rc == LAC_OK       # only the per-step path has the table


def test_decode_lean_steps_per_launch(sel):
    """cs: as many steps as kLeanBytes of CDF rows hold, in whole 64s, at least 64, at most chunk_steps."""
    kb = sel.K.kLeanBytes
    for V in (32000, 65536):
        for bits in (32, 64):
            for B in (1, 8, 16, 44):
                for chunk in (64, 1 << 20):
                    want = min(chunk, max(64, kb // (V * bits // 8) // B // 64 * 64))
                    p = dplan(sel, B, V=V, bits=bits, chunk_steps=chunk)
                    assert (p.lean, p.cs) == (1, want), (V, bits, B, chunk)
    assert dplan(sel, 1, chunk_steps=1 << 20).cs == 4160       # 512 MiB / 128000 B = 4194 rows
    assert dplan(sel, 8, chunk_steps=1 << 20).cs == 512
    assert dplan(sel, 44, chunk_steps=1 << 20).cs == 64
    assert dplan(sel, 1, V=65536, bits=64, chunk_steps=1 << 20).cs == 1024
    assert dplan(sel, 45, chunk_steps=1 << 20).cs == 1 << 20   # not lean: the context's chunk
