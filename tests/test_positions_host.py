"""Census of tests/positions.py for every parametrisation of tests/test_gpu_positions_logits.py
and tests/test_gpu_positions_pmf.py, without a GPU: every boundary class a row has is coded on
both sides, every segment of every group form is coded at its first and last entry, every kind
of row meets every class, the rows fit the memory budget, and a budget thins only the classes
that may be thinned.  A few positions are stated by hand from DESIGN.md section 5b, so that a
positions.py that silently lost a class fails here.
"""
import pytest

import positions as ps

CUS = 256                                                       # MI355X
NEVER_THINNED = ("row_end", "segment", "slot_step", "last_slot", "tile", "step_wave", "group", "run", "chunk")


@pytest.fixture(scope="module")
def sel():
    return ps.load_select()


def _both_sides(P):
    for c in P.classes:
        assert P.sides(c) == {"below", "above"}, (c, P.sides(c))


def _hard_classes_whole(P, full):
    for c in NEVER_THINNED:
        assert c not in P.thinned
        assert {p for p in P.pos if c in P.labels(p)} == {p for p in full.pos if c in full.labels(p)}, c
    for c in P.classes:                                         # what is thinned keeps its ends
        of = sorted(p for p in full.pos if c in full.labels(p))
        assert set(of[:4] + of[-4:]) <= set(P.pos), c


@pytest.mark.parametrize("dtype,V", ps.LOGITS_CASES)
def test_logits_census(sel, dtype, V):
    case = ps.logits_case(sel, dtype, V, CUS)
    P, tb = case.P, 2 if dtype == "bf16" else 4
    assert P.classes == set(P.census()) and all(0 <= p < V for p in P.pos)
    _both_sides(P)
    for first, last in P.segments:
        assert first in P.pos and last in P.pos, (first, last)
    # every position has a row, every kind meets every class
    nk = 6 if dtype == "bf16" else 5
    assert {p for p, _, _ in case.rows} == set(P.pos)
    met = {(k, c) for p, k, _ in case.rows for c in P.labels(p)}
    assert met == {(k, c) for k in range(nk) for c in P.classes}
    assert all(p >= 1 for p, k, _ in case.rows if k == 4)
    # the budget: whole steps per batch, every batch's logits within the device budget, and
    # nothing but the multiples of 256 vectors ever thinned for it
    assert 8 <= case.B <= 16 and len(case.rows) <= ps.LOGITS_ROWS
    assert [a for a, _ in case.batches] == [sum(n for _, n in case.batches[:i]) for i in range(len(case.batches))]
    assert sum(n for _, n in case.batches) == len(case.rows)
    for a, n in case.batches:
        assert a % case.B == 0 and 0 < -(-n // case.B) * case.B * V * tb <= ps.LOGITS_BYTES
    assert ps.LOGITS_THIN == ("mult256",) and set(P.thinned) <= {"mult256"}
    _hard_classes_whole(P, ps.logits_positions(sel, V, dtype, CUS))
    assert sorted(P.shapes) == [s for s in ps.LIVE if ps.q1_plan(sel, V, tb, False, CUS, s)] and len(P.shapes) >= 7


def test_logits_positions_named_by_hand(sel):
    def has(dtype, V, elem, cls):
        P = ps.logits_case(sel, dtype, V, CUS).P
        assert cls in P.labels(elem - 1) and cls in P.labels(elem), (dtype, V, elem, cls)

    has("f32", 32000, 4 * 512, "run")                          # shape 18: two rows of 512 threads per block
    has("f32", 32000, 4 * 8 * 512, "slot_step")
    has("f32", 32000, 4 * 15 * 512, "last_slot")
    has("f32", 32000, 4 * 64 * 8, "step_wave")                 # the fused step at R = 8
    has("bf16", 32000, 8 * 64 * 4, "step_wave")
    has("bf16", 32000, 8 * 64 * 17, "group")                   # rows of <= 4096 vectors: every group
    has("bf16", 128512, 8 * 15 * 1024, "last_slot")            # shape 15, the trimmed 16-copy form
    has("bf16", 128520, 8 * 8 * 1024, "slot_step")
    has("bf16", 163848, 8 * 20480, "slot_step")                # shape 22 with its LDS slots: one vector in them
    has("bf16", 163848, 8 * 512 * 39, "run")
    has("bf16", 262144, 8 * 16384, "segment")                  # shape 23: two blocks
    has("bf16", 262144, 8 * 64 * 8 * 8, "tile")                # the bf16 encode repair: tiles of (8, 8)
    has("f32", 151936, 4 * 19008, "segment")                   # Qwen2 f32: wide groups of 19008 vectors
    has("f32", 65540, 4 * 64 * 5, "chunk")                     # 16385 vectors: 5 groups per chunk
    has("f32", 262144, 4 * 256 * 33, "run")                    # shape 21: segments of 4096 vectors, 256 threads each
    P = ps.logits_case(sel, "f32", 262144, CUS).P
    assert {"segment", "slot_step", "last_slot", "tile", "chunk", "run", "group", "mult256", "row_end"} == P.classes
    P = ps.logits_case(sel, "f32", 24, CUS).P
    assert sorted(P.pos) == [0, 1, 22, 23]


@pytest.mark.parametrize("V,bits", ps.PMF_CASES)
def test_pmf_census(sel, V, bits):
    case = ps.pmf_case(sel, V, bits)
    P = case.P
    _both_sides(P)
    assert case.rows == sorted(P.pos) and all(0 <= p < V for p in P.pos)
    assert len(case.rows) <= case.B * case.steps and case.B * case.steps * V <= ps.PMF_ENTRIES
    assert case.batches == [(0, len(case.rows))]
    assert set(P.thinned) <= set(ps.PMF_THIN)
    _hard_classes_whole(P, ps.pmf_positions(sel, V, bits))
    vec = ps.pmf_vec(V, bits)
    assert vec == {5003: 1}.get(V, 4 if bits == 32 else 2)
    want = {"row_end", "iter"}
    if ps.lean_plan(sel, V, bits, ps.PMF_LEAN_B, ps.PMF_LEAN_PREC)[0]:
        want |= {"lean_chunk"}
    assert ("lean_chunk" in want) == ((V, bits) in {(32000, 32), (32004, 32), (16000, 64)})   # chunks of <= 4 iterations
    if V // vec <= 512 * 64:                                    # the fine and block kernels' limit
        want |= {"fine_wave", "block_wave"} if vec > 1 else set()
    assert P.classes == want


def test_pmf_positions_named_by_hand(sel):
    P = ps.pmf_case(sel, 131076, 32).P                          # 513 iterations of 256 entries
    assert {511 * 256 - 1, 511 * 256, 512 * 256 - 1, 512 * 256, 131075} <= set(P.pos)
    P = ps.pmf_case(sel, 32000, 32).P                           # 125 iterations, lean chunks of 2, fine NR = 2
    assert "lean_chunk" in P.labels(512) and "fine_wave" in P.labels(511) and "block_wave" in P.labels(4 * 256)
    assert "lean_chunk" not in P.labels(256)
    P = ps.pmf_case(sel, 5003, 32).P                            # scalar loads: iterations of 64 entries
    assert {63, 64, 4991, 4992, 5002} <= set(P.pos)
    P = ps.pmf_case(sel, 16000, 64).P                           # u64: 128 entries per iteration
    assert "iter" in P.labels(128) and "block_wave" in P.labels(16 * 128 - 1)
