"""The reference's NFA predictor through the drop-in coders (lac_amd.coder AC / A_to_bin /
A_from_bin): a predictor whose calc_dist and accept are NFA's -- lac_amd.coder.NFA, or a class
named NFA in a module named arith_code, as the reference's own is -- is coded in one finite-state
launch each way; a subclass overriding accept keeps the per-token path.  Results are the
reference's (tests/golden/nfa_cases.json) either way.
"""
import itertools
import sys
import types

import numpy as np
import pytest

from test_fsm_host import CASES, IDS, state_walk

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
SMALL = [c for c in CASES if c["K"] * c["V"] <= 4096]           # (conversion cost: the per-token runs are slow)
SMALL_IDS = [c["name"] for c in SMALL]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _foreign_nfa():
    """A class NFA in a module `arith_code`: what the reference's own class looks like to the
    recognition (its __init__ sets no dcache; the caller does)."""
    from lac_amd import coder
    mod = types.ModuleType("arith_code")

    class NFA(coder.ProbPredictor):
        def __init__(self, state, transitions):
            self.t = transitions
            self.s = state

        def calc_dist(self):
            self.dcache = self.t[self.s][0]
            return self.dcache

        def accept(self, symbol):
            self.s = self.t[self.s][1][symbol]
            return super().accept(symbol)

        def copy(self):
            p = NFA(self.s, self.t)
            p.dcache = None
            return p

    NFA.__qualname__ = "NFA"
    for f in (NFA.__init__, NFA.calc_dist, NFA.accept, NFA.copy):
        f.__module__ = "arith_code"
        f.__qualname__ = "NFA." + f.__name__
    NFA.__module__ = "arith_code"
    mod.NFA = NFA
    return NFA


def transitions(case):
    nxt = [list(range(case["V"]))] * case["K"] if case["next"] == "symbol" else case["next"]
    return [(list(itertools.accumulate(r)), n) for r, n in zip(case["tables"], nxt)]


def make(kind, case, state=None):
    from lac_amd import coder
    s = case["state"] if state is None else state
    if kind == "lac":
        return coder.NFA(s, transitions(case))
    p = _foreign_nfa()(s, transitions(case))
    p.dcache = None
    return p


def fixture_bits(case):
    b = np.unpackbits(np.frombuffer(bytes.fromhex(case["bytes"]), dtype=np.uint8))
    return b[:case["L"]].tolist()


class Spy:
    """Counts the BatchCoder calls that code symbols."""

    def __init__(self, monkeypatch):
        from lac_amd.batch import BatchCoder
        self.n = {}
        for name in ("encode", "encode_fsm", "decode", "decode_fsm"):
            self.n[name] = 0
            monkeypatch.setattr(BatchCoder, name, self._wrap(name, getattr(BatchCoder, name)))

    def _wrap(self, name, f):
        def g(*a, **k):
            self.n[name] += 1
            return f(*a, **k)
        return g


@pytest.mark.parametrize("kind", ("lac", "foreign"))
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_recognised_nfa_codes_in_one_launch(case, kind, monkeypatch):
    from lac_amd.coder import AC
    spy = Spy(monkeypatch)
    N = len(case["syms"])
    enc = AC(make(kind, case), case["prec"]).to_bin
    assert list(enc.bits(case["syms"])) == fixture_bits(case)
    assert spy.n["encode_fsm"] == 1 and spy.n["encode"] == 0
    assert enc.predictor.s == case["end_state"]                        # accept was replayed on the host predictor
    dec = AC(make(kind, case), case["prec"]).from_bin
    assert list(dec.run(fixture_bits(case), n=N)) == case["syms"]
    assert spy.n["decode_fsm"] == 1 and spy.n["decode"] == 0 and dec.predictor.s == case["end_state"]
    # the count-free form stops where the reference's run(bits, stop=0) stops
    for nbits, count in ((case["L"], case["decoded_count"]), (case["prefix_bits"], case["prefix_decoded_count"])):
        dec = AC(make(kind, case), case["prec"]).from_bin
        before = spy.n["decode_fsm"]
        assert list(dec.run(fixture_bits(case)[:nbits], stop=0)) == case["decoded"][:count]
        assert 1 <= spy.n["decode_fsm"] - before <= 12 and spy.n["decode"] == 0
        assert dec.predictor.s == state_walk(case, case["decoded"][:count])[-1]


@pytest.mark.parametrize("case", SMALL, ids=SMALL_IDS)
def test_run_digits_and_a_stream_continued_bit_by_bit(case, monkeypatch):
    """run(symbols) yields the per-token path's raw digits; a decoder that already holds a
    stream goes on bit by bit (the per-token path) and ends at the same symbols."""
    from lac_amd.coder import AC, A_to_bin, NFA

    class Slow(NFA):                                                   # same model, not recognised
        def accept(self, symbol):
            return super().accept(symbol)

        def copy(self):
            return Slow(self.s, self.t)

    spy = Spy(monkeypatch)
    fast = list(AC(make("lac", case), case["prec"]).to_bin.run(case["syms"]))
    assert spy.n["encode_fsm"] >= 1 and spy.n["encode"] == 0
    slow = list(AC(Slow(case["state"], transitions(case)), case["prec"]).to_bin.run(case["syms"]))
    assert spy.n["encode"] >= 1 and fast == slow
    half = case["L"] // 2
    dec = AC(make("lac", case), case["prec"]).from_bin
    out = list(dec.run(fixture_bits(case)[:half], stop=0))
    calls = spy.n["decode_fsm"]
    out += list(dec.run(fixture_bits(case)[half:], stop=0))           # holds a stream now: step(bit) each
    assert spy.n["decode_fsm"] == calls and out == case["decoded"]


@pytest.mark.parametrize("case", SMALL, ids=SMALL_IDS)
def test_unrecognised_predictors_keep_the_per_token_path(case, monkeypatch):
    from lac_amd.coder import AC, NFA

    class Counting(NFA):                                               # overrides accept
        def accept(self, symbol):
            self.seen = getattr(self, "seen", 0) + 1
            return super().accept(symbol)

        def copy(self):
            return Counting(self.s, self.t)

    class Declared(NFA):                                               # declares its own minp
        minp = 1

        def copy(self):
            return Declared(self.s, self.t)

    spy = Spy(monkeypatch)
    N = len(case["syms"])
    enc = AC(Counting(case["state"], transitions(case)), case["prec"]).to_bin
    assert list(enc.bits(case["syms"])) == fixture_bits(case)
    assert spy.n["encode_fsm"] == 0 and spy.n["encode"] >= 1 and enc.predictor.seen == N
    dec = AC(Counting(case["state"], transitions(case)), case["prec"]).from_bin
    assert list(dec.run(fixture_bits(case), n=N)) == case["syms"]
    assert spy.n["decode_fsm"] == 0
    if all(min(p for p in r if p) == 1 for r in case["tables"]):      # (a true declaration: results unchanged)
        enc = AC(Declared(case["state"], transitions(case)), case["prec"]).to_bin
        assert list(enc.bits(case["syms"])) == fixture_bits(case) and spy.n["encode_fsm"] == 0
    logged = AC(make("lac", case), case["prec"]).to_bin                # debug_log: the per-symbol path
    logged.debug_log = [("start",)]
    assert list(logged.bits(case["syms"])) == fixture_bits(case) and spy.n["encode_fsm"] == 0
