"""Markov_up_to_n through the drop-in coders (lac_amd.coder AC / A_to_bin / A_from_bin): a
predictor whose prob, accept and calc_dist are the class's own and whose lfunc is a CountWeights
is coded by the count-model kernels, one launch per job; a subclass overriding prob, or any other
lfunc, keeps the per-token path.  Results are the reference's (tests/golden/markov_cases.json)
either way, and the host predictor's table and past afterwards are those of a plain Python run.
"""
import numpy as np
import pytest

import counts as K
from test_counts_host import ALL, CASES, IDS

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
SMALL = [c for c in CASES if c["V"] <= 40]                        # (the per-token runs build every row in Python)
SMALL_IDS = [c["name"] for c in SMALL]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def make(case, **kw):
    from lac_amd.coder import CountWeights, Markov_up_to_n
    return Markov_up_to_n(case["V"], case["order"], CountWeights(case["weights"]), **kw)


def plain_run(case, syms):
    """table and past of a plain Python run over the symbols."""
    p = make(case)
    for s in syms:
        p.accept(s)
    return p.table, p.past


def fixture_bits(case):
    b = np.unpackbits(np.frombuffer(bytes.fromhex(case["bytes"]), dtype=np.uint8))
    return b[:case["L"]].tolist()


class Spy:
    """Counts the BatchCoder calls that code symbols."""

    def __init__(self, monkeypatch):
        from lac_amd.batch import BatchCoder
        self.n = {}
        for name in ("encode", "encode_counts", "decode", "decode_counts"):
            self.n[name] = 0
            monkeypatch.setattr(BatchCoder, name, self._wrap(name, getattr(BatchCoder, name)))

    def _wrap(self, name, f):
        def g(*a, **k):
            self.n[name] += 1
            return f(*a, **k)
        return g


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_recognised_model_codes_in_one_launch(case, monkeypatch):
    from lac_amd.coder import AC
    spy = Spy(monkeypatch)
    N = len(case["syms"])
    table, past = plain_run(case, case["syms"])
    enc = AC(make(case), case["prec"]).to_bin
    assert list(enc.bits(case["syms"])) == fixture_bits(case)
    assert spy.n["encode_counts"] == 1 and spy.n["encode"] == 0
    assert enc.predictor.table == table and enc.predictor.past == past == tuple(case["past"])   # accept was replayed
    R, L = AC(make(case), case["prec"]).to_bin.encode(case["syms"])
    assert L == case["L"] and R == int.from_bytes(bytes.fromhex(case["bytes"]), "big") >> (-L % 8)
    dec = AC(make(case), case["prec"]).from_bin
    assert list(dec.run(fixture_bits(case), n=N)) == case["syms"]
    assert spy.n["decode_counts"] == 1 and spy.n["decode"] == 0
    assert dec.predictor.table == table and dec.predictor.past == past
    # the count-free form stops where the reference's run(bits, stop=0) stops
    for nbits, count in ((case["L"], case["decoded_count"]), (case["prefix_bits"], case["prefix_decoded_count"])):
        dec = AC(make(case), case["prec"]).from_bin
        before = spy.n["decode_counts"]
        assert list(dec.run(fixture_bits(case)[:nbits], stop=0)) == case["decoded"][:count]
        assert 1 <= spy.n["decode_counts"] - before <= 12 and spy.n["decode"] == 0
        t, p = plain_run(case, case["decoded"][:count])
        assert dec.predictor.table == t and dec.predictor.past == p


def test_default_lfunc_is_the_fixtures_weights(monkeypatch):
    from lac_amd.coder import AC, Markov_up_to_n
    case = next(c for c in CASES if c.get("default_lfunc"))
    spy = Spy(monkeypatch)
    enc = AC(Markov_up_to_n(case["V"], case["order"]), case["prec"]).to_bin
    assert list(enc.bits(case["syms"])) == fixture_bits(case) and spy.n["encode_counts"] == 1 and spy.n["encode"] == 0


@pytest.mark.parametrize("case", SMALL, ids=SMALL_IDS)
def test_run_chunked_by_a_small_capacity_yields_the_per_token_digits(case, monkeypatch):
    from lac_amd.coder import AC, A_to_bin, Markov_up_to_n

    class Slow(Markov_up_to_n):                                        # same model, not recognised
        def prob(self, symbol):
            return super().prob(symbol)

    spy = Spy(monkeypatch)
    enc = AC(make(case), case["prec"]).to_bin
    fast = list(enc.run(case["syms"][:3], stop=0))                     # in mid-stream: the coder is not resized
    enc._coder.capacity_bits = 10 * (case["prec"] + 1) + A_to_bin._SLACK   # (claims less than it holds: a few steps per chunk)
    before = spy.n["encode_counts"]
    fast += list(enc.run(case["syms"][3:]))
    assert spy.n["encode_counts"] - before > 1 and spy.n["encode"] == 0
    table, past = plain_run(case, case["syms"])
    assert enc.predictor.table == table and enc.predictor.past == past
    from lac_amd.coder import CountWeights
    slow = list(AC(Slow(case["V"], case["order"], CountWeights(case["weights"])), case["prec"]).to_bin.run(case["syms"]))
    assert spy.n["encode"] >= 1 and fast == slow


@pytest.mark.parametrize("case", SMALL, ids=SMALL_IDS)
def test_a_predictor_handed_over_with_a_table_continues(case, monkeypatch):
    """Half the symbols by a plain Python run, the rest on the device: the second coder starts from
    the table and past it is given.  The whole is checked through the decoder, which is handed the
    same state, and through the per-token path."""
    from lac_amd.coder import AC, CountWeights, Markov_up_to_n

    class Slow(Markov_up_to_n):
        def prob(self, symbol):
            return super().prob(symbol)

    spy = Spy(monkeypatch)
    half = len(case["syms"]) // 2
    head, tail = case["syms"][:half], case["syms"][half:]
    table, past = plain_run(case, head)
    enc = AC(make(case, past=past, table=dict(table)), case["prec"]).to_bin
    bits = list(enc.bits(tail))
    assert spy.n["encode_counts"] == 1 and spy.n["encode"] == 0
    slow = AC(Slow(case["V"], case["order"], CountWeights(case["weights"]), past, dict(table)), case["prec"]).to_bin
    assert list(slow.bits(tail)) == bits and spy.n["encode"] >= 1
    full_t, full_p = plain_run(case, case["syms"])
    assert enc.predictor.table == full_t and enc.predictor.past == full_p
    dec = AC(make(case, past=past, table=dict(table)), case["prec"]).from_bin
    assert list(dec.run(bits, n=len(tail))) == tail and spy.n["decode_counts"] == 1
    assert dec.predictor.table == full_t and dec.predictor.past == full_p
    # the same encoder object goes on: its table is not empty now either
    more = list(enc.bits(head))
    again = AC(make(case, past=full_p, table=dict(full_t)), case["prec"]).to_bin
    assert list(again.bits(head)) == more


@pytest.mark.parametrize("case", SMALL[:4], ids=SMALL_IDS[:4])
def test_unrecognised_predictors_keep_the_per_token_path(case, monkeypatch):
    from lac_amd.coder import AC, Markov_up_to_n

    class Peeking(Markov_up_to_n):                                     # overrides prob
        def prob(self, symbol):
            self.asked = getattr(self, "asked", 0) + 1
            return super().prob(symbol)

    spy = Spy(monkeypatch)
    N = len(case["syms"])
    W = case["weights"]
    enc = AC(Peeking(case["V"], case["order"], lambda c, o, n, m: c * W[o]), case["prec"]).to_bin
    assert list(enc.bits(case["syms"])) == fixture_bits(case)
    assert spy.n["encode_counts"] == 0 and spy.n["encode"] >= 1 and enc.predictor.asked >= N * case["V"]
    # any callable that is no CountWeights: the per-token path too, the same bits
    enc = AC(Markov_up_to_n(case["V"], case["order"], lambda c, o, n, m: c * W[o]), case["prec"]).to_bin
    assert list(enc.bits(case["syms"])) == fixture_bits(case) and spy.n["encode_counts"] == 0
    dec = AC(Peeking(case["V"], case["order"], lambda c, o, n, m: c * W[o]), case["prec"]).from_bin
    assert list(dec.run(fixture_bits(case), n=N)) == case["syms"] and spy.n["decode_counts"] == 0
    logged = AC(make(case), case["prec"]).to_bin                       # debug_log: the per-symbol path
    logged.debug_log = [("start",)]
    assert list(logged.bits(case["syms"])) == fixture_bits(case) and spy.n["encode_counts"] == 0


def test_nonlinear_lfunc_on_the_per_token_path(monkeypatch):
    from lac_amd.coder import AC, Markov_up_to_n
    spy = Spy(monkeypatch)
    for case in (c for c in ALL if c["weights"] is None):
        enc = AC(Markov_up_to_n(case["V"], case["order"], K.LFUNCS[case["lfunc"]]), case["prec"]).to_bin
        assert list(enc.bits(case["syms"])) == fixture_bits(case)
        dec = AC(Markov_up_to_n(case["V"], case["order"], K.LFUNCS[case["lfunc"]]), case["prec"]).from_bin
        assert list(dec.run(fixture_bits(case), stop=0)) == case["decoded"]
    assert spy.n["encode_counts"] == 0 and spy.n["decode_counts"] == 0
