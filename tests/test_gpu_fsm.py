"""Finite-state models on the device (include/lac.h lac_fsm_*, BatchCoder.load_fsm / encode_fsm /
decode_fsm): the table of step t is pmf[q_t], q_{t+1} = next[q_t][sym_t], the kernel advances q.

Every expected value comes from outside the finite-state path: the reference's own bits for its
NFA predictor (tests/golden/nfa_cases.json), the C oracle on the gathered rows pmf[q_t] with the
states from a host walk of ``next``, and -- for registers, and for corrupt bits -- the pmf path
(encode / decode) of this library on those gathered rows.
"""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import errors as E
from test_fsm_host import CASES, IDS, next_table, state_walk

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENC_FIELDS = ("l", "h", "L", "wa", "wc", "nsym", "err", "nflush", "err_step")
DEC_FIELDS = ("l", "h", "x", "pos", "nsym", "err", "det", "err_step", "ndet")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _lib():
    from lac_amd import _lib
    return _lib


def _coder(m, B, cap=None):
    from lac_amd.batch import BatchCoder
    return BatchCoder(m.V, B, prec=m.prec, pmf_bits=m.bits, capacity_bits=cap or 140 * (m.prec + 2) + 256, device=DEV)


# ------------------------------------------------------------------ models and their host walk
class Model:
    def __init__(self, tables, nxt, prec, bits):
        self.tables = np.ascontiguousarray(tables, dtype=np.uint32 if bits == 32 else np.uint64)
        self.next = None if nxt is None else np.ascontiguousarray(nxt, dtype=np.int32)
        self.K, self.V = self.tables.shape
        self.prec, self.bits = prec, bits

    def walk(self, state0, sym):
        """states [T + 1, B]: row t the state step t codes in, row T the state after the job."""
        q = np.zeros((sym.shape[0] + 1, sym.shape[1]), dtype=np.int32)
        q[0] = state0
        for t in range(sym.shape[0]):
            q[t + 1] = self.next[q[t], sym[t]]
        return q

    def gathered(self, states):
        return self.tables[states]                                # [T, B, V]

    def draw(self, rng, state0, T, avoid=-1):
        """Symbols [T, B] with a positive entry in the row they are coded with (and no step into
        state ``avoid``)."""
        q = np.array(state0, dtype=np.int64)
        sym = np.zeros((T, len(q)), dtype=np.int32)
        for t in range(T):
            for b in range(len(q)):
                live = np.flatnonzero(self.tables[q[b]])
                sym[t, b] = rng.choice(live[self.next[q[b], live] != avoid])
            q = self.next[q, sym[t]]
        return sym


def fixture_model(case):
    return Model(case["tables"], next_table(case), case["prec"], case["pmf_bits"])


def random_model(rng, K, V, prec, bits, flavour="plain"):
    if flavour == "plain":                   # entries 1 .. 2^12, a fifth of them zero
        t = rng.integers(1, 1 << 12, size=(K, V)) * (rng.random((K, V)) > 0.2)
    elif flavour == "fudged":                # minp = 1 under totals far past 2^16: fudged at prec 16
        t = rng.choice([1, 1, 3, 40000, 90000], size=(K, V))
    elif flavour == "u32max":                # every row totals exactly 2^32 - 1
        t = np.zeros((K, V), dtype=np.uint64)
        for q in range(K):
            cut = np.sort(rng.integers(0, 1 << 32, size=V - 1)) if V > 1 else np.zeros(0, dtype=np.int64)
            t[q] = np.diff(np.concatenate(([0], cut, [(1 << 32) - 1])))
    elif flavour == "wide32":                # u32 rows whose totals pass 2^32: the CDF does not fit the entries
        t = rng.integers(1 << 30, 1 << 32, size=(K, V))
    elif flavour == "p60":                   # max(2, floor(p 2^60)) rows (the llama-scale tables)
        p = rng.dirichlet(np.full(V, 0.3), size=K)
        t = np.maximum(2, np.floor(p * float(1 << 60))).astype(np.uint64)
    elif flavour == "top":                   # u64 totals in [2^63, 2^64)
        t = np.zeros((K, V), dtype=np.uint64)
        for q in range(K):
            share = rng.integers(1, 1 << 20, size=V).astype(np.float64)
            total = (1 << 63) + int(rng.integers(0, 1 << 62))
            row = [int(total * s / share.sum()) for s in share]
            row[0] += total - sum(row)
            t[q] = np.array(row, dtype=np.uint64)
            assert (1 << 63) <= sum(int(x) for x in t[q]) < (1 << 64)
    else:
        raise ValueError(flavour)
    t = np.asarray(t).astype(np.uint64)
    for q in range(K):                       # no empty row
        if not t[q].any():
            t[q, rng.integers(0, V)] = 1
    return Model(t, rng.integers(0, K, size=(K, V)), prec, bits)


def verdict(m, pmf, sym):
    return E.verdict(types.SimpleNamespace(B=sym.shape[1], prec=m.prec), pmf, sym)


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def same_fields(got, want, fields, what):
    for f in fields:
        assert np.array_equal(got[f], want[f]), (what, f, got[f], want[f])


def job_equals_oracle(c, m, state0, sym, explicit=False, what=""):
    """encode_fsm_job against the oracle on the gathered rows, decode_fsm of its own output, and
    the states both leave -- in the walking or the explicit-states form."""
    q = m.walk(state0, sym)
    v = verdict(m, m.gathered(q[:-1]), sym)
    assert not v["code"].any(), what
    states = dev_i32(q[:-1]) if explicit else None
    c.encode_fsm_job(dev_i32(sym), state0=state0, states=states)
    assert c.status()[0] == 0, what
    got, n = E.stream_bytes(c)
    assert np.array_equal(n, v["nbits"]) and got == v["data"], what
    if not explicit:
        assert np.array_equal(c.fsm_states(), q[-1]), what
    c.decode_open()
    c.set_fsm_states(state0)
    out = c.decode_fsm(sym.shape[0], states=states).cpu().numpy()
    assert c.status()[0] == 0 and np.array_equal(out, sym), what
    assert np.array_equal(c.fsm_states(), state0 if explicit else q[-1]), what
    return got, n


# ------------------------------------------------------------------ the reference's fixtures
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixture(case):
    """encode_fsm_job gives the reference's bytes and bit count, decode_fsm its symbols, fsm_states
    the host walk's state; with set_decode_stop the stream stops where the reference's
    run(bits, stop=0) stops, on the whole stream and on the truncated prefix."""
    m = fixture_model(case)
    sym = np.array(case["syms"], dtype=np.int32)[:, None]
    N, s0 = len(sym), [case["state"]]
    with _coder(m, 1, cap=(N + 8) * (m.prec + 2) + 256) as c:
        c.load_fsm(m.tables, m.next)
        c.encode_fsm_job(dev_i32(sym), state0=s0)
        data, n = c.to_bytes()
        assert int(n[0]) == case["L"] and data[0].hex() == case["bytes"]
        assert c.fsm_states().tolist() == [case["end_state"]]
        c.decode_open()
        c.set_fsm_states(s0)
        assert np.array_equal(c.decode_fsm(N).cpu().numpy(), sym)
        assert c.status()[0] == 0 and c.fsm_states().tolist() == [case["end_state"]]
        bits = c.bits_tensor()
        c.set_decode_stop(True)
        for nbits, count in ((case["L"], case["decoded_count"]), (case["prefix_bits"], case["prefix_decoded_count"])):
            c.decode_open(bits, torch.tensor([nbits], dtype=torch.int64, device=DEV))
            c.set_fsm_states(s0)
            out = c.decode_fsm(case["decoded_count"] + 5).cpu().numpy()[:, 0]
            rc, err, step = c.status()
            assert rc == _lib().LAC_E_UNDETERMINED and step[0] == count, (nbits, rc, step)
            assert out[:count].tolist() == case["decoded"][:count] and (out[count:] == -1).all()
            assert c.determined().tolist() == [count]
            assert c.fsm_states().tolist() == [state_walk(case, case["decoded"][:count])[-1]]   # frozen at the stop


# ------------------------------------------------------------------ either path decodes the other's streams
@pytest.mark.parametrize("bits,prec,flavour", ((32, 16, "fudged"), (32, 48, "plain"), (64, 60, "p60")))
def test_cross_path(bits, prec, flavour):
    rng = np.random.default_rng(7)
    m, B, T = random_model(rng, 9, 37, prec, bits, flavour), 5, 100
    s0 = rng.integers(0, m.K, size=B)
    sym = m.draw(rng, s0, T)
    q = m.walk(s0, sym)
    pmf = E.dev_pmf(m.gathered(q[:-1]), DEV)
    with _coder(m, B) as c:
        c.load_fsm(m.tables, m.next)
        c.encode_fsm_job(dev_i32(sym), state0=s0)
        fsm_bytes = E.stream_bytes(c)
        c.decode_open()
        assert np.array_equal(c.decode(pmf).cpu().numpy(), sym)            # the pmf path reads FSM streams
        c.encode_job(pmf, dev_i32(sym))
        pmf_bytes = E.stream_bytes(c)
        assert pmf_bytes[0] == fsm_bytes[0] and np.array_equal(pmf_bytes[1], fsm_bytes[1])
        c.decode_open()
        c.set_fsm_states(s0)
        assert np.array_equal(c.decode_fsm(T).cpu().numpy(), sym)          # and the FSM path pmf streams
        assert c.status()[0] == 0


# ------------------------------------------------------------------ boundaries
T_EDGES = (1, 63, 64, 65, 130)
FORMS = ((32, 16, "fudged"), (32, 48, "plain"), (64, 60, "p60"))


@pytest.mark.parametrize("bits,prec,flavour", FORMS, ids=[f"u{b}p{p}" for b, p, _ in FORMS])
@pytest.mark.parametrize("V", (1, 4, 5, 255, 256, 260))
def test_boundaries(V, bits, prec, flavour):
    """B = 5 (a stream in a second workgroup), jobs of 1 .. 130 steps (the 64-step blocks), rows
    of one vector, just under / at / over one 64-vector round; walking and explicit states."""
    rng = np.random.default_rng(1000 * V + prec)
    m, B = random_model(rng, 6, V, prec, bits, flavour), 5
    s0 = rng.integers(0, m.K, size=B)
    sym = m.draw(rng, s0, max(T_EDGES))
    with _coder(m, B) as c:
        c.load_fsm(m.tables, m.next)
        for T in T_EDGES:
            a = job_equals_oracle(c, m, s0, sym[:T], what=("walk", T))
            b = job_equals_oracle(c, m, s0, sym[:T], explicit=True, what=("explicit", T))
            assert a[0] == b[0] and np.array_equal(a[1], b[1])
    with _coder(m, B) as c:                                      # a model with no transitions at all
        c.load_fsm(m.tables)
        job_equals_oracle(c, m, s0, sym[:65], explicit=True, what="no next")


@pytest.mark.parametrize("bits,prec,flavour", ((32, 48, "plain"), (64, 48, "p60")))
def test_longest_rows(bits, prec, flavour):
    """V = 65536 with K = 2: chunk bounds, then several rounds of 64 vectors."""
    rng = np.random.default_rng(65536 + bits)
    m, B = random_model(rng, 2, 65536, prec, bits, flavour), 5
    m.tables = np.maximum(m.tables, 1)
    s0 = rng.integers(0, m.K, size=B)
    sym = m.draw(rng, s0, 65)
    sym[::7] = np.array([0, 1, 65535, 65534, 32768])            # the row's first and last entries too
    assert all(m.tables[q, s] for q, s in zip(m.walk(s0, sym)[:-1].ravel(), sym.ravel()))
    with _coder(m, B) as c:
        c.load_fsm(m.tables, m.next)
        job_equals_oracle(c, m, s0, sym, what="V=65536")


@pytest.mark.parametrize("bits,prec,flavour", ((32, 48, "u32max"), (32, 48, "wide32"), (64, 60, "top"), (64, 48, "top"),
                                               (32, 16, "plain"), (64, 16, "p60")))
def test_totals(bits, prec, flavour):
    """u32 rows totalling 2^32 - 1 and past 2^32, u64 totals in [2^63, 2^64), and the general
    divisions' side of prec 50 / T 2^50."""
    rng = np.random.default_rng(prec + len(flavour))
    for V in (3, 300):
        m, B = random_model(rng, 4, V, prec, bits, flavour), 5
        s0 = rng.integers(0, m.K, size=B)
        sym = m.draw(rng, s0, 70)
        with _coder(m, B) as c:
            c.load_fsm(m.tables, m.next)
            job_equals_oracle(c, m, s0, sym, what=(flavour, V))


def test_one_state_self_loop_is_the_static_job():
    rng = np.random.default_rng(3)
    m = random_model(rng, 1, 100, 48, 32)
    m.next[:] = 0
    sym = m.draw(rng, [0] * 5, 130)
    with _coder(m, 5) as c:
        c.load_fsm(m.tables, m.next)
        c.encode_fsm_job(dev_i32(sym))
        fsm = E.stream_bytes(c)
        c.encode_job(E.dev_pmf(m.tables[0], DEV), dev_i32(sym))                # stride 0: one static row
        static = E.stream_bytes(c)
        assert fsm[0] == static[0] and np.array_equal(fsm[1], static[1])


# ------------------------------------------------------------------ errors
def _error_model():
    """K = 8 over V = 16 at prec 24: state 7's row is empty and symbol 3 alone leads to it; every
    row has a zero at symbol 15."""
    rng = np.random.default_rng(11)
    m = random_model(rng, 8, 16, 24, 32)
    m.tables[:, :15] = np.maximum(m.tables[:, :15], 1)
    m.tables[:, 15] = 0
    m.tables[7] = 0
    m.next = (m.next % 7).astype(np.int32)
    m.next[:, 3] = 7
    return m


@functools.lru_cache(maxsize=None)
def _error_job():
    """B = 8 streams of 130 steps: 0 clean; 1 / 2 / 3 a symbol out of range at step 0 / 63 / 64;
    4 the zero entry coded at step 70; 5 the empty row reached at step 3; 6 clean; 7 clean."""
    m = _error_model()
    rng = np.random.default_rng(12)
    B, T = 8, 130
    s0 = rng.integers(0, 7, size=B)
    sym = np.zeros((T, B), dtype=np.int32)
    q = np.zeros((T + 1, B), dtype=np.int32)
    q[0] = s0
    bad = {1: (0, m.V), 2: (63, -1), 3: (64, 2 ** 31 - 1), 4: (70, 15)}
    for t in range(T):
        for b in range(B):
            if b == 5 and t == 2:                                # the step into state 7
                sym[t, b] = 3
            elif b in bad and bad[b][0] == t:
                sym[t, b] = bad[b][1]
            else:
                sym[t, b] = rng.choice([s for s in np.flatnonzero(m.tables[q[t, b]]) if s != 3] or [0])
            q[t + 1, b] = m.next[q[t, b], sym[t, b]] if 0 <= sym[t, b] < m.V else q[t, b]
    code = np.array([0, E.LAC_E_SYMBOL_RANGE, E.LAC_E_SYMBOL_RANGE, E.LAC_E_SYMBOL_RANGE, E.LAC_E_ZERO_WIDTH,
                     E.LAC_E_TABLE, 0, 0], dtype=np.int32)
    step = np.array([-1, 0, 63, 64, 70, 3, -1, -1], dtype=np.int64)
    return m, s0, sym, q, code, step


def test_encode_errors():
    """Codes and steps are the oracle's on the gathered rows; a failed stream is frozen where the
    pmf path freezes it (registers, counters, plane words); its neighbours' bytes are the
    oracle's; the state stays at the failing step's."""
    m, s0, sym, q, code, step = _error_job()
    B, T = sym.shape[1], sym.shape[0]
    pmf = m.gathered(q[:-1])
    v = verdict(m, pmf, sym)
    assert np.array_equal(v["code"], code) and np.array_equal(v["step"], step)      # the yardstick itself
    assert np.array_equal(v["batch_status"], code)
    for explicit in (False, True):
        with _coder(m, B) as c, _coder(m, B) as ref:
            c.load_fsm(m.tables, m.next)
            c.reset()
            c.set_fsm_states(s0)
            c.encode_fsm(dev_i32(sym), states=dev_i32(q[:-1]) if explicit else None)
            ref.reset()
            ref.encode(E.dev_pmf(pmf, DEV), dev_i32(sym))
            rc, err, es = c.status()
            assert np.array_equal(err, code) and np.array_equal(es, step) and rc == E.first_code(code)
            a, b = c.checkpoint(), ref.checkpoint()
            same_fields(a["state"], b["state"], ENC_FIELDS, "frozen")
            assert np.array_equal(E.written(a), E.written(b))
            if not explicit:
                want = np.array([q[T if step[i] < 0 else step[i], i] for i in range(B)])
                assert np.array_equal(c.fsm_states(), want)
            c.finish()
            got, n = E.stream_bytes(c)
            for i in range(B):
                if code[i] == 0:
                    assert got[i] == v["data"][i] and n[i] == v["nbits"][i], i
                else:
                    assert n[i] == 0
            # sticky: more steps change nothing of a failed stream, and a reset clears it
            c.reset()
            assert c.status()[0] == 0


def test_explicit_state_out_of_range():
    m, s0, sym, q, _, _ = _error_job()
    sym, q = sym[:70, :3].copy(), q[:71, :3].copy()
    sym[:, 1], q[:, 1] = sym[:, 0], q[:, 0]                     # three clean streams (0 is clean in the job)
    sym[:, 2], q[:, 2] = sym[:, 0], q[:, 0]
    states = q[:-1].copy()
    states[64, 1], states[0, 2] = m.K, -1
    rows = m.gathered(np.clip(states, 0, m.K - 1)).copy()
    rows[64, 1] = 0                                             # the pmf path's LAC_E_TABLE at the same steps
    rows[0, 2] = 0
    v = verdict(m, rows, sym)
    assert v["code"].tolist() == [0, E.LAC_E_TABLE, E.LAC_E_TABLE] and v["step"].tolist() == [-1, 64, 0]
    with _coder(m, 3) as c, _coder(m, 3) as ref:
        c.load_fsm(m.tables)
        c.reset()
        c.encode_fsm(dev_i32(sym), states=dev_i32(states))
        ref.reset()
        ref.encode(E.dev_pmf(rows, DEV), dev_i32(sym))
        rc, err, es = c.status()
        assert np.array_equal(err, v["code"]) and np.array_equal(es, v["step"])
        same_fields(c.checkpoint()["state"], ref.checkpoint()["state"], ENC_FIELDS, "frozen")
        c.finish()
        got, n = E.stream_bytes(c)
        assert got[0] == v["data"][0] and n.tolist() == [v["nbits"][0], 0, 0]
        # decode: stream 0's bytes in all three slots, the same bad states
        bits = c.bits_tensor()
        bits[1:] = bits[0]
        nb = torch.full((3,), int(n[0]), dtype=torch.int64, device=DEV)
        c.decode_open(bits, nb)
        out = c.decode_fsm(70, states=dev_i32(states)).cpu().numpy()
        ref.decode_open(bits, nb)
        want = ref.decode(E.dev_pmf(rows, DEV)).cpu().numpy()
        assert np.array_equal(out, want) and np.array_equal(out[:, 0], sym[:, 0]) and (out[64:, 1] == -1).all()
        rc, err, es = c.status()
        assert err.tolist() == [0, E.LAC_E_TABLE, E.LAC_E_TABLE] and es.tolist() == [-1, 64, 0]
        same_fields(E.dec_state(c), E.dec_state(ref), DEC_FIELDS, "decode frozen")


def test_decode_errors_and_corrupt_bits():
    """Corrupt bits, and a walk that reaches the empty row: whatever decode_fsm returns, the pmf
    path returns on the rows of decode_fsm's own walk -- symbols, -1 fills, codes, steps and
    registers."""
    m, _, _, _, _, _ = _error_job()
    rng = np.random.default_rng(13)
    B, T = 6, 130
    s0 = rng.integers(0, 7, size=B)
    sym = m.draw(rng, s0, T, avoid=7)                             # the clean job stays off the empty row
    with _coder(m, B) as c, _coder(m, B) as ref:
        c.load_fsm(m.tables, m.next)
        c.encode_fsm_job(dev_i32(sym), state0=s0)
        assert c.status()[0] == 0
        bits, nb = c.bits_tensor(), c.nbits_tensor().clone()
        noise = torch.from_numpy(rng.integers(0, 256, size=(B, 40), dtype=np.uint8)).to(DEV)
        bits[1:4, 8:48] ^= noise[1:4]                             # streams 1..3 corrupt from byte 8 on
        c.decode_open(bits, nb)
        c.set_fsm_states(s0)
        out = c.decode_fsm(T).cpu().numpy()
        rc, err, es = c.status()
        # the rows of that walk, for the pmf path
        q = np.zeros((T, B), dtype=np.int64)
        q[0] = s0
        for t in range(1, T):
            ok = out[t - 1] >= 0
            q[t] = np.where(ok, m.next[q[t - 1], np.maximum(out[t - 1], 0)], q[t - 1])
        ref.decode_open(bits, nb)
        want = ref.decode(E.dev_pmf(m.gathered(q), DEV)).cpu().numpy()
        assert np.array_equal(out, want)
        rc2, err2, es2 = ref.status()
        assert rc == rc2 and np.array_equal(err, err2) and np.array_equal(es, es2)
        same_fields(E.dec_state(c), E.dec_state(ref), DEC_FIELDS, "registers")
        assert np.array_equal(out[:, 0], sym[:, 0]) and np.array_equal(out[:, 4:], sym[:, 4:])   # clean neighbours
        assert not np.array_equal(out[:, 1:4], sym[:, 1:4])       # (the corruption did change something)
        end = np.array([m.next[q[-1, b], out[-1, b]] if out[-1, b] >= 0 else q[int(es[b]), b] for b in range(B)])
        assert np.array_equal(c.fsm_states(), end)


def test_refusals_launch_nothing():
    from lac_amd._lib import LacError
    L = _lib()
    m = _error_model()
    m.tables[7] = 1

    def refused(code, f):
        with pytest.raises(LacError) as e:
            f()
        assert e.value.code == code, e.value

    def launches(c):
        ms, n = np.zeros(8), np.zeros(8, dtype=np.int64)
        L.check(c.lib.lac_profile_read(c.ctx, ms.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p), 0))
        return n.copy()

    with _coder(m, 3) as c:
        L.check(c.lib.lac_profile_enable(c.ctx, 1))
        sym = dev_i32(np.zeros((4, 3)))
        refused(L.LAC_E_STATE, lambda: c.encode_fsm(sym))                      # no model yet
        bad = m.next.copy()
        bad[5, 9] = m.K
        refused(L.LAC_E_TABLE, lambda: c.load_fsm(m.tables, bad))
        bad[5, 9] = -1
        refused(L.LAC_E_TABLE, lambda: c.load_fsm(m.tables, bad))
        refused(L.LAC_E_STATE, lambda: c.decode_fsm(4))                        # still no model
        c.load_fsm(m.tables, m.next)
        refused(L.LAC_E_STATE, lambda: c.decode_fsm(4))                        # no decode open
        c.set_mapping("floor")
        refused(L.LAC_E_STATE, lambda: c.encode_fsm(sym))
        c.set_mapping("ceil")
        c.reset()
        before = launches(c)
        c.encode_fsm(sym)
        assert (launches(c) - before).tolist() == [0, 1, 0, 0, 0, 0, 0, 0]     # one launch, under `encode`
        refused(L.LAC_E_STATE, lambda: c.load_fsm(m.tables, m.next))           # in mid-job
        before = launches(c)
        c.finish()
        c.load_fsm(m.tables)                                                   # between jobs: fine, and now no `next`
        refused(L.LAC_E_ARG, lambda: c.encode_fsm(sym))                        # ... so states are needed
        c.decode_open()
        refused(L.LAC_E_ARG, lambda: c.decode_fsm(4))
        c.decode_fsm(4, states=dev_i32(np.zeros((4, 3))))
        refused(L.LAC_E_STATE, lambda: c.load_fsm(m.tables, m.next))           # a decode job is running
        c.decode_open()
        c.load_fsm(m.tables, m.next)
        assert (launches(c) - before).tolist() == [0, 0, 1, 1, 0, 0, 0, 0]     # finish + the one decode launch
    big = types.SimpleNamespace(V=65536, prec=48, bits=32)
    with _coder(big, 1) as c:
        tab = torch.ones((257, 65536), dtype=torch.int32, device=DEV)          # K * V = 2^24 + 2^16
        refused(L.LAC_E_ARG, lambda: c.load_fsm(tab))
        c.load_fsm(tab[:256])
    over = types.SimpleNamespace(V=65537, prec=48, bits=32)
    with _coder(over, 1) as c:
        refused(L.LAC_E_ARG, lambda: c.load_fsm(torch.ones((1, 65537), dtype=torch.int32, device=DEV)))


# ------------------------------------------------------------------ composition
@functools.lru_cache(maxsize=None)
def _comp_job():
    rng = np.random.default_rng(21)
    m, B, T = random_model(rng, 12, 50, 48, 32), 5, 130
    s0 = rng.integers(0, m.K, size=B)
    sym = m.draw(rng, s0, T)
    q = m.walk(s0, sym)
    return m, s0, sym, q, verdict(m, m.gathered(q[:-1]), sym)


def test_stream_lengths():
    m, s0, sym, q, _ = _comp_job()
    T = sym.shape[0]
    lengths = np.array([0, 1, 64, T, 65])
    with _coder(m, 5) as c:
        c.load_fsm(m.tables, m.next)
        c.set_stream_lengths(lengths)
        c.encode_fsm_job(dev_i32(sym), state0=s0)
        got, n = E.stream_bytes(c)
        for b, k in enumerate(lengths):
            d, nb = E.oracle_prefix(m.gathered(q[:-1])[:, b], sym[:, b], int(k), m.prec)
            assert got[b] == d and n[b] == nb, b
        assert np.array_equal(c.fsm_states(), [q[k, b] for b, k in enumerate(lengths)])
        c.decode_open()
        c.set_fsm_states(s0)
        out = c.decode_fsm(T).cpu().numpy()
        for b, k in enumerate(lengths):
            assert np.array_equal(out[:k, b], sym[:k, b]) and (out[k:, b] == -1).all(), b
        assert c.status()[0] == 0
        assert np.array_equal(c.fsm_states(), [q[k, b] for b, k in enumerate(lengths)])


def test_three_calls_with_drains_equal_the_one_shot():
    m, s0, sym, q, v = _comp_job()
    B = 5
    with _coder(m, B, cap=70 * (m.prec + 2) + 256) as c:
        c.load_fsm(m.tables, m.next)
        slots = torch.zeros((B, 1024), dtype=torch.uint8, device=DEV)
        fill = torch.zeros(B, dtype=torch.int64, device=DEV)
        c.reset()
        c.set_fsm_states(s0)
        for a, b in ((0, 1), (1, 65), (65, 130)):
            c.encode_fsm(dev_i32(sym[a:b]))
            c.drain(slots, fill)
        c.finish()
        assert c.status()[0] == 0
        tail, n = E.stream_bytes(c)
        head, f = slots.cpu().numpy(), fill.cpu().numpy()
        for b in range(B):
            assert head[b, :f[b]].tobytes() + tail[b] == v["data"][b] and 8 * f[b] + n[b] == v["nbits"][b], b
        assert f.max() > 0 and np.array_equal(c.fsm_states(), q[-1])


def test_window_of_four_positions_with_refills():
    m, s0, sym, q, v = _comp_job()
    B, T, N = 5, sym.shape[0], 4
    stride = (max(len(d) for d in v["data"]) + 7) // 8 * 8 + 8
    buf = np.zeros((B, stride), dtype=np.uint8)
    for b, d in enumerate(v["data"]):
        buf[b, :len(d)] = np.frombuffer(d, dtype=np.uint8)
    bits, nb = torch.from_numpy(buf).to(DEV), torch.from_numpy(v["nbits"].copy()).to(DEV)
    with _coder(m, B, cap=N * (m.prec + 2) + 256) as c:
        c.load_fsm(m.tables, m.next)
        c.decode_open_window(bits, nb)
        c.set_fsm_states(s0)
        out = torch.empty((T, B), dtype=torch.int32, device=DEV)
        for t in range(0, T, N):
            c.decode_fsm(min(N, T - t), out=out[t:t + N])
            c.refill()
        c.refill()
        assert c.status()[0] == 0 and np.array_equal(out.cpu().numpy(), sym)
        assert np.array_equal(c.fsm_states(), q[-1])


# ------------------------------------------------------------------ one launch whatever the steps
def test_one_launch_each_way():
    L = _lib()
    rng = np.random.default_rng(31)
    m, B = random_model(rng, 5, 20, 48, 32), 5
    s0 = rng.integers(0, m.K, size=B)
    sym = m.draw(rng, s0, 700)
    counts = {}
    for T in (70, 700):
        with _coder(m, B, cap=T * (m.prec + 2) + 256) as c:
            c.load_fsm(m.tables, m.next)
            L.check(c.lib.lac_profile_enable(c.ctx, 1))
            c.encode_fsm_job(dev_i32(sym[:T]), state0=s0)
            c.decode_open()
            c.set_fsm_states(s0)
            out = c.decode_fsm(T).cpu().numpy()
            assert np.array_equal(out, sym[:T])
            ms, n = np.zeros(8), np.zeros(8, dtype=np.int64)
            L.check(c.lib.lac_profile_read(c.ctx, ms.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p), 0))
            counts[T] = n.tolist()
    enc, dec = L.KERNEL_IDS["encode"], L.KERNEL_IDS["decode_step"]
    assert counts[70][enc] == counts[700][enc] == 1 and counts[70][dec] == counts[700][dec] == 1, counts
