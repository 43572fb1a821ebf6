"""Finite-state models with sparse rows (include/lac.h lac_fsm_*): grammars, deterministic states
and indexed codebooks -- rows whose few positive entries sit at the chunk, vector and round bounds
of the decoder's two-level search, with zero runs of whole vectors and chunks between them; u64
rows totalling exactly 2^64 - 1 and 2^64; corrupt bits on such a model; the ``trace`` argument of
encode_fsm.

The layout numbers (entries per vector, vectors per chunk, long rows) come from fsm_layout through
tests/native/fsm_check.cpp.  Every expected value comes from outside the finite-state path: the C
oracle on the gathered rows pmf[q_t], built by construction from exact Python integers, and --
for registers, corrupt bits and traces -- the pmf path (encode / decode) of this library on those
rows.  That every chosen position is coded in its row is asserted on the host.
"""
import functools

import numpy as np
import pytest

import errors as E
from test_fsm_host import _layout, fc  # noqa: F401  (fc: the fixture)
from test_gpu_fsm import DEC_FIELDS, DEV, ENC_FIELDS, Model, _coder, _error_job, dev_i32, job_equals_oracle, same_fields, verdict

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
SENTINEL = -7


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


# ------------------------------------------------------------------ rows by construction
def positions(y, V):
    """P, and the chunk numbers (first, middle, last bound) it was built from."""
    vec, G = y["Vp"] // y["nvec"], y["G"]
    CE = G * vec                                                  # entries per chunk
    assert y["long"] and G >= 2
    last = (V - 2) // CE                                          # the last chunk bound with an entry after it and V - 1 apart
    first, mid = 1, (1 + last) // 2
    assert first < mid - 3 and mid < last - 1
    P = {0, V - 1}
    for c in (first, mid, last):
        P |= {c * CE - 1, c * CE}
    vb = mid * CE + vec                                           # a vector bound inside chunk `mid`
    P |= {vb - 1, vb}
    if G > 64:
        rb = (mid * G + 64) * vec                                 # a round of 64 vectors ends inside chunk `mid`
        P |= {rb - 1, rb}
    assert all(0 <= p < V for p in P) and len(P) == (12 if G > 64 else 10)
    return sorted(P), CE, (first, mid, last)


def longest_zero_run(row):
    at = np.flatnonzero(np.concatenate(([1], row, [1])))
    return int(np.diff(at).max()) - 1


def sparse_rows(rng, y, V, bits):
    """Six rows: 0 the whole of P (zero runs of many chunks between its bounds); 1 P without the two
    entries at the last chunk bound (a zero run crosses it, the CDF is equal across it); 2 the
    first vector alone (every later bound holds T); 3, 4, 5 one-hot at entry 0, at V - 1 and at a
    chunk's first entry.  -> (rows, per row the positions to code)."""
    P, CE, (first, mid, last) = positions(y, V)
    vec = y["Vp"] // y["nvec"]
    want = [list(P), [p for p in P if p not in (last * CE - 1, last * CE)], list(range(vec)), [0], [V - 1], [mid * CE]]
    rows = np.zeros((6, V), dtype=np.uint64)
    for q, pos in enumerate(want):
        rows[q, pos] = rng.integers(1, (1 << 12) + 1, size=len(pos))
    assert longest_zero_run(rows[0]) >= 2 * CE and longest_zero_run(rows[2]) == V - vec
    cdf1 = np.cumsum(rows[1])
    assert cdf1[last * CE - 1] == cdf1[last * CE] == cdf1[last * CE - 2] and rows[1, V - 1] > 0
    assert all(int((r > 0).sum()) == 1 for r in rows[3:])
    return rows, want


def connected(m):
    """Does every state reach every other through symbols of positive probability?"""
    reach = np.eye(m.K, dtype=bool)
    for k in range(m.K):
        reach[k, m.next[k, np.flatnonzero(m.tables[k])]] = True
    for _ in range(m.K):
        reach = reach | ((reach.astype(np.int64) @ reach.astype(np.int64)) > 0)
    return bool(reach.all())


def steer(rng, m, s0, T, want):
    """Symbols [T, B] that code every position of want[q] in state q: a stream in a state with
    positions left takes one (the one whose next state is nearest to more of them), else the entry
    that leads there; with nothing left anywhere, any positive entry.  -> (sym, what is left)."""
    todo = [set(int(p) for p in w) for w in want]
    live = [np.flatnonzero(m.tables[q]) for q in range(m.K)]
    q = [int(s) for s in s0]
    sym = np.zeros((T, len(q)), dtype=np.int32)
    for t in range(T):
        for b in range(len(q)):
            dist = [0 if todo[k] else 1 << 20 for k in range(m.K)]
            for _ in range(m.K):
                for k in range(m.K):
                    dist[k] = min(dist[k], 1 + min(dist[int(m.next[k, s])] for s in live[k]))
            here = [int(s) for s in live[q[b]] if int(s) in todo[q[b]]] or [int(s) for s in live[q[b]]]
            if not any(todo):
                s = int(rng.choice(here))
            else:
                s = min(here, key=lambda s: (dist[int(m.next[q[b], s])], s))
            todo[q[b]].discard(s)
            sym[t, b] = s
            q[b] = int(m.next[q[b], s])
    return sym, todo


FORMS = ((32, 48, 260), (32, 48, 1000), (32, 48, 4100), (64, 60, 129), (64, 60, 1000), (32, 48, 65536), (64, 48, 65536))
FORM_IDS = [f"u{b}p{p}v{v}" for b, p, v in FORMS]


@functools.lru_cache(maxsize=None)
def _sparse_models(bits, prec, V, vec, nvec, G):
    """The six rows as models of K = 6 states -- of K = 2 (rows 0 1, 2 3, 4 5) at V = 65536 --, a
    random `next`, and a steered job of B = 5 streams each.  -> [(model, s0, sym, want)], |P|."""
    y = {"Vp": vec * nvec, "nvec": nvec, "G": G, "long": int(nvec > 64)}
    rng = np.random.default_rng(V + bits)
    rows, want = sparse_rows(rng, y, V, bits)
    K, T = (2, 16) if V == 65536 else (6, 70)
    out = []
    for k0 in range(0, 6, K):
        for _ in range(200):                                      # a random `next` in which every state leads to every other
            m = Model(rows[k0:k0 + K], rng.integers(0, K, size=(K, V)), prec, bits)
            if connected(m):
                break
        assert connected(m)
        s0 = np.arange(5) % K
        sym, left = steer(rng, m, s0, T, want[k0:k0 + K])
        out.append((m, s0, sym, want[k0:k0 + K], left))
    return out, len(want[0])


def census(m, s0, sym, want):
    """Per state the positions coded in it, from the host walk."""
    q = m.walk(s0, sym)
    seen = [set() for _ in range(m.K)]
    for t in range(sym.shape[0]):
        for b in range(sym.shape[1]):
            assert m.tables[q[t, b], sym[t, b]] > 0
            seen[q[t, b]].add(int(sym[t, b]))
    return seen


@pytest.mark.parametrize("bits,prec,V", FORMS, ids=FORM_IDS)
def test_sparse_rows_and_chunk_positions(fc, bits, prec, V):  # noqa: F811
    y = _layout(fc, 6, V, bits, True)
    jobs, nP = _sparse_models(bits, prec, V, y["Vp"] // y["nvec"], y["nvec"], y["G"])
    assert nP == (12 if V == 65536 else 10)                       # |P|
    for m, s0, sym, want, left in jobs:
        assert not any(left), left
        seen = census(m, s0, sym, want)
        assert all(set(w) <= s for w, s in zip(want, seen)), (want, seen)   # every position, in its row
    for m, s0, sym, want, _ in jobs:
        T, B = sym.shape
        q = m.walk(s0, sym)
        with _coder(m, B) as c, _coder(m, B) as ref:
            c.load_fsm(m.tables, m.next)
            a = job_equals_oracle(c, m, s0, sym, what=("walk", V))
            b = job_equals_oracle(c, m, s0, sym, explicit=True, what=("explicit", V))
            assert a[0] == b[0] and np.array_equal(a[1], b[1])
            c.encode_fsm_job(dev_i32(sym), state0=s0)
            bits_t, nb = c.bits_tensor(), c.nbits_tensor().clone()
            c.decode_open(bits_t, nb)
            c.set_fsm_states(s0)
            out = c.decode_fsm(T).cpu().numpy()
            ref.decode_open(bits_t, nb)
            want_sym = ref.decode(E.dev_pmf(m.gathered(q[:-1]), DEV)).cpu().numpy()
            assert np.array_equal(out, sym) and np.array_equal(want_sym, sym)
            same_fields(E.dec_state(c), E.dec_state(ref), DEC_FIELDS, ("decoder", V))


@pytest.mark.parametrize("bits,prec,V", ((32, 48, 1000), (64, 60, 129)))
def test_one_hot_streams(fc, bits, prec, V):  # noqa: F811
    """Streams that only ever visit deterministic states (the explicit-states form names them): the
    oracle's bit count, which is that of the flush alone."""
    y = _layout(fc, 6, V, bits, True)
    (m, _, _, want, _), = _sparse_models(bits, prec, V, y["Vp"] // y["nvec"], y["nvec"], y["G"])[0]
    T, B = 40, 5
    rng = np.random.default_rng(V)
    states = rng.integers(3, 6, size=(T, B)).astype(np.int32)
    states[:, 0], states[:, 1] = 3, 4
    sym = np.array([[want[s][0] for s in r] for r in states], dtype=np.int32)
    rows = m.gathered(states)
    v = verdict(m, rows, sym)
    assert not v["code"].any() and (v["nbits"] <= 2).all(), v["nbits"]
    with _coder(m, B) as c:
        c.load_fsm(m.tables)
        c.encode_fsm_job(dev_i32(sym), states=dev_i32(states))
        got, n = E.stream_bytes(c)
        assert c.status()[0] == 0 and np.array_equal(n, v["nbits"]) and got == v["data"]
        c.decode_open()
        out = c.decode_fsm(T, states=dev_i32(states)).cpu().numpy()
        assert c.status()[0] == 0 and np.array_equal(out, sym)


# ------------------------------------------------------------------ totals
@functools.lru_cache(maxsize=None)
def _totals_job():
    """K = 3 over V = 300, u64: row 0 sparse and small; row 1 two large entries and sparse small
    ones, total exactly 2^64 - 1; row 2 the same with one more: 2^64.  Odd symbols lead to state 1,
    even ones to state 0, symbol 150 to state 2.  Stream 0 never takes 150; stream 1 takes it at
    step 7 and reaches the bad row at step 8; stream 2 starts in state 1."""
    V, T, B = 300, 20, 3
    rng = np.random.default_rng(300)
    pos = [0, 3, 4, 7, 64, 127, 128, 150, 201, 299]
    rows = [[0] * V for _ in range(3)]
    for p in pos:
        rows[0][p] = int(rng.integers(1, 1 << 12))
        rows[1][p] = int(rng.integers(1, 1 << 12))
    rows[0][5], rows[0][255] = 9, 1
    rows[1][5] = (1 << 63) - 12345
    rows[1][255] = (1 << 64) - 1 - sum(rows[1])
    rows[2] = list(rows[1])
    rows[2][128] += 1
    assert sum(rows[1]) == (1 << 64) - 1 and sum(rows[2]) == 1 << 64 and max(rows[2]) < 1 << 64
    assert rows[1][255] > 1 << 62 and sum(1 for x in rows[1] if x) == 12
    nxt = np.tile((np.arange(V) % 2).astype(np.int32), (3, 1))
    nxt[:, 150] = 2
    m = Model(np.array(rows, dtype=np.uint64), nxt, 60, 64)
    live = [p for p in pos + [5, 255] if p != 150]
    sym = rng.choice(live, size=(T, B)).astype(np.int32)
    sym[::3, 0] = [5, 255, 299, 127, 201, 5, 255]                 # the large entries, odd: state 1 follows
    sym[7, 1] = 150
    q = m.walk([0, 0, 1], sym)
    assert (q[:, 0] == 1).sum() >= 5 and 2 not in q[:, 0] and 2 not in q[:, 2]
    assert q[8, 1] == 2 and 2 not in q[:8, 1]
    return m, np.array([0, 0, 1]), sym, q


def test_totals_2_64_minus_1_and_2_64():
    m, s0, sym, q = _totals_job()
    T, B = sym.shape
    rows = m.gathered(q[:-1])
    v = verdict(m, rows, sym)
    assert v["code"].tolist() == [0, E.LAC_E_TABLE, 0] and v["step"].tolist() == [-1, 8, -1]
    # the bits the decoder reads: the pmf path's, with stream 1 on row 0 from step 8 on
    free = rows.copy()
    free[8:, 1] = m.tables[0]
    sym_free = sym.copy()
    sym_free[8:, 1] = 299
    vf = verdict(m, free, sym_free)
    assert not vf["code"].any()
    for explicit in (False, True):
        states = dev_i32(q[:-1]) if explicit else None
        with _coder(m, B) as c, _coder(m, B) as ref:
            c.load_fsm(m.tables, m.next)
            c.reset()
            c.set_fsm_states(s0)
            c.encode_fsm(dev_i32(sym), states=states)
            ref.reset()
            ref.encode(E.dev_pmf(rows, DEV), dev_i32(sym))
            rc, err, es = c.status()
            assert np.array_equal(err, v["code"]) and np.array_equal(es, v["step"]) and rc == E.LAC_E_TABLE
            same_fields(c.checkpoint()["state"], ref.checkpoint()["state"], ENC_FIELDS, "frozen")
            assert np.array_equal(E.written(c.checkpoint()), E.written(ref.checkpoint()))
            if not explicit:
                assert c.fsm_states().tolist() == [q[T, 0], 2, q[T, 2]]   # stream 1: the state of its failing step
            c.finish()
            got, n = E.stream_bytes(c)
            assert [got[0], got[2]] == [v["data"][0], v["data"][2]] and n.tolist() == [v["nbits"][0], 0, v["nbits"][2]]
            ref.encode_job(E.dev_pmf(free, DEV), dev_i32(sym_free))
            fb, fn = E.stream_bytes(ref)
            assert fb == vf["data"] and np.array_equal(fn, vf["nbits"])
            bits_t, nb = ref.bits_tensor(), ref.nbits_tensor().clone()
            c.decode_open(bits_t, nb)
            c.set_fsm_states(s0)
            out = c.decode_fsm(T, states=states).cpu().numpy()
            rc, err, es = c.status()
            assert np.array_equal(err, v["code"]) and np.array_equal(es, v["step"]), (err, es)
            assert np.array_equal(out[:, [0, 2]], sym[:, [0, 2]])
            assert np.array_equal(out[:8, 1], sym[:8, 1]) and (out[8:, 1] == -1).all()
            if not explicit:
                assert c.fsm_states().tolist() == [q[T, 0], 2, q[T, 2]]
            ref.decode_open(bits_t, nb)
            assert np.array_equal(ref.decode(E.dev_pmf(rows, DEV)).cpu().numpy(), out)
            same_fields(E.dec_state(c), E.dec_state(ref), DEC_FIELDS, "decoder")


# ------------------------------------------------------------------ corrupt bits
@pytest.mark.parametrize("bits,prec,V", ((32, 48, 1000), (64, 60, 129)))
def test_corrupt_bits_on_a_sparse_model(fc, bits, prec, V):  # noqa: F811
    """One flipped bit in streams 1..3: whatever decode_fsm returns, the pmf path returns on the
    rows of decode_fsm's own walk -- symbols, -1 fills, codes, steps and registers; no symbol
    outside [0, V) is ever reported."""
    y = _layout(fc, 6, V, bits, True)
    (m, s0, sym, _, _), = _sparse_models(bits, prec, V, y["Vp"] // y["nvec"], y["nvec"], y["G"])[0]
    T, B = sym.shape
    rng = np.random.default_rng(V + 1)
    with _coder(m, B) as c, _coder(m, B) as ref:
        c.load_fsm(m.tables, m.next)
        c.encode_fsm_job(dev_i32(sym), state0=s0)
        assert c.status()[0] == 0
        bits_t, nb = c.bits_tensor(), c.nbits_tensor().clone()
        n = nb.cpu().numpy()
        for b in range(1, 4):
            at = int(rng.integers(4, int(n[b]) // 2))
            bits_t[b, at // 8] ^= 0x80 >> (at % 8)
        c.decode_open(bits_t, nb)
        c.set_fsm_states(s0)
        out = c.decode_fsm(T).cpu().numpy()
        rc, err, es = c.status()
        assert ((out >= -1) & (out < V)).all()
        q = np.zeros((T, B), dtype=np.int64)                      # the rows of that walk, for the pmf path
        q[0] = s0
        for t in range(1, T):
            ok = out[t - 1] >= 0
            q[t] = np.where(ok, m.next[q[t - 1], np.maximum(out[t - 1], 0)], q[t - 1])
        ref.decode_open(bits_t, nb)
        want = ref.decode(E.dev_pmf(m.gathered(q), DEV)).cpu().numpy()
        assert np.array_equal(out, want)
        rc2, err2, es2 = ref.status()
        assert rc == rc2 and np.array_equal(err, err2) and np.array_equal(es, es2)
        same_fields(E.dec_state(c), E.dec_state(ref), DEC_FIELDS, "registers")
        assert np.array_equal(out[:, 0], sym[:, 0]) and np.array_equal(out[:, 4], sym[:, 4])   # clean neighbours
        assert not np.array_equal(out[:, 1:4], sym[:, 1:4])       # (the corruption did change something)


# ------------------------------------------------------------------ traces
def _trace_check(m, s0, sym, rows, code, step, what):
    T, B = sym.shape
    with _coder(m, B) as c, _coder(m, B) as ref:
        c.load_fsm(m.tables, m.next)
        tr = torch.full((T, B, 2), SENTINEL, dtype=torch.int64, device=DEV)
        rt = torch.full((T, B, 2), SENTINEL, dtype=torch.int64, device=DEV)
        c.reset()
        c.set_fsm_states(s0)
        c.encode_fsm(dev_i32(sym), trace=tr)
        ref.reset()
        ref.encode(E.dev_pmf(rows, DEV), dev_i32(sym), trace=rt)
        rc, err, es = c.status()
        assert np.array_equal(err, code) and np.array_equal(es, step), (what, err, es)
        a, b = c.checkpoint(), ref.checkpoint()
        same_fields(a["state"], b["state"], ENC_FIELDS, what)
        t, r = tr.cpu().numpy(), rt.cpu().numpy()
        assert np.array_equal(t, r), what
        for i in range(B):
            n = T if code[i] == 0 else int(step[i])
            assert (t[n:, i] == SENTINEL).all(), (what, i)
            assert (t[:n, i, 1] >= 0).all() and (t[:n, i, 1] <= 64).all(), (what, i)
            assert int(t[:n, i, 1].sum()) == int(a["state"]["L"][i]), (what, i)


def test_traces_are_the_pmf_paths(fc):  # noqa: F811
    """encode_fsm(sym, trace=...) writes {E, k} of every coded step as encode does on the gathered
    rows; the failing step's entry and every later one is not written."""
    y = _layout(fc, 6, 1000, 32, True)
    (m, s0, sym, _, _), = _sparse_models(32, 48, 1000, y["Vp"] // y["nvec"], y["nvec"], y["G"])[0]
    rows = m.gathered(m.walk(s0, sym)[:-1])
    v = verdict(m, rows, sym)
    assert not v["code"].any()
    _trace_check(m, s0, sym, rows, v["code"], v["step"], "sparse")
    m, s0, sym, q, code, step = _error_job()
    rows = m.gathered(q[:-1])
    v = verdict(m, rows, sym)
    assert np.array_equal(v["code"], code) and np.array_equal(v["step"], step)
    _trace_check(m, s0, sym, rows, code, step, "errors")
