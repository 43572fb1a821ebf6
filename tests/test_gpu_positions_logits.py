"""The logits path with the coded symbol, the row maximum and the special values placed on every
block, segment, slot and vector boundary of every row-statistics form (tests/positions.py names
them; tests/test_positions_host.py asserts their census), in both directions, against the C
oracle (``oracle.q1_quantize`` + ``oracle.encode_batch`` on the exact device bit patterns).

One row per position p, of six kinds dealt round-robin (positions.KINDS):

    plain            symbol p in an ordinary random row
    sole_max         symbol p, x[p] the row's only maximum
    nan_ninf         x[p] = NaN / -NaN / -inf in turn, symbol p (its table entry is 1)
    pinf_neighbour   x[p] = +inf, symbol a neighbour of p
    capped_pair      x[p] = 3.0e5, x[p - 1] = 3.0e5 - 0.25 (the capped path), in turn with
                     x[p] = 262143.5, x[p - 1] = 262140.5 (the fast path's largest f32 maximum) and,
                     bf16, where those round to a tie and to 2^18, x[p] = 261120, x[p - 1] = 260096
                     (the largest bf16 values below 2^18: the fast path); symbol p
    signed_zero_max  bf16: every logit negative but x[p] = -0.0 / +0.0, the maximum; symbol p

The rows of a parametrisation are coded in successive [steps, B, V] jobs, each with at most
positions.LOGITS_BYTES of logits on the device.  Everything is bit-exact; nothing is compared with
the kernels' own output.
"""
import functools
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import positions                                                   # noqa: E402
from test_gpu_logits import _coder, _device_logits, _host_bits, _logits   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PREC = 48


@functools.lru_cache(maxsize=None)
def _sel():
    return positions.load_select()


def _rows(case, dtype, V, first, count):
    """The host logits [steps, B, V] (f32) and symbols [steps, B] of rows first .. first + count of a case."""
    B, steps = case.B, -(-count // case.B)
    base = _logits(V + B, 1, B, V)[0]                              # B ordinary rows, each step's starting point
    x = np.broadcast_to(base, (steps, B, V)).copy()
    sym = np.random.default_rng(V).integers(0, V, size=(steps, B)).astype(np.int32)
    f = np.float32
    for r, (p, kind, n) in enumerate(case.rows[first:first + count]):
        row = x[r // B, r % B]
        s = p
        if kind == 1:
            row[p] = row.max() + f(4)
        elif kind == 2:
            row[p] = (f(np.nan), -f(np.nan), -f(np.inf))[n % 3]
        elif kind == 3:
            row[p] = np.inf
            s = p + 1 if p + 1 < V and n % 2 == 0 else p - 1 if p else p + 1
        elif kind == 4:
            pairs = [(3.0e5, 3.0e5 - 0.25), (262143.5, 262143.5 - 3.0)] + [(261120.0, 260096.0)] * (dtype == "bf16")
            row[p], row[p - 1] = (f(v) for v in pairs[n % len(pairs)])
        elif kind == 5:
            row[:] = -np.abs(row) - f(1)
            row[p] = f(-0.0) if n % 2 == 0 else f(0.0)
        sym[r // B, r % B] = s
    return x, sym


def _quantize(bits, prec):
    """oracle.q1_quantize over the rows, a few rows per thread (the C call releases the GIL)."""
    from oracle import oracle as coracle
    flat = bits.reshape(-1, bits.shape[-1])
    parts = [flat[i:i + 8] for i in range(0, flat.shape[0], 8)]
    with ThreadPoolExecutor(8) as ex:
        out = list(ex.map(lambda a: coracle.q1_quantize(a, prec), parts))
    return np.concatenate(out).reshape(bits.shape)


def _batch(case, dtype, V, first, count):
    """One batch of a case's rows: device logits, the oracle's tables, symbols and bytes."""
    from oracle import oracle as coracle
    x, sym = _rows(case, dtype, V, first, count)
    dl = _device_logits(x, dtype)
    assert dl.numel() * dl.element_size() <= positions.LOGITS_BYTES
    del x
    pmf = _quantize(_host_bits(dl), PREC)
    for r, (p, kind, n) in enumerate(case.rows[first:first + count]):   # the rows are what their kind says
        row = pmf[r // case.B, r % case.B]
        if kind == 2:
            assert row[p] == 1, (p, n)
        elif kind == 3:
            assert (row == 1).all(), p                             # inf - inf: a NaN entry too
        elif kind in (1, 5):
            assert row[p] == row.max() and (row == row[p]).sum() == 1, (p, kind)
        elif kind == 4 and dtype == "bf16" and n % 3 == 2:         # the fast path's maximum, alone
            assert row[p] == row.max() and (row == row[p]).sum() == 1, p
    out, nb, status, rc = coracle.encode_batch(pmf, sym, PREC, nthreads=16)
    assert rc == 0 and not status.any()
    want = [out[b, :(int(nb[b]) + 7) // 8].tobytes() for b in range(case.B)]
    return types.SimpleNamespace(rows=case.rows[first:first + count], dl=dl, pmf=pmf, sym=sym,
                                 dsym=torch.from_numpy(sym).to(DEV), want=want, nb=nb, B=case.B, steps=sym.shape[0])


@pytest.mark.parametrize("dtype,V", positions.LOGITS_CASES)
def test_every_form_codes_every_boundary_position(dtype, V):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = positions.logits_case(_sel(), dtype, V, cus)
    for first, count in case.batches:
        _code_batch(dtype, V, case, _batch(case, dtype, V, first, count))


def _code_batch(dtype, V, case, k):
    from lac_amd._lib import LacError
    B, steps = k.B, k.steps
    cap = steps * (PREC + 2) + 256
    c = _coder(V, B, PREC, cap=cap)
    # the tables
    got = c.quantize_logits(k.dl)
    assert torch.equal(got.view(torch.int32), torch.from_numpy(k.pmf.view(np.int32)).to(DEV)), "quantize_logits"
    del got
    # AUTO and every forced shape the selection accepts for the row: bytes, bit counts, symbols
    ran = []
    for sh in range(0, 24):
        try:
            c.set_q1_shape(sh)
            c.encode_logits_job(k.dl, k.dsym)
        except LacError:
            continue
        data, n = c.to_bytes()
        assert [int(v) for v in n] == [int(v) for v in k.nb], sh
        bad = [b for b in range(B) if data[b] != k.want[b]]
        assert not bad, (sh, bad)
        c.decode_open()
        dec = c.decode_logits(k.dl)
        if not torch.equal(dec, k.dsym):
            t, b = (int(v[0]) for v in torch.nonzero(dec != k.dsym, as_tuple=True))
            r = t * B + b
            raise AssertionError((sh, "first wrong row", r, k.rows[r] if r < len(k.rows) else None,
                                  int(dec[t, b]), int(k.dsym[t, b])))
        c.raise_on_error()
        ran.append(sh)
    assert ran == [0] + sorted(case.P.shapes), ran
    c.close()
    # the fused one-position step
    if (dtype, V) in positions.STEP_CASES:
        from test_gpu_logits_step import _stream_cap
        assert B <= _stream_cap()
        c = _coder(V, B, PREC, cap=cap)
        c.set_q1_step("fused")
        c.reset()
        for t in range(steps):
            c.encode_logits_step(k.dl[t], k.dsym[t])
        c.finish()
        data, n = c.to_bytes()
        assert [int(v) for v in n] == [int(v) for v in k.nb] and data == k.want, "fused step"
        c.decode_open()
        dec = torch.empty((steps, B), dtype=torch.int32, device=DEV)
        for t in range(steps):
            c.decode_logits_step(k.dl[t], out=dec[t:t + 1])
        assert torch.equal(dec, k.dsym), "fused step decode"
        c.raise_on_error()
        c.close()
