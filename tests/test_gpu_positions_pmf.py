"""The integer-table path with the coded symbol placed at the row ends and on either side of
every 64-load iteration, lean chunk and fine / block wave boundary (tests/positions.py;
tests/test_positions_host.py asserts the census): every encoder against the C oracle's bytes,
every decode path back to the symbols.  Tables are ``synth.make_batch`` rows with the symbols
overwritten by the positions; in a table with zero entries a position whose entry is zero keeps
its drawn symbol.  Everything is bit-exact."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import positions                                                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEAN_B, LEAN_PREC = positions.PMF_LEAN_B, positions.PMF_LEAN_PREC   # the run k_decode_lean takes
# ... where its chunks hold the row (at most 4 iterations each): stated by hand, checked against decode_plan
LEAN = {(32000, 32), (32004, 32), (16000, 64)}


@functools.lru_cache(maxsize=None)
def _sel():
    return positions.load_select()


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a.view(np.int64)).to(DEV)


def _oracle(pmf, sym, prec):
    from oracle import oracle as coracle
    out, nb, status, rc = coracle.encode_batch(pmf, sym, prec, nthreads=16)
    assert rc == 0 and not status.any()
    return [out[b, :(int(nb[b]) + 7) // 8].tobytes() for b in range(pmf.shape[1])], nb


def _tables(V, bits, kind):
    """-> (case, tables for prec 48, tables for prec 40 (totals below 2^39: no fudged row), symbols)."""
    from lac_amd import synth
    case = positions.pmf_case(_sel(), V, bits)
    T, B = case.steps, case.B
    pmf, sym = synth.make_batch(V + bits, T, B, V, kind, exp_range=16)
    assert pmf.dtype == np.uint32 and int(pmf.sum(axis=-1, dtype=np.uint64).max()) < 1 << 39
    for r, p in enumerate(case.rows):
        if pmf[r // B, r % B, p]:
            sym[r // B, r % B] = p
    if bits == 32:
        return case, pmf, pmf, sym
    wide = pmf.astype(np.uint64)
    return case, wide << np.uint64(8), wide, sym                # u64 at prec 48: totals past 2^32


CASES = [(V, bits, "loguniform") for V, bits in positions.PMF_CASES] + [(32004, 32, "zeros"), (16000, 64, "zeros")]


@pytest.mark.parametrize("V,bits,kind", CASES)
def test_every_path_codes_every_boundary_position(V, bits, kind):
    from lac_amd.batch import BatchCoder
    case, pmf48, pmf40, sym = _tables(V, bits, kind)
    T, B, prec = case.steps, case.B, 48
    want, wbits = _oracle(pmf48, sym, prec)
    dp, ds = _dev(pmf48), torch.from_numpy(sym).to(DEV)
    with BatchCoder(V, B, prec=prec, pmf_bits=bits, capacity_bits=T * (prec + 2) + 256, device=DEV) as c:
        for enc in ("split", "fused", "auto"):
            c.set_path(enc)
            c.encode_job(dp, ds)
            got, gbits = c.to_bytes()
            assert (gbits == wbits).all() and got == want, enc
        c.raise_on_error()
        runs = [(p, 0) for p in ("split", "fused", "fused_chunk", "stats", "auto")] + [("block", w) for w in (4, 8, 16)]
        for path, waves in runs:
            c.set_decode_path(path)
            c.set_block_waves(waves)
            c.decode_open()
            dec = c.decode(dp)
            wrong = torch.nonzero(dec != ds)
            assert not len(wrong), (path, waves, [(int(t), int(b), int(dec[t, b]), int(ds[t, b])) for t, b in wrong[:4]])
        c.raise_on_error()
    del dp
    # prec 40 at LEAN_B streams: decode_plan takes k_decode_lean where its chunks hold the row (the
    # lean_chunk positions exist exactly there), k_decode_seq where not.  (A row with a zero entry
    # leaves the lean step for k_decode_seq at run time: the "zeros" tables cross that hand-over.)
    prec = LEAN_PREC
    lean, ci = positions.lean_plan(_sel(), V, bits, LEAN_B, prec)
    assert lean == ((V, bits) in LEAN) and (not lean or ci <= 4), (lean, ci)
    assert ("lean_chunk" in case.P.classes) == lean
    assert (T * B) % LEAN_B == 0
    pmf, s = pmf40.reshape(-1, LEAN_B, V), sym.reshape(-1, LEAN_B)
    want, wbits = _oracle(pmf, s, prec)
    dp, ds = _dev(pmf), torch.from_numpy(s).to(DEV)
    with BatchCoder(V, LEAN_B, prec=prec, pmf_bits=bits, capacity_bits=pmf.shape[0] * (prec + 2) + 256,
                    device=DEV) as c:
        c.encode_job(dp, ds)
        got, gbits = c.to_bytes()
        assert (gbits == wbits).all() and got == want
        for path in ("stats", "auto"):
            c.set_decode_path(path)
            c.decode_open()
            assert torch.equal(c.decode(dp), ds), ("lean", path)
        c.raise_on_error()
