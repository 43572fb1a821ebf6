"""Range-level coding helpers (include/lac.h lac_encode_ranges / lac_decode_ranges_step).

The coder needs three integers per symbol -- ``lo = c_{s-1}``, ``hi = c_s`` and the total ``T`` --
which is all the reference's ``CDFPredictor.symbol_to_range`` reads of its ``dist``
(arith_code.py:98-110).  :class:`lac_amd.batch.BatchCoder` takes them directly
(``encode_ranges``, ``encode_ranges_job``, ``decode_ranges_step``), so a model whose distribution
is a formula, or whose alphabet is too large to write out per step, codes on the device with no
table.  Here: the triples of a table job, and the serving loop of a decode.

    class Uniform:                         # V equally likely symbols, V up to 2^(prec-1)
        def __init__(self, V): self.V = V
        def total(self, t): return self.V
        def lookup(self, t, targets): return targets, targets, targets + 1

    coder.encode_ranges_job(sym, sym + 1, V)       # sym int64 [steps, streams]
    coder.decode_open()
    out = decode_loop(coder, steps, Uniform(V))    # == sym
"""
from __future__ import annotations


def table_ranges(pmf, sym):
    """The triples of a table job: ``pmf`` [steps, streams, V] (or anything that broadcasts to it:
    [V], [streams, V], [steps, 1, V]) integer rows, ``sym`` [steps, streams] integer symbols in
    [0, V) -> ``(lo, hi, tot)`` int64 [steps, streams] with ``lo = c_{s-1}``, ``hi = c_s``,
    ``tot = c_{V-1}`` (cumsum + gather, on the tensors' device).  uint32 / uint64 rows kept in
    int32 / int64 storage are read as unsigned; totals must stay below 2^63."""
    import torch
    sym = sym.to(torch.int64)
    if sym.dim() == 1:
        sym = sym.unsqueeze(0)
    steps, streams = sym.shape
    p = pmf
    if p.dtype in (torch.int32, torch.uint32):
        p = p.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    elif p.dtype == torch.uint64:
        p = p.view(torch.int64)
    else:
        p = p.to(torch.int64)
    while p.dim() < 3:
        p = p.unsqueeze(0)
    cdf = torch.cumsum(p, dim=-1).expand(steps, streams, p.shape[-1])
    idx = sym.unsqueeze(-1)
    hi = torch.gather(cdf, 2, idx).squeeze(-1)
    lo = torch.where(sym > 0, torch.gather(cdf, 2, (idx - 1).clamp(min=0)).squeeze(-1), torch.zeros_like(hi))
    tot = cdf[..., -1]
    return lo.contiguous(), hi.contiguous(), tot.contiguous()


def decode_loop(coder, steps, model):
    """Decode ``steps`` symbols per stream from the opened bits, one launch per position:
    ``model.total(t)`` gives position t's totals (int64 device tensor [streams] or a Python int)
    and ``model.lookup(t, targets) -> (sym, lo, hi)`` maps the targets (int64 device tensor
    [streams]; -1 for a stream that is not decoding) to each stream's symbol and its range, on the
    device -- the model's ``val_to_symbol`` and ``symbol_to_range``.  -> int64 [steps, streams]
    symbols (-1 from the step a stream stopped at: a sticky error, its count, or
    ``set_decode_stop``).  No host synchronisation inside the loop; one before and one after it,
    to count what every stream decoded."""
    import torch
    B = coder.streams
    out = torch.full((steps, B), -1, dtype=torch.int64, device=coder.device)
    prev = None
    nsym0 = _decoded(coder)
    for t in range(steps):
        tot = model.total(t)
        if not isinstance(tot, torch.Tensor):
            tot = torch.full((B,), int(tot), dtype=torch.int64, device=coder.device)
        targets = coder.decode_ranges_step(prev, tot)
        sym, lo, hi = model.lookup(t, targets)
        out[t] = torch.where(targets >= 0, sym.to(torch.int64), torch.full_like(targets, -1))
        prev = (lo.to(torch.int64).contiguous(), hi.to(torch.int64).contiguous(), tot)
    if prev is not None:
        coder.decode_ranges_step(prev, None)                   # the last symbol's advance
    # a target names a symbol; the advance after it is what decodes it -- or refuses it
    done = torch.from_numpy(_decoded(coder) - nsym0).to(coder.device)
    rows = torch.arange(steps, device=coder.device).unsqueeze(1)
    return torch.where(rows < done.unsqueeze(0), out, torch.full_like(out, -1))


def _decoded(coder):
    """Symbols every stream has decoded (lac_decode_get_state's nsym); synchronises."""
    import ctypes as C

    import numpy as np

    from ._lib import check
    from .coder import _DEC_STATE
    st = np.zeros(coder.streams, dtype=_DEC_STATE)
    check(coder.lib.lac_decode_get_state(coder.ctx, st.ctypes.data_as(C.c_void_p), coder._stream))
    return st["nsym"].astype(np.int64)
