"""Sparse rows: at most K (symbol, weight) pairs over a uniform floor (include/lac.h
lac_encode_sparse / lac_decode_sparse_steps, BatchCoder.encode_sparse / decode_sparse).

A row is ``idx[..., K]`` (int32: ascending symbols, then -1 pads), ``wt[..., K]`` (their weights)
and one integer ``base``; it stands for the dense table ``pmf[s] = base + wt_j where s == idx_j``.

* :func:`dense_rows`      the dense uint64 rows, for checking and for users of the table paths
* :func:`topk_rows`       sparse rows from logits: the top k, a floor under the rest
* :func:`topk_rows_q1`    the same from one kernel and an integer-exact rule (BatchCoder.topk_logits)
* :class:`TopKCompressor` batched LLM compression that codes each position's top-k row
"""
from __future__ import annotations

import numpy as np


def dense_rows(idx, wt, base, V):
    """The dense rows of sparse rows: ``idx``, ``wt`` [..., K] (torch tensors or arrays) ->
    [..., V] with ``base`` everywhere plus ``wt_j`` at ``idx_j`` for the leading slots with
    ``idx >= 0``.  Torch tensors give an int64 tensor on their device (the bit pattern of the
    uint64 rows a ``pmf_bits = 64`` coder takes), arrays give a uint64 array."""
    V, base = int(V), int(base)
    try:
        import torch
        is_torch = isinstance(idx, torch.Tensor)
    except ImportError:                                        # pragma: no cover
        is_torch = False
    if is_torch:
        lead = (idx >= 0).to(torch.int64).cumprod(-1).bool()   # the leading pairs
        if bool((lead & (idx >= V)).any()):
            raise ValueError(f"a pair's symbol is outside [0, {V})")
        w = wt.to(torch.int64)
        if wt.dtype == torch.int32:
            w = w & 0xFFFFFFFF                                 # the bit pattern of uint32
        out = torch.full((*idx.shape[:-1], V), base, dtype=torch.int64, device=idx.device)
        out.scatter_add_(-1, torch.where(lead, idx, torch.zeros_like(idx)).to(torch.int64), torch.where(lead, w, torch.zeros_like(w)))
        return out
    idx = np.asarray(idx)
    w = np.asarray(wt).astype(np.int64) & 0xFFFFFFFF
    lead = np.cumprod(idx >= 0, axis=-1).astype(bool)
    if (lead & (idx >= V)).any():
        raise ValueError(f"a pair's symbol is outside [0, {V})")
    out = np.full((*idx.shape[:-1], V), base, dtype=np.uint64)
    flat_o, flat_i, flat_w, flat_l = out.reshape(-1, V), idx.reshape(-1, idx.shape[-1]), w.reshape(-1, idx.shape[-1]), \
        lead.reshape(-1, idx.shape[-1])
    for r in range(flat_o.shape[0]):
        np.add.at(flat_o[r], flat_i[r][flat_l[r]], flat_w[r][flat_l[r]].astype(np.uint64))
    return out


def topk_rows(logits, k, weight_bits=24, base=1, prec=48):
    """Sparse rows of logits [..., V]: ``torch.topk`` keeps k entries per row, the survivors are
    sorted by index, and ``wt = floor(2^weight_bits * exp(l - l_max))`` in float64 (the maximum
    gets exactly 2^weight_bits); K is k rounded up to a multiple of 4, padded with -1.
    -> (idx int32 [..., K], wt int64 [..., K], base).  Raises if the largest total such rows can
    have, ``base * V + K * 2^weight_bits``, exceeds 2^(prec-1): rows that could fudge are refused."""
    import torch
    V, k, weight_bits, base = logits.shape[-1], int(k), int(weight_bits), int(base)
    if not 1 <= k <= min(V, 256):
        raise ValueError(f"k = {k}: between 1 and min(V, 256)")
    if not 0 <= weight_bits < 32 or not 1 <= base < 1 << 32:
        raise ValueError("weight_bits in [0, 32), base in [1, 2^32)")
    K = (k + 3) // 4 * 4
    if base * V + K * (1 << weight_bits) > 1 << (prec - 1):
        raise ValueError(f"base * V + K * 2^weight_bits = {base * V + K * (1 << weight_bits)} exceeds 2^(prec-1) = "
                         f"2^{prec - 1}: lower weight_bits or base, or raise prec")
    vals, ids = torch.topk(logits, k, dim=-1)
    ids, order = torch.sort(ids, dim=-1)
    vals = torch.gather(vals, -1, order).to(torch.float64)
    lmax = vals.max(dim=-1, keepdim=True).values
    wt = torch.floor(torch.exp(vals - lmax) * float(1 << weight_bits)).to(torch.int64)
    idx = torch.full((*logits.shape[:-1], K), -1, dtype=torch.int32, device=logits.device)
    w = torch.zeros((*logits.shape[:-1], K), dtype=torch.int64, device=logits.device)
    idx[..., :k] = ids.to(torch.int32)
    w[..., :k] = wt
    return idx, w, base


def topk_rows_q1(coder, logits, k, weight_bits=24, base=1):
    """Sparse rows of logits by the integer-exact q1 rule, in one launch
    (:meth:`lac_amd.batch.BatchCoder.topk_logits`, include/lac.h lac_topk_logits): the k heaviest
    q1 entries per row, the lower symbol first among equal weights, ``wt = TAB[544 - level] >>
    (24 - weight_bits)``; K is k rounded up to a multiple of 4, padded with -1.
    -> (idx int32 [steps, streams, K], wt int32 bit patterns [steps, streams, K], base).  Raises as
    :func:`topk_rows` does if ``base * V + K * 2^weight_bits`` exceeds 2^(prec-1) of the coder."""
    V, k, weight_bits, base = coder.vocab, int(k), int(weight_bits), int(base)
    if not 1 <= k <= min(V, 256):
        raise ValueError(f"k = {k}: between 1 and min(V, 256)")
    if not 0 <= weight_bits <= 24 or not 1 <= base < 1 << 32:
        raise ValueError("weight_bits in [0, 24], base in [1, 2^32)")
    K = (k + 3) // 4 * 4
    if base * V + K * (1 << weight_bits) > 1 << (coder.prec - 1):
        raise ValueError(f"base * V + K * 2^weight_bits = {base * V + K * (1 << weight_bits)} exceeds 2^(prec-1) = "
                         f"2^{coder.prec - 1}: lower weight_bits or base, or raise prec")
    idx, wt = coder.topk_logits(logits, k, weight_bits, K)
    return idx, wt, base


class TopKCompressor:
    """Batched LLM compression over top-k rows: step t codes token t under the sparse row of the
    model's logits after ``[BOS] + tokens[:, :t]`` -- the k most likely tokens by their weights,
    every other token by the floor.  For incremental modules only (``init_cache`` / ``step``, e.g.
    ``lac_amd.llm.TinyCausalLM``): one cached model step per position on both sides,
    ``encode_sparse`` on compress and a one-step ``decode_sparse`` on decompress, so a position
    moves 8 K bytes to the coder where a dense row moves 8 V.  Both sides compute the rows the
    same way from bit-identical logits, so the code is lossless.  ``rule``: "float" (default) builds
    the rows with :func:`topk_rows` (torch.topk and a float64 exp on the device); "q1" builds them
    with :func:`topk_rows_q1`, one kernel and an integer-exact rule that does not depend on the
    platform's floating point or on how torch.topk breaks ties (weight_bits <= 24; the model's
    logits must be bf16 or f32 with a vocabulary that is a multiple of 8 or 4)."""

    def __init__(self, module, vocab, k, weight_bits=24, base=1, prec=48, bos=1, device="cuda", rule="float"):
        import torch
        if not (hasattr(module, "step") and hasattr(module, "init_cache")):
            raise TypeError("TopKCompressor needs an incremental module (init_cache / step)")
        self.module = module.to(device).eval()
        self.vocab, self.k, self.weight_bits, self.base = int(vocab), int(k), int(weight_bits), int(base)
        self.prec, self.bos = int(prec), int(bos)
        self.device = torch.device(device)
        if rule not in ("float", "q1"):
            raise ValueError('rule: "float" or "q1"')
        if rule == "q1" and not 0 <= self.weight_bits <= 24:
            raise ValueError('rule "q1": weight_bits in [0, 24]')
        self.rule = rule
        K = (self.k + 3) // 4 * 4
        if self.base * self.vocab + K * (1 << self.weight_bits) > 1 << (self.prec - 1):
            raise ValueError("base * vocab + K * 2^weight_bits exceeds 2^(prec-1)")

    def _row(self, lg, coder):
        """the sparse rows (idx [1, B, K], wt [1, B, K]) of one position's logits [B, V]"""
        import torch
        if self.rule == "q1":
            if lg.dtype not in (torch.bfloat16, torch.float32):
                lg = lg.float()
            idx, wt, _ = topk_rows_q1(coder, lg.contiguous(), self.k, self.weight_bits, self.base)
            return idx, wt
        idx, wt, _ = topk_rows(lg, self.k, self.weight_bits, self.base, self.prec)
        return idx[None], wt[None]

    def _steps(self, B, T, feed, coder=None):
        """yields (t, idx [1, B, K], wt [1, B, K]) for t < T; feed(t) -> the tokens [B] fed at t + 1.
        ``coder``: the B-stream coder whose topk_logits builds the rows under rule "q1"."""
        import torch
        cache = self.module.init_cache(B, T)
        tok = torch.full((B,), self.bos, dtype=torch.long, device=self.device)
        for t in range(T):
            with torch.no_grad():
                lg = self.module.step(tok, cache, t)[:, :self.vocab]
            idx, wt = self._row(lg, coder)
            yield t, idx, wt
            tok = feed(t)
            tok = torch.where(tok < 0, torch.full_like(tok, self.bos), tok)   # (a failed stream's -1: raised at the end)

    def rows(self, tokens):
        """The sparse rows compress codes tokens[B, T] with: (idx [T, B, K], wt [T, B, K], base)."""
        import torch
        tokens = tokens.to(self.device, torch.long)
        B, T = tokens.shape
        coder = self._coder(B, T) if self.rule == "q1" else None
        try:
            got = [(i, w) for _, i, w in self._steps(B, T, lambda t: tokens[:, t], coder)]
        finally:
            if coder is not None:
                coder.close()
        return torch.cat([i for i, _ in got], 0), torch.cat([w for _, w in got], 0), self.base

    def _coder(self, B, T):
        from .batch import BatchCoder
        return BatchCoder(self.vocab, B, prec=self.prec, pmf_bits=64, capacity_bits=T * (self.prec + 2) + 256,
                          device=self.device)

    def compress(self, tokens):
        """tokens: int tensor [B, T] -> (list of B byte strings, nbits uint64[B])."""
        import torch
        tokens = tokens.to(self.device, torch.long)
        B, T = tokens.shape
        sym = tokens.t().contiguous().to(torch.int32)              # [T, B]
        coder = self._coder(B, T)
        try:
            coder.reset()
            for t, idx, wt in self._steps(B, T, lambda t: tokens[:, t], coder):
                coder.encode_sparse(idx, wt, self.base, sym[t:t + 1])
            coder.finish()
            coder.raise_on_error()
            return coder.to_bytes()
        finally:
            coder.close()

    def decompress(self, data, nbits, T):
        """Inverse of compress: B byte strings + bit counts -> tokens [B, T] (long)."""
        import torch
        B = len(data)
        stride = max(8, (max((len(d) for d in data), default=0) + 8) // 8 * 8)
        buf = np.zeros((B, stride), dtype=np.uint8)
        for b, d in enumerate(data):
            buf[b, :len(d)] = np.frombuffer(d, dtype=np.uint8)
        coder = self._coder(B, T)
        try:
            coder.decode_open(torch.from_numpy(buf).to(self.device),
                              torch.as_tensor(np.asarray(nbits, dtype=np.int64), device=self.device))
            out = torch.empty((B, T), dtype=torch.long, device=self.device)
            for t, idx, wt in self._steps(B, T, lambda t: out[:, t], coder):
                out[:, t] = coder.decode_sparse(idx, wt, self.base)[0].to(torch.long)
            coder.raise_on_error()
            return out
        finally:
            coder.close()
