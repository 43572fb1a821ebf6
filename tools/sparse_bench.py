#!/usr/bin/env python3
"""Sparse rows (lac_encode_sparse / lac_decode_sparse_steps) against the means the coder had before:
the same job through encode_job / decode over the materialised dense u64 rows (measurement aid, not
the metric; results in profiles/sparse/README.md).

    python tools/sparse_bench.py [--steps 256] [--reps 10] [--streams 1,64,4096]

V = 32000, K = 64 pairs a row over a floor of 1 (weights below 2^24, as lac_amd.sparse.topk_rows
makes them), prec 48; the symbols are a pair of their row with probability 0.8 and uniform
otherwise.  The two sides alternate in one session, `reps` rounds after a warm round of each, device
events around every job:
  sparse  encode_sparse_job / decode_open + decode_sparse over idx, wt [steps, streams, K]
  dense   encode_job / decode_open + decode over dense_rows(idx, wt) as u64 [steps, streams, V]; where
          that does not fit --max-rows-gib the dense side keeps only the rows of as many steps as
          fit and both sides code that shorter job (`steps` in the line says how many) -- per step
          the dense side reads the same 8 V bytes a stream either way -- and the sparse side then
          runs once more alone at the full length
Bytes and decoded symbols are compared between the sides.  --only sparse|dense runs one side alone
(for a kernel trace of its own).  One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def job_ms(fn):
    """Device ms of one call of fn."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def draw(rng, T, B, V, K):
    """idx int32 [T, B, K] ascending, wt int64 [T, B, K] below 2^24, sym int32 [T, B]."""
    import numpy as np
    idx = np.cumsum(rng.integers(1, V // K + 1, size=(T, B, K)), axis=-1) - 1
    wt = np.floor((1 << 24) * np.exp(-8.0 * rng.random((T, B, K)))).astype(np.int64)
    at = np.take_along_axis(idx, rng.integers(0, K, size=(T, B, 1)), -1)[..., 0]
    sym = np.where(rng.random((T, B)) < 0.8, at, rng.integers(0, V, size=(T, B)))
    return idx.astype(np.int32), wt, sym.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--streams", default="1,64,4096")
    ap.add_argument("--vocab", type=int, default=32000)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--prec", type=int, default=48)
    ap.add_argument("--max-rows-gib", type=float, default=16.0)
    ap.add_argument("--only", choices=("sparse", "dense"), default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from lac_amd.batch import BatchCoder
    from lac_amd.sparse import dense_rows
    if not torch.cuda.is_available():
        sys.exit("sparse_bench: no HIP device (a timing needs the GPU)")
    dev = torch.device("cuda", 0)
    V, K, prec, base = a.vocab, a.slots, a.prec, 1

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    def run(B, only):
        row_gib = B * V * 8 / 2 ** 30
        T = a.steps if only == "sparse" else max(1, min(a.steps, int(a.max_rows_gib / row_gib)))
        idx, wt, sym = (torch.from_numpy(x).to(dev) for x in draw(np.random.default_rng(B), T, B, V, K))
        wt32 = wt.to(torch.int32)                              # (below 2^24: the same values; no conversion in the timed call)
        cap = T * (prec + 2) + 256
        out_s = torch.empty((T, B), dtype=torch.int32, device=dev)
        out_d = torch.empty((T, B), dtype=torch.int32, device=dev)
        with BatchCoder(V, B, prec=prec, pmf_bits=64, capacity_bits=cap, device=dev) as cs, \
                BatchCoder(V, B, prec=prec, pmf_bits=64, capacity_bits=cap, device=dev) as cd:
            pmf = None
            if only != "sparse":
                pmf = torch.empty((T, B, V), dtype=torch.int64, device=dev)
                for t in range(T):                             # step by step: no second copy of the rows
                    pmf[t] = dense_rows(idx[t], wt[t], base, V)

            def s_enc():
                cs.encode_sparse_job(idx, wt32, base, sym)

            def s_dec():
                cs.decode_open()
                cs.decode_sparse(idx, wt32, base, out=out_s)

            def d_enc():
                cd.encode_job(pmf, sym)

            def d_dec():
                cd.decode_open()
                cd.decode(pmf, out=out_d)

            sides = [s for s in ("sparse", "dense") if only in (None, s)]
            fns = {"sparse": (s_enc, s_dec), "dense": (d_enc, d_dec)}
            ms = {s: ([], []) for s in sides}
            for rep in range(a.reps + 1):                      # round 0 warms both sides up
                for s in sides:
                    e, d = job_ms(fns[s][0]), job_ms(fns[s][1])
                    if rep:
                        ms[s][0].append(e)
                        ms[s][1].append(d)
            same = None
            if only is None:
                bs, bd = cs.to_bytes(), cd.to_bytes()             # (the bytes of every stream: the slots past them are not compared)
                same = bool(bs[0] == bd[0] and np.array_equal(bs[1], bd[1]) and torch.equal(out_s, out_d))
            for s in sides:
                c = cs if s == "sparse" else cd
                c.raise_on_error()
                out = out_s if s == "sparse" else out_d
                enc, dec = float(np.median(ms[s][0])), float(np.median(ms[s][1]))
                row_bytes = 8 * K if s == "sparse" else 8 * V
                emit(what=s, streams=B, steps=T, vocab=V, slots=K, reps=a.reps, encode_ms=enc, decode_ms=dec,
                     encode_ms_min=min(ms[s][0]), encode_ms_max=max(ms[s][0]), decode_ms_min=min(ms[s][1]),
                     decode_ms_max=max(ms[s][1]), encode_us_per_step=enc * 1e3 / T, decode_us_per_step=dec * 1e3 / T,
                     row_bytes=row_bytes, encode_gb_s=T * B * row_bytes / enc / 1e6, decode_gb_s=T * B * row_bytes / dec / 1e6,
                     round_trip=bool(torch.equal(out, sym)), same_as_other_side=same,
                     bits_per_symbol=float(c.nbits_tensor().sum()) / (T * B))
            if only is None:
                emit(what="ratio", streams=B, steps=T, encode_dense_over_sparse=float(np.median(ms["dense"][0]) / np.median(ms["sparse"][0])),
                     decode_dense_over_sparse=float(np.median(ms["dense"][1]) / np.median(ms["sparse"][1])))

        return T

    for B in (int(x) for x in a.streams.split(",") if x):
        if run(B, a.only) < a.steps and a.only is None:        # the dense rows cut the job short: the sparse side at full length too
            run(B, "sparse")


if __name__ == "__main__":
    main()
