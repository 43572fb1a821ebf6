#!/usr/bin/env python3
"""Per-stream symbol counts (lac_set_stream_lengths): what they cost and what they save
(measurement aid, not the metric; results in profiles/ragged/README.md).

    python tools/ragged_bench.py --mode job  [--counts none|uniform] [--reps 5]
        the c3 job (V = 32000, 4096 streams, 16 steps): encode job + decode, device time of
        the kernels (liblac.so's hipEvents), with counts uniform in [0, tokens] from a
        fixed seed or with none; prints the live-row and all-row bytes for the
        FETCH_SIZE ratio.  Under `rocprofv3 --pmc FETCH_SIZE` (a run of its own) pass
        --reps 1 and read the kernels' counters with tools/pmc_summary.py.
    python tools/ragged_bench.py --mode few [--streams 8] [--tokens 512]
        few-stream decode: half of the streams ending at tokens / 2 against the same job
        with no counts, us per step for both.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ENC_KIDS, DEC_KIDS = (0, 1, 2, 4), (3, 5)


def _timed(coder, fn, reps):
    """Summed device ms per kernel id over `reps` calls of fn (after one warm call)."""
    import torch
    fn()
    torch.cuda.synchronize()
    ms = (C.c_double * 8)()
    cnt = (C.c_int64 * 8)()
    coder.lib.lac_profile_read(coder.ctx, None, None, 1)
    coder.lib.lac_profile_enable(coder.ctx, 1)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    coder.lib.lac_profile_enable(coder.ctx, 0)
    coder.lib.lac_profile_read(coder.ctx, C.cast(ms, C.c_void_p), C.cast(cnt, C.c_void_p), 1)
    return [ms[k] / reps for k in range(8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("job", "few"), default="job")
    ap.add_argument("--vocab", type=int, default=32000)
    ap.add_argument("--streams", type=int, default=None)
    ap.add_argument("--tokens", type=int, default=None)
    ap.add_argument("--prec", type=int, default=48)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--counts", choices=("none", "uniform"), default="uniform")
    ap.add_argument("--seed", type=int, default=2024)
    a = ap.parse_args()
    import numpy as np
    import torch
    from lac_amd import synth
    from lac_amd.batch import BatchCoder
    dev = torch.device("cuda", 0)
    V, P = a.vocab, a.prec
    B = a.streams or (4096 if a.mode == "job" else 8)
    T = a.tokens or (16 if a.mode == "job" else 512)
    coder = BatchCoder(V, B, prec=P, capacity_bits=T * (P + 2) + 256, device=dev)
    tab, sym = synth.softmax_tables(T, B, V, device=dev, scale_bits=31)
    if a.mode == "job":
        n = np.random.default_rng(a.seed).integers(0, T + 1, size=B) if a.counts == "uniform" else np.full(B, T)
    else:
        n = np.where(np.arange(B) % 2 == 0, T, T // 2) if a.counts == "uniform" else np.full(B, T)
    coder.set_stream_lengths(n if a.counts == "uniform" else None)
    want = sym.clone()
    live = torch.arange(T, device=dev)[:, None] < torch.as_tensor(n, device=dev)[None, :]
    want[~live] = -1

    def enc():
        coder.encode_job(tab, sym)

    def dec():
        coder.decode_open()
        return coder.decode(tab)

    if a.reps <= 1:                                             # a counter run: each kernel once
        enc()
        out = dec()
        torch.cuda.synchronize()
        e = d = None
    else:
        e = _timed(coder, enc, a.reps)
        d = _timed(coder, dec, a.reps)
        out = dec()
    coder.raise_on_error()
    ok = bool(torch.equal(out, want))
    row = V * 4
    res = {"mode": a.mode, "counts": a.counts, "vocab": V, "streams": B, "tokens": T, "reps": a.reps,
           "live_rows": int(n.sum()), "all_rows": B * T, "live_row_bytes": int(n.sum()) * row,
           "all_row_bytes": B * T * row, "round_trip": ok}
    if e is not None:
        res["encode_ms"] = sum(e[k] for k in ENC_KIDS)
        res["decode_ms"] = sum(d[k] for k in DEC_KIDS)
        res["decode_us_per_step"] = res["decode_ms"] * 1e3 / T
    print(json.dumps(res), flush=True)
    coder.close()


if __name__ == "__main__":
    main()
