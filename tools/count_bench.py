#!/usr/bin/env python3
"""Adaptive n-gram count models (lac_count_*): one launch each way against the means the coder
had before (measurement aid, not the metric; results in profiles/counts/README.md).

    python tools/count_bench.py [--tokens 4096] [--reps 20] [--streams 1,64,4096] [--orders 1,2]

Order-1 (W = [1]) and order-2 (W = [1, 300]) byte models (V = 256, u32 rows, prec 48), T tokens
per stream, the symbol two back repeated with probability 1/2:
  counts   encode_counts_job / decode_open + set_count_state + decode_counts, device events around
           `reps` jobs after a warm-up, per job and per coded step
  rows     the same symbols through encode_job on the materialised rows pmf[T, B, V] of the same
           job (built on the device by a step-by-step walk of the counts, not timed; same bytes,
           checked), while it fits --max-rows-gib
  loop     decode by a per-position loop -- the row built from the counts, one lac_decode_steps(1)
           launch, the symbol read back, the counts updated -- the only way the pmf path can decode
           such a model, at B <= 64 over --loop-tokens positions
One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WEIGHTS = {1: [1], 2: [1, 300]}


def timed(fn, reps):
    """Device ms per call of fn over `reps` calls, after one warm call."""
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


class Walk:
    """The counts of B streams as device tensors, for orders 1 and 2: the row of the next step
    and the update by the symbols taken (the host restatement of tests/counts.py, vectorised)."""

    def __init__(self, order, B, V, dev):
        import torch
        self.torch, self.order, self.W, self.V, self.t = torch, order, WEIGHTS[order], V, 0
        self.c0 = torch.zeros((B, V), dtype=torch.int32, device=dev)
        self.c1 = torch.zeros((B, V, V), dtype=torch.int32, device=dev) if order > 1 else None
        self.prev = None
        self.ar = torch.arange(B, device=dev)

    def row(self):
        row = 1 + self.W[0] * self.c0 if self.t >= 1 else self.torch.ones_like(self.c0)
        if self.order > 1 and self.t >= 2:
            row = row + self.W[1] * self.c1[self.ar, self.prev]
        return row

    def accept(self, s):
        s = s.long()
        if self.t >= 1:
            self.c0[self.ar, s] += 1
        if self.order > 1 and self.t >= 2:
            self.c1[self.ar, self.prev, s] += 1
        self.prev = s
        self.t += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--streams", default="1,64,4096")
    ap.add_argument("--orders", default="1,2")
    ap.add_argument("--loop-tokens", type=int, default=512)
    ap.add_argument("--max-rows-gib", type=float, default=24.0)
    ap.add_argument("--prec", type=int, default=48)
    a = ap.parse_args()
    import numpy as np
    import torch
    from lac_amd.batch import BatchCoder
    dev = torch.device("cuda", 0)
    T, P, V = a.tokens, a.prec, 256

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    def run(order, B):
        rng = np.random.default_rng(100 * order + B)
        s = rng.integers(0, V, size=(T, B), dtype=np.int32)
        rep = rng.random((T, B)) < 0.5
        for t in range(2, T):
            s[t] = np.where(rep[t], s[t - 2], s[t])
        sym = torch.from_numpy(s).to(dev)
        with BatchCoder(V, B, prec=P, capacity_bits=T * (P + 2) + 256, device=dev) as c:
            c.load_counts(order, WEIGHTS[order])
            enc = timed(lambda: c.encode_counts_job(sym), a.reps)
            out = torch.empty((T, B), dtype=torch.int32, device=dev)

            def dec():
                c.decode_open()
                c.set_count_state()
                c.decode_counts(T, out=out)
            d = timed(dec, a.reps)
            c.raise_on_error()
            ok = bool(torch.equal(out, sym))
            emit(what="counts", order=order, streams=B, tokens=T, reps=a.reps, encode_ms=enc, decode_ms=d,
                 encode_us_per_step=enc * 1e3 / T, decode_us_per_step=d * 1e3 / T,
                 encode_msym_s=T * B / enc / 1e3, decode_msym_s=T * B / d / 1e3, round_trip=ok,
                 counts_mib=B * c.count_layout["stride"] * 4 / 2 ** 20)
            c.encode_counts_job(sym)
            want = c.bits_tensor().clone(), c.nbits_tensor().clone()
            # the parent's means: the rows of the job, materialised
            gib = T * B * V * 4 / 2 ** 30
            if gib <= a.max_rows_gib:
                pmf = torch.empty((T, B, V), dtype=torch.int32, device=dev)
                w = Walk(order, B, V, dev)
                for t in range(T):
                    pmf[t] = w.row()
                    w.accept(sym[t])
                del w
                reps = max(3, min(a.reps, int(40 / max(gib, 0.05))))
                g = timed(lambda: c.encode_job(pmf, sym), reps)
                same = bool(torch.equal(c.bits_tensor(), want[0]) and torch.equal(c.nbits_tensor(), want[1]))
                emit(what="rows", order=order, streams=B, tokens=T, reps=reps, pmf_gib=gib, encode_ms=g,
                     encode_us_per_step=g * 1e3 / T, same_bytes=same)
                del pmf
            else:
                emit(what="rows", order=order, streams=B, tokens=T, skipped=f"the rows would take {gib:.0f} GiB")
            if B <= 64:
                n = min(a.loop_tokens, T)
                got = torch.empty((n, B), dtype=torch.int32, device=dev)

                def loop():
                    c.decode_open(*want)
                    w = Walk(order, B, V, dev)
                    for t in range(n):
                        s1 = c.decode(w.row().unsqueeze(0))[0]           # one lac_decode_steps(1) launch
                        got[t] = s1.cpu().to(dev)                        # the readback the next row waits for
                        w.accept(got[t])
                lp = timed(loop, 2)
                emit(what="loop", order=order, streams=B, tokens=n, reps=2, decode_ms=lp, decode_us_per_step=lp * 1e3 / n,
                     round_trip=bool(torch.equal(got, sym[:n])))

    for order in (int(x) for x in a.orders.split(",") if x):
        for B in (int(x) for x in a.streams.split(",") if x):
            run(order, B)


if __name__ == "__main__":
    main()
