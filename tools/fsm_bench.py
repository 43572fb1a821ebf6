#!/usr/bin/env python3
"""Finite-state models (lac_fsm_*): one launch each way against the means the coder had before
(measurement aid, not the metric; results in profiles/fsm/README.md).

    python tools/fsm_bench.py [--tokens 4096] [--reps 20] [--streams 1,64,4096] [--order2 4096]

An order-1 byte model (K = V = 256, u32 tables, prec 48; next[q][s] = s), T tokens per stream:
  fsm      encode_fsm_job / decode_open + decode_fsm, device events around `reps` jobs after a
           warm-up, per job and per coded step
  gathered the same symbols through encode_job on the materialised pmf[T, B, V] (V * 4 bytes
           per symbol where the finite-state job reads 4), while it fits --max-gather-gib
  loop     decode by a per-position lac_decode_step loop with the row picked on the host
           (a readback per symbol: the only way the pmf path can decode such a model), at
           B <= 64 over --loop-tokens positions
and one order-2 model (K = 65536: 64 MiB of tables, 64 MiB of CDF, 64 MiB of transitions) at
--order2 streams, to show the step once the tables leave the L2.  One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def model(order, seed=1):
    """(tables uint32 [K, 256] with every entry >= 1, next int32 [K, 256]) of an order-k byte model."""
    import numpy as np
    rng = np.random.default_rng(seed)
    K = 256 ** order
    t = rng.integers(1, 1 << 8, size=(K, 256), dtype=np.uint32)
    t[np.arange(K), rng.integers(0, 256, size=K)] += 1 << 14          # a likely successor per context
    q = np.arange(K, dtype=np.int64)[:, None]
    nxt = (((q & (K // 256 - 1)) << 8) | np.arange(256)[None, :]) if order > 1 else np.tile(np.arange(256), (K, 1))
    return t, nxt.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--streams", default="1,64,4096")
    ap.add_argument("--order2", type=int, default=4096, help="streams of the order-2 run (0: skip)")
    ap.add_argument("--loop-tokens", type=int, default=512)
    ap.add_argument("--max-gather-gib", type=float, default=24.0)
    ap.add_argument("--prec", type=int, default=48)
    a = ap.parse_args()
    import numpy as np
    import torch
    from lac_amd.batch import BatchCoder
    dev = torch.device("cuda", 0)
    T, P, V = a.tokens, a.prec, 256

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    def run(order, B, compare):
        tables, nxt = model(order)
        K = len(tables)
        rng = np.random.default_rng(100 + B)
        sym = torch.from_numpy(rng.integers(0, V, size=(T, B), dtype=np.int32)).to(dev)
        s0 = rng.integers(0, K, size=B)
        with BatchCoder(V, B, prec=P, capacity_bits=T * (P + 2) + 256, device=dev) as c:
            c.load_fsm(tables, nxt)
            enc = timed(lambda: c.encode_fsm_job(sym, state0=s0), a.reps)
            out = torch.empty((T, B), dtype=torch.int32, device=dev)

            def dec():
                c.decode_open()
                c.set_fsm_states(s0)
                c.decode_fsm(T, out=out)
            d = timed(dec, a.reps)
            c.raise_on_error()
            ok = bool(torch.equal(out, sym))
            emit(what="fsm", order=order, states=K, streams=B, tokens=T, reps=a.reps, encode_ms=enc, decode_ms=d,
                 encode_us_per_step=enc * 1e3 / T, decode_us_per_step=d * 1e3 / T,
                 encode_msym_s=T * B / enc / 1e3, decode_msym_s=T * B / d / 1e3, round_trip=ok)
            if not compare:
                return
            c.encode_fsm_job(sym, state0=s0)
            want = c.bits_tensor().clone(), c.nbits_tensor().clone()
            # the parent's means: the gathered pmf, materialised
            gib = T * B * V * 4 / 2 ** 30
            tab_dev = torch.from_numpy(tables.view(np.int32)).to(dev)
            nxt_dev = torch.from_numpy(nxt).to(dev).long()
            if gib <= a.max_gather_gib:
                q = torch.empty((T, B), dtype=torch.int64, device=dev)
                cur = torch.from_numpy(s0).to(dev).long()
                for t in range(T):
                    q[t] = cur
                    cur = nxt_dev[cur, sym[t].long()]
                pmf = tab_dev[q]                                         # [T, B, V]
                reps = max(3, min(a.reps, int(40 / max(gib, 0.05))))
                g = timed(lambda: c.encode_job(pmf, sym), reps)
                same = bool(torch.equal(c.bits_tensor(), want[0]) and torch.equal(c.nbits_tensor(), want[1]))
                emit(what="gathered", order=order, streams=B, tokens=T, reps=reps, pmf_gib=gib, encode_ms=g,
                     encode_us_per_step=g * 1e3 / T, same_bytes=same)
                del pmf
            else:
                emit(what="gathered", order=order, streams=B, tokens=T, skipped=f"the pmf would take {gib:.0f} GiB")
            if B <= 64:
                n = min(a.loop_tokens, T)

                def loop():
                    c.decode_open(*want)
                    cur = torch.from_numpy(s0).to(dev).long()
                    for t in range(n):
                        s = c.decode(tab_dev[cur].unsqueeze(0))[0]       # one lac_decode_steps(1) launch
                        s_host = s.cpu()                                 # the readback the next row waits for
                        cur = nxt_dev[cur, s_host.to(dev).long()]
                    return s_host
                lp = timed(loop, 2)
                emit(what="loop", order=order, streams=B, tokens=n, reps=2, decode_ms=lp, decode_us_per_step=lp * 1e3 / n)

    for B in (int(x) for x in a.streams.split(",") if x):
        run(1, B, True)
    if a.order2:
        run(2, a.order2, False)


if __name__ == "__main__":
    main()
