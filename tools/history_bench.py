#!/usr/bin/env python3
"""Match-history models (lac_hist_*): one launch each way against the means the coder had before
(measurement aid, not the metric; results in profiles/history/README.md).

    python tools/history_bench.py [--tokens 1024] [--reps 10] [--streams 1,64,4096]

A byte model (V = 256, P = 256, the reference's default weights n r^3 + 1, u64 rows -- 256 * 255^3
does not fit u32 -- prec 48), T tokens per stream; the symbols copy what lies `d` back with
probability 0.9 and are uniform otherwise, d redrawn now and then, so matches of many lengths occur:
  history  encode_history_job / decode_open + set_history_state + decode_history, device events
           around `reps` jobs after a warm-up, per job and per coded step
  rows     the same symbols through encode_job on the materialised rows pmf[T, B, V] of the same
           job (built on the device by a step-by-step walk of the rings in the incremental form,
           not timed; same bytes, checked), while it fits --max-rows-gib
  token    the per-token path of lac_amd.coder, all there was before: History with a plain-function
           lfunc through AC(...).to_bin.bits and from_bin.run, one stream, --token-tokens symbols,
           wall time (calc_dist in Python, O(P^2) a token, a row upload and a launch per position)
One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

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


class Walk:
    """The rings of B streams as device tensors, in the incremental form (lac_history.h): the row
    of the next step and the move by the symbols taken.  Every stream is at the same step, so the
    write index is one number."""

    def __init__(self, L, B, V, P, dev):
        import torch
        self.torch, self.V, self.P, self.pasti = torch, V, P, 0
        self.L = torch.tensor(L, dtype=torch.int64, device=dev)
        self.ring = torch.full((B, P), -1, dtype=torch.int64, device=dev)
        self.M = torch.full((B, P), P, dtype=torch.int64, device=dev)
        self.lag = torch.arange(P, device=dev)
        self.p = None

    def row(self):
        t = self.torch
        self.p = self.ring[:, (self.pasti - 1 - self.lag) % self.P]
        r = t.minimum(self.M, (self.P - 1 - self.lag)[None, :])
        w = t.where(self.p > 0, self.L[self.lag[None, :], r], t.zeros_like(r))
        row = t.ones((self.ring.shape[0], self.V), dtype=t.int64, device=self.ring.device)
        return row.scatter_add_(1, self.p.clamp(min=0), w)

    def accept(self, s):
        t = self.torch
        s = s.long()
        self.M = t.where(self.p == s[:, None], t.clamp(self.M + 1, max=self.P), t.zeros_like(self.M))
        self.ring[:, self.pasti] = s
        self.pasti = (self.pasti + 1) % self.P


def draw(rng, V, T, B):
    import numpy as np
    s = rng.integers(0, V, size=(T, B), dtype=np.int32)
    d = rng.integers(1, 200, size=B)
    for t in range(1, T):
        d = np.where(rng.random(B) < 0.02, rng.integers(1, 200, size=B), d)
        src = t - d
        copy = (rng.random(B) < 0.9) & (src >= 0)
        s[t] = np.where(copy, s[np.maximum(src, 0), np.arange(B)], s[t])
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--streams", default="1,64,4096")
    ap.add_argument("--token-tokens", type=int, default=48)
    ap.add_argument("--max-rows-gib", type=float, default=12.0)
    ap.add_argument("--prec", type=int, default=48)
    a = ap.parse_args()
    import numpy as np
    import torch
    from lac_amd.batch import BatchCoder
    from lac_amd.coder import AC, History
    dev = torch.device("cuda", 0)
    T, prec, V, P = a.tokens, a.prec, 256, 256
    L = [[V * r ** 3 + 1 for r in range(P)] for _ in range(P)]

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    def run(B):
        s = draw(np.random.default_rng(B), V, T, B)
        sym = torch.from_numpy(s).to(dev)
        with BatchCoder(V, B, prec=prec, pmf_bits=64, capacity_bits=T * (prec + 2) + 256, device=dev) as c:
            c.load_history(P, L)
            enc = timed(lambda: c.encode_history_job(sym), a.reps)
            out = torch.empty((T, B), dtype=torch.int32, device=dev)

            def dec():
                c.decode_open()
                c.set_history_state()
                c.decode_history(T, out=out)
            d = timed(dec, a.reps)
            c.raise_on_error()
            ok = bool(torch.equal(out, sym))
            c.encode_history_job(sym)
            want = c.bits_tensor().clone(), c.nbits_tensor().clone()
            emit(what="history", streams=B, tokens=T, reps=a.reps, encode_ms=enc, decode_ms=d,
                 encode_us_per_step=enc * 1e3 / T, decode_us_per_step=d * 1e3 / T,
                 encode_msym_s=T * B / enc / 1e3, decode_msym_s=T * B / d / 1e3, round_trip=ok,
                 bits_per_symbol=float(want[1].sum()) / (T * B))
            # the parent's batched means: the rows of the job, materialised
            gib = T * B * V * 8 / 2 ** 30
            if gib <= a.max_rows_gib:
                pmf = torch.empty((T, B, V), dtype=torch.int64, device=dev)
                w = Walk(L, B, V, P, dev)
                for t in range(T):
                    pmf[t] = w.row()
                    w.accept(sym[t])
                del w
                reps = max(3, min(a.reps, int(40 / max(gib, 0.05))))
                g = timed(lambda: c.encode_job(pmf, sym), reps)
                same = bool(torch.equal(c.bits_tensor(), want[0]) and torch.equal(c.nbits_tensor(), want[1]))
                emit(what="rows", streams=B, tokens=T, reps=reps, pmf_gib=gib, encode_ms=g,
                     encode_us_per_step=g * 1e3 / T, same_bytes=same)
                del pmf
            else:
                emit(what="rows", streams=B, tokens=T, skipped=f"the rows would take {gib:.0f} GiB")
        if B == 1:
            n = min(a.token_tokens, T)
            f = lambda r, i, nn, p: nn * r ** 3 + 1  # noqa: E731  (the reference's default, as a plain function)
            syms = s[:n, 0].tolist()
            list(AC(History(V, P, f), prec).to_bin.bits(syms[:2]))   # (the library and the context are up)
            t0 = time.perf_counter()
            bits = list(AC(History(V, P, f), prec).to_bin.bits(syms))
            t1 = time.perf_counter()
            got = list(AC(History(V, P, f), prec).from_bin.run(bits, n=n))
            t2 = time.perf_counter()
            emit(what="token", streams=1, tokens=n, encode_ms=(t1 - t0) * 1e3, decode_ms=(t2 - t1) * 1e3,
                 encode_us_per_step=(t1 - t0) * 1e6 / n, decode_us_per_step=(t2 - t1) * 1e6 / n, round_trip=got == syms)

    for B in (int(x) for x in a.streams.split(",") if x):
        run(B)


if __name__ == "__main__":
    main()
