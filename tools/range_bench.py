#!/usr/bin/env python3
"""Range-level coding (lac_encode_ranges_job, lac_decode_ranges_step) against the only way the
library had to code the same job on the device: encode_job / decode over the V = 4 uint64 tables
[lo, hi - lo, T - hi, 0] with symbol 1 (measurement aid, not the metric; results in
profiles/ranges/README.md).

    python tools/range_bench.py [--steps 256] [--streams 1,64,4096,65536,1048576] [--rounds 5]

Seeded random valid triples (totals below 2^40, prec 48), `steps` symbols per stream.  The two
ways run alternately, `rounds` times each; one timing is a window of at least --window seconds
of back-to-back calls between device events, after a warm call.  Reported per way: the median
of the rounds and their spread (min, max).  The outputs are compared equal (bytes and bit counts;
decoded symbols and decoder registers).
  ranges  encode_ranges_job (reset + one coder launch + finish); the decode is the serving loop
          lac_amd.ranges.decode_loop with a model that replays the job's triples: one launch per
          position, so its time includes the launches' host cost
  tables  encode_job / decode on the tables, the coder's own kernel selection
One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def window(fn, seconds):
    """Device ms per call of fn: back-to-back calls filling at least `seconds`, after a warm call."""
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    reps = max(2, int(seconds * 1e3 / max(a.elapsed_time(b), 1e-3)) + 1)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, reps


class Replay:
    def __init__(self, lo, hi, tot):
        self.lo, self.hi, self.tot = lo, hi, tot

    def total(self, t):
        return self.tot[t]

    def lookup(self, t, targets):
        return targets, self.lo[t], self.hi[t]


def triples(T, B, dev, seed):
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    r = lambda: torch.randint(0, 1 << 62, (T, B), dtype=torch.int64, device=dev, generator=g)  # noqa: E731
    tot = 1 + r() % ((1 << 40) - 1)
    hi = 1 + r() % tot
    lo = r() % hi
    return lo, hi, tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--streams", default="1,64,4096,65536,1048576")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--prec", type=int, default=48)
    ap.add_argument("--no-decode", action="store_true")
    a = ap.parse_args()
    import torch
    from lac_amd.batch import BatchCoder
    from lac_amd.ranges import decode_loop
    dev = torch.device("cuda", 0)
    T, prec = a.steps, a.prec

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    def summary(xs):
        return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "rounds_ms": xs}

    for B in (int(x) for x in a.streams.split(",") if x):
        lo, hi, tot = triples(T, B, dev, B)
        pmf = torch.stack([lo, hi - lo, tot - hi, torch.zeros_like(lo)], dim=-1)
        ones = torch.ones((T, B), dtype=torch.int32, device=dev)
        with BatchCoder(4, B, prec=prec, pmf_bits=64, capacity_bits=T * (prec + 2) + 256, device=dev) as c:
            enc = {"ranges": [], "tables": []}
            reps = {}
            for _ in range(a.rounds):                                  # alternating
                ms, reps["ranges"] = window(lambda: c.encode_ranges_job(lo, hi, tot), a.window)
                enc["ranges"].append(ms)
                ms, reps["tables"] = window(lambda: c.encode_job(pmf, ones), a.window)
                enc["tables"].append(ms)
            c.encode_job(pmf, ones)
            c.raise_on_error()
            want = c.bits_tensor().clone(), c.nbits_tensor().clone()
            c.encode_ranges_job(lo, hi, tot)
            c.raise_on_error()
            same = bool(torch.equal(c.bits_tensor(), want[0]) and torch.equal(c.nbits_tensor(), want[1]))
            for way in ("ranges", "tables"):
                emit(what="encode", way=way, streams=B, steps=T, prec=prec, reps=reps[way], same_bytes=same,
                     us_per_step=statistics.median(enc[way]) * 1e3 / T,
                     msym_s=T * B / statistics.median(enc[way]) / 1e3,
                     bits_per_symbol=float(want[1].sum()) / (T * B), **summary(enc[way]))
            if a.no_decode:
                continue
            model = Replay(lo, hi, tot)
            out = torch.empty((T, B), dtype=torch.int32, device=dev)

            def dec_ranges():
                c.decode_open()
                return decode_loop(c, T, model)

            def dec_tables():
                c.decode_open()
                return c.decode(pmf, out=out)
            dec = {"ranges": [], "tables": []}
            for _ in range(a.rounds):
                ms, reps["ranges"] = window(dec_ranges, a.window)
                dec["ranges"].append(ms)
                ms, reps["tables"] = window(dec_tables, a.window)
                dec["tables"].append(ms)
            got = dec_ranges()
            ok = bool(((got >= lo) & (got < hi)).all()) and c.status()[0] == 0
            ok_t = bool((dec_tables() == 1).all()) and c.status()[0] == 0
            for way in ("ranges", "tables"):
                emit(what="decode", way=way, streams=B, steps=T, prec=prec, reps=reps[way],
                     round_trip=ok if way == "ranges" else ok_t, us_per_step=statistics.median(dec[way]) * 1e3 / T,
                     msym_s=T * B / statistics.median(dec[way]) / 1e3, **summary(dec[way]))
        del lo, hi, tot, pmf, ones
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
