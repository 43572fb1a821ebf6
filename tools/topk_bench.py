"""Top-k rows from logits: the one-kernel q1 rule (BatchCoder.topk_logits) against the torch path it
replaces (lac_amd.sparse.topk_rows) and against the project's best reader of the same bytes, the q1
row-statistics kernel of encode_logits_job (lac_profile_read slot 6).

    python tools/topk_bench.py [--streams 4096] [--steps 16] [--k 64] [--rounds 7] [--skip-compressor]

Per shape (bf16 V = 32000, bf16 V = 128256, f32 V = 128256): `steps` positions of distinct logits
for `streams` streams, one warm round, then `rounds` rounds that alternate the three, each timed
with device events; median and min-max of the microseconds per position, bytes / time as a
fraction of 8 TB/s, and the ratios.  Then the whole TopKCompressor position (model step, rows,
coder) under rule "float" and rule "q1".  One JSON line per result.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from lac_amd.batch import BatchCoder  # noqa: E402
from lac_amd.sparse import TopKCompressor, topk_rows  # noqa: E402

PEAK = 8e12


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)                                   # ms


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def shape(V, dtype, a):
    dev = torch.device("cuda", 0)
    B, T, k = a.streams, a.steps, a.k
    eb = 2 if dtype == torch.bfloat16 else 4
    g = torch.Generator(device=dev).manual_seed(V + eb)
    lg = torch.empty((T, B, V), dtype=dtype, device=dev)
    for t in range(T):                                         # distinct logits, a peaked row like a model's
        lg[t] = (torch.randn((B, V), generator=g, device=dev) * 3.0).to(dtype)
    sym = torch.randint(0, V, (T, B), generator=g, device=dev, dtype=torch.int32)
    K = (k + 3) // 4 * 4
    out = (torch.empty((T, B, K), dtype=torch.int32, device=dev), torch.empty((T, B, K), dtype=torch.int32, device=dev))
    ms, cnt = (C.c_double * 8)(), (C.c_int64 * 8)()
    with BatchCoder(V, B, prec=48, capacity_bits=T * 50 + 256, device=dev) as c:
        form = c.topk_form(dtype)

        def new():
            return timed(lambda: c.topk_logits(lg, k, 24, K, out=out))

        def old():
            def run():
                for t in range(T):
                    topk_rows(lg[t], k)
            return timed(run)

        def reader():
            c.lib.lac_profile_read(c.ctx, None, None, 1)
            c.lib.lac_profile_enable(c.ctx, 1)
            c.encode_logits_job(lg, sym)
            torch.cuda.synchronize()
            c.lib.lac_profile_enable(c.ctx, 0)
            c.lib.lac_profile_read(c.ctx, C.cast(ms, C.c_void_p), C.cast(cnt, C.c_void_p), 1)
            return ms[6]

        res = {"new": [], "old": [], "reader": []}
        for r in range(a.rounds + 1):
            for name, fn in (("new", new), ("old", old), ("reader", reader)):
                v = fn()
                if r:                                          # round 0 warms
                    res[name].append(v * 1e3 / T)              # us per position
        # the rows are the same where no weight ties at the cut (the float rule breaks ties its own way)
        idx_old = topk_rows(lg[0], k)[0]
        same = float((out[0][0][:, :k] == idx_old[:, :k]).all(-1).float().mean())
    byt = B * V * eb
    line = {"vocab": V, "dtype": str(dtype).split(".")[-1], "streams": B, "steps": T, "k": k, "form": form,
            "bytes_per_step": byt, "rows_equal_to_torch_topk": same}
    for name in res:
        s = stats(res[name])
        line[name + "_us_per_step"] = s
        line[name + "_frac_of_8TBps"] = byt / (s["median"] * 1e-6) / PEAK
    line["new_over_old"] = line["new_us_per_step"]["median"] / line["old_us_per_step"]["median"]
    line["new_over_reader"] = line["new_us_per_step"]["median"] / line["reader_us_per_step"]["median"]
    print(json.dumps(line), flush=True)
    del lg
    torch.cuda.empty_cache()


def compressor(a):
    from lac_amd.llm import TinyCausalLM
    V, B, T = 32000, a.streams, a.steps
    model = TinyCausalLM(vocab=V, d=64, layers=2, heads=4, max_len=64, seed=0)
    tokens = torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(1))
    line = {"compressor": "TinyCausalLM vocab 32000", "streams": B, "steps": T, "k": a.k}
    for rule in ("float", "q1"):
        comp = TopKCompressor(model, V, a.k, device="cuda:0", rule=rule)
        xs = []
        for r in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            data, nbits = comp.compress(tokens)
            torch.cuda.synchronize()
            if r:
                xs.append((time.perf_counter() - t0) * 1e6 / T)
        line[rule + "_us_per_step"] = stats(xs)
        line[rule + "_bits"] = int(sum(int(n) for n in nbits))
    print(json.dumps(line), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--streams", type=int, default=4096)
    p.add_argument("--steps", type=int, default=16)
    p.add_argument("--k", type=int, default=64)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--skip-compressor", action="store_true")
    a = p.parse_args()
    for V, dtype in ((32000, torch.bfloat16), (128256, torch.bfloat16), (128256, torch.float32)):
        shape(V, dtype, a)
    if not a.skip_compressor:
        compressor(a)


if __name__ == "__main__":
    main()
