#!/usr/bin/env python3
"""The receive side of the wire: lac_unpack_jobs against the torch unpack_bitstreams, and the
host time of container.decompress_batch (measurement aid, not the metric; results in
profiles/unpack/README.md).

    python tools/unpack_bench.py --case gather
        (a) the gatherer's shape: 8 jobs x 4096 streams, 2048-bit slots, 2-byte headers, the
        counts of 16-step V = 32000 jobs (encoded here: one softmax table per step, each
        stream its own symbols drawn from it).  One lac_unpack_jobs launch for the 8 jobs
        against 8 unpack_bitstreams calls (BitstreamGatherer.last_unpacked's old form, one
        per job); results compared first.
    python tools/unpack_bench.py --case long
        (b) one stream of 8 Mbit (1 MiB slot, 4-byte header), same comparison.
    python tools/unpack_bench.py --case container [--tree PATH]
        (c) host wall time of decompress_batch for a 4096-stream, 16-step V = 32000 container
        (one table per step for all streams), the call's final synchronise included.
        --tree imports lac_amd from another checkout (the parent commit, with its library
        built), so both versions run from this one script.

Device times are hipEvent pairs around `--iters` back-to-back calls after a warm-up, repeated
`--reps` times; each line reports the repeats' median per call and their min / max.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_us(fn, iters, reps, warm=10):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return out


def host_us(fn, iters, reps, warm=3):
    import torch
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6 / iters)
    return out


def summary(us):
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "reps": len(us)}


def shared_table_job(coder, steps, V, seed, dev):
    """One job: a softmax table per step shared by all streams, each stream's symbols drawn from it."""
    import torch

    from lac_amd import synth
    pmf, _ = synth.softmax_tables(steps, 1, V, seed=seed, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    p = (pmf[:, 0].to(torch.int64) & 0xFFFFFFFF).double()
    sym = torch.multinomial(p / p.sum(-1, keepdim=True), coder.streams, replacement=True, generator=g).to(torch.int32)
    return pmf, sym.contiguous()                               # [steps, 1, V], [steps, streams]


def case_gather(args, dev):
    import torch

    from lac_amd import dist as ldist
    from lac_amd.batch import BatchCoder
    jobs, B, stride, hdr = 8, 4096, 256, 2
    coder = BatchCoder(32000, B, prec=48, capacity_bits=8 * stride - 64, device=dev)
    assert coder.bits_stride() == stride
    buf = torch.zeros(jobs * B * (hdr + stride), dtype=torch.uint8, device=dev)
    ends = torch.zeros(jobs + 1, dtype=torch.int64, device=dev)
    for j in range(jobs):
        pmf, sym = shared_table_job(coder, 16, 32000, 100 + j, dev)
        coder.encode_job(pmf, sym)
        coder.pack_bits_at(buf, hdr, ends[j:j + 1], ends[j + 1:j + 2])
    coder.raise_on_error()
    off = ends.tolist()
    payload = buf[:off[-1]]
    parts = [payload[off[j]:off[j + 1]] for j in range(jobs)]

    def native():
        return ldist.unpack_jobs(payload, jobs, B, stride, hdr)

    def torch_ref():
        return [ldist.unpack_bitstreams(p, B, stride, hdr) for p in parts]

    bits, nbits, e, status = native()
    ref = torch_ref()
    assert status.tolist() == [0] * jobs and e.tolist() == off[1:]
    assert all(torch.equal(bits[j], ref[j][0]) and torch.equal(nbits[j], ref[j][1]) for j in range(jobs))
    mean_bits = float(nbits.double().mean())
    return {"case": "gather", "jobs": jobs, "streams": B, "stride": stride, "hdr": hdr, "payload_bytes": off[-1],
            "mean_bits_per_stream": round(mean_bits, 1),
            "native": summary(device_us(native, args.iters, args.reps)),
            "torch": summary(device_us(torch_ref, args.iters, args.reps))}


def case_long(args, dev):
    import torch

    from lac_amd import dist as ldist
    stride, hdr = 1 << 20, 4
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    bits = torch.randint(0, 256, (1, stride), generator=g, device=dev, dtype=torch.uint8)
    packed, L = ldist.pack_bitstreams(bits, torch.tensor([8 * stride], device=dev), hdr)
    payload = packed[:int(L)].clone()

    def native():
        return ldist.unpack_jobs(payload, 1, 1, stride, hdr)

    def torch_ref():
        return ldist.unpack_bitstreams(payload, 1, stride, hdr)

    got, ref = native(), torch_ref()
    assert torch.equal(got[0][0], ref[0]) and torch.equal(got[0][0], bits) and torch.equal(got[1][0], ref[1])
    return {"case": "long", "streams": 1, "stride": stride, "hdr": hdr, "payload_bytes": int(L),
            "native": summary(device_us(native, args.iters, args.reps)),
            "torch": summary(device_us(torch_ref, args.iters, args.reps))}


def case_container(args, dev):
    import torch

    import lac_amd
    from lac_amd import container
    from lac_amd.batch import BatchCoder
    B = 4096
    coder = BatchCoder(32000, B, prec=48, capacity_bits=2048, device=dev)
    pmf, sym = shared_table_job(coder, 16, 32000, 200, dev)
    blob = container.compress_batch(coder, pmf, sym)
    coder.close()
    out, n = container.decompress_batch(blob, pmf)
    assert n == [16] * B and torch.equal(out, sym)
    return {"case": "container", "tree": os.path.dirname(os.path.dirname(os.path.abspath(lac_amd.__file__))),
            "streams": B, "blob_bytes": len(blob),
            "decompress_batch_host": summary(host_us(lambda: container.decompress_batch(blob, pmf), args.iters,
                                                     args.reps))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("gather", "long", "container"), required=True)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tree", default=None, help="import lac_amd from this checkout instead of this one")
    args = ap.parse_args()
    if args.iters < 50 or args.reps < 3:
        ap.error("at least 3 repeats of at least 50 iterations")
    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else REPO)
    import torch
    if not torch.cuda.is_available():
        sys.exit("unpack_bench.py needs a HIP device: there is no CPU timing of a GPU path")
    dev = torch.device("cuda", 0)
    res = {"gather": case_gather, "long": case_long, "container": case_container}[args.case](args, dev)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
