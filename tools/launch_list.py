#!/usr/bin/env python3
"""Tiny jobs over every kernel-selection case, to list what they launch.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 tools/launch_list.py
    python3 tools/launch_list.py --list OUT/.../*_kernel_trace.csv > launches.txt

The first form runs, in one process, a 2-step encode job + decode for: the logits rows
DESIGN.md 5b names (AUTO, 8 streams), every live forced q1 shape on a row it holds, and
the pmf decode paths by stream count, knob and forced path (tests/test_select_host.py has
the same cases on the CPU).  The second prints the library's kernels of such a trace in
launch order as `name grid workgroup`: two builds that select alike give equal lists
(LAC_LIB picks the library, lac_amd/_lib.py).
"""
import csv
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS = 2
# (V, dtype): bf16 / f32 rows of 4000 .. 37984 vectors
LOGITS_AUTO = [(32000, "bf16"), (32000, "f32"), (16384, "f32"), (128256, "bf16"), (131072, "bf16"), (65536, "f32"),
               (151936, "bf16"), (202048, "bf16"), (100280, "f32"), (128256, "f32"), (256000, "bf16"), (151936, "f32"),
               (262144, "bf16")]
# forced shape -> a bf16 V it holds (vectors: V / 8)
LOGITS_FORCED = {1: 2048, 2: 8192, 3: 16384, 4: 32000, 6: 32000, 8: 151936, 10: 151936, 14: 151936, 15: 128256,
                 17: 32000, 18: 65536, 19: 256000, 20: 151936, 21: 151936, 22: 202048, 23: 262144}


def run():
    import torch
    from lac_amd import synth
    from lac_amd.batch import BatchCoder
    dev = "cuda:0"

    def logits_case(V, dt, shape):
        B = 8
        tdt = torch.bfloat16 if dt == "bf16" else torch.float32
        g = torch.Generator(device=dev)
        g.manual_seed(V + shape)
        lg = (torch.randn((STEPS, B, V), generator=g, device=dev) * 3.0).to(tdt)
        sym = lg.float().argmax(dim=-1).to(torch.int32)        # (a symbol of positive probability)
        with BatchCoder(V, B, prec=48, capacity_bits=4096, device=dev) as c:
            c.set_q1_shape(shape)
            c.encode_logits_job(lg, sym)
            c.decode_open()
            out = c.decode_logits(lg)
            torch.cuda.synchronize()
            assert torch.equal(out, sym), (V, dt, shape)

    for V, dt in LOGITS_AUTO:
        logits_case(V, dt, 0)
    for shape, V in LOGITS_FORCED.items():
        logits_case(V, "bf16", shape)
        logits_case(V // 2, "f32", shape)

    def pmf_case(B, V=None, bits=32, prec=48, static=False, unaligned=False, lengths=False, setup=None):
        V = V or (4096 if B >= 160 else 32000)
        pmf, sym = synth.softmax_tables(1 if static else STEPS, B, V, seed=B, device=dev,
                                        scale_bits=40 if bits == 64 else 24, storage_bits=bits)
        if static:
            pmf, sym = pmf.expand(STEPS, B, V), sym.expand(STEPS, B).contiguous()
        if unaligned:                                          # rows 4 / 8 bytes off a 16-byte boundary
            flat = torch.empty(pmf.numel() + 1, dtype=pmf.dtype, device=dev)
            flat[1:] = pmf.reshape(-1)
            pmf = flat[1:].view(STEPS, B, V)
        with BatchCoder(V, B, prec=prec, pmf_bits=bits, capacity_bits=4096, device=dev) as c:
            c.encode_job(pmf, sym)
            if setup:
                setup(c)
            if lengths:
                c.set_stream_lengths([1 + b % 2 for b in range(B)])
            c.decode_open()
            out = c.decode(pmf)
            torch.cuda.synchronize()
            if not lengths:
                assert torch.equal(out, sym), (B, V, bits)

    for B in (1, 8, 16, 44, 45, 128, 160, 256, 300, 1024, 1536, 2048):
        pmf_case(B)
    pmf_case(8, setup=lambda c: c.set_decode_stop(True))
    pmf_case(2048, setup=lambda c: c.set_decode_stop(True))
    pmf_case(8, lengths=True)
    pmf_case(8, prec=51)
    pmf_case(8, static=True)
    pmf_case(300, static=True)
    for B in (8, 160, 2048):
        pmf_case(B, unaligned=True)
        pmf_case(B, V=4097 if B >= 160 else 32001)
        pmf_case(B, bits=64)
    pmf_case(2048, setup=lambda c: c.set_decode_path("fused_chunk"))
    for nw in (4, 8, 16):
        pmf_case(160, setup=lambda c: c.set_block_waves(nw))
    for path in ("split", "fused", "stats", "block"):
        for B in (8, 300):
            pmf_case(B, setup=lambda c: c.set_decode_path(path))
            pmf_case(B, bits=64, setup=lambda c: c.set_decode_path(path))
    pmf_case(300, unaligned=True, setup=lambda c: c.set_decode_path("split"))
    print("launch_list: all cases ran")


def listing(path):
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))
    for r in rows:
        name = r["Kernel_Name"]
        if not re.search(r"(^|[\s:(])k_[a-z]", name):           # the library's kernels are k_*; the rest is torch's
            continue
        name = re.sub(r"\(anonymous namespace\)::", "", name)
        name = re.sub(r" \[clone \.kd\]$|\.kd$", "", name)
        grid = "x".join(r[f"Grid_Size_{a}"] for a in "XYZ")
        wg = "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ")
        print(name, grid, wg)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--list":
        listing(sys.argv[2])
    else:
        run()
