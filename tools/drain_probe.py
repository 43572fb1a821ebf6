"""Cost of one lac_encode_drain launch at B = 4096 after 64 coded steps -- the c3 pmf shape
(V = 32000 u32 tables) and the bf16 logits shape -- beside the 64 steps' encode calls, in contexts
of capacity_bits 2^14 and 2^22 (profiles/drain/README.md).  hipEvents around the calls
(torch.cuda.Event), five repeats after one warm-up repeat; one JSON line per case.

    python tools/drain_probe.py [--out FILE]
    LAC_LIB=older/liblac.so python tools/drain_probe.py --encode-only     # the encode calls alone
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lac_amd._lib import check  # noqa: E402
from lac_amd.batch import ENC_STATE, BatchCoder  # noqa: E402

DEV = "cuda:0"
B, V, PREC, CH, NCH = 4096, 32000, 48, 16, 4                 # 64 steps as 4 calls of 16 (the bench's job size)


def stream_bits(c):
    """Every stream's L (the registers without the planes: a 2^22-bit context's planes are 4 GiB)."""
    st = np.zeros(c.streams, dtype=ENC_STATE)
    check(c.lib.lac_encode_get_state(c.ctx, st.ctypes.data_as(C.c_void_p), None, c._stream))
    return st["L"].astype(np.int64)


def ev():
    return torch.cuda.Event(enable_timing=True)


def run(kind, cap_bits, drain, reps=5):
    """drain: time the drain launch that follows the 64 steps (else the 64 steps' encode calls)."""
    g = torch.Generator(device=DEV).manual_seed(1)
    if kind == "pmf":
        tab = torch.randint(1, 1000, (CH, B, V), generator=g, device=DEV, dtype=torch.int32)
    else:
        tab = (torch.randn((CH, B, V), generator=g, device=DEV) * 4).to(torch.bfloat16)
    sym = torch.randint(0, V, (NCH * CH, B), generator=g, device=DEV, dtype=torch.int32)
    c = BatchCoder(V, B, prec=PREC, capacity_bits=cap_bits, device=DEV)
    stage = torch.zeros((B, 2048), dtype=torch.uint8, device=DEV)
    fill = torch.zeros(B, dtype=torch.int64, device=DEV)
    ms, info = [], {}
    for rep in range(reps + 1):
        c.reset()
        fill.zero_()
        torch.cuda.synchronize()
        e0, e1 = ev(), ev()
        e0.record()
        for k in range(NCH):
            s = sym[k * CH:(k + 1) * CH]
            c.encode(tab, s) if kind == "pmf" else c.encode_logits(tab, s)
        before = None
        if drain:
            before = stream_bits(c) if rep == reps else None
            torch.cuda.synchronize()
            e0.record()
            c.drain(stage, fill)
        e1.record()
        torch.cuda.synchronize()
        assert c.status()[0] == 0
        if rep:                                                 # (rep 0 warms up)
            ms.append(e0.elapsed_time(e1))
        if before is not None:
            words, kept, out = (before - 1) // 64 + 1, (stream_bits(c) - 1) // 64 + 1, fill.cpu().numpy()
            info = {"bits_per_stream_mean": float(before.mean()), "resident_words_total": int(words.sum()),
                    "drained_bytes_total": int(out.sum()), "kept_words_total": int(kept.sum()),
                    "kept_words_max": int(kept.max()),
                    # both planes of every resident word read once (the guard search re-reads at most one
                    # block), the drained bytes and both planes of the kept words written
                    "plane_bytes_read": int(words.sum()) * 16, "bytes_written": int(out.sum()) + int(kept.sum()) * 16}
    c.close()
    return ms, info


if __name__ == "__main__":
    encode_only = "--encode-only" in sys.argv
    out = open(sys.argv[sys.argv.index("--out") + 1], "w") if "--out" in sys.argv else None
    for kind in ("pmf", "logits"):
        for cap in ((1 << 14,) if encode_only else (1 << 14, 1 << 22)):
            r = {"kind": kind, "capacity_bits": cap, "lib": os.environ.get("LAC_LIB", "tree"),
                 "encode_64_steps_ms": run(kind, cap, False)[0]}
            if not encode_only:
                r["drain_ms"], info = run(kind, cap, True)
                r.update(info)
            line = json.dumps(r)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
