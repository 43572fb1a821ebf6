"""Cost of the windowed decode (lac_decode_open_window / lac_decode_refill) beside the whole-stream
decode (profiles/refill/README.md), V = 32000 u32 tables, prec 48:

  (a) B = 4096, 256 steps on the AUTO path as 16 calls of 16 steps (the bench's job size, one
      16-step table reused), whole-stream open against a window sized for 64 steps with a refill
      every 64 steps;
  (b) B = 1, lac_decode_step over a stream of 4 Mbit and of 64 Mbit (random bits: every bit
      string decodes), 256 calls, whole-stream open against a window of 64 steps;
  (c) one k_dec_refill launch after 64 steps, at B = 1 and B = 4096, the source in device
      memory and in lac_host_alloc memory.

hipEvents around the calls (torch.cuda.Event), five repeats after one warm-up repeat; one JSON
line per case.

    python tools/refill_probe.py [--out FILE]
    LAC_LIB=older/liblac.so python tools/refill_probe.py --plain-only   # the whole-stream decodes alone
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lac_amd.batch import BatchCoder  # noqa: E402

DEV = "cuda:0"
V, PREC, CH, EVERY = 32000, 48, 16, 64
CAP_WINDOW = EVERY * (PREC + 2) + 256


def ev():
    return torch.cuda.Event(enable_timing=True)


def coded_job(B, steps):
    """`steps` symbols per stream coded with one CH-step table reused -> table, symbols, streams."""
    g = torch.Generator(device=DEV).manual_seed(1)
    tab = torch.randint(1, 1000, (CH, B, V), generator=g, device=DEV, dtype=torch.int32)
    sym = torch.randint(0, V, (steps, B), generator=g, device=DEV, dtype=torch.int32)
    with BatchCoder(V, B, prec=PREC, capacity_bits=steps * (PREC + 2) + 256, device=DEV) as c:
        c.reset()
        for k in range(0, steps, CH):
            c.encode(tab, sym[k:k + CH])
        c.finish()
        assert c.status()[0] == 0
        bits, nbits = c.bits_tensor(), c.nbits_tensor().clone()
        data, nb = c.to_bytes()
    return tab, sym, bits, nbits, data, nb


def random_job(nbits):
    """One stream of `nbits` random bits and a one-step table."""
    g = torch.Generator(device=DEV).manual_seed(2)
    tab = torch.randint(1, 1000, (1, 1, V), generator=g, device=DEV, dtype=torch.int32)
    raw = torch.randint(0, 256, (1, nbits // 8), generator=g, device=DEV, dtype=torch.int32).to(torch.uint8)
    return tab, raw, torch.tensor([nbits], dtype=torch.int64, device=DEV), [raw[0].cpu().numpy().tobytes()], np.array([nbits])


def decode_run(B, steps, call_steps, tab, src, nbits, cap, window, sym=None, reps=5):
    """`steps` symbols in calls of `call_steps`, a refill every EVERY steps and one at the end when
    `window` -> ms per repeat of the whole decode, ms per repeat of its refill launches alone."""
    c = BatchCoder(V, B, prec=PREC, capacity_bits=cap, device=DEV)
    out = torch.empty((steps, B), dtype=torch.int32, device=DEV)
    total, refills = [], []
    for rep in range(reps + 1):
        c.decode_open_window(src, nbits) if window else c.decode_open(src, nbits)
        torch.cuda.synchronize()
        e0, e1, marks = ev(), ev(), []
        e0.record()
        for t in range(0, steps, call_steps):
            c.decode(tab[:call_steps], out[t:t + call_steps])
            if window and (t + call_steps) % EVERY == 0:
                a, b = ev(), ev()
                a.record()
                c.refill()
                b.record()
                marks.append((a, b))
        e1.record()
        torch.cuda.synchronize()
        assert c.status()[0] == 0
        if sym is not None:
            assert torch.equal(out, sym)
        if rep:                                                 # (rep 0 warms up)
            total.append(e0.elapsed_time(e1))
            refills.append(sum(a.elapsed_time(b) for a, b in marks))
    c.close()
    return total, refills


def refill_run(B, tab, src, nbits, reps=5):
    """One refill launch after EVERY decoded steps, µs per repeat."""
    c = BatchCoder(V, B, prec=PREC, capacity_bits=CAP_WINDOW, device=DEV)
    out = torch.empty((EVERY, B), dtype=torch.int32, device=DEV)
    us = []
    for rep in range(reps + 1):
        c.decode_open_window(src, nbits)
        for t in range(0, EVERY, tab.shape[0]):
            c.decode(tab, out[t:t + tab.shape[0]])
        torch.cuda.synchronize()
        e0, e1 = ev(), ev()
        e0.record()
        c.refill()
        e1.record()
        torch.cuda.synchronize()
        assert c.status()[0] == 0 and int(c.window_base().min()) > 0
        if rep:
            us.append(1000.0 * e0.elapsed_time(e1))
    c.close()
    return us


if __name__ == "__main__":
    plain_only = "--plain-only" in sys.argv
    sink = open(sys.argv[sys.argv.index("--out") + 1], "w") if "--out" in sys.argv else None
    lib = os.environ.get("LAC_LIB", "tree")

    def emit(r):
        line = json.dumps(dict(r, lib=lib))
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")

    B, steps = 4096, 256
    tab, sym, bits, nbits, data, nb = coded_job(B, steps)
    whole_cap = steps * (PREC + 2) + 256
    emit({"case": "a", "B": B, "steps": steps, "open": "whole", "bits_per_stream_mean": float(np.mean(nb)),
          "decode_ms": decode_run(B, steps, CH, tab, bits, nbits, whole_cap, False, sym)[0]})
    if not plain_only:
        from lac_amd.batch import HostBits
        ms, rf = decode_run(B, steps, CH, tab, bits, nbits, CAP_WINDOW, True, sym)
        emit({"case": "a", "B": B, "steps": steps, "open": "window", "capacity_bits": CAP_WINDOW, "decode_ms": ms,
              "refill_launches_ms": rf})
        host = HostBits(data, nb, DEV)
        emit({"case": "c", "B": B, "source": "device", "refill_us": refill_run(B, tab, bits, nbits)})
        emit({"case": "c", "B": B, "source": "host", "refill_us": refill_run(B, tab, host, None)})
        torch.cuda.synchronize()
        host.close()
    del tab, sym, bits, nbits

    for sbits in (1 << 22, 1 << 26):                            # 4 Mbit, and 64 Mbit for the trend
        tab, raw, n1, data1, nb1 = random_job(sbits)
        ms = decode_run(1, 256, 1, tab, raw, n1, CAP_WINDOW, False)[0]
        emit({"case": "b", "B": 1, "stream_bits": sbits, "open": "whole", "decode_ms": ms,
              "per_call_us": [1000.0 * m / 256 for m in ms]})
        if plain_only:
            continue
        ms, rf = decode_run(1, 256, 1, tab, raw, n1, CAP_WINDOW, True)
        emit({"case": "b", "B": 1, "stream_bits": sbits, "open": "window", "capacity_bits": CAP_WINDOW,
              "decode_ms": ms, "per_call_us": [1000.0 * m / 256 for m in ms], "refill_launches_ms": rf})
        if sbits != 1 << 22:
            continue
        host = HostBits(data1, nb1, DEV)
        emit({"case": "c", "B": 1, "source": "device", "refill_us": refill_run(1, tab, raw, n1)})
        emit({"case": "c", "B": 1, "source": "host", "refill_us": refill_run(1, tab, host, None)})
        torch.cuda.synchronize()
        host.close()
