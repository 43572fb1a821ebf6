"""Self-describing container for lac bitstreams.

The reference writes bare bytes: ``measure_compress`` returns
``bytes(group_bits(bits))`` (arith_code.py:401-420) and stores neither the
symbol count n nor the bit length L, so its decoder cannot know where to stop
(arith_code.py:322-334; SURVEY.md finding 5).  This container adds a header in
front of exactly those bytes; the payload of each stream is unchanged.

Layout (little-endian):

    magic   4 B   b"LAC1"
    version u16   1
    prec    u8    coder precision (arith_code.py:157-160)
    flags   u8    bit0 mapping (0 ceil / CDFPredictor, 1 floor / Predictor, ACSampler)
                  bit1 termination (0 A_to_bin.flush, 1 ACSampler.flush_compress)
                  bit2 pmf_bits == 64
                  bit3 tables are q1-quantised logits (lac.h "logits path"): decode
                       needs the same logits, not a pmf
    vocab   u32
    streams u32
    then per stream: n_symbols u64, n_bits u64
    then per stream: ceil(n_bits / 8) payload bytes (MSB first, zero padded)
"""
from __future__ import annotations

import struct

MAGIC = b"LAC1"
VERSION = 1
_HDR = struct.Struct("<4sHBBII")
_ENT = struct.Struct("<QQ")


def pack(streams, n_symbols, n_bits, prec, vocab, mapping="ceil", termination="flush", pmf_bits=32,
         q1_logits=False) -> bytes:
    """streams: list of per-stream payload bytes (group_bits format)."""
    if not (len(streams) == len(n_symbols) == len(n_bits)):
        raise ValueError("streams, n_symbols and n_bits must have equal length")
    flags = ((mapping == "floor") | ((termination == "acsampler") << 1) | ((pmf_bits == 64) << 2)
             | (bool(q1_logits) << 3))
    out = [_HDR.pack(MAGIC, VERSION, prec, flags, vocab, len(streams))]
    for n, L, data in zip(n_symbols, n_bits, streams):
        if len(data) != (int(L) + 7) // 8:
            raise ValueError("payload length does not match n_bits")
        out.append(_ENT.pack(int(n), int(L)))
    out.extend(bytes(d) for d in streams)
    return b"".join(out)


def unpack(blob: bytes):
    """-> dict(prec, vocab, mapping, termination, pmf_bits, q1_logits, n_symbols, n_bits, streams)."""
    magic, ver, prec, flags, vocab, ns = _HDR.unpack_from(blob, 0)
    if magic != MAGIC:
        raise ValueError("not a LAC1 container")
    if ver != VERSION:
        raise ValueError(f"unsupported container version {ver}")
    off = _HDR.size
    n_symbols, n_bits = [], []
    for _ in range(ns):
        n, L = _ENT.unpack_from(blob, off)
        off += _ENT.size
        n_symbols.append(n)
        n_bits.append(L)
    streams = []
    for L in n_bits:
        k = (L + 7) // 8
        streams.append(blob[off:off + k])
        off += k
    if off != len(blob):
        raise ValueError("trailing bytes in container")
    return {"prec": prec, "vocab": vocab, "mapping": "floor" if flags & 1 else "ceil",
            "termination": "acsampler" if flags & 2 else "flush", "pmf_bits": 64 if flags & 4 else 32,
            "q1_logits": bool(flags & 8), "n_symbols": n_symbols, "n_bits": n_bits, "streams": streams}


def _is_logits(tables):
    import torch
    return tables.dtype in (torch.bfloat16, torch.float32)


def compress_batch(coder, pmf, sym, n_symbols=None) -> bytes:
    """Encode a batch with a BatchCoder and wrap it in a container.  ``pmf``:
    integer tables (one lac_encode_job) or bf16/f32 logits (the q1 logits path).
    ``n_symbols`` (a sequence of ``streams`` counts in [0, steps]): stream b codes only its
    first n_symbols[b] symbols (BatchCoder.set_stream_lengths, left set on the coder) and the
    header records those counts.  None leaves the coder as it is and records ``steps`` for
    every stream, which is right for a coder with no counts set: clear counts set earlier
    (``coder.set_stream_lengths(None)``) or pass them here."""
    logits = _is_logits(pmf)
    steps = sym.shape[0]
    if n_symbols is None:
        counts = [steps] * coder.streams
    else:
        counts = [int(n) for n in n_symbols]
        if len(counts) != coder.streams or any(n < 0 or n > steps for n in counts):
            raise ValueError(f"n_symbols: {coder.streams} counts in [0, {steps}]")
        coder.set_stream_lengths(counts)
    if logits:
        coder.encode_logits_job(pmf, sym)
    else:
        coder.encode_job(pmf, sym)
    data, nbits = coder.to_bytes()
    return pack(data, counts, [int(x) for x in nbits], coder.prec, coder.vocab,
                pmf_bits=coder.pmf_bits, q1_logits=logits)


def decompress_batch(blob: bytes, pmf, device=None):
    """Decode a container produced by :func:`compress_batch` given the same tables
    (the same logits for a q1 container).  -> (out [max(n_symbols), streams] int32, n_symbols);
    where the streams' counts differ, out is -1 past each stream's count."""
    import torch

    from .batch import BatchCoder
    h, n_symbols, n_bits, body = _index(blob)
    B = len(n_bits)
    steps = int(n_symbols.max()) if B else 0
    coder = BatchCoder(h["vocab"], B, prec=h["prec"], pmf_bits=h["pmf_bits"],
                       capacity_bits=(int(n_bits.max()) if B else 64) + 64, device=device or pmf.device)
    coder.set_mapping(h["mapping"])
    # the body as it is -- the streams' bytes back to back, the wire format without a header --
    # and the counts go up; the coder unpacks them into its slots on the device
    # (BatchCoder.decode_open_packed): no per-stream work here
    payload = torch.frombuffer(bytearray(body) or bytearray(8), dtype=torch.uint8).to(coder.device)
    nb = torch.from_numpy(n_bits.astype("<i8")).to(coder.device)
    # a ragged container: each stream decodes its own count and no further (out is -1 past it)
    if B and bool((n_symbols != steps).any()):
        coder.set_stream_lengths(n_symbols)
    coder.decode_open_packed(payload, 0, counts=nb)
    if h["q1_logits"] != _is_logits(pmf):
        raise ValueError("container and tables disagree: q1 logits vs integer pmf")
    out = coder.decode_logits(pmf[:steps]) if h["q1_logits"] else coder.decode(pmf[:steps])
    coder.raise_on_error()
    coder.close()
    return out, n_symbols.tolist()


def _index(blob):
    """The container's header and count table without slicing the streams: -> (header fields
    as :func:`unpack` names them, n_symbols uint64 [streams], n_bits uint64 [streams], body);
    raises what :func:`unpack` raises for a blob that is not a whole container."""
    import numpy as np
    magic, ver, prec, flags, vocab, ns = _HDR.unpack_from(blob, 0)
    off = _HDR.size + ns * _ENT.size
    if magic != MAGIC or ver != VERSION or len(blob) < off:
        unpack(blob)                                           # raises for each of these
    ent = np.frombuffer(blob, dtype="<u8", count=2 * ns, offset=_HDR.size).reshape(ns, 2)
    n_bits = ent[:, 1]
    nbytes = (n_bits >> np.uint64(3)) + ((n_bits & np.uint64(7)) != 0).astype(np.uint64)
    # (a count beyond the blob cannot match, and without one the uint64 sum cannot wrap)
    if ns and (int(nbytes.max()) > len(blob) or off + int(nbytes.sum()) != len(blob)) or not ns and off != len(blob):
        raise ValueError("trailing bytes in container")
    h = {"prec": prec, "vocab": vocab, "mapping": "floor" if flags & 1 else "ceil",
         "termination": "acsampler" if flags & 2 else "flush", "pmf_bits": 64 if flags & 4 else 32,
         "q1_logits": bool(flags & 8)}
    return h, ent[:, 0], n_bits, memoryview(blob)[off:]
