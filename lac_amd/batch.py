"""Batched device API: B independent streams coded on one MI355X.

This is the batched counterpart of the reference's single-stream coder
(``A_to_bin`` / ``A_from_bin``, /root/reference/arith_code.py:156-334) and of
``measure_compress`` (:401-420).  Tables stay in HBM as torch tensors; they
cross into liblac.so as raw device pointers (see include/lac.h).

    coder = BatchCoder(vocab=32000, streams=4096, prec=48)
    coder.encode(pmf, sym)           # pmf [steps, streams, V] uint32 in int32 storage
    coder.finish()
    data = coder.to_bytes()          # list of per-stream bytes (group_bits format)

    coder.decode_open()              # decode this coder's own output
    out = coder.decode(pmf)          # [steps, streams] int32 symbols
"""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np

from . import _lib
from ._lib import LacError, check



def _torch():
    import torch
    return torch


def _stream_handle(device):
    torch = _torch()
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


# include/lac.h lac_enc_state (EncState in lac_amd/csrc/lac_core.h)
ENC_STATE = np.dtype([("l", "<i8"), ("h", "<i8"), ("L", "<u8"), ("wa", "<u8"), ("wc", "<u8"), ("nsym", "<i8"),
                      ("err", "<i4"), ("nflush", "<i4"), ("err_step", "<i8"), ("flush", "i1", (8,))])


class StreamError(LacError):
    """A coder error on one or more streams (sticky, reported per stream)."""

    def __init__(self, code, err, err_step):
        first = int(np.flatnonzero(err)[0]) if np.any(err) else -1
        super().__init__(code, f"stream {first} failed at step {int(err_step[first]) if first >= 0 else -1}")
        self.err = err
        self.err_step = err_step
        self.first_stream = first


class BatchCoder:
    """Encoder/decoder for ``streams`` independent streams (one liblac context)."""

    def __init__(self, vocab: int, streams: int, prec: int = 48, pmf_bits: int = 32,
                 capacity_bits: int | None = None, device=None):
        torch = _torch()
        self.lib = _lib.load()
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("BatchCoder needs a HIP device (torch 'cuda' device on ROCm)")
        self.vocab, self.streams, self.prec, self.pmf_bits = int(vocab), int(streams), int(prec), int(pmf_bits)
        self.capacity_bits = int(capacity_bits or 1 << 16)
        ctx = C.c_void_p()
        check(self.lib.lac_open(self.device.index or 0, self.prec, self.vocab, self.streams, self.pmf_bits,
                                self.capacity_bits, C.byref(ctx)))
        self.ctx = ctx

    # ------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "ctx", None):
            self.lib.lac_close(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def _stream(self):
        return _stream_handle(self.device)

    # ------------------------------------------------------------ checks
    def _check_pmf(self, pmf):
        torch = _torch()
        want = (torch.int32, torch.uint32) if self.pmf_bits == 32 else (torch.int64, torch.uint64)
        if pmf.dtype not in want:
            raise TypeError(f"pmf must be {want[0]} (bit pattern of uint{self.pmf_bits}), got {pmf.dtype}")
        if pmf.device != self.device:
            raise ValueError(f"pmf is on {pmf.device}, coder on {self.device}")
        if pmf.shape[-1] != self.vocab:
            raise ValueError(f"pmf rows have {pmf.shape[-1]} entries, vocab is {self.vocab}")
        if pmf.stride(-1) != 1:
            raise ValueError("pmf rows must be contiguous")

    def _check_out(self, out, steps):
        torch = _torch()
        if out.dtype != torch.int32 or out.device != self.device:
            raise TypeError("out must be an int32 tensor on the coder's device")
        if tuple(out.shape) != (steps, self.streams) or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous [{steps}, {self.streams}] tensor")

    # ------------------------------------------------------------ encode
    def reset(self):
        check(self.lib.lac_encode_reset(self.ctx, self._stream))

    def _encode_args(self, pmf, sym, trace):
        torch = _torch()
        self._check_pmf(pmf)
        if sym.dtype != torch.int32 or sym.device != self.device:
            raise TypeError("sym must be an int32 tensor on the coder's device")
        sym = sym.contiguous()
        steps = sym.shape[0] if sym.dim() == 2 else 1
        if sym.numel() != steps * self.streams:
            raise ValueError(f"sym must be [steps, {self.streams}]")
        if pmf.dim() == 1:
            step_stride, stream_stride = 0, 0
        elif pmf.dim() == 2:
            if steps != 1 or pmf.shape[0] != self.streams:
                raise ValueError("a 2-D pmf is [streams, V] for one step")
            step_stride, stream_stride = 0, pmf.stride(0)
        else:
            if pmf.shape[0] not in (1, steps) or pmf.shape[1] not in (1, self.streams):
                raise ValueError("pmf must be [steps, streams, V]")
            step_stride = pmf.stride(0) if pmf.shape[0] > 1 else 0
            stream_stride = pmf.stride(1) if pmf.shape[1] > 1 else 0
        tp = None
        if trace is not None:
            if trace.dtype != torch.int64 or trace.numel() != steps * self.streams * 2 or not trace.is_contiguous():
                raise ValueError("trace must be a contiguous int64 tensor [steps, streams, 2]")
            tp = C.c_void_p(trace.data_ptr())
        self._keep = (pmf, sym)
        return (self.ctx, C.c_void_p(pmf.data_ptr()), step_stride, stream_stride, C.c_void_p(sym.data_ptr()),
                steps, tp, self._stream)

    def encode(self, pmf, sym, trace=None):
        """Encode sym[t, b] with row pmf[t, b, :] (or pmf[b, :] / pmf[:] broadcast).

        ``pmf`` [steps, streams, V], [streams, V] (steps == 1), [V] (a static
        row for every step and stream) or [steps, 1, V] / [1, streams, V] with
        stride-0 broadcasting via ``expand``.  ``sym`` int32 [steps, streams].
        ``trace`` (optional int64 device tensor [steps, streams, 2]) receives
        per symbol {E, k} -- its raw digits.  Streams continue from where the
        previous call left them.
        """
        check(self.lib.lac_encode(*self._encode_args(pmf, sym, trace)))

    def encode_job(self, pmf, sym, trace=None):
        """reset + encode + finish in one call (one kernel at >= 2048 streams)."""
        check(self.lib.lac_encode_job(*self._encode_args(pmf, sym, trace)))

    def set_mapping(self, mapping):
        """'ceil' (CDFPredictor, default) or 'floor' (Predictor / ACSampler Region.map)."""
        v = {"ceil": _lib.LAC_MAP_CEIL, "floor": _lib.LAC_MAP_FLOOR}[mapping]
        check(self.lib.lac_set_option(self.ctx, _lib.LAC_OPT_MAPPING, v))

    def set_termination(self, term):
        """'flush' (A_to_bin.flush, default) or 'acsampler' (ACSampler.flush_compress)."""
        v = {"flush": _lib.LAC_TERM_FLUSH, "acsampler": _lib.LAC_TERM_ACSAMPLER}[term]
        check(self.lib.lac_set_option(self.ctx, _lib.LAC_OPT_TERMINATION, v))

    def set_decode_path(self, path):
        """'auto', 'split' (one workgroup per stream per step), 'fused' (one wave per
        stream, one launch; per-iteration row totals), 'fused_chunk' (the same with
        <= 64 chunk totals per row), 'stats' (all rows' chunk totals at once, then
        a sequential per-stream kernel) or 'block' (one workgroup per stream, the
        row scans pipelined a step ahead of the coder wave); identical results."""
        v = {"auto": _lib.LAC_PATH_AUTO, "split": _lib.LAC_PATH_SPLIT, "fused": _lib.LAC_PATH_FUSED,
             "fused_chunk": _lib.LAC_PATH_FUSED, "stats": _lib.LAC_PATH_STATS, "block": _lib.LAC_PATH_BLOCK}[path]
        check(self.lib.lac_set_option(self.ctx, _lib.LAC_OPT_DECODE_PATH, v))
        check(self.lib.lac_set_option(self.ctx, _lib.LAC_OPT_DECODE_FINE, 0 if path == "fused_chunk" else 1))

    def set_decode_stop(self, on: bool):
        """Stop each stream before the first symbol its bits do not determine (include/lac.h
        LAC_OPT_DECODE_STOP): its status becomes LAC_E_UNDETERMINED with the registers
        as they were before that symbol, where A_from_bin.run(bits, stop=0) stops
        (arith_code.py:268-299); decodes then take the stats path."""
        check(self.lib.lac_set_option(self.ctx, _lib.LAC_OPT_DECODE_STOP, 1 if on else 0))

    def set_block_waves(self, n: int):
        """Waves per stream of the 'block' decode path: 4, 8, 16 (0 = by stream count)."""
        check(self.lib.lac_set_option(self.ctx, _lib.LAC_OPT_BLOCK_WAVES, int(n)))

    def set_path(self, path):
        """'auto', 'split' or 'fused' encode kernels (bit-identical results)."""
        v = {"auto": _lib.LAC_PATH_AUTO, "split": _lib.LAC_PATH_SPLIT, "fused": _lib.LAC_PATH_FUSED}[path]
        check(self.lib.lac_set_option(self.ctx, _lib.LAC_OPT_ENCODE_PATH, v))

    def finish(self):
        check(self.lib.lac_encode_finish(self.ctx, self._stream))

    def rebase(self):
        """Drop every stream's completed output words, keeping its registers
        (include/lac.h lac_encode_rebase): for callers that take the digits from
        ``trace`` and only need the coder state to continue."""
        check(self.lib.lac_encode_rebase(self.ctx, self._stream))

    def drain(self, out, fill):
        """Move every stream's settled output, as final bytes, behind the ``fill[b]`` bytes of
        row b of ``out`` and keep coding in the words that remain (include/lac.h
        lac_encode_drain): capacity then bounds the bits coded between two drains, not the
        stream.  ``out``: a contiguous uint8 device tensor [streams, stride], 8-byte aligned,
        stride a multiple of 8 (row b is stream b's slot); ``fill``: a contiguous int64/uint64 device tensor
        [streams], bytes already in each row, grown by what is written.  A stream whose settled
        bytes do not fit its row drains nothing.  The drained bytes followed by the bytes of the
        final :meth:`finish` are the undrained stream.  Asynchronous; no host sync."""
        torch = _torch()
        if out.dtype != torch.uint8 or out.device != self.device:
            raise TypeError("out must be a uint8 tensor on the coder's device")
        if out.dim() != 2 or out.shape[0] != self.streams or not out.is_contiguous():
            raise ValueError("out must be a contiguous [streams, stride] tensor (a row is a slot)")
        stride = out.shape[1]
        if stride % 8 or out.data_ptr() % 8:
            raise ValueError("out rows must be 8-byte aligned (row length a multiple of 8 bytes)")
        if fill.dtype not in (torch.int64, torch.uint64) or fill.device != self.device:
            raise TypeError("fill must be an int64/uint64 tensor on the coder's device")
        if tuple(fill.shape) != (self.streams,) or not fill.is_contiguous():
            raise ValueError(f"fill must be a contiguous [{self.streams}] tensor")
        self._drain_keep = (out, fill)
        check(self.lib.lac_encode_drain(self.ctx, C.c_void_p(out.data_ptr()), stride,
                                        C.c_void_p(fill.data_ptr()), self._stream))

    def status(self):
        err = np.zeros(self.streams, dtype=np.int32)
        step = np.zeros(self.streams, dtype=np.int64)
        rc = self.lib.lac_stream_status(self.ctx, err.ctypes.data_as(C.c_void_p), step.ctypes.data_as(C.c_void_p),
                                        self._stream)
        return rc, err, step

    def raise_on_error(self):
        rc, err, step = self.status()
        if rc:
            raise StreamError(rc, err, step)

    def registers(self):
        l = np.zeros(self.streams, dtype=np.int64)
        h = np.zeros(self.streams, dtype=np.int64)
        check(self.lib.lac_encoder_registers(self.ctx, l.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p),
                                             self._stream))
        return l, h

    def checkpoint(self):
        """Everything the encoder holds (include/lac.h lac_encode_get_state): per-stream
        registers and counters (a numpy ENC_STATE array) and the output planes
        ([2, streams, cap_words] uint64).  restore() continues from it bit for bit."""
        st = np.zeros(self.streams, dtype=ENC_STATE)
        words = self.bits_stride() // 8
        planes = np.zeros((2, self.streams, words), dtype=np.uint64)
        check(self.lib.lac_encode_get_state(self.ctx, st.ctypes.data_as(C.c_void_p),
                                            planes.ctypes.data_as(C.c_void_p), self._stream))
        return {"state": st, "planes": planes, "prec": self.prec, "vocab": self.vocab}

    def restore(self, ckpt):
        """Load a checkpoint() of a coder with the same prec, vocab, streams and capacity."""
        st, planes = ckpt["state"], ckpt["planes"]
        if ckpt.get("prec", self.prec) != self.prec or ckpt.get("vocab", self.vocab) != self.vocab:
            raise ValueError("checkpoint of a coder with another prec / vocab")
        if st.dtype != ENC_STATE or st.shape != (self.streams,):
            raise ValueError(f"state must be ENC_STATE[{self.streams}]")
        if planes.dtype != np.uint64 or planes.shape != (2, self.streams, self.bits_stride() // 8):
            raise ValueError("planes of another capacity or stream count")
        st, planes = np.ascontiguousarray(st), np.ascontiguousarray(planes)
        check(self.lib.lac_encode_set_state(self.ctx, st.ctypes.data_as(C.c_void_p),
                                            planes.ctypes.data_as(C.c_void_p), self._stream))

    def set_stream_lengths(self, lengths):
        """Per-stream symbol counts (include/lac.h lac_set_stream_lengths): stream b codes
        only its first ``lengths[b]`` symbols -- counted since the last reset / decode_open,
        over any number of calls -- and every later step is a no-op for it: nothing of its
        row or symbol is read, encode writes no trace entry, decode writes -1.  ``lengths``:
        a sequence, numpy array or tensor of ``streams`` integers >= 0; None clears.  The
        values are copied (uploaded as int64), nothing is borrowed; they persist across
        reset, the jobs and decode_open.  Not to be confused with :meth:`lengths`, the
        encoded bit counts."""
        if lengths is None:
            check(self.lib.lac_set_stream_lengths(self.ctx, None, self._stream))
            return
        torch = _torch()
        if isinstance(lengths, torch.Tensor):
            lengths = lengths.detach().cpu().numpy()
        n = np.asarray(lengths)
        if n.shape != (self.streams,):
            raise ValueError(f"lengths must have shape [{self.streams}], got {list(n.shape)}")
        if n.dtype.kind not in "iu":
            raise TypeError(f"lengths must be integers, got {n.dtype}")
        if n.size and int(n.min()) < 0:
            raise ValueError("lengths must be >= 0")
        if n.size and int(n.max()) > np.iinfo(np.int64).max:
            raise ValueError("lengths must fit int64")
        dev = torch.from_numpy(np.ascontiguousarray(n, dtype=np.int64)).to(self.device)
        check(self.lib.lac_set_stream_lengths(self.ctx, C.c_void_p(dev.data_ptr()), self._stream))
        # the library copies on the stream: keep the staging tensor until that copy is queued
        # behind everything else (the caching allocator reuses it in stream order)
        self._len_keep = dev

    def lengths(self):
        """Encoded bit counts per stream (after finish / a job).  The per-stream *symbol*
        counts of ragged batches are :meth:`set_stream_lengths`."""
        n = np.zeros(self.streams, dtype=np.uint64)
        check(self.lib.lac_encoded_lengths(self.ctx, n.ctypes.data_as(C.c_void_p), self._stream))
        return n

    def device_bits(self):
        """(int pointer, stride_bytes, nbits pointer) of the packed output in HBM."""
        p, s, n = C.c_void_p(), C.c_uint64(), C.c_void_p()
        check(self.lib.lac_encoded_device(self.ctx, C.byref(p), C.byref(s), C.byref(n)))
        return p.value, s.value, n.value

    def bits_tensor(self, stride=None):
        """Packed output copied into a fresh uint8 device tensor [streams, stride]."""
        torch = _torch()
        _, s, _ = self.device_bits()
        stride = int(stride or s)
        out = torch.zeros((self.streams, stride), dtype=torch.uint8, device=self.device)
        check(self.lib.lac_copy_bits_dev(self.ctx, C.c_void_p(out.data_ptr()), stride, self._stream))
        return out

    def bits_stride(self):
        """Bytes per stream of the packed output buffer (capacity rounded to 8-byte words)."""
        return int(self.device_bits()[1])

    def copy_bits_into(self, out):
        """Copy the packed output into a uint8 device tensor [streams, W] with
        contiguous rows (W <= bits_stride() keeps the first W bytes), asynchronously."""
        if out.dim() != 2 or out.shape[0] != self.streams or out.stride(1) != 1 or out.dtype != _torch().uint8:
            raise ValueError("out must be a uint8 [streams, W] tensor with contiguous rows")
        check(self.lib.lac_copy_bits_dev(self.ctx, C.c_void_p(out.data_ptr()), out.stride(0), self._stream))
        return out

    def copy_nbits_into(self, out):
        """Copy the per-stream bit counts into a contiguous 8-byte integer device tensor [streams]."""
        if out.shape != (self.streams,) or not out.is_contiguous() or out.element_size() != 8:
            raise ValueError("out must be a contiguous 8-byte integer tensor [streams]")
        check(self.lib.lac_copy_nbits_dev(self.ctx, C.c_void_p(out.data_ptr()), self._stream))
        return out

    def pack_bits(self, out, hdr_bytes, length):
        """The finished streams packed for the wire into the uint8 device tensor ``out``
        (include/lac.h lac_pack_bits: a header of bit counts, ``hdr_bytes`` = 2 or 4 each,
        then each stream's bytes back to back); ``length`` (a one-element 8-byte integer
        device tensor) receives the packed length.  Asynchronous; no host sync."""
        if hdr_bytes not in (2, 4) or (hdr_bytes == 2 and self.bits_stride() * 8 >= 1 << 16):
            raise ValueError(f"hdr_bytes={hdr_bytes}: 2-byte headers need streams of < 65536 bits "
                             f"(this coder's hold {self.bits_stride() * 8}), else 4")
        need = self.streams * (hdr_bytes + self.bits_stride())
        if out.dtype != _torch().uint8 or not out.is_contiguous() or out.numel() < need or out.device != self.device:
            raise ValueError(f"out must be a contiguous uint8 device tensor of >= {need} bytes on {self.device}")
        if length.numel() != 1 or length.element_size() != 8 or length.device != self.device:
            raise ValueError("length must be a one-element 8-byte integer tensor on the coder's device")
        check(self.lib.lac_pack_bits(self.ctx, C.c_void_p(out.data_ptr()), int(hdr_bytes),
                                     C.c_void_p(length.data_ptr()), self._stream))
        return out, length

    def pack_bits_at(self, out, hdr_bytes, base, end, len_out=None):
        """pack_bits appended at byte offset ``base[0]`` of ``out`` (include/lac.h
        lac_pack_bits_at): ``base`` / ``end`` are one-element 8-byte integer device
        tensors (``base`` may be None: offset 0), ``end`` receives base + the packed
        length; ``len_out`` is None or a device address (int) of 8 bytes -- e.g. from
        lac_host_alloc -- for the packed length.  Asynchronous; no host sync."""
        if hdr_bytes not in (2, 4) or (hdr_bytes == 2 and self.bits_stride() * 8 >= 1 << 16):
            raise ValueError(f"hdr_bytes={hdr_bytes}: 2-byte headers need streams of < 65536 bits "
                             f"(this coder's hold {self.bits_stride() * 8}), else 4")
        if out.dtype != _torch().uint8 or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"out must be a contiguous uint8 device tensor on {self.device}")
        for t in (base, end):
            if t is not None and (t.numel() < 1 or t.element_size() != 8 or t.device != self.device):
                raise ValueError("base / end must be 8-byte integer tensors on the coder's device")
        check(self.lib.lac_pack_bits_at(self.ctx, C.c_void_p(out.data_ptr()), out.numel(), int(hdr_bytes),
                                        None if base is None else C.c_void_p(base.data_ptr()),
                                        C.c_void_p(end.data_ptr()),
                                        None if len_out is None else C.c_void_p(int(len_out)), self._stream))
        return out

    def set_output(self, planes=None, nbits=None):
        """Direct later encodes' output (plane A and the bit counts, include/lac.h
        lac_set_output) into caller-owned device tensors: ``planes`` of >= streams *
        cap_words + 1 int64 (``output_words()``), ``nbits`` of streams int64; None, None
        restores the coder's own.  The tensors are kept referenced while in use.
        Only between jobs: raises LacError(LAC_E_STATE) while a decode is open or an
        encode has coded symbols it has not finished (``encode`` since ``reset``, no
        ``finish`` yet).  Afterwards the coder counts as finished (``pack_bits``) only
        when the buffers are those its last finished job went to."""
        if (planes is None) != (nbits is None):
            raise ValueError("planes and nbits: both or neither")
        if planes is not None:
            for t, n in ((planes, self.output_words()), (nbits, self.streams)):
                if t.element_size() != 8 or not t.is_contiguous() or t.numel() < n or t.device != self.device:
                    raise ValueError(f"output buffers: contiguous 8-byte tensors of >= {n} elements on {self.device}")
        check(self.lib.lac_set_output(self.ctx, None if planes is None else C.c_void_p(planes.data_ptr()),
                                      None if nbits is None else C.c_void_p(nbits.data_ptr())))
        self._output = (planes, nbits)

    def output_words(self):
        """uint64 words of one job's plane A (set_output): streams * cap_words + 1."""
        return self.streams * (self.bits_stride() // 8) + 1

    def nbits_tensor(self):
        """Per-stream bit counts as a fresh int64 device tensor (asynchronous copy)."""
        torch = _torch()
        out = torch.empty((self.streams,), dtype=torch.int64, device=self.device)
        check(self.lib.lac_copy_nbits_dev(self.ctx, C.c_void_p(out.data_ptr()), self._stream))
        return out

    def to_bytes(self):
        """Per-stream bytes (MSB first, last byte zero padded: group_bits format)."""
        self.raise_on_error()
        n = self.lengths()
        _, s, _ = self.device_bits()
        host = np.zeros((self.streams, s), dtype=np.uint8)
        check(self.lib.lac_copy_bits(self.ctx, host.ctypes.data_as(C.c_void_p), s, self._stream))
        return [host[b, :(int(n[b]) + 7) // 8].tobytes() for b in range(self.streams)], n

    def flush_digits(self):
        d = np.zeros((self.streams, 8), dtype=np.int8)
        c = np.zeros(self.streams, dtype=np.int32)
        check(self.lib.lac_flush_digits(self.ctx, d.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p),
                                        self._stream))
        return [d[b, :max(int(c[b]), 0)].tolist() for b in range(self.streams)]

    # ------------------------------------------------------------ decode
    def decode_open(self, bits=None, nbits=None):
        """Decode this coder's own output (no args), or ``bits`` (uint8 device
        tensor [streams, stride], stride % 8 == 0) with ``nbits`` (uint64/int64
        device tensor [streams])."""
        if bits is None:
            check(self.lib.lac_decode_open(self.ctx, None, 0, None, self._stream))
            self._dec_keep = None
            return
        torch = _torch()
        if bits.dtype != torch.uint8 or bits.device != self.device:
            raise TypeError("bits must be a uint8 tensor on the coder's device")
        if bits.dim() != 2 or bits.shape[0] != self.streams or bits.stride(1) != 1:
            raise ValueError("bits must be [streams, stride] with contiguous rows")
        if bits.stride(0) % 8 or bits.data_ptr() % 8:
            raise ValueError("bits rows must be 8-byte aligned (row stride a multiple of 8 bytes)")
        if nbits is None or nbits.dtype not in (torch.int64, torch.uint64) or nbits.device != self.device:
            raise TypeError("nbits must be an int64/uint64 tensor on the coder's device")
        if tuple(nbits.shape) != (self.streams,) or not nbits.is_contiguous():
            raise ValueError(f"nbits must be a contiguous [{self.streams}] tensor")
        # nbits[b] > 8 * stride fails that stream with a sticky LAC_E_ARG in the library
        self._dec_keep = (bits, nbits)                        # borrowed by the library
        check(self.lib.lac_decode_open(self.ctx, C.c_void_p(bits.data_ptr()), bits.stride(0),
                                       C.c_void_p(nbits.data_ptr()), self._stream))

    def decode_open_packed(self, payload, hdr_bytes, counts=None, base=None, end=None):
        """decode_open straight from the wire (include/lac.h lac_decode_open_packed): one packed
        job -- what :meth:`pack_bits` writes, ``hdr_bytes`` = 2 or 4; or with ``hdr_bytes`` = 0
        the streams' bytes back to back and their bit counts in ``counts`` (an 8-byte integer
        device tensor [streams]) -- is unpacked from the uint8 device tensor ``payload`` (any
        alignment; its size bounds every read) into slots the coder owns, and the decoder opens
        on them.  ``base`` / ``end``: one-element 8-byte integer device tensors or None; the job
        starts at byte ``base[0]`` (0 when None) and ``end`` receives the offset just past it,
        the next job's ``base``.  Asynchronous, no host sync, and nothing is borrowed: once the
        queued work has run ``payload`` may be overwritten.  A job that does not fit the
        payload fails every stream with a sticky LAC_E_ARG, a stream longer than the coder's
        capacity fails alone (:meth:`status`)."""
        torch = _torch()
        if hdr_bytes not in (0, 2, 4):
            raise ValueError(f"hdr_bytes={hdr_bytes}: 2 or 4, or 0 with counts")
        if payload.dtype != torch.uint8 or payload.dim() != 1 or not payload.is_contiguous() \
                or payload.device != self.device:
            raise ValueError(f"payload must be a contiguous 1-D uint8 device tensor on {self.device}")
        if payload.numel() == 0:
            raise ValueError("payload is empty")
        if hdr_bytes == 0:
            if counts is None or counts.element_size() != 8 or counts.is_floating_point() \
                    or counts.device != self.device:
                raise ValueError("hdr_bytes=0 needs counts: an 8-byte integer tensor on the coder's device")
            if tuple(counts.shape) != (self.streams,) or not counts.is_contiguous():
                raise ValueError(f"counts must be a contiguous [{self.streams}] tensor")
        for t in (base, end):
            if t is not None and (t.numel() < 1 or t.element_size() != 8 or t.device != self.device):
                raise ValueError("base / end must be 8-byte integer tensors on the coder's device")
        check(self.lib.lac_decode_open_packed(self.ctx, C.c_void_p(payload.data_ptr()), payload.numel(),
                                              int(hdr_bytes),
                                              C.c_void_p(counts.data_ptr()) if hdr_bytes == 0 else None,
                                              None if base is None else C.c_void_p(base.data_ptr()),
                                              None if end is None else C.c_void_p(end.data_ptr()), self._stream))
        self._dec_keep = None                                 # the decoder reads the coder's own slots

    def decode_open_window(self, bits, nbits=None, base=None):
        """decode_open through a sliding window (include/lac.h lac_decode_open_window): the
        coder keeps ``bits_stride()`` bytes per stream on the device and :meth:`refill` slides
        them over streams of any length, so ``capacity_bits`` bounds the bits decoded between
        two refills (``N * (prec + 2) + 256`` for N steps), not the stream.  ``bits``: a
        :class:`HostBits` (the streams stay in host memory) or a uint8 device tensor
        [streams, stride] with ``nbits`` as in :meth:`decode_open`; ``base``: None, or per
        stream the source word the window starts at (a sequence or an 8-byte integer device
        tensor [streams]) -- with :meth:`set_state`-style resume, what :meth:`window_base`
        returned.  The source is borrowed until the next open.  Everything after it -- every
        decode path, :meth:`set_stream_lengths`, :meth:`set_decode_stop`, the logits decode --
        is what it is after :meth:`decode_open`; decoder positions are window-relative."""
        torch = _torch()
        if isinstance(bits, HostBits):
            if bits.streams != self.streams or bits.device != self.device:
                raise ValueError("HostBits of another stream count or device")
            if bits.dev_addr is None:
                raise ValueError("HostBits is closed")
            ptr, stride, nbits = bits.dev_addr, bits.stride, bits.nbits
        else:
            if bits.dtype != torch.uint8 or bits.device != self.device:
                raise TypeError("bits must be a uint8 tensor on the coder's device")
            if bits.dim() != 2 or bits.shape[0] != self.streams or bits.stride(1) != 1:
                raise ValueError("bits must be [streams, stride] with contiguous rows")
            ptr, stride = bits.data_ptr(), bits.stride(0)       # (alignment: the library's LAC_E_ARG)
        if nbits is None or nbits.dtype not in (torch.int64, torch.uint64) or nbits.device != self.device:
            raise TypeError("nbits must be an int64/uint64 tensor on the coder's device")
        if tuple(nbits.shape) != (self.streams,) or not nbits.is_contiguous():
            raise ValueError(f"nbits must be a contiguous [{self.streams}] tensor")
        if base is not None and not isinstance(base, torch.Tensor):
            b = np.asarray(base)
            if b.shape != (self.streams,) or b.dtype.kind not in "iu" or (b.size and int(b.min()) < 0):
                raise ValueError(f"base must be {self.streams} integers >= 0")
            base = torch.from_numpy(np.ascontiguousarray(b).astype(np.int64)).to(self.device)
        if base is not None and (base.element_size() != 8 or base.is_floating_point() or base.device != self.device
                                 or tuple(base.shape) != (self.streams,) or not base.is_contiguous()):
            raise ValueError(f"base must be a contiguous 8-byte integer [{self.streams}] tensor on the coder's device")
        check(self.lib.lac_decode_open_window(self.ctx, C.c_void_p(ptr), stride, C.c_void_p(nbits.data_ptr()),
                                              None if base is None else C.c_void_p(base.data_ptr()), self._stream))
        self._dec_keep = (bits, nbits, base)                  # borrowed by the library

    def refill(self):
        """Slide every stream's window up to the decoder's position (include/lac.h
        lac_decode_refill): call it at least every N steps for a window sized for N, and once
        after the last step -- a stream that outran its window is found here (sticky
        LAC_E_CAPACITY in :meth:`status`), not by the steps.  One launch; no host sync."""
        check(self.lib.lac_decode_refill(self.ctx, self._stream))

    def window_base(self):
        """Per stream: the source word the window starts at (uint64 [streams]); a decoder
        position ``pos`` is bit ``pos + 64 * window_base()`` of the stream.  Synchronises."""
        n = np.zeros(self.streams, dtype=np.uint64)
        check(self.lib.lac_decode_window_base(self.ctx, n.ctypes.data_as(C.c_void_p), self._stream))
        return n

    def determined(self):
        """Per stream: leading decoded symbols fixed by the available bits (the
        count the reference's A_from_bin.run(bits, stop=0) emits)."""
        n = np.zeros(self.streams, dtype=np.int64)
        check(self.lib.lac_decode_determined(self.ctx, n.ctypes.data_as(C.c_void_p), self._stream))
        return n

    def decode(self, pmf, out=None):
        """Decode one symbol per stream per step; pmf as in :meth:`encode`."""
        torch = _torch()
        self._check_pmf(pmf)
        if pmf.dim() == 2:
            pmf = pmf.unsqueeze(0)
        if pmf.dim() != 3:
            raise ValueError("give decode a [steps, streams, V] (or expanded) table")
        if pmf.shape[1] not in (1, self.streams):
            raise ValueError(f"pmf must be [steps, {self.streams} or 1, {self.vocab}], got {tuple(pmf.shape)}")
        steps = pmf.shape[0]
        step_stride = pmf.stride(0) if steps > 1 else 0
        stream_stride = pmf.stride(1) if pmf.shape[1] > 1 else 0
        if out is None:
            out = torch.empty((steps, self.streams), dtype=torch.int32, device=self.device)
        else:
            self._check_out(out, steps)
        check(self.lib.lac_decode_steps(self.ctx, C.c_void_p(pmf.data_ptr()), step_stride, stream_stride, steps,
                                        C.c_void_p(out.data_ptr()), self._stream))
        return out

    # ------------------------------------------------------------ finite-state models
    def load_fsm(self, tables, next=None):
        """Load a finite-state model (include/lac.h lac_fsm_load; the reference's
        NFA(state, transitions), arith_code.py:423-434): ``tables`` [K, vocab] integer pmf rows,
        one per state (a numpy array, or a device tensor in the coder's entry type), ``next``
        [K, vocab] int32 transitions or None for a model coded with explicit states only.  The
        model is copied into a prepared form the coder owns -- the arguments are free afterwards
        -- and every stream's state becomes 0.  Only between jobs.  K * vocab <= 2^24 and
        vocab <= 65536; a transition outside [0, K) raises LacError(LAC_E_TABLE)."""
        torch = _torch()
        if isinstance(tables, torch.Tensor):
            self._check_pmf(tables)
            tab = tables.contiguous()
        else:
            a = np.asarray(tables)
            if a.dtype.kind not in "iu":
                raise TypeError(f"tables must be integers, got {a.dtype}")
            u, i = (np.uint32, np.int32) if self.pmf_bits == 32 else (np.uint64, np.int64)
            tab = torch.from_numpy(np.ascontiguousarray(a.astype(u)).view(i)).to(self.device)
        if tab.dim() != 2 or tab.shape[1] != self.vocab:
            raise ValueError(f"tables must be [states, {self.vocab}], got {tuple(tab.shape)}")
        nxt = None
        if next is not None:
            nxt = next if isinstance(next, torch.Tensor) else torch.from_numpy(
                np.ascontiguousarray(np.asarray(next), dtype=np.int32))
            if nxt.dtype != torch.int32 or tuple(nxt.shape) != tuple(tab.shape):
                raise ValueError(f"next must be int32 {tuple(tab.shape)}")
            nxt = nxt.to(self.device).contiguous()
        check(self.lib.lac_fsm_load(self.ctx, C.c_void_p(tab.data_ptr()),
                                    None if nxt is None else C.c_void_p(nxt.data_ptr()), tab.shape[0], self._stream))
        self.fsm_states_count = int(tab.shape[0])

    def _fsm_state_rows(self, states, steps):
        """-> a contiguous int32 device tensor [steps, streams] (kept referenced), or None."""
        if states is None:
            return None
        torch = _torch()
        if not isinstance(states, torch.Tensor):
            states = torch.from_numpy(np.ascontiguousarray(np.asarray(states), dtype=np.int32))
        if states.dtype != torch.int32 or tuple(states.shape) != (steps, self.streams):
            raise ValueError(f"states must be int32 [{steps}, {self.streams}]")
        return states.to(self.device).contiguous()

    def set_fsm_states(self, states=None):
        """The current state of every stream (lac_fsm_set_states): ``streams`` integers, or
        None for state 0 everywhere.  Copied; kept in the coder across calls."""
        if states is None:
            check(self.lib.lac_fsm_set_states(self.ctx, None, self._stream))
            return
        torch = _torch()
        arr = states.detach().cpu().numpy() if isinstance(states, torch.Tensor) else np.asarray(states)
        dev = self._fsm_state_rows(arr.reshape(1, -1), 1)
        check(self.lib.lac_fsm_set_states(self.ctx, C.c_void_p(dev.data_ptr()), self._stream))
        self._fsm_keep = dev

    def fsm_states(self):
        """Every stream's current state (int32 numpy [streams]); synchronises."""
        torch = _torch()
        out = torch.empty((self.streams,), dtype=torch.int32, device=self.device)
        check(self.lib.lac_fsm_get_states(self.ctx, C.c_void_p(out.data_ptr()), self._stream))
        return out.cpu().numpy()

    def encode_fsm(self, sym, states=None, trace=None):
        """Continue every stream by ``sym`` [steps, streams] (int32 device tensor) under the
        loaded model, in one launch: step t codes with the row of the stream's state and moves
        it by ``next`` -- or, with ``states`` [steps, streams], with the row of states[t, b].
        Bit for bit :meth:`encode` on the gathered rows; ``trace`` as there."""
        torch = _torch()
        if sym.dtype != torch.int32 or sym.device != self.device:
            raise TypeError("sym must be an int32 tensor on the coder's device")
        sym = sym.contiguous()
        steps = sym.shape[0] if sym.dim() == 2 else 1
        if sym.numel() != steps * self.streams:
            raise ValueError(f"sym must be [steps, {self.streams}]")
        st = self._fsm_state_rows(states, steps)
        tp = None
        if trace is not None:
            if trace.dtype != torch.int64 or trace.numel() != steps * self.streams * 2 or not trace.is_contiguous():
                raise ValueError("trace must be a contiguous int64 tensor [steps, streams, 2]")
            tp = C.c_void_p(trace.data_ptr())
        self._keep = (sym, st)
        check(self.lib.lac_fsm_encode(self.ctx, C.c_void_p(sym.data_ptr()),
                                      None if st is None else C.c_void_p(st.data_ptr()), steps, tp, self._stream))

    def encode_fsm_job(self, sym, state0=None, states=None):
        """reset + set_fsm_states(state0) + encode_fsm + finish."""
        self.reset()
        self.set_fsm_states(state0)
        self.encode_fsm(sym, states)
        self.finish()

    def decode_fsm(self, steps, states=None, out=None):
        """Decode ``steps`` symbols per stream under the loaded model in one launch (after any
        decode_open*); ``states`` as in :meth:`encode_fsm`.  -> int32 [steps, streams]."""
        torch = _torch()
        steps = int(steps)
        if out is None:
            out = torch.empty((steps, self.streams), dtype=torch.int32, device=self.device)
        else:
            self._check_out(out, steps)
        st = self._fsm_state_rows(states, steps)
        self._keep = (st,)
        check(self.lib.lac_fsm_decode(self.ctx, None if st is None else C.c_void_p(st.data_ptr()), steps,
                                      C.c_void_p(out.data_ptr()), self._stream))
        return out

    # ------------------------------------------------------------ adaptive count models
    def load_counts(self, order, weights):
        """Load an adaptive n-gram count model (include/lac.h lac_count_load; the reference's
        Markov_up_to_n, arith_code.py:443-464, with lfunc(c, o, n, order) == c * weights[o]):
        every stream gets zeroed counts and an empty past.  Only between jobs.  1 <= order <= 4,
        vocab <= 4096, sum vocab^(i+1) <= 2^25 counts per stream, weights < 2^30."""
        order = int(order)
        w = [int(x) for x in weights]
        if len(w) != order:
            raise ValueError(f"give {order} weights, got {len(w)}")
        if any(x < 0 or x >= 1 << 32 for x in w):
            raise ValueError("weights must be in [0, 2^30)")
        arr = (C.c_uint32 * max(order, 1))(*w)
        check(self.lib.lac_count_load(self.ctx, order, arr, self._stream))
        out = (C.c_int64 * 6)()
        check(self.lib.lac_count_layout(self.ctx, out))
        self.count_order = order
        self.count_weights = w
        self.count_layout = {"Vc": int(out[0]), "stride": int(out[1]), "off": [int(out[2 + i]) for i in range(order)]}

    def _need_counts(self):
        if getattr(self, "count_layout", None) is None:
            from ._lib import LacError, LAC_E_STATE
            raise LacError(LAC_E_STATE, "no count model: call load_counts first")

    def set_count_state(self, counts=None, past=None):
        """Every stream's counts (uint32 [streams, stride] in the layout of ``count_layout``,
        numpy or a device int32 / uint32 tensor; None: all zero) and past ([streams, order]
        integers, most recent last, -1 absent; None: empty).  Copied."""
        torch = _torch()
        self._need_counts()
        cd = pd = None
        if counts is not None:
            if isinstance(counts, torch.Tensor):
                cd = counts.to(self.device).contiguous()
            else:
                cd = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.uint32).view(np.int32)).to(self.device)
            if cd.element_size() != 4 or cd.numel() != self.streams * self.count_layout["stride"]:
                raise ValueError(f"counts must be 32-bit [{self.streams}, {self.count_layout['stride']}]")
        if past is not None:
            arr = past.detach().cpu().numpy() if isinstance(past, torch.Tensor) else np.asarray(past)
            if arr.size != self.streams * self.count_order:
                raise ValueError(f"past must be [{self.streams}, {self.count_order}]")
            pd = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.int32)).to(self.device)
        check(self.lib.lac_count_set_state(self.ctx, None if cd is None else C.c_void_p(cd.data_ptr()),
                                           None if pd is None else C.c_void_p(pd.data_ptr()), self._stream))
        self._count_keep = (cd, pd)

    def count_state(self, device=False):
        """-> (counts uint32 [streams, stride], past int32 [streams, order]) as numpy arrays, or
        (``device=True``) as device tensors (counts as int32 bit patterns); synchronises."""
        torch = _torch()
        self._need_counts()
        counts = torch.empty((self.streams, self.count_layout["stride"]), dtype=torch.int32, device=self.device)
        past = torch.empty((self.streams, self.count_order), dtype=torch.int32, device=self.device)
        check(self.lib.lac_count_get_state(self.ctx, C.c_void_p(counts.data_ptr()), C.c_void_p(past.data_ptr()),
                                           self._stream))
        if device:
            torch.cuda.current_stream(self.device).synchronize()
            return counts, past
        return counts.cpu().numpy().view(np.uint32), past.cpu().numpy()

    def encode_counts(self, sym, trace=None):
        """Continue every stream by ``sym`` [steps, streams] (int32 device tensor) under the
        loaded count model, in one launch: step t codes with the row the stream's counts give
        and then counts the symbol.  Bit for bit :meth:`encode` on those rows; ``trace`` as
        there."""
        torch = _torch()
        if sym.dtype != torch.int32 or sym.device != self.device:
            raise TypeError("sym must be an int32 tensor on the coder's device")
        sym = sym.contiguous()
        steps = sym.shape[0] if sym.dim() == 2 else 1
        if sym.numel() != steps * self.streams:
            raise ValueError(f"sym must be [steps, {self.streams}]")
        tp = None
        if trace is not None:
            if trace.dtype != torch.int64 or trace.numel() != steps * self.streams * 2 or not trace.is_contiguous():
                raise ValueError("trace must be a contiguous int64 tensor [steps, streams, 2]")
            tp = C.c_void_p(trace.data_ptr())
        self._keep = (sym,)
        check(self.lib.lac_count_encode(self.ctx, C.c_void_p(sym.data_ptr()), steps, tp, self._stream))

    def encode_counts_job(self, sym):
        """reset + set_count_state() (zero counts, empty past) + encode_counts + finish."""
        self.reset()
        self.set_count_state()
        self.encode_counts(sym)
        self.finish()

    def decode_counts(self, steps, out=None):
        """Decode ``steps`` symbols per stream under the loaded count model in one launch (after
        any decode_open*), from the counts and past the streams hold.  -> int32 [steps, streams]."""
        torch = _torch()
        steps = int(steps)
        if out is None:
            out = torch.empty((steps, self.streams), dtype=torch.int32, device=self.device)
        else:
            self._check_out(out, steps)
        check(self.lib.lac_count_decode(self.ctx, steps, C.c_void_p(out.data_ptr()), self._stream))
        return out

    # ------------------------------------------------------------ match-history models
    def load_history(self, P, weights):
        """Load a match-history model (include/lac.h lac_hist_load; the reference's History,
        arith_code.py:364-398, with lfunc(r, i, n, P) == weights[i][r]): a ring of the last ``P``
        symbols per stream, all -1, write index 0.  ``weights``: [P, P] non-negative integers
        below 2^48.  Only between jobs.  1 <= P <= 256, vocab <= 4096."""
        P = int(P)
        try:
            w = np.array([[int(x) for x in row] for row in weights], dtype=object).reshape(max(P, 0), max(P, 0))
        except (TypeError, ValueError):
            raise ValueError(f"weights must be [{P}, {P}] integers") from None
        if any(x < 0 or x >= 1 << 64 for x in w.ravel().tolist()):
            raise ValueError("weights must be in [0, 2^48)")
        arr = np.ascontiguousarray(w.astype(np.uint64)) if P > 0 else np.zeros(1, dtype=np.uint64)
        check(self.lib.lac_hist_load(self.ctx, P, arr.ctypes.data_as(C.c_void_p), self._stream))
        self.history_past = P
        self.history_weights = arr

    def _need_history(self):
        if getattr(self, "history_past", None) is None:
            from ._lib import LacError, LAC_E_STATE
            raise LacError(LAC_E_STATE, "no history model: call load_history first")

    def set_history_state(self, ring=None, pasti=None):
        """Every stream's ring ([streams, P] integers in [-1, vocab), -1 unset; None: all -1) and
        write index ([streams] integers in [0, P); None: 0).  Copied; the match lengths the
        kernels keep are rebuilt from them."""
        torch = _torch()
        self._need_history()
        rd = pd = None
        if ring is not None:
            arr = ring.detach().cpu().numpy() if isinstance(ring, torch.Tensor) else np.asarray(ring)
            if arr.size != self.streams * self.history_past:
                raise ValueError(f"ring must be [{self.streams}, {self.history_past}]")
            rd = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.int32)).to(self.device)
        if pasti is not None:
            arr = pasti.detach().cpu().numpy() if isinstance(pasti, torch.Tensor) else np.asarray(pasti)
            if arr.size != self.streams:
                raise ValueError(f"pasti must be [{self.streams}]")
            pd = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.int32)).to(self.device)
        check(self.lib.lac_hist_set_state(self.ctx, None if rd is None else C.c_void_p(rd.data_ptr()),
                                          None if pd is None else C.c_void_p(pd.data_ptr()), self._stream))
        self._history_keep = (rd, pd)

    def history_state(self):
        """-> (ring int32 [streams, P], pasti int32 [streams]) as numpy arrays; synchronises."""
        torch = _torch()
        self._need_history()
        ring = torch.empty((self.streams, self.history_past), dtype=torch.int32, device=self.device)
        pasti = torch.empty((self.streams,), dtype=torch.int32, device=self.device)
        check(self.lib.lac_hist_get_state(self.ctx, C.c_void_p(ring.data_ptr()), C.c_void_p(pasti.data_ptr()),
                                          self._stream))
        return ring.cpu().numpy(), pasti.cpu().numpy()

    def encode_history(self, sym, trace=None):
        """Continue every stream by ``sym`` [steps, streams] (int32 device tensor) under the
        loaded history model, in one launch: step t codes with the row the stream's ring gives
        and then writes the symbol into it.  Bit for bit :meth:`encode` on those rows; ``trace``
        as there."""
        torch = _torch()
        if sym.dtype != torch.int32 or sym.device != self.device:
            raise TypeError("sym must be an int32 tensor on the coder's device")
        sym = sym.contiguous()
        steps = sym.shape[0] if sym.dim() == 2 else 1
        if sym.numel() != steps * self.streams:
            raise ValueError(f"sym must be [steps, {self.streams}]")
        tp = None
        if trace is not None:
            if trace.dtype != torch.int64 or trace.numel() != steps * self.streams * 2 or not trace.is_contiguous():
                raise ValueError("trace must be a contiguous int64 tensor [steps, streams, 2]")
            tp = C.c_void_p(trace.data_ptr())
        self._keep = (sym,)
        check(self.lib.lac_hist_encode(self.ctx, C.c_void_p(sym.data_ptr()), steps, tp, self._stream))

    def encode_history_job(self, sym):
        """reset + set_history_state() (empty rings) + encode_history + finish."""
        self.reset()
        self.set_history_state()
        self.encode_history(sym)
        self.finish()

    def decode_history(self, steps, out=None):
        """Decode ``steps`` symbols per stream under the loaded history model in one launch (after
        any decode_open*), from the rings the streams hold.  -> int32 [steps, streams]."""
        torch = _torch()
        steps = int(steps)
        if out is None:
            out = torch.empty((steps, self.streams), dtype=torch.int32, device=self.device)
        else:
            self._check_out(out, steps)
        check(self.lib.lac_hist_decode(self.ctx, steps, C.c_void_p(out.data_ptr()), self._stream))
        return out

    # ------------------------------------------------------------ range-level coding
    def _range_tensor(self, x, what, shape):
        torch = _torch()
        if not isinstance(x, torch.Tensor) or x.dtype not in (torch.int64, torch.uint64) or x.device != self.device:
            raise TypeError(f"{what} must be an int64 (bit pattern of uint64) tensor on the coder's device")
        if tuple(x.shape) != shape:
            raise ValueError(f"{what} must be {list(shape)}, got {list(x.shape)}")
        return x.contiguous()

    def _range_args(self, lo, hi, tot, trace):
        torch = _torch()
        if not isinstance(lo, torch.Tensor) or lo.dim() not in (1, 2):
            raise ValueError(f"lo must be a [steps, {self.streams}] tensor")
        steps = lo.shape[0] if lo.dim() == 2 else 1
        shape = (steps, self.streams) if lo.dim() == 2 else (self.streams,)
        lo, hi = self._range_tensor(lo, "lo", shape), self._range_tensor(hi, "hi", shape)
        if isinstance(tot, int) and not isinstance(tot, bool):          # one total for the whole job
            if not 0 <= tot < 1 << 64:
                raise ValueError("tot must fit uint64")
            tot = torch.tensor([tot - (1 << 64) if tot >> 63 else tot], dtype=torch.int64, device=self.device)
            step_stride = stream_stride = 0
        elif isinstance(tot, torch.Tensor) and tot.dim() == 1 and lo.dim() == 2:   # a total per stream
            tot = self._range_tensor(tot, "tot", (self.streams,))
            step_stride, stream_stride = 0, 1
        else:
            tot = self._range_tensor(tot, "tot", shape)
            step_stride, stream_stride = self.streams, 1
        tp = None
        if trace is not None:
            if trace.dtype != torch.int64 or trace.numel() != steps * self.streams * 2 or not trace.is_contiguous():
                raise ValueError("trace must be a contiguous int64 tensor [steps, streams, 2]")
            tp = C.c_void_p(trace.data_ptr())
        self._keep = (lo, hi, tot)
        return (self.ctx, C.c_void_p(lo.data_ptr()), C.c_void_p(hi.data_ptr()), C.c_void_p(tot.data_ptr()),
                step_stride, stream_stride, steps, tp, self._stream)

    def encode_ranges(self, lo, hi, tot, trace=None):
        """Continue every stream by symbols given as ranges (include/lac.h lac_encode_ranges): step t
        of stream b narrows by ``lo[t, b] = c_{s-1}``, ``hi[t, b] = c_s`` out of ``tot`` -- what
        ``symbol_to_range`` reads of a CDF -- with no table anywhere.  ``lo``, ``hi``: int64 device
        tensors [steps, streams] (bit patterns of uint64); ``tot``: the same shape, [streams] (a
        total per stream) or a Python int (one total for the job).  Valid: 0 < tot <= 2^(prec-1)
        and lo < hi <= tot.  Bit for bit :meth:`encode` on the tables [lo, hi - lo, tot - hi] with
        symbol 1; one launch whatever the steps; ``trace`` as there."""
        check(self.lib.lac_encode_ranges(*self._range_args(lo, hi, tot, trace)))

    def encode_ranges_job(self, lo, hi, tot, trace=None):
        """reset + :meth:`encode_ranges` + finish."""
        check(self.lib.lac_encode_ranges_job(*self._range_args(lo, hi, tot, trace)))

    def decode_ranges_step(self, prev=None, next_tot=None, out=None):
        """One position of a range-level decode (include/lac.h lac_decode_ranges_step), one launch:
        advance every stream by ``prev = (lo, hi, tot)``, the range of the symbol its last target
        named (int64 device tensors [streams]; None: no advance), then peek the next targets under
        the totals ``next_tot`` ([streams] or a Python int; None: no peek).  -> int64 [streams]
        targets ``floor((x - l) * T' / w)`` (``out`` or a new tensor; -1, the bit pattern of
        UINT64_MAX, for a stream with a sticky error, at its count, or with an invalid total), or
        None without a peek.  The caller's model maps a target to its symbol and range."""
        torch = _torch()
        lo = hi = tot = None
        if prev is not None:
            lo, hi, tot = (self._range_tensor(x, n, (self.streams,)) for x, n in zip(prev, ("lo", "hi", "tot")))
        nt = None
        if next_tot is not None:
            if isinstance(next_tot, int) and not isinstance(next_tot, bool):
                nt = torch.full((self.streams,), next_tot - (1 << 64) if next_tot >> 63 else next_tot,
                                dtype=torch.int64, device=self.device)
            else:
                nt = self._range_tensor(next_tot, "next_tot", (self.streams,))
            if out is None:
                out = torch.empty((self.streams,), dtype=torch.int64, device=self.device)
            elif out.dtype != torch.int64 or out.device != self.device or tuple(out.shape) != (self.streams,) \
                    or not out.is_contiguous():
                raise ValueError(f"out must be a contiguous int64 [{self.streams}] tensor on the coder's device")
        p = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
        self._keep = (lo, hi, tot, nt)
        check(self.lib.lac_decode_ranges_step(self.ctx, p(lo), p(hi), p(tot), p(nt), p(out) if nt is not None else None,
                                              self._stream))
        return out if nt is not None else None

    # ------------------------------------------------------------ sparse rows
    def _sparse_rows(self, idx, wt, base, steps=None):
        """-> (idx, wt, K, step_stride, stream_stride, base, steps) of a [steps, streams or 1, K] or
        [streams or 1, K] pair of tensors; strides (in slots) are taken from idx, and wt is brought
        to the same layout as uint32 bit patterns."""
        torch = _torch()
        if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int32 or idx.device != self.device:
            raise TypeError("idx must be an int32 tensor on the coder's device")
        if not isinstance(wt, torch.Tensor) or wt.dtype not in (torch.int32, torch.int64) or wt.device != self.device:
            raise TypeError("wt must be an int64 or int32 (bit pattern of uint32) tensor on the coder's device")
        if idx.shape != wt.shape:
            raise ValueError(f"idx is {list(idx.shape)}, wt is {list(wt.shape)}")
        if isinstance(base, bool) or not isinstance(base, int) or not 0 <= base < 1 << 32:
            raise ValueError("base must be a Python int that fits uint32")
        if idx.dim() == 2:
            if steps not in (None, 1):
                raise ValueError("a 2-D idx is [streams or 1, K] for one step")
            idx, wt = idx.unsqueeze(0), wt.unsqueeze(0)
        if idx.dim() != 3 or idx.shape[1] not in (1, self.streams) or (steps is not None and idx.shape[0] not in (1, steps)):
            raise ValueError(f"idx must be [steps, {self.streams} or 1, K], got {list(idx.shape)}")
        if idx.stride(-1) != 1:
            raise ValueError("the K slots of a row must be contiguous")
        if wt.dtype != torch.int32 or wt.stride() != idx.stride() or wt.data_ptr() % 16:
            # one copy of the rows idx really holds (its expanded dims re-use theirs), laid out as idx's
            core = tuple(slice(0, 1) if st == 0 and n > 1 else slice(None) for st, n in zip(idx.stride(), idx.shape))
            ci, cw = idx[core], wt[core]
            if cw.dtype == torch.int64:                          # uint32 values held in int64 -> their bit patterns
                if bool(((cw < 0) | (cw >= 1 << 32)).any()):     # (synchronises; int32 weights are taken as they are)
                    raise ValueError("an int64 weight outside [0, 2^32)")
                cw = torch.where(cw >= 1 << 31, cw - (1 << 32), cw)
            buf = torch.empty_strided(ci.shape, ci.stride(), dtype=torch.int32, device=self.device)
            buf.copy_(cw)
            wt = buf.expand(idx.shape)
        steps = idx.shape[0] if steps is None else steps
        step_stride = idx.stride(0) if idx.shape[0] > 1 else 0
        stream_stride = idx.stride(1) if idx.shape[1] > 1 else 0
        return idx, wt, idx.shape[2], step_stride, stream_stride, base, steps

    def _sparse_encode_args(self, idx, wt, base, sym, trace):
        torch = _torch()
        if sym.dtype != torch.int32 or sym.device != self.device:
            raise TypeError("sym must be an int32 tensor on the coder's device")
        sym = sym.contiguous()
        steps = sym.shape[0] if sym.dim() == 2 else 1
        if sym.numel() != steps * self.streams:
            raise ValueError(f"sym must be [steps, {self.streams}]")
        idx, wt, K, step_stride, stream_stride, base, steps = self._sparse_rows(idx, wt, base, steps)
        tp = None
        if trace is not None:
            if trace.dtype != torch.int64 or trace.numel() != steps * self.streams * 2 or not trace.is_contiguous():
                raise ValueError("trace must be a contiguous int64 tensor [steps, streams, 2]")
            tp = C.c_void_p(trace.data_ptr())
        self._keep = (idx, wt, sym)
        return (self.ctx, C.c_void_p(idx.data_ptr()), C.c_void_p(wt.data_ptr()), K, step_stride, stream_stride, base,
                C.c_void_p(sym.data_ptr()), steps, tp, self._stream)

    def encode_sparse(self, idx, wt, base, sym, trace=None):
        """Continue every stream by ``sym[t, b]`` under sparse rows (include/lac.h lac_encode_sparse):
        row (t, b) is the K slots ``idx[t, b, :]`` (int32: ascending symbols, then -1 pads) with the
        weights ``wt[t, b, :]`` (int64 in [0, 2^32), checked, or int32 bit patterns of uint32) over the floor ``base`` -- the
        dense row ``base + wt_j at idx_j``.  ``idx``, ``wt``: [steps, streams or 1, K] or
        [streams or 1, K] (one step), K a multiple of 4 in [4, 256]; ``expand``-ed dims re-use rows,
        strides are taken from ``idx`` (multiples of 4, rows 16-byte aligned).  Bit for bit
        :meth:`encode` of a ``pmf_bits = 64`` coder on ``lac_amd.sparse.dense_rows``; one launch
        whatever the steps; ``trace`` as there."""
        check(self.lib.lac_encode_sparse(*self._sparse_encode_args(idx, wt, base, sym, trace)))

    def encode_sparse_job(self, idx, wt, base, sym, trace=None):
        """reset + :meth:`encode_sparse` + finish."""
        check(self.lib.lac_encode_sparse_job(*self._sparse_encode_args(idx, wt, base, sym, trace)))

    def decode_sparse(self, idx, wt, base, out=None):
        """Decode one symbol per stream per step under sparse rows (include/lac.h
        lac_decode_sparse_steps); rows as in :meth:`encode_sparse`.  -> int32 [steps, streams]."""
        torch = _torch()
        idx, wt, K, step_stride, stream_stride, base, steps = self._sparse_rows(idx, wt, base)
        if out is None:
            out = torch.empty((steps, self.streams), dtype=torch.int32, device=self.device)
        else:
            self._check_out(out, steps)
        self._keep = (idx, wt)
        check(self.lib.lac_decode_sparse_steps(self.ctx, C.c_void_p(idx.data_ptr()), C.c_void_p(wt.data_ptr()), K,
                                               step_stride, stream_stride, base, steps, C.c_void_p(out.data_ptr()),
                                               self._stream))
        return out

    # ------------------------------------------------------------ logits path
    def _logits_args(self, logits, steps=None):
        """-> (type, step_stride, stream_stride, steps) for a [steps, streams, V]
        bf16/f32 logits tensor (stride-0 broadcasts allowed, rows contiguous)."""
        torch = _torch()
        typ = {torch.bfloat16: _lib.LAC_LOGITS_BF16, torch.float32: _lib.LAC_LOGITS_F32}.get(logits.dtype)
        if typ is None:
            raise TypeError(f"logits must be bfloat16 or float32, got {logits.dtype}")
        if logits.device != self.device:
            raise ValueError(f"logits are on {logits.device}, coder on {self.device}")
        if logits.dim() == 2:
            logits = logits.unsqueeze(0)
        if logits.dim() != 3 or logits.shape[1] not in (1, self.streams) or logits.shape[2] != self.vocab:
            raise ValueError(f"logits must be [steps, {self.streams}, {self.vocab}]")
        if logits.stride(2) != 1:
            raise ValueError("logit rows must be contiguous")
        n = logits.shape[0] if steps is None else steps
        if logits.shape[0] not in (1, n):
            raise ValueError("logits steps do not match the symbols")
        step_stride = logits.stride(0) if logits.shape[0] > 1 else 0
        stream_stride = logits.stride(1) if logits.shape[1] > 1 else 0
        return typ, step_stride, stream_stride, n, logits

    def _logits_encode_args(self, logits, sym, trace):
        torch = _torch()
        if sym.dtype != torch.int32 or sym.device != self.device:
            raise TypeError("sym must be an int32 tensor on the coder's device")
        sym = sym.contiguous()
        steps = sym.shape[0] if sym.dim() == 2 else 1
        if sym.numel() != steps * self.streams:
            raise ValueError(f"sym must be [steps, {self.streams}]")
        typ, ss, bs, steps, logits = self._logits_args(logits, steps)
        tp = None
        if trace is not None:
            if trace.dtype != torch.int64 or trace.numel() != steps * self.streams * 2 or not trace.is_contiguous():
                raise ValueError("trace must be a contiguous int64 tensor [steps, streams, 2]")
            tp = C.c_void_p(trace.data_ptr())
        self._keep = (logits, sym)
        return (self.ctx, C.c_void_p(logits.data_ptr()), typ, ss, bs, C.c_void_p(sym.data_ptr()), steps, tp,
                self._stream)

    def encode_logits(self, logits, sym, trace=None):
        """Incremental logits encode: continue every stream by ``steps`` symbols
        (no reset, no finish -- call :meth:`finish` at the end).  Steps may be
        interleaved with :meth:`encode` on integer pmfs."""
        check(self.lib.lac_encode_logits(*self._logits_encode_args(logits, sym, trace)))

    def encode_logits_job(self, logits, sym, trace=None):
        """reset + encode + finish with tables computed in-kernel from logits by
        the q1 quantiser (include/lac.h "logits path"): the pmf never touches
        HBM.  ``logits`` [steps, streams, V] bf16/f32, ``sym`` [steps, streams]."""
        check(self.lib.lac_encode_logits_job(*self._logits_encode_args(logits, sym, trace)))

    def decode_logits(self, logits, out=None):
        """Decode one symbol per stream per step with q1 tables from ``logits``."""
        torch = _torch()
        typ, ss, bs, steps, logits = self._logits_args(logits)
        if out is None:
            out = torch.empty((steps, self.streams), dtype=torch.int32, device=self.device)
        else:
            self._check_out(out, steps)
        check(self.lib.lac_decode_logits_steps(self.ctx, C.c_void_p(logits.data_ptr()), typ, ss, bs, steps,
                                               C.c_void_p(out.data_ptr()), self._stream))
        return out

    def _logits_step_args(self, logits):
        typ, _, bs, steps, logits = self._logits_args(logits)
        if steps != 1:
            raise ValueError(f"one position: logits must be [{self.streams}, {self.vocab}]")
        return typ, bs, logits

    def decode_logits_step(self, logits, out=None):
        """One position of a serving loop: ``logits`` [streams, V] (or [1, streams, V]) ->
        int32 [1, streams], what :meth:`decode_logits` returns for one step -- in one launch
        where the job fits (:meth:`set_q1_step`; lac.h lac_decode_logits_step)."""
        torch = _torch()
        typ, bs, logits = self._logits_step_args(logits)
        if out is None:
            out = torch.empty((1, self.streams), dtype=torch.int32, device=self.device)
        else:
            self._check_out(out, 1)
        check(self.lib.lac_decode_logits_step(self.ctx, C.c_void_p(logits.data_ptr()), typ, bs,
                                              C.c_void_p(out.data_ptr()), self._stream))
        return out

    def encode_logits_step(self, logits, sym, trace=None):
        """One position of a serving loop: :meth:`encode_logits` of one step (``sym``
        [streams] or [1, streams]) -- in one launch where the job fits (:meth:`set_q1_step`)."""
        args = self._logits_encode_args(logits, sym, trace)
        if args[6] != 1:
            raise ValueError(f"one position: sym must be [{self.streams}]")
        check(self.lib.lac_encode_logits_step(*args[:3], args[4], args[5], args[7], args[8]))

    def set_q1_step(self, mode):
        """How the one-position logits calls run (include/lac.h LAC_OPT_Q1_STEP; identical
        results): "auto" (0) the fused one-launch step where it holds the job, "fused" (1)
        always -- a job it cannot hold raises LacError (LAC_E_ARG) from the step call --,
        "split" (2) the two launches of a one-step :meth:`decode_logits` / :meth:`encode_logits`."""
        v = _lib.Q1_STEP_MODES.get(mode, mode)
        check(self.lib.lac_set_option(self.ctx, _lib.LAC_OPT_Q1_STEP, int(v)))

    def quantize_logits(self, logits):
        """The q1 tables themselves: int32 tensor (uint32 bit patterns) [steps, streams, V]."""
        torch = _torch()
        typ, ss, bs, steps, logits = self._logits_args(logits)
        out = torch.empty((steps, self.streams, self.vocab), dtype=torch.int32, device=self.device)
        check(self.lib.lac_quantize_logits(self.ctx, C.c_void_p(logits.data_ptr()), typ, ss, bs, steps,
                                           C.c_void_p(out.data_ptr()), self._stream))
        return out

    # ------------------------------------------------------------ top-k rows from logits
    def topk_logits(self, logits, k, weight_bits=24, K=None, out=None):
        """The sparse rows of logits in one launch (include/lac.h lac_topk_logits): per row the k
        heaviest q1 entries -- weights ``TAB[544 - level]``, the lower symbol first among equal
        weights -- in ascending symbol order with ``wt = g >> (24 - weight_bits)``, then pads
        (idx -1, wt 0) up to ``K`` slots (default: k rounded up to a multiple of 4).  ``logits``
        [steps, streams or 1, V] or [streams or 1, V], bf16 / f32, laid out as the logits path takes
        them.  -> (idx int32, wt int32 bit patterns of uint32), both [steps, streams, K]: what
        :meth:`encode_sparse` / :meth:`decode_sparse` take without conversion.  ``out``: such a
        pair to write into.  Touches no stream state; integer-exact, so both sides of a codec get
        identical rows from identical logits."""
        torch = _torch()
        typ, ss, bs, steps, logits = self._logits_args(logits)
        k = int(k)
        K = (k + 3) // 4 * 4 if K is None else int(K)
        shape = (steps, self.streams, K)
        if out is None:
            idx = torch.empty(shape, dtype=torch.int32, device=self.device)
            wt = torch.empty(shape, dtype=torch.int32, device=self.device)
        else:
            idx, wt = out
            for t in (idx, wt):
                if (not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != self.device
                        or tuple(t.shape) != shape or not t.is_contiguous()):
                    raise ValueError(f"out must be two contiguous int32 tensors {list(shape)} on the coder's device")
        self._keep = (logits, idx, wt)
        check(self.lib.lac_topk_logits(self.ctx, C.c_void_p(logits.data_ptr()), typ, ss, bs, steps, k, int(weight_bits),
                                       K, C.c_void_p(idx.data_ptr()), C.c_void_p(wt.data_ptr()), self._stream))
        return idx, wt

    def set_topk_form(self, form):
        """Which kernel form :meth:`topk_logits` runs (include/lac.h LAC_OPT_TOPK_FORM; identical
        results): "auto" (0) the registers form where a row is at most 16384 16-byte vectors, else
        the streamed form; "registers" (1) always -- a longer row raises LacError (LAC_E_ARG) from
        the call --; "streamed" (2) always."""
        v = _lib.TOPK_FORMS.get(form, form)
        check(self.lib.lac_set_option(self.ctx, _lib.LAC_OPT_TOPK_FORM, int(v)))

    def topk_form(self, dtype):
        """The form (1 registers, 2 streamed) :meth:`topk_logits` runs for logits of ``dtype``."""
        torch = _torch()
        typ = {torch.bfloat16: _lib.LAC_LOGITS_BF16, torch.float32: _lib.LAC_LOGITS_F32}[dtype]
        rc = self.lib.lac_topk_form(self.ctx, typ)
        if rc < 0:
            check(rc)
        return rc

    def set_q1_shape(self, shape: int):
        """Logits row-stats block shape (include/lac.h LAC_OPT_Q1_SHAPE; identical
        results, only speed differs): 0 auto, 1..4 / 6 / 8 / 10 / 14 / 15 / 17 / 18
        forced single-block forms, 19 / 20 / 21 row groups -- a row of > 16384
        vectors in 2..16 segments, one per row slot of 1 / 2 / 4 rows per 16-wave
        block --, 22 one row of <= 26112 vectors in the registers (+ LDS slots) of
        one 8-wave block, 23 groups of such blocks.  The retired shapes 5, 7, 9, 11,
        12, 13 and 16 (never chosen by AUTO) raise LacError (LAC_E_ARG)."""
        check(self.lib.lac_set_option(self.ctx, _lib.LAC_OPT_Q1_SHAPE, int(shape)))

    def q1_k(self):
        """The q1 table scale: max entry 2^k, k = min(24, prec - 1 - ceil(log2 V)) (lac.h lac_q1_k)."""
        return int(self.lib.lac_q1_k(self.prec, self.vocab))


class DrainSink:
    """Streams longer than the coder's capacity: collects what :meth:`BatchCoder.drain` hands
    out.  Owns a device staging tensor [streams, stage_bytes] (one coder capacity wide by
    default, so a drain always fits after a pull) and its ``fill`` counts.

        sink = DrainSink(coder)
        for t in range(T):
            coder.encode(pmf[t:t + 1], sym[t:t + 1])
            if (t + 1) % 64 == 0:
                sink.pull()
        data, nbits = sink.finish()              # what to_bytes() returns for the whole streams
    """

    def __init__(self, coder: BatchCoder, stage_bytes: int | None = None):
        torch = _torch()
        self.coder = coder
        self.stage_bytes = int(stage_bytes if stage_bytes is not None else coder.bits_stride())
        if self.stage_bytes <= 0 or self.stage_bytes % 8:
            raise ValueError("stage_bytes must be a positive multiple of 8")
        self.stage = torch.zeros((coder.streams, self.stage_bytes), dtype=torch.uint8, device=coder.device)
        self.fill = torch.zeros((coder.streams,), dtype=torch.int64, device=coder.device)
        self.parts = [bytearray() for _ in range(coder.streams)]

    def pull(self):
        """Drain, copy the bytes drained to the per-stream host ``bytearray``s (``parts``) and
        empty the staging rows.  Synchronises (the copy to the host)."""
        self.coder.drain(self.stage, self.fill)
        n = self.fill.cpu().numpy()
        if n.any():
            host = self.stage[:, :int(n.max())].cpu().numpy()
            for b in np.flatnonzero(n):
                self.parts[b] += host[b, :int(n[b])].tobytes()
            self.fill.zero_()
        return n

    def finish(self):
        """pull, finish the coder -> (list of per-stream bytes, nbits uint64 [streams]) of the
        whole streams: the drained bytes followed by the finished tail."""
        self.pull()
        self.coder.finish()
        tail, nb = self.coder.to_bytes()
        drained = np.array([len(p) for p in self.parts], dtype=np.uint64)
        return [bytes(p) + t for p, t in zip(self.parts, tail)], nb + 8 * drained


class HostBits:
    """Compressed streams kept in host memory for :meth:`BatchCoder.decode_open_window`, the
    decode mirror of :class:`DrainSink`: the bytes stay on the host (liblac's lac_host_alloc,
    pinned and mapped into the device, [streams, stride] with ``stride`` a multiple of 8) and
    :meth:`BatchCoder.refill` reads only the words that enter a window, so the device holds
    ``streams x window`` whatever the streams' length.  ``data``: per-stream ``bytes``;
    ``nbits``: their bit counts (kept as a device tensor).

        src = HostBits(data, nbits, coder.device)
        coder.decode_open_window(src)
        for t in range(T):
            coder.decode(pmf[t:t + 1], out[t:t + 1])
            if (t + 1) % 64 == 0:
                coder.refill()
        coder.refill()
        src.close()                              # after the last refill has run
    """

    def __init__(self, data, nbits, device):
        torch = _torch()
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.streams = len(data)
        nb = np.ascontiguousarray(np.asarray(nbits).astype(np.int64))
        if nb.shape != (self.streams,) or (nb.size and int(nb.min()) < 0):
            raise ValueError(f"nbits must be {self.streams} counts >= 0")
        for b, d in enumerate(data):
            if 8 * len(d) < int(nb[b]):
                raise ValueError(f"stream {b}: {len(d)} bytes hold fewer than {int(nb[b])} bits")
        self.stride = max(8, (max((len(d) for d in data), default=0) + 7) // 8 * 8)
        self.nbytes = self.stride * max(self.streams, 1)
        h, d = C.c_void_p(), C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.lac_host_alloc(self.nbytes, C.byref(h), C.byref(d)))
        self._h, self.dev_addr = h.value, d.value
        self.array = np.ctypeslib.as_array((C.c_uint8 * self.nbytes).from_address(self._h)) \
            .reshape(max(self.streams, 1), self.stride)
        self.array[...] = 0
        for b, s in enumerate(data):
            self.array[b, :len(s)] = np.frombuffer(s, dtype=np.uint8)
        self.nbits = torch.from_numpy(nb).to(self.device)

    def close(self):
        """Free the host memory: only once every refill that reads it has run."""
        if getattr(self, "_h", None):
            self.array = None
            self.lib.lac_host_free(self._h)
            self._h = self.dev_addr = None

    def __del__(self):
        if sys is None or sys.is_finalizing():                # (the HIP runtime may be torn down already)
            return
        try:
            self.close()
        except Exception:
            pass


def logits_row_multiple(dtype) -> int:
    """Entries per 16-B vector of a logits row (8 bf16, 4 f32): the logits path
    (lac_encode_logits, include/lac.h) needs vocab and row strides to be multiples of it."""
    torch = _torch()
    if dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"logits must be bfloat16 or float32, got {dtype}")
    return 8 if dtype == torch.bfloat16 else 4


def pad_logits(logits):
    """[..., V] logits -> contiguous [..., Vp] with Vp the next multiple of
    logits_row_multiple, the new entries -inf (q1 gives each the minimum weight, 1).
    Encode and decode must both code the padded rows."""
    torch = _torch()
    m = logits_row_multiple(logits.dtype)
    V = logits.shape[-1]
    Vp = (V + m - 1) // m * m
    if Vp != V:
        logits = torch.nn.functional.pad(logits, (0, Vp - V), value=float("-inf"))
    return logits.contiguous()


def digits_of(E: int, k: int):
    """Raw digits of one symbol from its trace entry (first digit 0..3)."""
    if k <= 0:
        return []
    return [E >> (k - 1)] + [(E >> (k - 1 - i)) & 1 for i in range(1, k)]
