"""lac_unpack_jobs / lac_decode_open_packed on the GPU: the unpack kernel against the torch
reference lac_amd.dist.unpack_bitstreams (byte for byte), its bounds on both sides, chained
and malformed payloads, and wire -> unpack -> decode through BatchCoder and the container."""
import ctypes as C

import numpy as np
import pytest
import torch

from lac_amd import _lib, container, synth
from lac_amd import dist as ldist
from lac_amd.batch import BatchCoder
from lac_amd.coder import _DEC_STATE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EDGES = (0, 1, 7, 8, 9, 63, 64, 65)


def counts_for(streams, stride, seed, fill="mixed"):
    """Bit counts for one job: every edge value the slot holds, its exact capacity, random ones."""
    cap = 8 * stride
    if fill == "zero":
        return np.zeros(streams, dtype=np.int64)
    if fill == "cap":
        return np.full(streams, cap, dtype=np.int64)
    rng = np.random.default_rng(seed)
    c = rng.integers(0, cap + 1, streams, dtype=np.int64)
    edges = [e for e in EDGES if e <= cap] + [cap]
    fixed = {255: cap, 256: 1, streams - 1: cap} if streams > 300 else {}   # both sides of a workgroup tile, the last stream
    for b, v in fixed.items():
        c[b] = v
    pos = [b for b in rng.permutation(streams) if b not in fixed][:len(edges)]
    c[pos] = edges[:len(pos)]
    return c


def make_job(streams, stride, hdr, seed, fill="mixed", counts=None):
    """-> (payload [L] uint8 on the device, reference bits, reference nbits) by the torch pack / unpack."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    bits = torch.randint(0, 256, (streams, stride), generator=g, device=DEV, dtype=torch.uint8)
    nb = torch.from_numpy(counts_for(streams, stride, seed, fill) if counts is None else np.asarray(counts)).to(DEV)
    payload, L = ldist.pack_bitstreams(bits, nb, hdr)
    payload = payload[:int(L)].clone()
    ref_bits, ref_nb = ldist.unpack_bitstreams(payload, streams, stride, hdr)
    assert torch.equal(ref_nb, nb)
    return payload, ref_bits, ref_nb


def raw_unpack(src, src_bytes, hdr, jobs, streams, dst, stride, job_stride, counts=None, base=None):
    """lac_unpack_jobs into the caller's destination -> (rc, nbits [jobs, streams], ends, status)."""
    lib = _lib.load()
    nbits = torch.full((jobs, streams), 0x5A5A, dtype=torch.int64, device=DEV)
    ends = torch.full((jobs,), 0x5A5A, dtype=torch.int64, device=DEV)
    status = torch.full((jobs,), 0x5A5A, dtype=torch.int32, device=DEV)
    rc = lib.lac_unpack_jobs(0, C.c_void_p(src.data_ptr()), src_bytes, hdr,
                             None if counts is None else C.c_void_p(counts.data_ptr()),
                             None if base is None else C.c_void_p(base.data_ptr()), jobs, streams,
                             C.c_void_p(dst.data_ptr()), stride, job_stride, C.c_void_p(nbits.data_ptr()),
                             C.c_void_p(ends.data_ptr()), C.c_void_p(status.data_ptr()),
                             C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    return rc, nbits, ends, status


# ------------------------------------------------------------------ kernel == torch reference
@pytest.mark.parametrize("hdr", [2, 4])
@pytest.mark.parametrize("stride", [8, 64, 200])
@pytest.mark.parametrize("streams", [1, 3, 1025, 2500])
def test_unpack_equals_torch_reference(streams, stride, hdr):
    payload, ref_bits, ref_nb = make_job(streams, stride, hdr, 100 * streams + stride + hdr)
    bits, nbits, ends, status = ldist.unpack_jobs(payload, 1, streams, stride, hdr)
    assert bits.shape == (1, streams, stride) and nbits.dtype == torch.int64
    assert torch.equal(bits[0], ref_bits) and torch.equal(nbits[0], ref_nb)
    assert ends.tolist() == [payload.numel()] and status.tolist() == [0]


@pytest.mark.parametrize("fill", ["zero", "cap"])
@pytest.mark.parametrize("streams,stride,hdr", [(3, 8, 2), (1025, 64, 4), (2500, 200, 2)])
def test_unpack_all_empty_and_all_full(streams, stride, hdr, fill):
    payload, ref_bits, ref_nb = make_job(streams, stride, hdr, 5, fill)
    assert payload.numel() == streams * hdr + (streams * stride if fill == "cap" else 0)
    bits, nbits, ends, status = ldist.unpack_jobs(payload, 1, streams, stride, hdr)
    assert torch.equal(bits[0], ref_bits) and torch.equal(nbits[0], ref_nb)
    assert ends.tolist() == [payload.numel()] and status.tolist() == [0]


def test_unpack_long_slots():
    """Slots of 256 words and more are copied stream by stream, the longest split over workgroups."""
    for streams, stride, seed in ((3, 2048, 1), (2, 2056, 2), (1, 1 << 17, 3), (2, 24 * 2048 + 8, 4)):
        payload, ref_bits, ref_nb = make_job(streams, stride, 4, seed,
                                             counts=[8 * stride, 8 * stride - 67, 9][:streams])
        bits, nbits, ends, status = ldist.unpack_jobs(payload, 1, streams, stride, 4)
        assert torch.equal(bits[0], ref_bits) and torch.equal(nbits[0], ref_nb), (streams, stride)
        assert ends.tolist() == [payload.numel()] and status.tolist() == [0]


# ------------------------------------------------------------------ alignment and bounds
@pytest.mark.parametrize("via_base", [False, True])
@pytest.mark.parametrize("off", [0, 1, 3, 13])
def test_unpack_alignment_and_sentinels(off, via_base):
    streams, stride, hdr, gap = 259, 24, 2, 40
    made = [make_job(streams, stride, hdr, 40 + j) for j in range(2)]
    L = sum(m[0].numel() for m in made)
    big = torch.full((off + L + 64,), 0xAA, dtype=torch.uint8, device=DEV)
    big[off:off + L] = torch.cat([m[0] for m in made])
    job_stride = streams * stride + gap
    dst = torch.full((64 + 2 * job_stride + 64,), 0x5C, dtype=torch.uint8, device=DEV)
    assert dst.data_ptr() % 8 == 0
    if via_base:
        base = torch.tensor([off], dtype=torch.int64, device=DEV)
        rc, nbits, ends, status = raw_unpack(big, off + L, hdr, 2, streams, dst[64:], stride, job_stride, base=base)
    else:
        rc, nbits, ends, status = raw_unpack(big[off:], L, hdr, 2, streams, dst[64:], stride, job_stride)
    assert rc == 0 and status.tolist() == [0, 0]
    start = off if via_base else 0
    assert ends.tolist() == [start + made[0][0].numel(), start + L]
    body = dst[64:64 + 2 * job_stride].reshape(2, job_stride)
    for j in range(2):
        assert torch.equal(body[j, :streams * stride].reshape(streams, stride), made[j][1])
        assert torch.equal(nbits[j], made[j][2])
    assert bool((body[:, streams * stride:] == 0x5C).all())     # between the jobs' slots
    assert bool((dst[:64] == 0x5C).all()) and bool((dst[64 + 2 * job_stride:] == 0x5C).all())
    assert bool((big[:off] == 0xAA).all()) and bool((big[off + L:] == 0xAA).all())


# ------------------------------------------------------------------ job chain
@pytest.mark.parametrize("streams", [5, 1030])
def test_unpack_job_chain_and_headerless(streams):
    stride, hdr = 64, 4
    made = [make_job(streams, stride, hdr, 70 + j) for j in range(3)]
    payload = torch.cat([m[0] for m in made])
    bits, nbits, ends, status = ldist.unpack_jobs(payload, 3, streams, stride, hdr)
    assert status.tolist() == [0, 0, 0]
    assert ends.tolist() == np.cumsum([m[0].numel() for m in made]).tolist()
    base = None
    for j in range(3):                                          # one job per call, chained through ends
        b1, n1, e1, s1 = ldist.unpack_jobs(payload, 1, streams, stride, hdr, base=base)
        assert torch.equal(b1[0], bits[j]) and torch.equal(n1[0], nbits[j]) and torch.equal(e1[0], ends[j])
        assert torch.equal(b1[0], made[j][1]) and s1.tolist() == [0]
        base = e1
    # the same streams with no headers, the counts beside them
    body = torch.cat([m[0][streams * hdr:] for m in made])
    counts = torch.cat([m[2] for m in made])
    b0, n0, e0, s0 = ldist.unpack_jobs(body, 3, streams, stride, 0, counts=counts)
    assert torch.equal(b0, bits) and torch.equal(n0, nbits) and s0.tolist() == [0, 0, 0]
    assert e0.tolist() == np.cumsum([m[0].numel() - streams * hdr for m in made]).tolist()


# ------------------------------------------------------------------ malformed payloads
@pytest.mark.parametrize("where", ["header", "payload"])
def test_unpack_truncated_job(where):
    """The whole payload is in memory; only the declared size is short."""
    streams, stride, hdr = 300, 16, 2
    made = [make_job(streams, stride, hdr, 90 + j) for j in range(3)]
    payload = torch.cat([m[0] for m in made])
    end0, end1 = made[0][0].numel(), made[0][0].numel() + made[1][0].numel()
    cut = end0 + 7 if where == "header" else end1 - 1
    bits, nbits, ends, status = ldist.unpack_jobs(payload[:cut], 3, streams, stride, hdr)
    assert status.tolist() == [0, _lib.LAC_E_ARG, _lib.LAC_E_ARG] and ends.tolist() == [end0, end0, end0]
    assert torch.equal(bits[0], made[0][1]) and torch.equal(nbits[0], made[0][2])
    assert bool((nbits[1:] == -1).all()) and not bool(bits[1:].any())     # -1: UINT64_MAX in the int64 view


def test_unpack_stream_longer_than_its_slot():
    streams, hdr = 300, 2
    counts = counts_for(streams, 8, 11)
    counts[257] = 65
    payload, _, _ = make_job(streams, 16, hdr, 11, counts=counts)     # packed from 16-byte rows
    want, want_nb = ldist.unpack_bitstreams(payload, streams, 8, hdr)
    bits, nbits, ends, status = ldist.unpack_jobs(payload, 1, streams, 8, hdr)
    assert status.tolist() == [_lib.LAC_E_CAPACITY] and ends.tolist() == [payload.numel()]
    assert torch.equal(nbits[0], want_nb) and int(nbits[0, 257]) == 65
    assert not bool(bits[0, 257].any())
    keep = torch.arange(streams, device=DEV) != 257
    assert torch.equal(bits[0][keep], want[keep])


# ------------------------------------------------------------------ through the coder
def int_tables(steps, streams, V, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    pmf = torch.randint(1, 1 << 20, (steps, streams, V), generator=g, device=DEV, dtype=torch.int32)
    sym = torch.randint(0, V, (steps, streams), generator=g, device=DEV, dtype=torch.int32)
    return pmf, sym


def dec_state(c):
    st = np.zeros(c.streams, dtype=_DEC_STATE)
    _lib.check(c.lib.lac_decode_get_state(c.ctx, st.ctypes.data_as(C.c_void_p), c._stream))
    return st


def roundtrip(c, tables, sym, logits=False, lengths=None, stop=False):
    """encode -> pack -> decode_open_packed -> decode on one side stream with no sync between,
    the payload overwritten before the decode runs; -> (decoded, the classic decode_open's
    result, statuses of both)."""
    steps, B = sym.shape
    hdr = 2
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        if lengths is not None:
            c.set_stream_lengths(lengths)
        c.set_decode_stop(stop)
        (c.encode_logits_job if logits else c.encode_job)(tables, sym)
        bt, nt = c.bits_tensor(), c.nbits_tensor()
        payload = torch.empty(B * (hdr + c.bits_stride()), dtype=torch.uint8, device=DEV)
        length = torch.zeros(1, dtype=torch.int64, device=DEV)
        c.pack_bits(payload, hdr, length)
        saved = payload.clone()
        c.decode_open_packed(payload, hdr)
        payload.fill_(0xFF)                                       # nothing is borrowed
        got = (c.decode_logits if logits else c.decode)(tables)
    side.synchronize()
    _, got_err, _ = c.status()
    # the registers right after opening, against decode_open on the same output
    with torch.cuda.stream(side):
        c.decode_open_packed(saved, hdr)
        st_packed = dec_state(c)
        c.decode_open(bt, nt)
        st_classic = dec_state(c)
        want = (c.decode_logits if logits else c.decode)(tables)
    side.synchronize()
    _, want_err, _ = c.status()
    for f in _DEC_STATE.names:
        assert np.array_equal(st_packed[f], st_classic[f]), f
    assert int(length) == B * hdr + int(((nt + 7) // 8).sum())
    return got, want, got_err, want_err


@pytest.mark.parametrize("streams", [5, 1030])
def test_coder_roundtrip_from_packed(streams):
    c = BatchCoder(64, streams, prec=32, capacity_bits=20 * 32 + 64, device=DEV)
    pmf, sym = int_tables(20, streams, 64, streams)
    got, want, ge, we = roundtrip(c, pmf, sym)
    assert torch.equal(got, sym) and torch.equal(want, sym) and not ge.any() and not we.any()
    c.close()


@pytest.mark.parametrize("streams", [5, 1030])
def test_coder_roundtrip_ragged(streams):
    c = BatchCoder(64, streams, prec=32, capacity_bits=20 * 32 + 64, device=DEV)
    pmf, sym = int_tables(20, streams, 64, streams + 1)
    lengths = np.array([(0, 20, 7, 13, 1)[b % 5] for b in range(streams)], dtype=np.int64)
    got, want, ge, we = roundtrip(c, pmf, sym, lengths=lengths)
    live = torch.arange(20, device=DEV)[:, None] < torch.from_numpy(lengths).to(DEV)[None, :]
    masked = torch.where(live, sym, torch.full_like(sym, -1))
    assert torch.equal(got, masked) and torch.equal(want, masked) and not ge.any() and not we.any()
    c.close()


@pytest.mark.parametrize("streams", [5, 1030])
def test_coder_roundtrip_decode_stop(streams):
    c = BatchCoder(64, streams, prec=32, capacity_bits=20 * 32 + 64, device=DEV)
    pmf, sym = int_tables(20, streams, 64, streams + 2)
    got, want, ge, we = roundtrip(c, pmf, sym, stop=True)
    assert torch.equal(got, want) and np.array_equal(ge, we)
    assert set(np.unique(ge).tolist()) <= {0, _lib.LAC_E_UNDETERMINED}
    known = got >= 0                                              # every symbol it emitted is the coded one
    assert torch.equal(got[known], sym[known]) and bool(known.any())
    c.close()


def test_coder_roundtrip_logits():
    c = BatchCoder(64, 3, prec=32, capacity_bits=20 * 32 + 64, device=DEV)
    logits, sym = synth.logits_batch(20, 3, 64, seed=5, device=DEV, dtype=torch.bfloat16, quantise=c.quantize_logits)
    got, want, ge, we = roundtrip(c, logits, sym, logits=True)
    assert torch.equal(got, sym) and torch.equal(want, sym) and not ge.any() and not we.any()
    c.close()


# ------------------------------------------------------------------ sticky errors
def test_truncated_payload_fails_every_stream():
    c = BatchCoder(64, 5, prec=32, capacity_bits=20 * 32 + 64, device=DEV)
    pmf, sym = int_tables(20, 5, 64, 21)
    c.encode_job(pmf, sym)
    payload = torch.empty(5 * (2 + c.bits_stride()), dtype=torch.uint8, device=DEV)
    length = torch.zeros(1, dtype=torch.int64, device=DEV)
    c.pack_bits(payload, 2, length)
    L = int(length)
    end = torch.full((1,), 77, dtype=torch.int64, device=DEV)
    c.decode_open_packed(payload[:L - 1], 2, end=end)
    rc, err, _ = c.status()
    assert rc == _lib.LAC_E_ARG and (err == _lib.LAC_E_ARG).all() and int(end) == 0
    c.decode_open_packed(payload[:L], 2, end=end)                 # the whole job opens
    assert torch.equal(c.decode(pmf), sym) and c.status()[0] == 0 and int(end) == L
    c.close()


def test_stream_beyond_the_decoders_capacity_fails_alone():
    steps, B = 40, 5
    lengths = np.array([2, 2, steps, 2, 0], dtype=np.int64)
    pmf, sym = int_tables(steps, B, 64, 22)
    enc = BatchCoder(64, B, prec=32, capacity_bits=steps * 32 + 64, device=DEV)
    enc.set_stream_lengths(lengths)
    enc.encode_job(pmf, sym)
    payload = torch.empty(B * (2 + enc.bits_stride()), dtype=torch.uint8, device=DEV)
    length = torch.zeros(1, dtype=torch.int64, device=DEV)
    enc.pack_bits(payload, 2, length)
    dec = BatchCoder(64, B, prec=32, capacity_bits=64, device=DEV)
    cap = 8 * dec.bits_stride()
    nb = enc.lengths()
    assert nb[2] > cap and (np.delete(nb, 2) <= cap).all()        # the case is what it claims to be
    dec.set_stream_lengths(lengths)
    dec.decode_open_packed(payload, 2)
    out = dec.decode(pmf)
    rc, err, _ = dec.status()
    assert rc == _lib.LAC_E_ARG and err.tolist() == [0, 0, _lib.LAC_E_ARG, 0, 0]
    for b in (0, 1, 3):
        assert torch.equal(out[:2, b], sym[:2, b]) and bool((out[2:, b] == -1).all())
    assert bool((out[:, 4] == -1).all())
    enc.close()
    dec.close()


# ------------------------------------------------------------------ container
def test_container_roundtrip_1030_streams_with_empty_ones():
    steps, B = 20, 1030
    pmf, sym = int_tables(steps, B, 64, 23)
    counts = [(steps, 0, 9, steps, 1)[b % 5] for b in range(B)]
    c = BatchCoder(64, B, prec=32, capacity_bits=steps * 32 + 64, device=DEV)
    blob = container.compress_batch(c, pmf, sym, n_symbols=counts)
    c.close()
    out, n = container.decompress_batch(blob, pmf)
    assert n == counts
    live = torch.arange(steps, device=DEV)[:, None] < torch.tensor(counts, device=DEV)[None, :]
    assert torch.equal(out, torch.where(live, sym, torch.full_like(sym, -1)))
