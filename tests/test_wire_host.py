"""Host check of the wire arithmetic (lac_amd/csrc/lac_wire.h): where packed jobs lie, whether
they fit the bytes received, and wire_unpack_host -- lac_unpack_jobs in plain loops, the rules
the kernel shares -- against the torch reference lac_amd.dist.unpack_bitstreams.

Compiles tests/native/wire_check.cpp (plain C++ over the header, nothing else linked); no GPU
needed.  The checker holds each payload in a heap block of exactly the declared size.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import REPO
from lac_amd import dist as ldist

SO = os.path.join(REPO, "tests", "native", "libwirecheck.so")
SRC = os.path.join(REPO, "tests", "native", "wire_check.cpp")

LAC_OK, LAC_E_ARG, LAC_E_CAPACITY = 0, -1, -7
U64MAX = (1 << 64) - 1
EDGES = (0, 1, 7, 8, 9, 63, 64, 65)                            # plus the slot's exact capacity
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def wc():
    hdr = os.path.join(REPO, "lac_amd", "csrc", "lac_wire.h")
    deps = [SRC, hdr, os.path.join(REPO, "include", "lac.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(REPO, "lac_amd", "csrc"),
                        "-I", os.path.join(REPO, "include"), SRC, "-o", SO], check=True)
    lib = C.CDLL(SO)
    u64, vp = C.c_uint64, C.c_void_p
    for name, args in (("wc_sat_add", [u64, u64]), ("wc_sat_mul", [u64, u64]), ("wc_stream_bytes", [u64])):
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, u64
    lib.wc_span_fits.argtypes = [u64, u64, u64]
    lib.wc_stream_fits.argtypes = [u64, u64]
    lib.wc_job_status.argtypes = [C.c_int, C.c_int]
    lib.wc_read_count.argtypes, lib.wc_read_count.restype = [vp, u64, C.c_int, vp, C.c_int64], u64
    lib.wc_unpack.argtypes = [vp, u64, C.c_int, vp, u64, C.c_int64, C.c_int64, vp, u64, u64, vp, vp, vp]
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def unpack(wc, payload, src_bytes, hdr, jobs, streams, stride, counts=None, base=0, gap=0):
    """wire_unpack_host into a sentinel-filled destination with `gap` bytes between the jobs'
    regions -> (rc, bits [jobs, streams, stride], nbits, ends, status, untouched)."""
    job_stride = streams * stride + gap
    dst = np.full(16 + jobs * job_stride + 16, SENTINEL, dtype=np.uint8)
    assert dst.ctypes.data % 8 == 0
    nbits = np.full(jobs * streams, 0x5A5A, dtype=np.uint64)
    ends = np.full(jobs, 0x5A5A, dtype=np.uint64)
    status = np.full(jobs, 0x5A5A, dtype=np.int32)
    payload = np.ascontiguousarray(payload, dtype=np.uint8)
    cnt = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint64)
    rc = wc.wc_unpack(_ptr(payload), src_bytes, hdr, _ptr(cnt), base, jobs, streams, _ptr(dst[16:]), stride,
                      job_stride, _ptr(nbits), _ptr(ends), _ptr(status))
    body = dst[16:16 + jobs * job_stride].reshape(jobs, job_stride)
    untouched = bool((dst[:16] == SENTINEL).all() and (dst[16 + jobs * job_stride:] == SENTINEL).all()
                     and (body[:, streams * stride:] == SENTINEL).all())
    bits = body[:, :streams * stride].reshape(jobs, streams, stride).copy()
    return rc, bits, nbits.reshape(jobs, streams), ends, status, untouched


def make_job(rng, counts, stride, hdr):
    """One packed job by the CPU-tensor pack_bitstreams -> (payload bytes, reference bits, nbits)."""
    streams = len(counts)
    bits = torch.from_numpy(rng.integers(0, 256, (streams, stride), dtype=np.uint8))
    nb = torch.tensor(counts, dtype=torch.int64)
    payload, L = ldist.pack_bitstreams(bits, nb, hdr)
    payload = payload[:int(L)].clone()
    ref_bits, ref_nb = ldist.unpack_bitstreams(payload, streams, stride, hdr)
    assert torch.equal(ref_nb, nb)
    return payload.numpy(), ref_bits.numpy(), ref_nb.numpy().astype(np.uint64)


def job_counts(streams, stride, seed):
    """Three jobs of different counts covering every edge value and the slot's capacity."""
    edges = EDGES + (8 * stride,)
    if streams == 1:
        return [[[edges[(i + j) % len(edges)]] for j in range(3)] for i in range(len(edges))]
    rng = np.random.default_rng(seed)
    jobs = []
    for j in range(3):
        c = [edges[(b + 3 * j) % len(edges)] for b in range(streams)]
        for b in range(len(edges), streams, 2):                 # and random ones between them
            c[b] = int(rng.integers(0, 8 * stride + 1))
        jobs.append(c)
    return [jobs]


# ------------------------------------------------------------------ the arithmetic
def test_saturating_arithmetic(wc):
    assert wc.wc_sat_add(U64MAX - 1, 1) == U64MAX and wc.wc_sat_add(U64MAX - 1, 2) == U64MAX
    assert wc.wc_sat_add(U64MAX, U64MAX) == U64MAX and wc.wc_sat_add(3, 4) == 7
    assert wc.wc_sat_mul(1 << 32, 1 << 32) == U64MAX and wc.wc_sat_mul((1 << 32) - 1, 1 << 32) == U64MAX - (1 << 32) + 1
    assert wc.wc_sat_mul(0, U64MAX) == 0 and wc.wc_sat_mul(4, U64MAX // 4 + 1) == U64MAX
    assert [wc.wc_stream_bytes(n) for n in (0, 1, 7, 8, 9, 63, 64, 65)] == [0, 1, 1, 1, 2, 8, 8, 9]
    assert wc.wc_stream_bytes(U64MAX) == 1 << 61 and wc.wc_stream_bytes(U64MAX - 7) == (1 << 61) - 1
    assert wc.wc_span_fits(0, 0, 0) and wc.wc_span_fits(5, 3, 8) and not wc.wc_span_fits(5, 4, 8)
    assert not wc.wc_span_fits(9, 0, 8) and not wc.wc_span_fits(U64MAX, 2, 100) and not wc.wc_span_fits(2, U64MAX, 100)
    assert wc.wc_stream_fits(64, 8) and not wc.wc_stream_fits(65, 8) and wc.wc_stream_fits(0, 0)
    assert not wc.wc_stream_fits(U64MAX, 1 << 60) and wc.wc_stream_fits(U64MAX, 1 << 61)
    assert [wc.wc_job_status(f, o) for f, o in ((1, 0), (1, 1), (0, 0), (0, 1))] == [
        LAC_OK, LAC_E_CAPACITY, LAC_E_ARG, LAC_E_ARG]


def test_read_count(wc):
    src = np.array([0xEE, 0x34, 0x12, 0xFF, 0xFE, 0x78, 0x56, 0x34, 0x12], dtype=np.uint8)
    assert wc.wc_read_count(_ptr(src), 1, 2, None, 0) == 0x1234 and wc.wc_read_count(_ptr(src), 1, 2, None, 1) == 0xFEFF
    assert wc.wc_read_count(_ptr(src), 1, 4, None, 1) == 0x12345678
    cnt = np.array([5, U64MAX], dtype=np.uint64)
    assert wc.wc_read_count(None, 0, 0, _ptr(cnt), 1) == U64MAX


# ------------------------------------------------------------------ against the torch reference
@pytest.mark.parametrize("hdr", [2, 4])
@pytest.mark.parametrize("stride", [16, 72])
@pytest.mark.parametrize("streams", [1, 3, 70])
def test_host_unpack_equals_torch_reference(wc, streams, stride, hdr):
    rng = np.random.default_rng(1000 * streams + 10 * stride + hdr)
    for jobs in job_counts(streams, stride, streams + stride):
        made = [make_job(rng, c, stride, hdr) for c in jobs]
        want_bits = np.stack([m[1] for m in made])
        want_nb = np.stack([m[2] for m in made])
        want_ends = np.cumsum([len(m[0]) for m in made]).astype(np.uint64)
        for base in (0, 5):
            payload = np.concatenate([np.full(base, 0xEE, np.uint8)] + [m[0] for m in made])
            rc, bits, nb, ends, status, untouched = unpack(wc, payload, len(payload), hdr, 3, streams, stride,
                                                           base=base, gap=24)
            assert rc == LAC_OK and untouched
            assert np.array_equal(bits, want_bits) and np.array_equal(nb, want_nb)
            assert np.array_equal(ends, want_ends + base) and (status == LAC_OK).all()
        # the same streams by plain concatenation, the counts beside them: hdr_bytes == 0
        body = np.concatenate([m[0][streams * hdr:] for m in made])
        want_ends0 = np.cumsum([len(m[0]) - streams * hdr for m in made]).astype(np.uint64)
        rc, bits, nb, ends, status, untouched = unpack(wc, body if len(body) else np.zeros(1, np.uint8), len(body), 0,
                                                       3, streams, stride, counts=want_nb.reshape(-1), gap=8)
        assert rc == LAC_OK and untouched
        assert np.array_equal(bits, want_bits) and np.array_equal(nb, want_nb)
        assert np.array_equal(ends, want_ends0) and (status == LAC_OK).all()


# ------------------------------------------------------------------ verdicts
@pytest.mark.parametrize("hdr", [2, 4])
def test_truncation_at_every_byte(wc, hdr):
    """A 3-stream, 2-job payload cut at every byte: jobs that still fit are intact, the first
    that does not and every later one fail, and nothing past the cut is read (the checker's
    block ends there)."""
    rng = np.random.default_rng(7)
    stride = 16
    made = [make_job(rng, c, stride, hdr) for c in ([65, 9, 128], [1, 64, 17])]
    payload = np.concatenate([m[0] for m in made])
    job_end = np.cumsum([len(m[0]) for m in made])
    for cut in range(len(payload) + 1):
        rc, bits, nb, ends, status, untouched = unpack(wc, payload, cut, hdr, 2, 3, stride, gap=8)
        assert rc == LAC_OK and untouched
        good = int(np.searchsorted(job_end, cut, side="right"))     # jobs wholly inside the cut
        for j in range(2):
            if j < good:
                assert status[j] == LAC_OK and ends[j] == job_end[j], (cut, j)
                assert np.array_equal(bits[j], made[j][1]) and np.array_equal(nb[j], made[j][2]), (cut, j)
            else:
                assert status[j] == LAC_E_ARG and ends[j] == (job_end[good - 1] if good else 0), (cut, j)
                assert (nb[j] == U64MAX).all() and not bits[j].any(), (cut, j)


def test_stream_longer_than_its_slot(wc):
    rng = np.random.default_rng(8)
    payload, _, _ = make_job(rng, [64, 65, 9], 16, 2)             # packed from 16-byte rows ...
    want, want_nb = ldist.unpack_bitstreams(torch.from_numpy(payload), 3, 8, 2)
    rc, bits, nb, ends, status, untouched = unpack(wc, payload, len(payload), 2, 1, 3, 8, gap=8)   # ... into 8-byte slots
    assert rc == LAC_OK and untouched
    assert status[0] == LAC_E_CAPACITY and ends[0] == len(payload)
    assert nb[0].tolist() == [64, 65, 9] == want_nb.tolist()
    assert not bits[0, 1].any()
    assert np.array_equal(bits[0, 0], want[0].numpy()) and np.array_equal(bits[0, 2], want[2].numpy())


def test_hostile_counts_saturate(wc):
    # eight streams of 2^61 bytes sum to 2^64: a wrapping sum would make this job 2 bytes long
    counts = [U64MAX] * 8 + [16]
    rc, bits, nb, ends, status, untouched = unpack(wc, np.array([1, 2], np.uint8), 2, 0, 1, 9, 8, counts=counts)
    assert rc == LAC_OK and untouched
    assert status[0] == LAC_E_ARG and ends[0] == 0 and (nb == U64MAX).all() and not bits.any()
    # a count of nearly 2^64 bits alone, and behind a job that fits
    counts = [16, 8, U64MAX - 6, 8]
    rc, bits, nb, ends, status, untouched = unpack(wc, np.array([1, 2, 3, 4], np.uint8), 4, 0, 2, 2, 8, counts=counts)
    assert rc == LAC_OK and untouched and status.tolist() == [LAC_OK, LAC_E_ARG] and ends.tolist() == [3, 3]
    assert bits[0, 0, :2].tolist() == [1, 2] and bits[0, 1, 0] == 3 and nb[0].tolist() == [16, 8]
    assert (nb[1] == U64MAX).all() and not bits[1].any()
    # a start near 2^64: start + header must not wrap into the payload
    rc, bits, nb, ends, status, untouched = unpack(wc, np.zeros(64, np.uint8), 64, 2, 1, 3, 8, base=U64MAX - 3)
    assert rc == LAC_OK and untouched and status[0] == LAC_E_ARG and ends[0] == U64MAX - 3 and (nb == U64MAX).all()


def test_refusals(wc):
    p = np.zeros(64, np.uint8)
    ok = dict(payload=p, src_bytes=64, hdr=2, jobs=1, streams=3, stride=8)
    assert unpack(wc, **ok)[0] == LAC_OK
    assert unpack(wc, **{**ok, "hdr": 3})[0] == LAC_E_ARG
    assert unpack(wc, **{**ok, "hdr": 0})[0] == LAC_E_ARG          # no counts
    assert unpack(wc, **{**ok, "stride": 12})[0] == LAC_E_ARG
    assert unpack(wc, **{**ok, "gap": 4})[0] == LAC_E_ARG
