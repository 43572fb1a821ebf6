"""CPU-side checks of lac_unpack_jobs / lac_decode_open_packed at the C-ABI boundary: every
refusal include/lac.h lists is returned before any HIP call, so it holds without a GPU."""
import ctypes as C

import pytest

from lac_amd import _lib

SRC, BITS, NBITS, COUNTS = 0x10000, 0x20000, 0x30000, 0x40000      # never dereferenced: refused first


@pytest.fixture(scope="module")
def lib():
    from lac_amd import build
    build.build(verbose=False)
    return _lib.load()


def call(lib, **kw):
    a = dict(device=0, src=SRC, src_bytes=64, hdr=2, counts=None, base=None, jobs=1, streams=3, bits=BITS, stride=8,
             job_stride=24, nbits=NBITS, ends=None, status=None, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return lib.lac_unpack_jobs(a["device"], a["src"], a["src_bytes"], a["hdr"], a["counts"], a["base"], a["jobs"],
                               a["streams"], a["bits"], a["stride"], a["job_stride"], a["nbits"], a["ends"],
                               a["status"], a["stream"])


@pytest.mark.parametrize("kw", [
    dict(hdr=1), dict(hdr=3), dict(hdr=8), dict(hdr=-2),
    dict(hdr=0),                                               # no counts_dev
    dict(jobs=-1), dict(streams=0), dict(streams=-5),
    dict(bits=BITS + 4), dict(stride=12), dict(job_stride=28),
    dict(jobs=2, job_stride=16),                               # < streams * stride_bytes with several jobs
    dict(src=None), dict(bits=None), dict(nbits=None),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_unpack_jobs_refusals(lib, kw):
    assert call(lib, **kw) == _lib.LAC_E_ARG
    assert lib.lac_last_error()


def test_unpack_jobs_zero_jobs_is_ok_without_a_launch(lib):
    assert call(lib, jobs=0) == _lib.LAC_OK
    assert call(lib, jobs=0, hdr=0, counts=COUNTS) == _lib.LAC_OK
    assert call(lib, jobs=0, hdr=5) == _lib.LAC_E_ARG          # the refusals come first


def test_decode_open_packed_null_context(lib):
    assert lib.lac_decode_open_packed(None, SRC, 64, 2, None, None, None, None) == _lib.LAC_E_ARG
