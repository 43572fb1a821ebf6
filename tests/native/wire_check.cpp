// Host-side check of lac_amd/csrc/lac_wire.h -- test infrastructure.
//
// C wrappers over the wire arithmetic and wire_unpack_host for ctypes
// (tests/test_wire_host.py).  Plain C++: nothing else is linked.  wc_unpack copies the payload
// into a heap block of exactly src_bytes bytes before it unpacks, so a build of this file
// with a host address sanitizer sees any read past the declared end.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "lac_wire.h"

using namespace lac::wire;

extern "C" {

uint64_t wc_sat_add(uint64_t a, uint64_t b) { return sat_add(a, b); }
uint64_t wc_sat_mul(uint64_t a, uint64_t b) { return sat_mul(a, b); }
uint64_t wc_stream_bytes(uint64_t nbits) { return stream_bytes(nbits); }
int wc_span_fits(uint64_t at, uint64_t len, uint64_t limit) { return span_fits(at, len, limit); }
int wc_stream_fits(uint64_t nbits, uint64_t stride_bytes) { return stream_fits(nbits, stride_bytes); }
int wc_job_status(int fits, int over) { return job_status(fits != 0, over != 0); }
uint64_t wc_read_count(const uint8_t *src, uint64_t job_start, int hdr, const uint64_t *counts, int64_t b) {
    return read_count(src, job_start, hdr, counts, b);
}

// wire_unpack_host over the first src_bytes bytes of `payload`, held in an exactly sized block
// (src_bytes = 0: a 1-byte block, of which nothing may be read).
int wc_unpack(const uint8_t *payload, uint64_t src_bytes, int hdr, const uint64_t *counts, uint64_t base, int64_t jobs,
              int64_t streams, uint8_t *bits, uint64_t stride_bytes, uint64_t job_stride_bytes, uint64_t *nbits,
              uint64_t *ends, int32_t *status) {
    uint8_t *src = payload ? static_cast<uint8_t *>(malloc(src_bytes ? src_bytes : 1)) : nullptr;
    if (src && src_bytes) memcpy(src, payload, src_bytes);
    const int rc = wire_unpack_host(src, src_bytes, hdr, counts, base, jobs, streams, bits, stride_bytes,
                                    job_stride_bytes, nbits, ends, status);
    free(src);
    return rc;
}

}  // extern "C"
