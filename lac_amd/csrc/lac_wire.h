// lac_wire.h -- the arithmetic of the packed wire format (lac_pack_jobs' output, the body of
// a LAC1 container) as plain functions: where a job's header and streams lie, whether they
// fit the bytes received, and what a job or a stream that does not fit gets.  No HIP calls,
// no allocation: k_unpack (lac_encode.hip) places and judges everything through these
// functions, wire_unpack_host below is the same contract in plain loops (the CPU oracle),
// and tests/test_wire_host.py checks it without a GPU.
//
// A job is `streams` bit counts of `hdr` = 2 or 4 bytes each (little endian), then stream
// b's ceil(nbits_b / 8) bytes for b = 0, 1, ...; hdr = 0: no header in the payload, the
// counts come from a uint64 array.  The payload is untrusted: every sum saturates at
// UINT64_MAX, so a hostile count cannot wrap a fit test, and nothing is read before the
// test that covers it has passed.
#pragma once
#include <stdint.h>
#include <string.h>

#include "lac.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LAC_WIRE_HD __host__ __device__
#else
#define LAC_WIRE_HD
#endif

namespace lac {
namespace wire {

constexpr uint64_t kNone = ~0ull;                 // the bit count of a stream of a job that does not fit

LAC_WIRE_HD inline uint64_t sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }
LAC_WIRE_HD inline uint64_t sat_mul(uint64_t a, uint64_t b) { return a && b > ~0ull / a ? ~0ull : a * b; }

// ceil(nbits / 8) with no nbits + 7 to wrap
LAC_WIRE_HD inline uint64_t stream_bytes(uint64_t nbits) { return (nbits >> 3) + ((nbits & 7) != 0); }
LAC_WIRE_HD inline uint64_t header_bytes(int hdr, int64_t streams) {
    return sat_mul((uint64_t)hdr, (uint64_t)streams);
}

// [at, at + len) lies inside [0, limit)
LAC_WIRE_HD inline bool span_fits(uint64_t at, uint64_t len, uint64_t limit) {
    return at <= limit && len <= limit - at;
}

// Stream b's bit count of the job whose header starts at byte `job_start` of src; `counts` is
// that job's row of the count array (hdr == 0).  Byte loads: src has any alignment.  The
// caller has tested span_fits(job_start, header_bytes(hdr, streams), src_bytes).
LAC_WIRE_HD inline uint64_t read_count(const uint8_t *src, uint64_t job_start, int hdr, const uint64_t *counts,
                                       int64_t b) {
    if (hdr == 0) return counts[b];
    const uint8_t *p = src + job_start + (uint64_t)b * (uint64_t)hdr;
    uint64_t v = (uint64_t)p[0] | (uint64_t)p[1] << 8;         // (straight-line: the loads are independent)
    if (hdr == 4) v |= (uint64_t)p[2] << 16 | (uint64_t)p[3] << 24;
    return v;
}

// Per-stream verdict: the stream fits its slot iff nbits <= 8 * stride_bytes.
LAC_WIRE_HD inline bool stream_fits(uint64_t nbits, uint64_t stride_bytes) {
    return stream_bytes(nbits) <= stride_bytes;
}

// Per-job verdict.  `fits`: header and payload lie inside the bytes received (and so did every
// earlier job of the call); `over`: some stream does not fit its slot.
LAC_WIRE_HD inline int32_t job_status(bool fits, bool over) {
    return !fits ? LAC_E_ARG : over ? LAC_E_CAPACITY : LAC_OK;
}

// One job of the walk over a call's jobs.  start: the job's first byte (for a job after one
// that did not fit: that job's start, the last offset known); fits as in job_status.
struct Walk {
    uint64_t start;
    bool fits;
};
// Before reading the job's counts: does its header fit?
LAC_WIRE_HD inline bool walk_header(Walk &w, int hdr, int64_t streams, uint64_t src_bytes) {
    w.fits = w.fits && span_fits(w.start, header_bytes(hdr, streams), src_bytes);
    return w.fits;
}
// With `payload` = the saturated sum of the job's stream_bytes: does the job fit?
LAC_WIRE_HD inline bool walk_payload(Walk &w, int hdr, int64_t streams, uint64_t payload, uint64_t src_bytes) {
    w.fits = w.fits && span_fits(w.start + header_bytes(hdr, streams), payload, src_bytes);
    return w.fits;
}
// The offset just past a job that fits (no wrap: it is <= src_bytes): the next job's start.
LAC_WIRE_HD inline uint64_t job_end(const Walk &w, int hdr, int64_t streams, uint64_t payload) {
    return w.start + header_bytes(hdr, streams) + payload;
}

// One 8-byte word of a slot: word `wi` of a stream of `n` bytes at byte `off` of src, zero
// past the stream (n = 0: a stream that is not unpacked).  Full words are one 8-byte load of
// exactly the stream's bytes, the last partial word is byte loads: nothing outside
// [off, off + n) is touched.  The word goes out with an aligned 8-byte store; bytes keep
// their memory order on the little-endian hosts and GPUs this runs on.
LAC_WIRE_HD inline uint64_t slot_word(const uint8_t *src, uint64_t off, uint64_t n, uint64_t wi) {
    const uint64_t full = n >> 3;
    uint64_t v = 0;
    if (wi < full) {
        memcpy(&v, src + off + 8 * wi, 8);
    } else if (wi == full) {
        const uint8_t *p = src + off + 8 * wi;
        for (uint64_t k = 0; k < (n & 7); k++) v |= (uint64_t)p[k] << (8 * k);
    }
    return v;
}

// The refusals of lac_unpack_jobs (include/lac.h), checked before anything runs.
inline const char *check_args(const uint8_t *src, int hdr, const uint64_t *counts, int64_t jobs, int64_t streams,
                              const uint8_t *bits, uint64_t stride_bytes, uint64_t job_stride_bytes,
                              const uint64_t *nbits) {
    if (hdr != 0 && hdr != 2 && hdr != 4) return "hdr_bytes must be 0, 2 or 4";
    if (hdr == 0 && !counts) return "hdr_bytes = 0 needs counts_dev";
    if (jobs < 0 || jobs > 65535) return "jobs outside [0, 65535]";
    if (streams <= 0) return "streams must be >= 1";
    if (!src || !bits || !nbits) return "src_dev, bits_dev and nbits_dev must not be NULL";
    if ((uintptr_t)bits % 8 || stride_bytes % 8 || job_stride_bytes % 8)
        return "bits_dev, stride_bytes and job_stride_bytes must be multiples of 8";
    if (jobs > 1 && job_stride_bytes < sat_mul((uint64_t)streams, stride_bytes))
        return "job_stride_bytes is smaller than streams * stride_bytes";
    return nullptr;
}

// lac_unpack_jobs in plain loops over host memory: the same arguments (base by value), the
// same outputs, the same verdicts.  Returns LAC_E_ARG for the refusals, else LAC_OK.
inline int wire_unpack_host(const uint8_t *src, uint64_t src_bytes, int hdr, const uint64_t *counts, uint64_t base,
                            int64_t jobs, int64_t streams, uint8_t *bits, uint64_t stride_bytes,
                            uint64_t job_stride_bytes, uint64_t *nbits, uint64_t *ends, int32_t *status) {
    if (check_args(src, hdr, counts, jobs, streams, bits, stride_bytes, job_stride_bytes, nbits)) return LAC_E_ARG;
    Walk w{base, true};
    for (int64_t j = 0; j < jobs; j++) {
        const uint64_t *cj = counts ? counts + j * streams : nullptr;
        uint64_t payload = 0;
        if (walk_header(w, hdr, streams, src_bytes)) {
            for (int64_t b = 0; b < streams; b++)
                payload = sat_add(payload, stream_bytes(read_count(src, w.start, hdr, cj, b)));
            walk_payload(w, hdr, streams, payload, src_bytes);
        }
        bool over = false;
        uint64_t off = w.start + header_bytes(hdr, streams);       // (used only while the job fits)
        for (int64_t b = 0; b < streams; b++) {
            const uint64_t nb = w.fits ? read_count(src, w.start, hdr, cj, b) : kNone;
            const bool sf = w.fits && stream_fits(nb, stride_bytes);
            over = over || (w.fits && !sf);
            const uint64_t n = sf ? stream_bytes(nb) : 0;
            uint8_t *slot = bits + (uint64_t)j * job_stride_bytes + (uint64_t)b * stride_bytes;
            for (uint64_t wi = 0; wi < stride_bytes / 8; wi++) {
                const uint64_t v = slot_word(src, off, n, wi);
                memcpy(slot + 8 * wi, &v, 8);
            }
            nbits[j * streams + b] = nb;
            if (w.fits) off += stream_bytes(nb);
        }
        if (status) status[j] = job_status(w.fits, over);
        if (w.fits) w.start = job_end(w, hdr, streams, payload);
        if (ends) ends[j] = w.start;
    }
    return LAC_OK;
}

}  // namespace wire
}  // namespace lac
