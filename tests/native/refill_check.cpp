// refill_check.cpp -- test infrastructure: the window rules of lac_amd/csrc/lac_refill.h on the
// host, as a shared library whose rc_* functions tests/test_refill_host.py drives.  Plain C++
// over lac_refill.h; every pointer is used exactly as the caller gives it, so sentinels around
// the caller's arrays show a word out of bounds.
#include <stdint.h>

#include "lac_refill.h"

using namespace lac;

extern "C" {

uint64_t rc_stream_words(uint64_t nbits) { return refill::stream_words(nbits); }
int rc_bad_source(uint64_t nbits, uint64_t base, uint64_t stride_bytes) {
    return refill::bad_source(nbits, base, stride_bytes);
}
uint64_t rc_held_bits(uint64_t nbits, uint64_t base, uint64_t W) { return refill::held_bits(nbits, base, W); }
int rc_complete(uint64_t nbits, uint64_t base, uint64_t W) { return refill::complete(nbits, base, W); }
int rc_ran_dry(uint64_t pos, uint64_t held, int complete) { return refill::ran_dry(pos, held, complete != 0); }
uint64_t rc_drop_words(uint64_t pos, int prec) { return refill::drop_words(pos, prec); }

// open_stream_host: win [W] and *held out -> 1, or 0 for a bad source (nothing touched).
int rc_open(const uint64_t *src, uint64_t stride_bytes, uint64_t nbits, uint64_t base, uint64_t W, uint64_t *win,
            uint64_t *held) {
    return refill::open_stream_host(src, stride_bytes, nbits, base, W, win, held);
}

// refill_stream_host: st = {base, held, pos} in/out -> REFILL_IDLE / _MOVED / _DRY.
int rc_refill(const uint64_t *src, uint64_t stride_bytes, uint64_t nbits, int prec, int32_t err, uint64_t W,
              uint64_t *win, uint64_t *st) {
    return refill::refill_stream_host(src, stride_bytes, nbits, prec, err, W, win, st[0], st[1], st[2]);
}

}  // extern "C"
