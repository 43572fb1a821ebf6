// lac_refill.h -- the bit window a decoder slides over a stream of any length, as plain functions
// (no HIP calls, no allocation).  k_dec_refill (lac_decode.hip; lac_decode_open_window and
// lac_decode_refill in include/lac.h) fills and slides the window through these functions;
// refill_stream_host below is the whole refill of one stream in plain loops (the CPU oracle), and
// tests/test_refill_host.py checks it without a GPU.  The decode mirror of lac_drain.h.
//
// The stream is nbits bits, nw = ceil(nbits / 64) big-endian words.  The window is W words per
// stream (the context's cap_words); window word j holds source word base + j, and the decode
// kernels are given the window as their bit buffer with held_bits() as the stream's bit count.
// Three facts of the decoder (lac_dec_dev.h) make that exact:
//   1. it never reads a bit below pos - prec: x holds bits [pos - prec, pos), bit_window loads
//      words pos >> 6 and the next;
//   2. one step pulls k = prec - bitlen(nh - nl) <= prec fresh bits (decode_advance,
//      decode_advance_nb), so N steps advance pos by at most N * prec;
//   3. everything a step derives from the stream's end -- the zero padding, `past` in
//      decode_symbol, det / ndet, LAC_OPT_DECODE_STOP -- uses pos - nbits only, which is unchanged
//      when pos and nbits shift together by whole words.
// So a decoder on the window [64 base, 64 base + held) computes what the whole-stream decoder
// computes, provided no read passes the bits the window holds while more of the stream lies
// outside it (ran_dry).  A window that reaches the stream's end (complete) has the exact count
// and the exact zeros past it, and stays where it is.
//
// Sizing.  After a refill pos <= prec + 63 (drop_words); N steps add at most N * prec; a read may
// end at `held` exactly.  So N steps between two refills never run dry when
//     64 W >= prec + 63 + N * prec = (N + 1) * prec + 63.
// The encode side's sizing for N symbols between drains, capacity_bits = N * (prec + 2) + 256,
// gives 64 W >= N * prec + 2 N + 256 >= (N + 1) * prec + 63 for every N >= 0 whenever
// prec <= 193, so for every prec <= 61 the library takes.  (A fresh window starts at pos = prec,
// below the bound's prec + 63.)
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LAC_REFILL_HD __host__ __device__
#else
#define LAC_REFILL_HD
#endif

namespace lac {
namespace refill {

LAC_REFILL_HD inline uint64_t stream_words(uint64_t nbits) { return (nbits >> 6) + ((nbits & 63) != 0); }

// A stream no window is opened on: it claims more bits than its source slot holds, or its
// window would start past its end.  (64 * base > nbits without the product's overflow.)
LAC_REFILL_HD inline bool bad_source(uint64_t nbits, uint64_t base, uint64_t stride_bytes) {
    return nbits > 8 * stride_bytes || base > (nbits >> 6);
}

// The bit count the decode kernels see as nbits (64 * base <= nbits).
LAC_REFILL_HD inline uint64_t held_bits(uint64_t nbits, uint64_t base, uint64_t W) {
    const uint64_t rest = nbits - 64 * base;
    return rest < 64 * W ? rest : 64 * W;
}

// The window reaches the stream's end: past-the-end zeros are then exact.
LAC_REFILL_HD inline bool complete(uint64_t nbits, uint64_t base, uint64_t W) { return base + W >= stream_words(nbits); }

// A step since the last refill read bits the window did not hold (pos == held is fine: the
// last bit read is held - 1).
LAC_REFILL_HD inline bool ran_dry(uint64_t pos, uint64_t held, bool is_complete) { return !is_complete && pos > held; }

// Whole words below every bit the decoder still needs: the new position pos - 64 g lies in
// [prec, prec + 63], which keeps lac_decode_set_state's pos >= prec and the bits of x in the
// window.  (pos >= prec in every state a decoder reaches.)
LAC_REFILL_HD inline uint64_t drop_words(uint64_t pos, int prec) {
    return pos >= (uint64_t)prec ? (pos - (uint64_t)prec) >> 6 : 0;
}

// Source word i as the window stores it: zero at or past the stream's end.  The last word's
// bits past nbits stay as the source has them (the decoders mask by the count).
inline uint64_t source_word_host(const uint64_t *src, uint64_t nw, uint64_t i) { return i < nw ? src[i] : 0; }

// lac_decode_open_window for one stream: window words 0..W-1 from source word base on, *held
// the count.  Returns false (nothing read or written) for a bad source.
inline bool open_stream_host(const uint64_t *src, uint64_t stride_bytes, uint64_t nbits, uint64_t base, uint64_t W,
                             uint64_t *win, uint64_t *held) {
    if (bad_source(nbits, base, stride_bytes)) return false;
    const uint64_t nw = stream_words(nbits);
    for (uint64_t j = 0; j < W; j++) win[j] = source_word_host(src, nw, base + j);
    *held = held_bits(nbits, base, W);
    return true;
}

enum { REFILL_IDLE = 0, REFILL_MOVED = 1, REFILL_DRY = 2 };

// lac_decode_refill for one stream in plain loops over host memory: the source (words 0..nw-1
// are read and nothing beyond), the window (the kept W - g words moved to the front, g words
// taken from the source), base, held and pos (updated).  err != 0: the stream is left alone.
// REFILL_DRY: nothing is changed (the kernel sets err = LAC_E_CAPACITY, err_step = nsym).
inline int refill_stream_host(const uint64_t *src, uint64_t stride_bytes, uint64_t nbits, int prec, int32_t err,
                              uint64_t W, uint64_t *win, uint64_t &base, uint64_t &held, uint64_t &pos) {
    if (err != 0 || bad_source(nbits, base, stride_bytes)) return REFILL_IDLE;
    const bool done = complete(nbits, base, W);
    if (ran_dry(pos, held, done)) return REFILL_DRY;
    if (done) return REFILL_IDLE;                             // the window holds the stream's end: it stays
    const uint64_t g = drop_words(pos, prec);
    if (g == 0) return REFILL_IDLE;
    const uint64_t nw = stream_words(nbits);                  // (pos <= held <= 64 W: g < W)
    for (uint64_t j = 0; j + g < W; j++) win[j] = win[j + g]; // (index j < index j + g: ascending is safe)
    for (uint64_t j = W - g; j < W; j++) win[j] = source_word_host(src, nw, base + g + j);
    base += g;
    held = held_bits(nbits, base, W);
    pos -= 64 * g;
    return REFILL_MOVED;
}

}  // namespace refill
}  // namespace lac
