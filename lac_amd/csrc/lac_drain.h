// lac_drain.h -- which part of an open stream's output is settled, as plain functions (no HIP
// calls, no allocation).  k_enc_drain (lac_encode.hip, lac_encode_drain in include/lac.h) finds,
// resolves and moves words through these functions; drain_stream_host below is the whole drain of
// one stream in plain loops (the CPU oracle), and tests/test_drain_host.py checks it without a GPU.
//
// The output integer is held as two planes of 64-bit words, word 0 the most significant
// (lac_core.h): R = A + C + flush.  The active word wlast = (L - 1) >> 6 holds bit L - 1 and lives
// in EncState.wa / wc (mirrored to pa[wlast] / pc[wlast]); words below it are never written again.
// What can still reach a written word i < wlast is a carry-in from its right only: every later
// carry bit lands on the then-last bit, in the active word or later, and the signed flush tail is
// added below everything.  A carry-in is -1, 0 or +1 (the flush digits may be -1).
//
//   Rule 1, guard word.  A word g < wlast with low64(A_g + C_g) not in {0, 2^64 - 1} absorbs a
//   carry-in of +-1 without passing it on: its carry-out is (A_g + C_g) >> 64 whatever follows,
//   so words [0, g) are final.  The largest such g is taken.
//   Rule 2, certain state.  With 0 <= l and h < 2^prec (the reference's `certain`,
//   arith_code.py:228) every later value stays below one unit of bit L - 1, so no later digit
//   carries into what is written: g = wlast.  (Streams whose output is a long run of 0s or 1s
//   have no guard word and drain by this rule alone.)
//
// Words [0, g) are resolved backward from that carry exactly as finish_stream does (the carry out
// of word 0 is 0) and leave as big-endian bytes; words g..wlast become the new words 0..wlast-g,
// word g stored resolved (A' = low64(A_g + C_g), C' = 0, so the finish's carry-out-of-word-0 test
// stays valid) and L -= 64 g.  Under rule 2 the active word is the resolved one: the sum's bits
// below bit L - 1 are zero, so later appends OR into it as before.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LAC_DRAIN_HD __host__ __device__
#else
#define LAC_DRAIN_HD
#endif

namespace lac {
namespace drain {

// Rule 1's test of one word below the active word.
LAC_DRAIN_HD inline bool is_guard(uint64_t a, uint64_t c) {
    const uint64_t s = a + c;
    return s != 0 && s != ~0ull;
}

// Rule 2's test of the registers.
LAC_DRAIN_HD inline bool is_certain(int64_t l, int64_t h, int prec) { return l >= 0 && h < ((int64_t)1 << prec); }

// A stream a drain leaves alone whatever it holds: failed, finished, or with no word below the
// active one.
LAC_DRAIN_HD inline bool is_idle(int32_t err, int32_t nflush, uint64_t L) { return err != 0 || nflush >= 0 || L <= 64; }

// One word of the resolved prefix: low64(a + c + cin) with cin in {0, 1}; *cout in {0, 1}.
LAC_DRAIN_HD inline uint64_t resolve_word(uint64_t a, uint64_t c, uint64_t cin, uint64_t *cout) {
    const uint64_t s = a + c, r = s + cin;
    *cout = (uint64_t)(s < a) | (uint64_t)(r < s);
    return r;
}

// The carry-lookahead form of the same add over a block of up to 64 words, bit j of each mask
// one word and bit 0 the least significant (the kernel's lane 0): gen = the words whose a + c
// wraps, prop = those whose low64(a + c) is 2^64 - 1 (disjoint).  The integer add
// (prop | gen) + gen + cin ripples exactly as the words' carries do, so its sum bits differ from
// prop where a carry enters: bit j of the result is word j's carry-in, *cout the carry out of
// word 63.
LAC_DRAIN_HD inline uint64_t block_carries(uint64_t gen, uint64_t prop, uint64_t cin, uint64_t *cout) {
    const uint64_t u = prop | gen, r1 = u + gen, r = r1 + cin;
    *cout = (uint64_t)(r1 < u) | (uint64_t)(r < r1);
    return r ^ prop;
}

// All or nothing: the 8 g bytes of a stream go behind the `fill` bytes its slot holds, or the
// stream is left alone.  A fill that is no multiple of 8 (not one this call produced) fits nothing.
LAC_DRAIN_HD inline bool slot_fits(uint64_t g, uint64_t fill, uint64_t stride_bytes) {
    return (fill & 7) == 0 && fill <= stride_bytes && g <= (stride_bytes - fill) >> 3;
}

LAC_DRAIN_HD inline uint64_t to_big_endian(uint64_t x) { return __builtin_bswap64(x); }

// The words a drain emits: g, with the low word *sg and carry-out *cy of word g.  0: nothing
// drains.  pa / pc: the stream's planes (words 0..wlast-1 are read); wa / wc: the active word.
inline uint64_t choose_g_host(int64_t l, int64_t h, int prec, uint64_t L, uint64_t wa, uint64_t wc,
                              const uint64_t *pa, const uint64_t *pc, uint64_t *sg, uint64_t *cy) {
    if (L <= 64) return 0;
    const uint64_t wlast = (L - 1) >> 6;
    if (is_certain(l, h, prec)) {
        *sg = resolve_word(wa, wc, 0, cy);
        return wlast;
    }
    for (uint64_t i = wlast; i-- > 0;)
        if (is_guard(pa[i], pc[i])) {
            *sg = resolve_word(pa[i], pc[i], 0, cy);
            return i;
        }
    return 0;
}

// lac_encode_drain for one stream in plain loops over host memory: the registers l, h (read),
// the plane state L, wa, wc (updated), the planes (words 0..wlast read, the kept words moved to
// the front), the caller's slot of stride_bytes and its fill (grown by 8 g).  Returns g, the
// words drained; 0 leaves everything as it was.
inline uint64_t drain_stream_host(int64_t l, int64_t h, int prec, int32_t err, int32_t nflush, uint64_t &L,
                                  uint64_t &wa, uint64_t &wc, uint64_t *pa, uint64_t *pc, uint8_t *slot,
                                  uint64_t stride_bytes, uint64_t &fill) {
    if (is_idle(err, nflush, L)) return 0;
    const uint64_t wlast = (L - 1) >> 6;
    uint64_t sg = 0, carry = 0;
    const uint64_t g = choose_g_host(l, h, prec, L, wa, wc, pa, pc, &sg, &carry);
    if (g == 0 || !slot_fits(g, fill, stride_bytes)) return 0;
    for (uint64_t i = g; i-- > 0;) {
        const uint64_t w = to_big_endian(resolve_word(pa[i], pc[i], carry, &carry));
        memcpy(slot + fill + 8 * i, &w, 8);
    }
    for (uint64_t j = 1; j + g <= wlast; j++) {             // (index j < index j + g: ascending is safe)
        pa[j] = pa[j + g];
        pc[j] = pc[j + g];
    }
    pa[0] = sg;
    pc[0] = 0;
    if (g == wlast) {                                       // rule 2: the active word is the resolved one
        wa = sg;
        wc = 0;
    }
    pa[wlast - g] = wa;                                     // the active word's mirror (store_state)
    pc[wlast - g] = wc;
    L -= 64 * g;
    fill += 8 * g;
    return g;
}

}  // namespace drain
}  // namespace lac
