// lac_ranges.h -- plain host/device rules of range-level coding (include/lac.h
// lac_encode_ranges / lac_decode_ranges_step): the coder is handed the three integers
// symbol_to_range needs -- lo = c_{s-1}, hi = c_s and T (arith_code.py:98-110 reads dist[s-1],
// dist[s] and dist[-1] only) -- instead of a table.  Here: which triples are valid and in what
// order their defects are reported, the three-entry table a triple stands for, the launch
// geometry, and the whole encode and decode step one lane runs -- the same functions the
// kernels of lac_ranges.hip call, checked without a GPU (tests/native/ranges_check.cpp).
//
// Equivalence.  The triple (lo, hi, T) codes exactly as the table [lo, hi - lo, T - hi] codes
// its symbol 1.  A table fudges at width w iff T > w minp (:84); every coder state has
// w > 2^(prec-1), so with T <= 2^(prec-1) no width fudges whatever the table's other two
// entries are, and the unfudged mapping a = ceil(lo w / T), b = ceil(hi w / T) reads only the
// triple.  T > 2^(prec-1) is therefore refused (fudging needs the whole table).
#pragma once
#include <stdint.h>

#include "lac.h"
#include "lac_core.h"

namespace lac {

// ------------------------------------------------------------------ validity
// A triple is valid when 0 < T <= 2^(prec-1) and lo < hi <= T.  Defects in the order they are
// reported: LAC_E_TABLE (T = 0, T > 2^(prec-1), hi > T or lo > hi), then LAC_E_ZERO_WIDTH
// (lo == hi); LAC_OK otherwise.
__host__ __device__ inline bool range_total_ok(uint64_t T, int prec) { return T != 0 && T <= (1ull << (prec - 1)); }
__host__ __device__ inline int range_check(uint64_t lo, uint64_t hi, uint64_t T, int prec) {
    if (!range_total_ok(T, prec) || hi > T || lo > hi) return LAC_E_TABLE;
    if (lo == hi) return LAC_E_ZERO_WIDTH;
    return LAC_OK;
}

// The table a valid triple stands for (its symbol 1 is the triple's symbol).
__host__ __device__ inline void range_table(uint64_t lo, uint64_t hi, uint64_t T, uint64_t row[3]) {
    row[0] = lo;
    row[1] = hi - lo;
    row[2] = T - hi;
}

// ------------------------------------------------------------------ launch geometry
// One lane per stream, 256-thread workgroups: no row is scanned, so a wave per stream would idle
// 63 of its lanes.  Lanes past the last stream are masked, never returned early.
constexpr int kRangeThreads = 256;
inline unsigned range_blocks(int64_t B) { return (unsigned)((B + kRangeThreads - 1) / kRangeThreads); }

// ------------------------------------------------------------------ the mapping
// a = ceil(lo w / T), b = ceil(hi w / T) for a valid triple and w < 2^63: the products are
// 128-bit (T <= 2^60, w <= 2^61 for every renormalised state), the quotients at most w.
// inv = recip(T), which depends on the triple alone and so is computed off the step's chain.
__host__ __device__ inline void range_map(uint64_t lo, uint64_t hi, uint64_t T, double inv, uint64_t w, uint64_t *a,
                                          uint64_t *b) {
    *a = div_floor_inv((u128)lo * w + (T - 1), T, inv);
    *b = div_floor_inv((u128)hi * w + (T - 1), T, inv);
}

// The decoder's target floor(v T / w) for v < w (below T), inv_w = recip(w).
__host__ __device__ inline uint64_t range_target(uint64_t v, uint64_t T, uint64_t w, double inv_w) {
    return div_floor_inv((u128)v * T, w, inv_w);
}

// ------------------------------------------------------------------ encode step
// plane_append (lac_core.h) for k <= 63 digits without its loop: the digits span at most two
// plane words, so the append is straight-line and `store` runs at most once -- in the kernel
// under a short masked branch, everything else predicated.  Same results, word for word.
template <typename Store>
__host__ __device__ inline bool range_append(uint64_t &L, uint64_t &wa, uint64_t &wc, int k, uint64_t E,
                                             uint64_t cap_words, Store store) {
    if (k <= 0) return true;
    const int off = (int)(L & 63);
    const uint64_t elo = E & ((1ull << k) - 1);
    if (E >> k) wc |= 1ull << (63 - ((L - 1) & 63));          // the carry lands on bit L-1
    const int room = off ? 64 - off : 0;                      // free bits in the word of bit L-1
    const int first = k < room ? k : room, rest = k - first;  // digits into that word / into the next
    if (first > 0) wa |= (elo >> rest) << (room - first);
    if (rest > 0) {
        if (L > 0) {                                          // the word of bit L-1 is complete
            const uint64_t idx = ((L + (uint64_t)first) >> 6) - 1;
            if (idx >= cap_words) { L += (uint64_t)first; return false; }
            store(idx, wa, wc);
            wa = 0;
            wc = 0;
        }
        wa |= (elo & ((1ull << rest) - 1)) << (64 - rest);
    }
    L += (uint64_t)k;
    return ((L - 1) >> 6) < cap_words;
}

// One symbol of one stream: coder_step (lac_dev.h) on the table range_table() gives, symbol 1.
// Returns LAC_OK or the stream's new sticky error (st.err is the caller's to set); on
// LAC_E_TABLE / LAC_E_ZERO_WIDTH nothing has changed, on LAC_E_CAPACITY the registers are the
// narrowed ones, as coder_step leaves them.  *k, *E: the step's digits (the trace entry), set
// whenever the narrowing happened (*k = -1 otherwise).
template <typename Store>
__host__ __device__ inline int range_encode_step(EncState &st, int64_t &l, int64_t &h, uint64_t lo, uint64_t hi,
                                                 uint64_t T, double inv, int prec, uint64_t cap_words, Store store,
                                                 int *k, uint64_t *E) {
    *k = -1;
    *E = 0;
    const int rc = range_check(lo, hi, T, prec);
    if (rc) return rc;
    const uint64_t w = (uint64_t)(h - l + 1);
    uint64_t a, b;
    range_map(lo, hi, T, inv, w, &a, &b);
    if (a >= b) return LAC_E_ZERO_WIDTH;                      // (only a state narrower than T: w <= 2^(prec-1))
    h = l + (int64_t)b - 1;
    l = l + (int64_t)a;
    renorm(l, h, prec, k, E);
    if (!range_append(st.L, st.wa, st.wc, *k, *E, cap_words, store)) return LAC_E_CAPACITY;
    st.nsym++;
    return LAC_OK;
}

// ------------------------------------------------------------------ decode step
// The advance half of lac_decode_ranges_step for one stream: decode_symbol's frame
// (lac_dec_dev.h) without its search -- the caller names the symbol's range.  `past` = window
// bits past the stream's end (pos - nbits when positive, else 0), `pull(k)` returns the next k
// bits (zeros past the end).  Tests in order: the triple (LAC_E_TABLE), the registers, the
// target in [lo, hi) (LAC_E_DECODE_RANGE), the determined test (LAC_E_UNDETERMINED with
// `stop`); then narrow, renormalise, pull.  Any error leaves st as it was.
template <typename Pull>
__host__ __device__ inline int range_decode_step(DecState &st, uint64_t lo, uint64_t hi, uint64_t T, double inv,
                                                 int prec, uint64_t past, bool stop, Pull pull) {
    if (!range_total_ok(T, prec) || hi > T || lo > hi) return LAC_E_TABLE;
    const int64_t l = st.l, h = st.h, x = st.x;
    if (x < l || x > h) return LAC_E_DECODE_RANGE;            // corrupted state / bits
    const uint64_t w = (uint64_t)(h - l + 1), v = (uint64_t)(x - l);
    const double iw = recip(w);
    const uint64_t tgt = range_target(v, T, w, iw);
    if (tgt < lo || tgt >= hi) return LAC_E_DECODE_RANGE;     // the range misses the target (lo == hi always does)
    const int u = past < (uint64_t)prec ? (int)past : prec;
    const uint64_t vhi = v + ((1ull << u) - 1);
    const bool det = vhi < w && (vhi == v || range_target(vhi, T, w, iw) < hi);
    if (stop && !det) return LAC_E_UNDETERMINED;
    uint64_t a, b;
    range_map(lo, hi, T, inv, w, &a, &b);
    if (!(l + (int64_t)a <= x && x <= l + (int64_t)b - 1)) return LAC_E_DECODE_RANGE;   // :277-278 (cannot happen: tgt in [lo, hi))
    if (st.det && det) st.ndet++;
    else st.det = 0;
    int64_t nl = l + (int64_t)a, nh = l + (int64_t)b - 1;
    int k;
    uint64_t E;
    renorm(nl, nh, prec, &k, &E);
    if (k > 0) {
        st.x = (int64_t)((((uint64_t)x - (E << (prec - k))) << k) | pull(k));
        st.pos += (uint64_t)k;
    }
    st.l = nl;
    st.h = nh;
    st.nsym++;
    return LAC_OK;
}

// The peek half: floor((x - l) T' / w), or UINT64_MAX for a total that is not valid or
// registers with x outside [l, h] (the advance that uses them raises the error).
constexpr uint64_t kRangeNoTarget = ~0ull;
__host__ __device__ inline uint64_t range_peek(const DecState &st, uint64_t T, int prec) {
    if (!range_total_ok(T, prec) || st.x < st.l || st.x > st.h) return kRangeNoTarget;
    const uint64_t w = (uint64_t)(st.h - st.l + 1);
    return range_target((uint64_t)(st.x - st.l), T, w, recip(w));
}

}  // namespace lac
