// lac_fsm.h -- plain host rules of the finite-state models (include/lac.h lac_fsm_*): the
// limits a model must keep, the layout of the prepared model the kernels of lac_fsm.hip read,
// and what one prepared row holds -- checked without a GPU (tests/native/fsm_check.cpp).
//
// A model has K states over the context's V symbols: pmf[K][V] integer tables and, unless the
// caller names every step's state, next[K][V].  The reference ships the family as
// NFA(state, transitions) (arith_code.py:423-434): calc_dist returns the current state's CDF,
// accept moves the state by next[state][symbol].
//
// The prepared model is one allocation of five 256-B aligned sections:
//   meta    [K]       FsmMeta: T, the smallest positive entry, ceil(T / minp), 1 / T
//   cdf     [K][Vp]   per-entry inclusive CDF in the entries' own width; entries V .. Vp - 1 hold T
//   pmf     [K][Vp]   the rows themselves, zero padded (the fudged scans walk them)
//   bounds  [K][64]   long rows only: the CDF value at the end of each of <= 64 chunks
//   next    [K][V]    int32, absent in the explicit-states form
// Vp pads a row to whole 16-B vectors, so V needs no alignment and every row starts on one.
#pragma once
#include <stdint.h>

namespace lac {

constexpr int64_t kFsmMaxVocab = 65536;                // V <= 2^16
constexpr int64_t kFsmMaxEntries = (int64_t)1 << 24;   // K * V <= 2^24: an order-2 byte model fits

// LAC_E_ARG beyond either limit
inline bool fsm_limits_ok(int64_t K, int64_t V) {
    return K >= 1 && V >= 1 && V <= kFsmMaxVocab && K <= kFsmMaxEntries / V;
}

struct FsmMeta {       // 32 bytes per state
    uint64_t T;        // row total; 0 marks a bad row (empty, or total >= 2^64): LAC_E_TABLE at the
                       // step that reaches it
    uint64_t minp;     // smallest positive entry (CDFPredictor.minp, arith_code.py:79-82)
    uint64_t fthr;     // ceil(T / minp), at most 2^62: the row fudges at width w iff w < fthr (:84)
    double inv_T;      // 1.0 / T correctly rounded (0 for a bad row)
};
// A u32 row with T >= 2^32 is wide: its CDF does not fit the entries, so both coders scan its
// pmf row instead (the pmf path's own scans; such rows are legal and rare).
template <typename E>
constexpr bool fsm_row_wide(uint64_t T) { return sizeof(E) == 4 && (T >> 32) != 0; }

struct FsmLayout {
    int64_t K, V;
    int esize, vec;            // entry bytes (4 / 8), entries per 16-B vector
    int64_t Vp, nvec;          // padded row length in entries / in vectors
    int long_rows;             // nvec > 64: the row is searched by chunk bounds first
    int64_t G;                 // vectors per chunk (ceil(nvec / 64)); chunk c = vectors [c G, (c + 1) G)
    uint64_t off_meta, off_cdf, off_pmf, off_bounds, off_next, bytes;
};

inline uint64_t fsm_align(uint64_t x) { return (x + 255) & ~(uint64_t)255; }

inline FsmLayout fsm_layout(int64_t K, int64_t V, int pmf_bits, bool has_next) {
    FsmLayout y;
    y.K = K;
    y.V = V;
    y.esize = pmf_bits / 8;
    y.vec = 16 / y.esize;
    y.Vp = (V + y.vec - 1) / y.vec * y.vec;
    y.nvec = y.Vp / y.vec;
    y.long_rows = y.nvec > 64;
    y.G = (y.nvec + 63) / 64;
    uint64_t o = 0;
    y.off_meta = o;
    o = fsm_align(o + (uint64_t)K * sizeof(FsmMeta));
    y.off_cdf = o;
    o = fsm_align(o + (uint64_t)K * (uint64_t)y.Vp * (uint64_t)y.esize);
    y.off_pmf = o;
    o = fsm_align(o + (uint64_t)K * (uint64_t)y.Vp * (uint64_t)y.esize);
    y.off_bounds = o;
    if (y.long_rows) o = fsm_align(o + (uint64_t)K * 64 * (uint64_t)y.esize);
    y.off_next = o;
    if (has_next) o = fsm_align(o + (uint64_t)K * (uint64_t)V * sizeof(int32_t));
    y.bytes = o;
    return y;
}

constexpr uint64_t kFsmThrCap = (uint64_t)1 << 62;     // w <= 2^61 < the cap: w < fthr is unchanged by it

// What the prepare kernel writes for one row (the same integers, by a plain scan): cdf[Vp],
// pmf_pad[Vp], bounds[64] (when the layout has long rows) and the meta.
template <typename E>
inline void fsm_prepare_row(const E *row, const FsmLayout &y, E *cdf, E *pmf_pad, E *bounds, FsmMeta *meta) {
    typedef unsigned __int128 u128;
    u128 T = 0;
    uint64_t minp = 0;
    for (int64_t i = 0; i < y.V; i++) {
        T += row[i];
        if (row[i] && (!minp || (uint64_t)row[i] < minp)) minp = (uint64_t)row[i];
    }
    const uint64_t t = (T >> 64) ? 0 : (uint64_t)T;
    meta->T = t;
    meta->minp = t ? minp : 0;
    uint64_t thr = t ? (uint64_t)((T + (minp - 1)) / minp) : 0;
    meta->fthr = thr < kFsmThrCap ? thr : kFsmThrCap;
    meta->inv_T = t ? 1.0 / (double)t : 0.0;
    uint64_t c = 0;                                    // wraps for bad and wide rows, whose CDF is not read
    for (int64_t i = 0; i < y.Vp; i++) {
        if (i < y.V) c += (uint64_t)row[i];
        cdf[i] = i < y.V ? (E)c : (E)t;
        pmf_pad[i] = i < y.V ? row[i] : (E)0;
    }
    if (y.long_rows)
        for (int64_t ch = 0; ch < 64; ch++) {
            const int64_t end = (ch + 1) * y.G * y.vec;             // one past the chunk's last entry
            bounds[ch] = end <= y.Vp ? cdf[end - 1] : (ch * y.G * y.vec < y.Vp ? cdf[y.Vp - 1] : (E)t);
        }
}

// The O(1) lookup of the encoder: symbol s of a prepared row -> lo = c_{s-1}, hi = c_s
// (rows that are neither bad nor wide; 0 <= s < V).
template <typename E>
inline void fsm_lookup(const E *cdf, int64_t s, uint64_t *lo, uint64_t *hi) {
    *lo = s > 0 ? (uint64_t)cdf[s - 1] : 0;
    *hi = (uint64_t)cdf[s];
}

// The decoder's search on a prepared row: the symbol whose range holds the target,
// s = |{i : c_i <= tgt}| (bisect_right, arith_code.py:94-97), by chunk bounds for long rows.
// tgt < T.  (The kernel does the same with one ballot per level.)
template <typename E>
inline int64_t fsm_search(const E *cdf, const E *bounds, const FsmLayout &y, uint64_t tgt) {
    int64_t e0 = 0, e1 = y.Vp;
    if (y.long_rows) {
        int64_t ch = 0;
        while (ch < 63 && (uint64_t)bounds[ch] <= tgt) ch++;
        e0 = ch * y.G * y.vec;
        e1 = e0 + y.G * y.vec < y.Vp ? e0 + y.G * y.vec : y.Vp;
    }
    int64_t s = e0;
    while (s < e1 && (uint64_t)cdf[s] <= tgt) s++;
    return s;
}

}  // namespace lac
