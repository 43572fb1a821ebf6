// lac_sparse.h -- plain host/device rules of sparse-row coding (include/lac.h lac_encode_sparse /
// lac_decode_sparse_steps): a row is at most K (symbol, weight) pairs over a uniform floor, and
// the coder computes the triple (lo, hi, T) of its symbol from the pairs and runs the range step
// (lac_ranges.h).  Every rule is written twice: once as the literal whole-row rule over arrays,
// and once as the per-lane partials plus their combination that the kernels of lac_sparse.hip
// run -- the same functions, held to each other, to Python integers and to the C oracle on the
// dense rows without a GPU (tests/native/sparse_check.cpp).
//
// The row form.  A call names a base weight `base` (uint32, >= 1), a slot count K (a multiple of 4
// in [4, 256]) and two arrays idx (int32) and wt (uint32); row (t, b) is the K slots at element
// t * step_stride + b * stream_stride of both.  With n the number of leading slots with idx >= 0
// the row stands for the dense table over the context's V symbols
//     pmf[s] = base + (wt_j if s == idx_j for some j < n, else 0),   T = base V + sum_{j<n} wt_j
// A row is valid when every pair has idx_j in [0, V), the pairs are strictly ascending in idx,
// every slot j >= n has idx == -1 (its weight is ignored) and T <= 2^(prec-1); wt_j = 0 is legal.
// Said per slot: slot m is well formed iff idx_m == -1, or 0 <= idx_m < V and (m == 0 or
// 0 <= idx_{m-1} < idx_m) -- a pair after a pad, an equal or descending index, an idx < -1 and an
// idx >= V all fail it.  Any other row is LAC_E_TABLE.
//
// Why no row fudges.  Every entry is at least 1 and T <= 2^(prec-1) < w <= w minp at every coder
// state, so the fudge test T > w minp (arith_code.py:84) never holds and the unfudged mapping
// reads the triple alone (lac_ranges.h).  Larger totals are refused: fudging needs the whole table.
//
// Sizes.  base < 2^32, V <= 2^31 and at most 256 weights below 2^32: base V < 2^63 and
// sum wt < 2^40, so every sum here fits uint64 without wrapping.  The caller hands base V as
// `baseV`, clamped to 2^62 where the product is larger (such a row is invalid at every prec).
#pragma once
#include <stdint.h>

#include "lac.h"
#include "lac_core.h"
#include "lac_ranges.h"

namespace lac {

constexpr int kSparseMaxSlots = 256;                          // 64 lanes of 4 slots
constexpr int kSparseLaneSlots = 4;                           // one 16-B vector of idx, one of wt
constexpr int32_t kSparseNoPrev = -2;                         // "the slot before slot 0"
constexpr uint64_t kSparseBaseVCap = 1ull << 62;

// ------------------------------------------------------------------ the call's arguments
// LAC_E_ARG with nothing launched unless all hold: K a multiple of 4 in [4, 256], base >= 1,
// strides that are non-negative multiples of 4 (slots), arrays that are not NULL and 16-B aligned.
inline bool sparse_slots_ok(int64_t K) { return K >= 4 && K <= kSparseMaxSlots && K % 4 == 0; }
inline bool sparse_stride_ok(int64_t s) { return s >= 0 && s % 4 == 0; }
inline bool sparse_ptr_ok(const void *p) { return p != nullptr && ((uintptr_t)p & 15) == 0; }
inline bool sparse_args_ok(const void *idx, const void *wt, int64_t K, int64_t step_stride, int64_t stream_stride,
                           uint32_t base) {
    return sparse_slots_ok(K) && base >= 1 && sparse_stride_ok(step_stride) && sparse_stride_ok(stream_stride) &&
           sparse_ptr_ok(idx) && sparse_ptr_ok(wt);
}
// base V as the kernels take it
inline uint64_t sparse_base_v(uint32_t base, int64_t V) {
    const u128 p = (u128)base * (u128)(uint64_t)V;
    return p > (u128)kSparseBaseVCap ? kSparseBaseVCap : (uint64_t)p;
}

// ------------------------------------------------------------------ one slot
// the slot's well-formedness given the index of the slot before it (kSparseNoPrev before slot 0)
__host__ __device__ inline bool sparse_slot_ok(int32_t idx, int32_t prev, int64_t V) {
    if (idx == -1) return true;
    if (idx < 0 || (int64_t)idx >= V) return false;
    return prev == kSparseNoPrev || (prev >= 0 && prev < idx);
}
// the weight a slot adds: a pad's is ignored
__host__ __device__ inline uint64_t sparse_slot_wt(int32_t idx, uint32_t wt) { return idx >= 0 ? (uint64_t)wt : 0; }

// ================================================================== the literal whole-row rules
// n, the leading slots with idx >= 0
inline int sparse_row_pairs(const int32_t *idx, int K) {
    int n = 0;
    while (n < K && idx[n] >= 0) n++;
    return n;
}
// LAC_OK or LAC_E_TABLE; *T_out the total of a valid row (0 otherwise)
inline int sparse_row_check(const int32_t *idx, const uint32_t *wt, int K, uint64_t baseV, int64_t V, int prec,
                            uint64_t *T_out) {
    *T_out = 0;
    const int n = sparse_row_pairs(idx, K);
    uint64_t T = baseV;
    for (int j = 0; j < K; j++) {
        if (j >= n) {
            if (idx[j] != -1) return LAC_E_TABLE;             // a pair after a pad, or an idx < -1
            continue;
        }
        if ((int64_t)idx[j] >= V) return LAC_E_TABLE;
        if (j > 0 && idx[j - 1] >= idx[j]) return LAC_E_TABLE;
        T += wt[j];
    }
    if (!range_total_ok(T, prec)) return LAC_E_TABLE;
    *T_out = T;
    return LAC_OK;
}
// the encode triple of symbol s in [0, V) on a valid row:
//     lo = base s + sum_{idx_j < s} wt_j,   hi = lo + base + sum_{idx_j == s} wt_j
inline void sparse_row_range(const int32_t *idx, const uint32_t *wt, int K, uint32_t base, int64_t s, uint64_t *lo,
                             uint64_t *hi) {
    const int n = sparse_row_pairs(idx, K);
    uint64_t below = 0, at = 0;
    for (int j = 0; j < n; j++) {
        if ((int64_t)idx[j] < s) below += wt[j];
        if ((int64_t)idx[j] == s) at += wt[j];
    }
    *lo = (uint64_t)base * (uint64_t)s + below;
    *hi = *lo + base + at;
}
// the decode search for a target t < T on a valid row: with P_j = sum_{m<j} wt_m,
// A_j = base idx_j + P_j, B_j = A_j + base + wt_j (strictly increasing) and j* = #{j : B_j <= t}:
// the symbol is idx_{j*} with range [A_{j*}, B_{j*}) when j* < n and t >= A_{j*}; otherwise it lies
// in the run of plain entries before pair j*: start = B_{j*-1}, first = idx_{j*-1} + 1 (0 and 0 for
// j* = 0), q = (t - start) / base, the symbol first + q, the range [start + q base, start + (q+1) base).
inline void sparse_row_search(const int32_t *idx, const uint32_t *wt, int K, uint32_t base, uint64_t t, int64_t *s,
                              uint64_t *lo, uint64_t *hi) {
    const int n = sparse_row_pairs(idx, K);
    uint64_t P = 0, start = 0;
    int64_t first = 0;
    for (int j = 0; j < n; j++) {
        const uint64_t A = (uint64_t)base * (uint64_t)idx[j] + P, B = A + base + wt[j];
        if (B > t) {                                          // j = j*
            if (t >= A) {
                *s = idx[j];
                *lo = A;
                *hi = B;
                return;
            }
            break;
        }
        P += wt[j];
        start = B;
        first = (int64_t)idx[j] + 1;
    }
    const uint64_t q = (t - start) / base;
    *s = first + (int64_t)q;
    *lo = start + q * base;
    *hi = *lo + base;
}

// ================================================================== the per-lane form
// Lane j of 64 owns slots 4 j .. 4 j + 3 (lanes past K / 4 hold pads: idx -1, wt 0).  `prev` is the
// last index of the lane before (kSparseNoPrev for lane 0): the order test needs each lane's last
// index against its neighbour's first.
struct SparseLane {
    int32_t idx[kSparseLaneSlots];
    uint32_t wt[kSparseLaneSlots];
};

// a lane of pads
__host__ __device__ inline SparseLane sparse_lane_pads() {
    SparseLane s;
    for (int q = 0; q < kSparseLaneSlots; q++) {
        s.idx[q] = -1;
        s.wt[q] = 0;
    }
    return s;
}

// Partial 1, the row's form: a slot of this lane is not well formed.  Combination: OR over lanes.
__host__ __device__ inline bool sparse_lane_bad(const SparseLane &s, int32_t prev, int64_t V) {
    bool bad = false;
#pragma unroll
    for (int q = 0; q < kSparseLaneSlots; q++) {
        bad |= !sparse_slot_ok(s.idx[q], prev, V);
        prev = s.idx[q];
    }
    return bad;
}

// Partial 2, encode: the lane's weights below s, at s and in all.  Combination: three sums over
// lanes; lo = base s + sum below, hi = lo + base + sum at, T = baseV + sum all (sparse_encode_triple).
__host__ __device__ inline void sparse_lane_sums(const SparseLane &s, int32_t sym, uint64_t *below, uint64_t *at,
                                                 uint64_t *all) {
    uint64_t b = 0, a = 0, t = 0;
#pragma unroll
    for (int q = 0; q < kSparseLaneSlots; q++) {
        const uint64_t w = sparse_slot_wt(s.idx[q], s.wt[q]);
        b += s.idx[q] < sym ? w : 0;                          // (a pad's weight is 0)
        a += s.idx[q] == sym ? w : 0;
        t += w;
    }
    *below = b;
    *at = a;
    *all = t;
}
// T = 0 marks the row LAC_E_TABLE (a slot not well formed, or a total above 2^(prec-1))
__host__ __device__ inline void sparse_encode_triple(uint32_t base, uint64_t baseV, int32_t sym, uint64_t below,
                                                     uint64_t at, uint64_t all, bool bad, int prec, uint64_t *lo,
                                                     uint64_t *hi, uint64_t *T) {
    *lo = (uint64_t)base * (uint64_t)(uint32_t)sym + below;
    *hi = *lo + base + at;
    const uint64_t tot = baseV + all;
    *T = (bad || !range_total_ok(tot, prec)) ? 0 : tot;
}

// Partial 3, decode: with `ex` the weights of all lanes before this one (the exclusive scan of the
// lanes' sums), the number of this lane's leading slots that are pairs with B <= t.  B is strictly
// increasing over a valid row and pads count as "not below", so the lanes with count 4 are a
// prefix: j* = 4 L + count_L for the first lane L whose count is below 4 (256 when there is none).
__host__ __device__ inline uint64_t sparse_lane_weight(const SparseLane &s) {
    uint64_t t = 0;
#pragma unroll
    for (int q = 0; q < kSparseLaneSlots; q++) t += sparse_slot_wt(s.idx[q], s.wt[q]);
    return t;
}
__host__ __device__ inline int sparse_lane_count(const SparseLane &s, uint32_t base, uint64_t ex, uint64_t t) {
    int c = 0;
    bool run = true;
    uint64_t P = ex;
#pragma unroll
    for (int q = 0; q < kSparseLaneSlots; q++) {
        const uint64_t w = sparse_slot_wt(s.idx[q], s.wt[q]);
        const uint64_t B = (uint64_t)base * (uint64_t)(uint32_t)s.idx[q] + P + base + w;
        run = run && s.idx[q] >= 0 && B <= t;
        c += run ? 1 : 0;
        P += w;
    }
    return c;
}
// What the winning lane broadcasts: slot c of it (c in [0, 4]; 4 only in lane 63 of a full row,
// "the slot past the row"): whether it is a pair, its index, P_{j*}, and the index before it.
struct SparsePick {
    int32_t idx;                                              // idx_{j*}, -1 where j* is no pair
    int32_t before;                                           // idx_{j*-1}, < 0 for j* = 0
    uint32_t wt;                                              // wt_{j*}
    uint64_t P;                                               // P_{j*}
};
__host__ __device__ inline SparsePick sparse_lane_pick(const SparseLane &s, int32_t prev, uint64_t ex, int c) {
    SparsePick p;
    p.idx = -1;
    p.wt = 0;
    p.before = prev;
    p.P = ex;
#pragma unroll
    for (int q = 0; q < kSparseLaneSlots; q++) {
        if (q == c) {
            p.idx = s.idx[q];
            p.wt = s.wt[q];
        }
        if (q < c) {
            p.before = s.idx[q];
            p.P += sparse_slot_wt(s.idx[q], s.wt[q]);
        }
    }
    return p;
}
// The combination: the symbol and its range from the broadcast pick.  The division by base runs
// only on a gap hit, and not at all for base = 1.
__host__ __device__ inline void sparse_resolve(const SparsePick &p, uint32_t base, uint64_t t, int64_t *s, uint64_t *lo,
                                               uint64_t *hi) {
    const uint64_t A = (uint64_t)base * (uint64_t)(uint32_t)p.idx + p.P;
    if (p.idx >= 0 && t >= A) {
        *s = p.idx;
        *lo = A;
        *hi = A + base + p.wt;
        return;
    }
    const int64_t first = p.before < 0 ? 0 : (int64_t)p.before + 1;
    const uint64_t start = (uint64_t)base * (uint64_t)first + p.P;   // B_{j*-1} = base (idx_{j*-1} + 1) + P_{j*}
    const uint64_t d = t - start;
    const uint64_t q = base == 1 ? d : d / base;
    *s = first + (int64_t)q;
    *lo = start + q * base;
    *hi = *lo + base;
}

// ================================================================== whole steps on the host
// One symbol of one stream by the literal rule: precedence LAC_E_SYMBOL_RANGE, LAC_E_TABLE, then
// range_encode_step's LAC_E_CAPACITY after the narrowing (zero width cannot occur: lo < hi).
template <typename Store>
inline int sparse_encode_step(EncState &st, int64_t &l, int64_t &h, const int32_t *idx, const uint32_t *wt, int K,
                              uint32_t base, int64_t V, int64_t s, int prec, uint64_t cap_words, Store store, int *k,
                              uint64_t *E) {
    *k = -1;
    *E = 0;
    if (s < 0 || s >= V) return LAC_E_SYMBOL_RANGE;
    uint64_t T, lo, hi;
    const int rc = sparse_row_check(idx, wt, K, sparse_base_v(base, V), V, prec, &T);
    if (rc) return rc;
    sparse_row_range(idx, wt, K, base, s, &lo, &hi);
    return range_encode_step(st, l, h, lo, hi, T, recip(T), prec, cap_words, store, k, E);
}
// One decoded symbol by the literal rule: the row first (LAC_E_TABLE), then the registers
// (LAC_E_DECODE_RANGE), then range_decode_step's frame (undetermined with `stop`).
template <typename Pull>
inline int sparse_decode_step(DecState &st, const int32_t *idx, const uint32_t *wt, int K, uint32_t base, int64_t V,
                              int prec, uint64_t past, bool stop, Pull pull, int64_t *s_out) {
    uint64_t T;
    const int rc = sparse_row_check(idx, wt, K, sparse_base_v(base, V), V, prec, &T);
    if (rc) return rc;
    if (st.x < st.l || st.x > st.h) return LAC_E_DECODE_RANGE;
    const uint64_t w = (uint64_t)(st.h - st.l + 1);
    const uint64_t t = range_target((uint64_t)(st.x - st.l), T, w, recip(w));
    uint64_t lo, hi;
    int64_t s;
    sparse_row_search(idx, wt, K, base, t, &s, &lo, &hi);
    if (s >= V) return LAC_E_DECODE_RANGE;
    const int r2 = range_decode_step(st, lo, hi, T, recip(T), prec, past, stop, pull);
    if (!r2) *s_out = s;
    return r2;
}

}  // namespace lac
