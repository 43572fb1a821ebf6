// lac_topk.h -- plain host/device rules of top-k rows from logits (include/lac.h lac_topk_logits):
// one logits row -> its sparse form, the k heaviest q1 entries in symbol order with integer
// weights, a valid lac_encode_sparse row by construction.  Every rule is written twice: once as
// the literal whole-row rule over arrays (topk_row_literal), and once as the pieces the kernels of
// lac_topk.hip run -- the level histogram, the threshold found by the lanes of one wave, the
// ordered rank of an entry from prefix counts in symbol order -- walked over the kernels' own
// layout of tiles, waves, register rounds and lanes (topk_row_lanes).  The two are held to each
// other and to Python integers on the C oracle's q1 tables without a GPU
// (tests/native/topk_check.cpp).
//
// The rule.  Entry i of a row x[0..V) weighs g_i = TAB[544 - j_i] (include/lac_q1_table.h), j_i
// the q1 level of x_i: m = max x (NaN ignored), c = RNE_f32(544 - 32 m), j = sat_u32(fmaf(x, 32,
// c)) capped at 544, NaN / -inf / negatives 0.  That is the q1 table at k = 24, whatever the
// context's prec.  The k entries largest by g survive, the lower symbol first among equal g.  The
// key is g, not j: TAB has fewer distinct values than levels, so the entries that tie with the
// k-th are those of a whole class of adjacent levels.  Output slots 0..k-1: the survivors in
// ascending symbol order, idx int32 and wt = g >> (24 - weight_bits); slots k..K-1: idx -1, wt 0.
//
// Selection without a sort.  With hist[j] the number of entries at level j, g* the weight of the
// k-th heaviest entry, `above` the entries heavier than g* (< k) and r = k - above (>= 1) the
// number of ties to take, an entry survives iff g > g*, or g == g* and fewer than r ties precede
// it in symbol order; its slot is (heavier entries before it) + min(ties before it, r).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "lac.h"
#include "lac_q1_table.h"

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#define __device__
#endif
#endif

namespace lac {

constexpr int kTopkMaxK = 256;                                // survivors, and slots, per row
constexpr int kTopkL = LAC_Q1_DMAX * LAC_Q1_STEPS;            // 544: the top level
constexpr int kTopkLevels = kTopkL + 1;
constexpr int kTopkLaneBins = 9;                              // the threshold wave: 64 lanes of 9 levels, top down
constexpr int kTopkMaxThreads = 1024;
constexpr int kTopkMaxR = 16;                                 // 16-B vectors a thread holds
constexpr int kTopkRegMaxVec = kTopkMaxThreads * kTopkMaxR;   // 16384: bf16 V <= 131072, f32 V <= 65536
constexpr int kTopkStreamR = 8;
enum { TOPK_FORM_AUTO = 0, TOPK_FORM_REGS = 1, TOPK_FORM_STREAM = 2 };   // LAC_OPT_TOPK_FORM
static_assert(64 * kTopkLaneBins >= kTopkLevels, "one wave holds the histogram");

// ------------------------------------------------------------------ the call's arguments
// LAC_E_ARG with nothing launched or written unless all hold (steps > 0; steps == 0 is LAC_OK with
// no launch, steps < 0 refused): a known logit type, non-negative strides, rows 16-B aligned with V
// and the strides multiples of the elements per 16 bytes, k in [1, min(V, 256)], K a multiple of 4
// in [k, 256], weight_bits in [0, 24], outputs not NULL and 16-B aligned.
inline int topk_type_bytes(int logit_type) {
    return logit_type == LAC_LOGITS_BF16 ? 2 : logit_type == LAC_LOGITS_F32 ? 4 : 0;
}
inline bool topk_layout_ok(uintptr_t lg, int logit_type, int64_t V, int64_t step_stride, int64_t stream_stride) {
    const int tb = topk_type_bytes(logit_type);
    if (!tb || step_stride < 0 || stream_stride < 0 || V < 1) return false;
    const int n = 16 / tb;
    return lg != 0 && lg % 16 == 0 && V % n == 0 && step_stride % n == 0 && stream_stride % n == 0;
}
inline bool topk_k_ok(int64_t k, int64_t V) { return k >= 1 && k <= V && k <= kTopkMaxK; }
inline bool topk_slots_ok(int64_t K, int64_t k) { return K % 4 == 0 && K >= k && K <= kTopkMaxK; }
inline bool topk_bits_ok(int64_t weight_bits) { return weight_bits >= 0 && weight_bits <= LAC_Q1_KMAX; }
inline bool topk_out_ok(uintptr_t p) { return p != 0 && p % 16 == 0; }
inline bool topk_args_ok(uintptr_t lg, int logit_type, int64_t V, int64_t step_stride, int64_t stream_stride,
                         int64_t k, int64_t weight_bits, int64_t K, uintptr_t idx, uintptr_t wt) {
    return topk_layout_ok(lg, logit_type, V, step_stride, stream_stride) && topk_k_ok(k, V) && topk_slots_ok(K, k) &&
           topk_bits_ok(weight_bits) && topk_out_ok(idx) && topk_out_ok(wt);
}

// ------------------------------------------------------------------ one entry: its level
// sat_u32 is v_cvt_u32_f32's own saturation (NaN, -inf and negatives -> 0, >= 2^32 -> 2^32 - 1,
// truncation), written as asm on the device because a C++ cast of such values is undefined.
__host__ __device__ inline uint32_t topk_sat_u32(float y) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r;
    asm("v_cvt_u32_f32 %0, %1" : "=v"(r) : "v"(y));
    return r;
#else
    if (!(y > 0.0f)) return 0;
    if (y >= 4294967296.0f) return 0xFFFFFFFFu;
    return (uint32_t)y;
#endif
}
__host__ __device__ inline float topk_c(float m) { return (float)kTopkL - (float)LAC_Q1_STEPS * m; }   // 32 m exact
__host__ __device__ inline uint32_t topk_level(float x, float c) {
    const uint32_t j = topk_sat_u32(fmaf(x, (float)LAC_Q1_STEPS, c));
    return j < (uint32_t)kTopkL ? j : (uint32_t)kTopkL;
}
// an element of a row as a float (bf16: the bit pattern in the high half)
inline float topk_load(const void *row, int type_bytes, int64_t i) {
    uint32_t u;
    if (type_bytes == 2) u = (uint32_t)((const uint16_t *)row)[i] << 16;
    else u = ((const uint32_t *)row)[i];
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// the weight of a level (tab: LAC_Q1_TAB, 545 entries, non-increasing, the last ones 1), and what a slot holds
__host__ __device__ inline uint32_t topk_g(const uint32_t *tab, uint32_t j) { return tab[kTopkL - (int)j]; }
__host__ __device__ inline uint32_t topk_wt(uint32_t g, int weight_bits) { return g >> (LAC_Q1_KMAX - weight_bits); }

// ------------------------------------------------------------------ the level -> class rule
// Levels j and j' are one tie class iff TAB[544 - j] == TAB[544 - j'].  TAB is monotone, so a class
// is a run of adjacent levels [lo, hi].
inline int topk_class_lo(const uint32_t *tab, int j) {
    while (j > 0 && topk_g(tab, j - 1) == topk_g(tab, j)) j--;
    return j;
}
inline int topk_class_hi(const uint32_t *tab, int j) {
    while (j < kTopkL && topk_g(tab, j + 1) == topk_g(tab, j)) j++;
    return j;
}

// ------------------------------------------------------------------ the threshold
struct TopkCut {
    int jlo, jhi;                                             // the tie class of the k-th heaviest entry
    uint32_t above;                                           // entries heavier than the class (< k)
    uint32_t r;                                               // ties to take: k - above, in [1, ties]
    uint32_t ties;                                            // entries in the class
};
// The literal search over hist[0..544] (its sum is V >= k), in three steps.
inline TopkCut topk_threshold(const uint32_t *hist, const uint32_t *tab, int k) {
    uint64_t acc = 0;                                         // 1. from the top until the count reaches k
    int j = kTopkL;
    while (j > 0 && acc + hist[j] < (uint64_t)k) acc += hist[j--];
    TopkCut c;                                                // 2. widen to the whole tie class
    c.jlo = topk_class_lo(tab, j);
    c.jhi = topk_class_hi(tab, j);
    uint64_t above = 0, ties = 0;                             // 3. g*'s class, the count above it, the ties to take
    for (int i = kTopkL; i > c.jhi; i--) above += hist[i];
    for (int i = c.jhi; i >= c.jlo; i--) ties += hist[i];
    c.above = (uint32_t)above;
    c.r = (uint32_t)k - c.above;
    c.ties = (uint32_t)ties;
    return c;
}
// The same search as one wave runs it: lane l owns the levels 544 - 9 l - i, i < 9 (those >= 0), top
// down.  Partial 1: the lane's count.  Combination: an inclusive scan over lanes; the one lane with
// excl < k <= incl walks its levels for j*.
__host__ __device__ inline int topk_lane_level(int lane, int i) { return kTopkL - kTopkLaneBins * lane - i; }
__host__ __device__ inline int topk_lane_find(const uint32_t (&hv)[kTopkLaneBins], int lane, uint32_t excl, uint32_t k) {
    int js = -1;
    uint32_t acc = excl;
#pragma unroll
    for (int i = 0; i < kTopkLaneBins; i++) {
        if (js < 0 && acc + hv[i] >= k) js = topk_lane_level(lane, i);
        acc += hv[i];
    }
    return js;
}
// Partial 2, given g* = TAB[544 - j*]: the lane's entries heavier than g*, its entries at g*, and
// the lowest and highest of its levels at g*.  Combination: two sums, a minimum and a maximum.
struct TopkLaneClass {
    uint32_t above, ties;
    int lo, hi;                                               // kTopkLevels / -1 where the lane has none
};
__host__ __device__ inline TopkLaneClass topk_lane_class(const uint32_t (&hv)[kTopkLaneBins], const uint32_t *tab,
                                                         int lane, uint32_t gstar) {
    TopkLaneClass p = {0, 0, kTopkLevels, -1};
#pragma unroll
    for (int i = 0; i < kTopkLaneBins; i++) {
        const int j = topk_lane_level(lane, i);
        if (j < 0) continue;
        const uint32_t g = topk_g(tab, (uint32_t)j);
        p.above += g > gstar ? hv[i] : 0;
        if (g == gstar) {
            p.ties += hv[i];
            p.lo = j < p.lo ? j : p.lo;
            p.hi = j > p.hi ? j : p.hi;
        }
    }
    return p;
}
inline TopkCut topk_threshold_lanes(const uint32_t *hist, const uint32_t *tab, int k) {
    uint32_t hv[64][kTopkLaneBins], incl[64];
    uint32_t run = 0;
    for (int l = 0; l < 64; l++) {
        for (int i = 0; i < kTopkLaneBins; i++) {
            const int j = topk_lane_level(l, i);
            hv[l][i] = j >= 0 ? hist[j] : 0;
            run += hv[l][i];
        }
        incl[l] = run;
    }
    int js = -1;
    for (int l = 0; l < 64; l++) {
        const uint32_t excl = l ? incl[l - 1] : 0;
        if (excl < (uint32_t)k && incl[l] >= (uint32_t)k) js = topk_lane_find(hv[l], l, excl, (uint32_t)k);
    }
    TopkCut c = {kTopkLevels, -1, 0, 0, 0};
    if (js < 0) return c;                                     // (fewer than k entries: no row has that)
    const uint32_t gstar = topk_g(tab, (uint32_t)js);
    for (int l = 0; l < 64; l++) {
        const TopkLaneClass p = topk_lane_class(hv[l], tab, l, gstar);
        c.above += p.above;
        c.ties += p.ties;
        c.jlo = p.lo < c.jlo ? p.lo : c.jlo;
        c.jhi = p.hi > c.jhi ? p.hi : c.jhi;
    }
    c.r = (uint32_t)k - c.above;
    return c;
}

// ------------------------------------------------------------------ one entry: its rank
// `ties_before` and `above_before`: the ties / heavier entries before it in symbol order
__host__ __device__ inline bool topk_is_above(uint32_t j, int jhi) { return (int)j > jhi; }
__host__ __device__ inline bool topk_is_tie(uint32_t j, int jlo, int jhi) { return (int)j >= jlo && (int)j <= jhi; }
__host__ __device__ inline bool topk_take(bool above, bool tie, uint32_t ties_before, uint32_t r) {
    return above || (tie && ties_before < r);
}
__host__ __device__ inline uint32_t topk_slot(uint32_t above_before, uint32_t ties_before, uint32_t r) {
    return above_before + (ties_before < r ? ties_before : r);
}
// A lane's counts of one 16-B vector, packed: ties in the low half, heavier entries in the high
// half.  A lane holds at most 8 entries per vector and 16 vectors, a wave 64 lanes: every sum of a
// wave's counts stays below 2^16 per half.
constexpr uint32_t kTopkAboveOne = 1u << 16;
__host__ __device__ inline uint32_t topk_pack(uint32_t j, int jlo, int jhi) {
    return topk_is_above(j, jhi) ? kTopkAboveOne : (topk_is_tie(j, jlo, jhi) ? 1u : 0u);
}
__host__ __device__ inline uint32_t topk_pack_ties(uint32_t p) { return p & 0xFFFFu; }
__host__ __device__ inline uint32_t topk_pack_above(uint32_t p) { return p >> 16; }

// ------------------------------------------------------------------ the form and its layout
// registers: the row's vectors are loaded once into the workgroup's registers (R = 8 or 16 per
// thread), rows of at most 16384 vectors.  streamed: the same algorithm in tiles of threads x 8
// vectors over three passes; any row, sized for about four tiles.  In both, vector
// tile * threads * R + w * 64 R + 64 j + l is register j of lane l of wave w: symbol order is
// tile, wave, register round, lane, entry.
struct TopkPlan {
    int rc;                                                   // LAC_E_ARG: a forced form that cannot hold the row
    int form, R, threads, tiles;
};
inline TopkPlan topk_plan(int64_t V, int type_bytes, int forced) {
    TopkPlan p = {LAC_OK, forced, 0, 0, 1};
    const int64_t nvec = V / (16 / type_bytes);
    const bool fits = nvec >= 1 && nvec <= kTopkRegMaxVec;
    if (forced == TOPK_FORM_AUTO) p.form = fits ? TOPK_FORM_REGS : TOPK_FORM_STREAM;
    if (nvec < 1 || nvec > (int64_t)1 << 28 || (p.form == TOPK_FORM_REGS && !fits) ||
        (p.form != TOPK_FORM_REGS && p.form != TOPK_FORM_STREAM)) {
        p.rc = LAC_E_ARG;
        return p;
    }
    auto waves64 = [](int64_t thr) {
        thr = (thr + 63) / 64 * 64;
        return (int)(thr < 64 ? 64 : thr > kTopkMaxThreads ? kTopkMaxThreads : thr);
    };
    if (p.form == TOPK_FORM_REGS) {
        p.R = nvec <= 8 * kTopkMaxThreads ? 8 : 16;
        p.threads = waves64((nvec + p.R - 1) / p.R);
    } else {
        p.R = kTopkStreamR;
        p.threads = waves64((nvec + 4 * p.R - 1) / (4 * p.R));
        p.tiles = (int)((nvec + (int64_t)p.threads * p.R - 1) / ((int64_t)p.threads * p.R));
    }
    return p;
}
// the first symbol after each kind of seam of a plan: thread (one vector), register round (64
// vectors), wave (64 R vectors), tile (threads x R vectors)
inline void topk_seams(const TopkPlan &p, int type_bytes, int64_t out[4]) {
    const int64_t n = 16 / type_bytes;
    out[0] = n;
    out[1] = 64 * n;
    out[2] = 64 * (int64_t)p.R * n;
    out[3] = (int64_t)p.threads * p.R * n;
}

// ================================================================== whole rows on the host
inline float topk_row_c(const void *row, int type_bytes, int64_t V) {
    float m = -INFINITY;
    for (int64_t i = 0; i < V; i++) m = fmaxf(m, topk_load(row, type_bytes, i));
    return topk_c(m);
}
inline void topk_row_pads(int k, int K, int32_t *idx_out, uint32_t *wt_out) {
    for (int s = k; s < K; s++) {
        idx_out[s] = -1;
        wt_out[s] = 0;
    }
}
// The rule written literally: every weight, the k largest with the lower symbol first among
// equals, in symbol order.
inline void topk_row_literal(const void *row, int type_bytes, int64_t V, const uint32_t *tab, int k, int weight_bits,
                             int K, int32_t *idx_out, uint32_t *wt_out) {
    const float c = topk_row_c(row, type_bytes, V);
    std::vector<uint32_t> g((size_t)V);
    std::vector<int32_t> order((size_t)V);
    for (int64_t i = 0; i < V; i++) {
        g[(size_t)i] = topk_g(tab, topk_level(topk_load(row, type_bytes, i), c));
        order[(size_t)i] = (int32_t)i;
    }
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return g[(size_t)a] > g[(size_t)b]; });
    std::sort(order.begin(), order.begin() + k);
    for (int s = 0; s < k; s++) {
        idx_out[s] = order[(size_t)s];
        wt_out[s] = topk_wt(g[(size_t)order[(size_t)s]], weight_bits);
    }
    topk_row_pads(k, K, idx_out, wt_out);
}
// The kernels' form: the level histogram, the threshold by the lanes, then the plan's tiles, waves,
// register rounds and lanes in order, each lane placing its entries from the prefix counts of
// everything before it.  Slots nobody writes keep `fill` (the caller's sentinel).
inline void topk_row_lanes(const void *row, int type_bytes, int64_t V, const uint32_t *tab, const TopkPlan &p, int k,
                           int weight_bits, int K, int32_t *idx_out, uint32_t *wt_out) {
    const int n = 16 / type_bytes, nw = p.threads / 64;
    const int64_t nvec = V / n;
    const float c = topk_row_c(row, type_bytes, V);
    uint32_t hist[kTopkLevels] = {0};
    for (int64_t i = 0; i < V; i++) hist[topk_level(topk_load(row, type_bytes, i), c)]++;
    const TopkCut cut = topk_threshold_lanes(hist, tab, k);
    uint32_t base_t = 0, base_a = 0;                          // ties / heavier entries before the tile
    for (int tile = 0; tile < p.tiles; tile++) {
        uint32_t pre_t = base_t, pre_a = base_a;              // ... before the wave, then before the round
        for (int w = 0; w < nw; w++) {
            for (int j = 0; j < p.R; j++) {
                uint32_t excl = 0;                            // the round's exclusive scan over lanes, packed
                for (int l = 0; l < 64; l++) {
                    const int64_t vi = (int64_t)tile * p.threads * p.R + (int64_t)w * 64 * p.R + 64 * j + l;
                    if (vi >= nvec) continue;
                    uint32_t tb = pre_t + topk_pack_ties(excl), ab = pre_a + topk_pack_above(excl), cnt = 0;
                    for (int e = 0; e < n; e++) {
                        const int64_t s = vi * n + e;
                        const uint32_t lv = topk_level(topk_load(row, type_bytes, s), c);
                        const bool above = topk_is_above(lv, cut.jhi), tie = topk_is_tie(lv, cut.jlo, cut.jhi);
                        if (topk_take(above, tie, tb, cut.r)) {
                            const uint32_t pos = topk_slot(ab, tb, cut.r);
                            if (pos < (uint32_t)k) {
                                idx_out[pos] = (int32_t)s;
                                wt_out[pos] = topk_wt(topk_g(tab, lv), weight_bits);
                            }
                        }
                        tb += tie ? 1 : 0;
                        ab += above ? 1 : 0;
                        cnt += topk_pack(lv, cut.jlo, cut.jhi);
                    }
                    excl += cnt;
                }
                pre_t += topk_pack_ties(excl);
                pre_a += topk_pack_above(excl);
            }
        }
        base_t = pre_t;
        base_a = pre_a;
        if (topk_slot(base_a, base_t, cut.r) >= (uint32_t)k) break;   // every survivor is placed
    }
    topk_row_pads(k, K, idx_out, wt_out);
}

}  // namespace lac
