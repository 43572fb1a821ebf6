// lac_topk.hip -- top-k rows straight from logits (include/lac.h lac_topk_logits): one kernel reads
// each logits row once and writes its sparse form, the k heaviest q1 entries in symbol order with
// integer weights -- the rows lac_encode_sparse / lac_decode_sparse_steps take.  The rules live in
// lac_topk.h in both of their forms; this file is their device form.
//
//   k_topk<LT, R, STREAM>  one workgroup per row, grid = steps x streams.  Vector w * 64 R + 64 j + l
//                    of a tile is register j of lane l of wave w (q1_step_row's layout), so symbol
//                    order is tile, wave, register round, lane, entry.
//       registers (STREAM = false): the row's 16-B vectors are loaded once (nontemporal) and stay in
//                    registers: row maximum -> c -> levels into an LDS histogram (LDS atomics: counts
//                    are order-free; level 0, where most of a peaked row lands, is counted in
//                    registers and added once per wave) -> the threshold by wave 0 (lac_topk.h's
//                    lane form) -> each lane's packed (ties, heavier) counts per register -> the
//                    waves' totals through LDS -> per register round one wave scan, and the lanes
//                    that hold a survivor place it.  Three barriers, no second read of the row.
//       streamed (STREAM = true): the same in tiles of threads x 8 vectors over three passes
//                    (maximum, histogram, placement), one barrier per tile of the third pass; it
//                    stops at the tile that places the last survivor.
//                    Neither form uses scratch.
#include <type_traits>

#include "lac_host.h"
#include "lac_topk.h"

namespace {

__constant__ uint32_t c_topk_tab[LAC_Q1_TAB_SIZE] = LAC_Q1_TAB_INIT;

// (the q1 row primitives of lac_logits.hip, restated: that unit's kernels are left as they are)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
template <typename LT> struct TopkN { static constexpr int N = 16 / sizeof(LT); };
template <typename LT>
__device__ inline float topk_logit_at(const u32x4 &v, int j) {
    if constexpr (sizeof(LT) == 2) {
        const uint32_t w = v[j >> 1];
        return __uint_as_float((j & 1) ? (w & 0xFFFF0000u) : (w << 16));
    } else {
        return __uint_as_float(v[j]);
    }
}
template <bool NT>
__device__ inline u32x4 topk_ld16(const void *row, int vi) {
    const u32x4 *p = reinterpret_cast<const u32x4 *>(row) + vi;
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}
__device__ inline float topk_wave_max(float v) {
    auto mx = [](uint32_t a, uint32_t b) { return __float_as_uint(fmaxf(__uint_as_float(a), __uint_as_float(b))); };
    return __uint_as_float(wave_reduce(__float_as_uint(v), mx));
}
__device__ inline uint32_t topk_wave_sum(uint32_t v) {
    return wave_reduce(v, [](uint32_t a, uint32_t b) { return a + b; });
}

constexpr int kTopkWaves = kTopkMaxThreads / 64;
struct TopkShared {
    uint32_t hist[kTopkLevels];                               // entries per level
    float wmax[kTopkWaves];
    uint32_t wcnt[2][kTopkWaves];                             // the waves' packed counts of a tile (alternating)
    int jlo, jhi;                                             // the threshold (TopkCut)
    uint32_t r;
};

// The threshold search by one whole wave (lac_topk.h topk_threshold_lanes): false where the
// histogram holds fewer than k entries.
__device__ inline bool topk_wave_cut(const uint32_t *hist, uint32_t k, int lane, int *jlo, int *jhi, uint32_t *above) {
    uint32_t hv[kTopkLaneBins], ls = 0;
#pragma unroll
    for (int i = 0; i < kTopkLaneBins; i++) {
        const int j = topk_lane_level(lane, i);
        hv[i] = j >= 0 ? hist[j] : 0;
        ls += hv[i];
    }
    const uint32_t incl = wave_incl_scan_u32(ls), excl = incl - ls;
    const bool hit = excl < k && incl >= k;                   // at most one lane
    const int js = hit ? topk_lane_find(hv, lane, excl, k) : -1;
    auto imax = [](uint32_t a, uint32_t b) { return (uint32_t)((int)a > (int)b ? (int)a : (int)b); };
    const int jstar = (int)wave_reduce((uint32_t)js, imax);
    if (jstar < 0) return false;                              // wave-uniform
    const TopkLaneClass p = topk_lane_class(hv, c_topk_tab, lane, topk_g(c_topk_tab, (uint32_t)jstar));
    *above = topk_wave_sum(p.above);
    *jlo = (int)wave_min_u32((uint32_t)p.lo);
    *jhi = (int)wave_reduce((uint32_t)p.hi, imax);
    return true;
}

template <typename LT, int R, bool STREAM>
__global__ __launch_bounds__(kTopkMaxThreads) void k_topk(const LT *__restrict__ lg, int64_t step_stride,
                                                          int64_t stream_stride, int64_t B, int64_t V, int k, int weight_bits,
                                                          int K, int32_t *__restrict__ idx_out,
                                                          uint32_t *__restrict__ wt_out) {
    __shared__ TopkShared sh;
    constexpr int N = TopkN<LT>::N;
    const int lane = (int)lane_id(), w = wave_in_block(), nw = (int)(blockDim.x >> 6);
    const int64_t row_i = (int64_t)blockIdx.x;
    const LT *row = lg + (row_i / B) * step_stride + (row_i % B) * stream_stride;
    int32_t *io = idx_out + row_i * K;
    uint32_t *wo = wt_out + row_i * K;
    const int nvec = (int)(V / N), tile_vec = nw * 64 * R;
    const int ntiles = STREAM ? (nvec + tile_vec - 1) / tile_vec : 1;
    const int v0 = w * 64 * R + lane;
    u32x4 x[R];
    // a tile's vectors; lanes past the row load its last vector: a duplicate cannot change the
    // maximum, and the counts mask it (in_row)
    auto load = [&](int tile, auto nt) {
#pragma unroll
        for (int j = 0; j < R; j++) {
            const int vi = tile * tile_vec + v0 + 64 * j;
            x[j] = topk_ld16<decltype(nt)::value>(row, vi < nvec ? vi : nvec - 1);
        }
    };
    auto in_row = [&](int tile, int j) { return tile * tile_vec + v0 + 64 * j < nvec; };
    // the unpacked bf16 row is twice the registers: each pass unpacks the vectors again
    auto forget = [&]() {
#pragma unroll
        for (int j = 0; j < R; j++) asm volatile("" : "+v"(x[j]));
    };
    typedef std::integral_constant<bool, true> Once;          // nontemporal: the last read of these bytes
    typedef std::integral_constant<bool, false> Again;

    if (!STREAM) load(0, Once());
    for (int i = threadIdx.x; i < kTopkLevels; i += blockDim.x) sh.hist[i] = 0;
    for (int i = threadIdx.x; i < K - k; i += blockDim.x) {   // the pads
        io[k + i] = -1;
        wo[k + i] = 0;
    }
    // ---- the maximum (NaN ignored, +-inf kept)
    float mx = -INFINITY;
    for (int tile = 0; tile < ntiles; tile++) {
        if (STREAM) load(tile, Again());
#pragma unroll
        for (int j = 0; j < R; j++)
#pragma unroll
            for (int e = 0; e < N; e++) mx = fmaxf(mx, topk_logit_at<LT>(x[j], e));
    }
    mx = topk_wave_max(mx);
    if (lane == 0) sh.wmax[w] = mx;
    forget();
    __syncthreads();
    float m = sh.wmax[0];
    for (int i = 1; i < nw; i++) m = fmaxf(m, sh.wmax[i]);
    const float c = topk_c(m);
    // ---- the level histogram; level 0, where most of a peaked row lands, is counted in registers
    // and added once per wave
    uint32_t zeros = 0;
    for (int tile = 0; tile < ntiles; tile++) {
        if (STREAM) load(tile, Again());
#pragma unroll
        for (int j = 0; j < R; j++) {
            if (!in_row(tile, j)) continue;
#pragma unroll
            for (int e = 0; e < N; e++) {
                const uint32_t lv = topk_level(topk_logit_at<LT>(x[j], e), c);
                if (lv) atomicAdd(&sh.hist[lv], 1u);
                else zeros++;
            }
        }
    }
    zeros = topk_wave_sum(zeros);
    if (lane == 0 && zeros) atomicAdd(&sh.hist[0], zeros);
    forget();
    __syncthreads();
    // ---- the threshold, by wave 0
    if (w == 0) {
        int jlo = 0, jhi = 0;
        uint32_t above = 0;
        (void)topk_wave_cut(sh.hist, (uint32_t)k, lane, &jlo, &jhi, &above);   // (the row holds V >= k entries)
        if (lane == 0) {
            sh.jlo = jlo;
            sh.jhi = jhi;
            sh.r = (uint32_t)k - above;
        }
    }
    __syncthreads();
    const int jlo = sh.jlo, jhi = sh.jhi;
    const uint32_t r = sh.r;
    // ---- placement: every entry's prefix counts in symbol order
    uint32_t base_t = 0, base_a = 0;                          // ties / heavier entries before the tile
    for (int tile = 0, par = 0; tile < ntiles; tile++, par ^= 1) {
        if (STREAM) load(tile, Once());
        uint32_t cnt[R], tot = 0;                             // packed (lac_topk.h topk_pack)
#pragma unroll
        for (int j = 0; j < R; j++) {
            uint32_t n = 0;
            if (in_row(tile, j)) {
#pragma unroll
                for (int e = 0; e < N; e++) n += topk_pack(topk_level(topk_logit_at<LT>(x[j], e), c), jlo, jhi);
            }
            cnt[j] = n;
            tot += n;
        }
        tot = topk_wave_sum(tot);
        if (lane == 0) sh.wcnt[par][w] = tot;
        forget();
        __syncthreads();
        uint32_t pre_t = base_t, pre_a = base_a;              // ... before this wave, then before the round
        for (int i = 0; i < nw; i++) {
            const uint32_t t = sh.wcnt[par][i];
            base_t += topk_pack_ties(t);
            base_a += topk_pack_above(t);
            if (i < w) {
                pre_t += topk_pack_ties(t);
                pre_a += topk_pack_above(t);
            }
        }
#pragma unroll
        for (int j = 0; j < R; j++) {
            if (__ballot(cnt[j] != 0) == 0) continue;         // wave-uniform: most rounds hold no survivor
            const uint32_t incl = wave_incl_scan_u32(cnt[j]), excl = incl - cnt[j];
            if (cnt[j]) {
                uint32_t tb = pre_t + topk_pack_ties(excl), ab = pre_a + topk_pack_above(excl);
                const int s0 = (tile * tile_vec + v0 + 64 * j) * N;
#pragma unroll
                for (int e = 0; e < N; e++) {
                    const uint32_t lv = topk_level(topk_logit_at<LT>(x[j], e), c);
                    const bool above = topk_is_above(lv, jhi), tie = topk_is_tie(lv, jlo, jhi);
                    const uint32_t pos = topk_slot(ab, tb, r);
                    if (topk_take(above, tie, tb, r) && pos < (uint32_t)k) {
                        io[pos] = s0 + e;
                        wo[pos] = topk_wt(topk_g(c_topk_tab, lv), weight_bits);
                    }
                    tb += tie ? 1 : 0;
                    ab += above ? 1 : 0;
                }
            }
            const uint32_t seg = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            pre_t += topk_pack_ties(seg);
            pre_a += topk_pack_above(seg);
        }
        if (STREAM && topk_slot(base_a, base_t, r) >= (uint32_t)k) break;   // block-uniform: every survivor is placed
    }
}

template <typename LT>
int topk_launch(lac_ctx *c, const TopkPlan &p, const void *lg, int64_t step_stride, int64_t stream_stride, int64_t rows,
                int k, int weight_bits, int K, int32_t *idx, uint32_t *wt, hipStream_t st) {
    ProfScope ps(c, KID_Q1_STATS, st);
    const unsigned grid = (unsigned)rows, thr = (unsigned)p.threads;
#define LAC_TOPK_ARGS (const LT *)lg, step_stride, stream_stride, c->B, c->V, k, weight_bits, K, idx, wt
    if (p.form == TOPK_FORM_STREAM) k_topk<LT, kTopkStreamR, true><<<grid, thr, 0, st>>>(LAC_TOPK_ARGS);
    else if (p.R == 8) k_topk<LT, 8, false><<<grid, thr, 0, st>>>(LAC_TOPK_ARGS);
    else k_topk<LT, 16, false><<<grid, thr, 0, st>>>(LAC_TOPK_ARGS);
#undef LAC_TOPK_ARGS
    CHECK_LAUNCH();
    return LAC_OK;
}

}  // namespace

extern "C" {

int lac_topk_logits(lac_ctx *c, const void *logits_dev, int logit_type, int64_t step_stride, int64_t stream_stride,
                    int64_t steps, int k, int weight_bits, int K, int32_t *idx_out_dev, uint32_t *wt_out_dev,
                    void *stream) {
    if (!c) return fail(LAC_E_ARG, "ctx is NULL");
    const int tb = topk_type_bytes(logit_type);
    if (!tb) return fail(LAC_E_ARG, "logit type %d", logit_type);
    if (steps < 0 || step_stride < 0 || stream_stride < 0) return fail(LAC_E_ARG, "negative size/stride");
    if (!topk_k_ok(k, c->V)) return fail(LAC_E_ARG, "k = %d: between 1 and min(V, %d)", k, kTopkMaxK);
    if (!topk_slots_ok(K, k)) return fail(LAC_E_ARG, "K = %d: a multiple of 4 in [k, %d]", K, kTopkMaxK);
    if (!topk_bits_ok(weight_bits)) return fail(LAC_E_ARG, "weight_bits = %d: in [0, %d]", weight_bits, LAC_Q1_KMAX);
    if (steps == 0) return LAC_OK;
    if (!logits_dev || !idx_out_dev || !wt_out_dev) return fail(LAC_E_ARG, "NULL argument");
    if (!topk_layout_ok((uintptr_t)logits_dev, logit_type, c->V, step_stride, stream_stride))
        return fail(LAC_E_ARG, "logits rows must be 16-byte aligned with vocab and strides multiples of %d", 16 / tb);
    if (!topk_out_ok((uintptr_t)idx_out_dev) || !topk_out_ok((uintptr_t)wt_out_dev))
        return fail(LAC_E_ARG, "idx_out_dev and wt_out_dev must be 16-byte aligned");
    const TopkPlan p = topk_plan(c->V, tb, c->topk_form);
    if (p.rc) return fail(p.rc, "top-k form %d cannot hold a row of %lld entries", c->topk_form, (long long)c->V);
    const int64_t rows = steps * c->B;
    if (steps > INT32_MAX / c->B) return fail(LAC_E_ARG, "steps x streams above 2^31 - 1");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = S(stream);
    return logit_type == LAC_LOGITS_BF16
               ? topk_launch<uint16_t>(c, p, logits_dev, step_stride, stream_stride, rows, k, weight_bits, K, idx_out_dev,
                                       wt_out_dev, st)
               : topk_launch<float>(c, p, logits_dev, step_stride, stream_stride, rows, k, weight_bits, K, idx_out_dev,
                                    wt_out_dev, st);
}

int lac_topk_form(lac_ctx *c, int logit_type) {
    if (!c) return fail(LAC_E_ARG, "ctx is NULL");
    const int tb = topk_type_bytes(logit_type);
    if (!tb || c->V % (16 / tb)) return fail(LAC_E_ARG, "logit type %d at vocab %lld", logit_type, (long long)c->V);
    const TopkPlan p = topk_plan(c->V, tb, c->topk_form);
    return p.rc ? fail(p.rc, "top-k form %d cannot hold a row of %lld entries", c->topk_form, (long long)c->V) : p.form;
}

}  // extern "C"
