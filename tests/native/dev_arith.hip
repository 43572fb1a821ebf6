// dev_arith.hip -- test infrastructure: the coder's float-assisted divisions (lac_core.h,
// lac_dec_dev.h) evaluated on the device, one case per thread (the plain __host__
// __device__ functions) or one case per wave (the wave-uniform wrappers that go through
// rfl_u64 / nonneg_uni), on arrays the harness owns.  Compiled with lac_amd.build.FLAGS,
// so contraction and optimisation match liblac.so (tests/dev_arith.py loads it and holds
// the case generators; tests/test_gpu_arith.py compares with exact Python integers).
//
// Two entry points, da_thread and da_wave: `fam` names the primitive family below, `inv`
// the reciprocal it divides with.  Each copies its host arrays in, launches one kernel,
// synchronises, copies the outputs back and returns the HIP status (-1: unknown family).
// A kernel reads in[k][i] and writes out[k][i] only, for its own case i < n.
#include "lac_host.h"
#include "lac_dec_dev.h"

namespace {

constexpr int kIn = 6, kOut = 4;
struct Args {
    const uint64_t *in[kIn];
    uint64_t *out[kOut];
    int64_t n;
};

enum { INV_RECIP = 0, INV_RECIP_SMALL = 1, INV_RECIP2_SMALL = 2, INV_IEEE = 3 };
// one case per thread
enum { T_RECIP = 0, T_RECIP_SMALL, T_F64_SMALL, T_DIV_FLOOR, T_DIV_SMALL, T_DIV_NEAR, T_DIV_MID, T_FRAC, T_RANGES,
       T_FUDGE, T_IS_FUDGED, T_CR_RATIO, T_FIX, T_COUNT };
// one case per wave
enum { W_SMALL_U = 0, W_SMALL_U2, W_NEAR_U, W_NEAR_U2, W_MID_U2, W_FRAC_UNI, W_DIV_PAIR, W_FRAC_PAIR, W_FIX, W_COUNT };

__device__ inline uint64_t bits_of(double x) { return __builtin_bit_cast(uint64_t, x); }
__device__ inline double f64_of(uint64_t b) { return __builtin_bit_cast(double, b); }

// 1/d the way the coder gets it: recip (v_rcp_f64 + Newton), recip_small (the same from the
// 2^52 magic), recip2_small (two Newton steps), or the IEEE divide k_dec_stats stores in
// its LeanMeta (1.0 / (double)T)
template <int INV>
__device__ inline double inv_of(uint64_t d) {
    if constexpr (INV == INV_RECIP) return recip(d);
    else if constexpr (INV == INV_RECIP_SMALL) return recip_small(d);
    else if constexpr (INV == INV_RECIP2_SMALL) return recip2_small(d);
    else return 1.0 / (double)d;
}

template <int FAM, int INV>
__global__ __launch_bounds__(256) void k_thread(Args a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    uint64_t x[kIn], o[kOut] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < kIn; k++) x[k] = a.in[k] ? a.in[k][i] : 0;
    if constexpr (FAM == T_RECIP) {
        o[0] = bits_of(recip(x[0]));
        o[1] = bits_of(1.0 / (double)x[0]);
        o[2] = bits_of((double)x[0]);
    } else if constexpr (FAM == T_RECIP_SMALL) {
        o[0] = bits_of(recip_small(x[0]));
        o[1] = bits_of(recip2_small(x[0]));
        o[2] = bits_of(small_to_f64(x[0]));
    } else if constexpr (FAM == T_F64_SMALL) {
        o[0] = f64_to_small(f64_of(x[0]));
    } else if constexpr (FAM == T_DIV_FLOOR) {
        const u128 N = ((u128)x[0] << 64) | x[1];
        int fix = 0;
        o[0] = div_floor(N, x[2]);
        o[1] = div_floor_inv_n(N, x[2], recip(x[2]), &fix);
        o[2] = (uint64_t)fix;
    } else if constexpr (FAM == T_DIV_SMALL) {
        const uint64_t e = div_small_est(x[0], x[1], x[2], inv_of<INV>(x[3]));
        o[0] = div_small_fix_mask(e, x[0], x[1], x[2], x[3]);
        o[1] = e;
        o[2] = div_small_fix(e, x[0], x[1], x[2], x[3]);
    } else if constexpr (FAM == T_DIV_NEAR) {
        const uint64_t e = div_small_est(x[0], x[1], x[2], inv_of<INV>(x[3]));
        o[0] = div_near_fix<false>(e, x[0], x[1], x[2], x[3]);
        o[1] = e;
        o[2] = div_near_fix<true>(e, x[0], x[1], x[2], x[3]);      // (meaningful for n < 2^32)
    } else if constexpr (FAM == T_DIV_MID) {
        const double inv = inv_of<INV>(x[3]);
        const uint64_t e = div_mid_est_w(x[0], x[1], f64_of(x[4]), inv), e2 = div_mid_est(x[0], x[1], x[2], inv);
        o[0] = div_mid_fix(e, x[0], x[1], x[2], x[3]);
        o[1] = e;
        o[2] = div_mid_fix(e2, x[0], x[1], x[2], x[3]);
        o[3] = e2;
    } else if constexpr (FAM == T_FRAC) {                         // c, w, T, ceil
        const uint64_t c = x[0], w = x[1], T = x[2];
        const bool ceil = x[3] != 0;
        const uint64_t f = row_frac(c, T);
        o[0] = f;
        o[1] = f == kNoFrac ? ~0ull : frac_mul_div<false>(f, c, w, T, ceil);
        o[2] = (f == kNoFrac || (T >> 62)) ? ~0ull : frac_mul_div<true>(f, c, w, T, ceil);
        if (f == kNoFrac || (T >> 32) || c > T) o[3] = ~0ull;
        else o[3] = ceil ? frac_mul_div32<true>(f, (uint32_t)c, w, (uint32_t)T)
                         : frac_mul_div32<false>(f, (uint32_t)c, w, (uint32_t)T);
    } else if constexpr (FAM == T_RANGES) {                       // lo, hi, T, w
        unfudged_range_inv(x[0], x[1], x[2], inv_of<INV>(x[2]), x[3], &o[0], &o[1]);
        floor_range(x[0], x[1], x[2], x[3], &o[2], &o[3]);
    } else if constexpr (FAM == T_FUDGE) {                        // i, c, j, T, w, V
        const i128 X = fudge_x(x[1], (int64_t)x[2], x[4], x[3]);
        o[0] = fudge_f((int64_t)x[0], X, x[3], x[4], (int64_t)x[5]);
        o[1] = (uint64_t)(u128)X;
        o[2] = (uint64_t)((u128)X >> 64);
    } else if constexpr (FAM == T_IS_FUDGED) {                    // T, w, minp
        o[0] = is_fudged(x[0], x[1], x[2]) ? 1 : 0;
    } else if constexpr (FAM == T_CR_RATIO) {
        o[0] = bits_of(cr_ratio(x[0], x[1]));
    } else if constexpr (FAM == T_FIX) {                          // n, m, add, d and a given estimate
        o[0] = div_small_fix_mask(x[4], x[0], x[1], x[2], x[3]);
        o[1] = div_near_fix<false>(x[4], x[0], x[1], x[2], x[3]);
        o[2] = div_near_fix<true>(x[4], x[0], x[1], x[2], x[3]);   // (meaningful for n < 2^32)
        o[3] = div_mid_fix(x[4], x[0], x[1], x[2], x[3]);
    }
#pragma unroll
    for (int k = 0; k < kOut; k++)
        if (a.out[k]) a.out[k][i] = o[k];
}

// One case per wave: all 64 lanes load the same inputs, which go to SGPRs as the decoders'
// state does (rfl_u64); lane 0 stores.
template <int FAM, int INV>
__global__ __launch_bounds__(256) void k_wave(Args a) {
    const int64_t i = (int64_t)blockIdx.x * kWavesPerBlock + wave_in_block();
    if (i >= a.n) return;
    uint64_t x[kIn], o[kOut] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < kIn; k++) x[k] = a.in[k] ? rfl_u64(a.in[k][i]) : 0;
    if constexpr (FAM == W_SMALL_U) {                             // n, m, add, d
        const double inv = inv_of<INV>(x[3]);
        o[0] = div_small_u<true>(x[0], x[1], x[2], x[3], inv);
        o[1] = rfl_u64(div_small_est(x[0], x[1], x[2], inv));
        o[2] = div_small_u<false>(x[0], x[1], x[2], x[3], inv);
    } else if constexpr (FAM == W_SMALL_U2) {                     // n0, n1, m, add, d
        const double inv = inv_of<INV>(x[4]);
        div_small_u2<true>(x[0], x[1], x[2], x[3], x[4], inv, &o[0], &o[1]);
        div_small_u2<false>(x[0], x[1], x[2], x[3], x[4], inv, &o[2], &o[3]);
    } else if constexpr (FAM == W_NEAR_U) {                       // n, m, add, d
        const double inv = inv_of<INV>(x[3]);
        o[0] = div_near_u(x[0], x[1], x[2], x[3], inv);
        o[1] = rfl_u64(div_small_est(x[0], x[1], x[2], inv));
    } else if constexpr (FAM == W_NEAR_U2) {                      // n0, n1, m, add, d
        const double inv = inv_of<INV>(x[4]);
        div_near_u2<false>(x[0], x[1], x[2], x[3], x[4], inv, &o[0], &o[1]);
        div_near_u2<true>(x[0], x[1], x[2], x[3], x[4], inv, &o[2], &o[3]);   // (meaningful for n < 2^32)
    } else if constexpr (FAM == W_MID_U2) {                       // n0, n1, m, add, d, addd (bits)
        const double inv = inv_of<INV>(x[4]), addd = f64_of(x[5]);
        div_mid_u2(x[0], x[1], x[2], x[3], addd, x[4], inv, &o[0], &o[1]);
        o[2] = rfl_u64(div_mid_est_w(x[0], x[2], addd, inv));
        o[3] = rfl_u64(div_mid_est_w(x[1], x[2], addd, inv));
    } else if constexpr (FAM == W_FRAC_UNI) {                     // c, w, T, ceil  (T < 2^62)
        const uint64_t f = rfl_u64(row_frac(x[0], x[2]));
        o[0] = f;
        o[1] = (f == kNoFrac || (x[2] >> 62)) ? ~0ull : frac_mul_div<true>(f, x[0], x[1], x[2], x[3] != 0);
    } else if constexpr (FAM == W_DIV_PAIR) {                     // n0, n1, m, add, d
        div_pair(x[0], x[1], x[2], x[3], x[4], inv_of<INV>(x[4]), &o[0], &o[1]);
    } else if constexpr (FAM == W_FRAC_PAIR) {                    // c0, c1, w, T, ceil  (T < 2^63)
        const uint64_t f0 = row_frac(x[0], x[3]), f1 = row_frac(x[1], x[3]);
        if (f0 == kNoFrac) o[0] = o[1] = ~0ull;
        else frac_pair(f0, f1, x[0], x[1], x[2], x[3], x[4] != 0, &o[0], &o[1]);
    } else if constexpr (FAM == W_FIX) {                          // n, m, add, d and a given estimate
        o[0] = div_small_fix_u<true>(x[4], x[0], x[1], x[2], x[3]);
        o[1] = div_small_fix_u<false>(x[4], x[0], x[1], x[2], x[3]);
    }
    if (lane_id() == 0) {
#pragma unroll
        for (int k = 0; k < kOut; k++)
            if (a.out[k]) a.out[k][i] = o[k];
    }
}

template <typename Launch>
int run(int64_t n, const uint64_t *const *in, uint64_t *const *out, Launch launch) {
    if (n <= 0) return 0;
    const size_t bytes = (size_t)n * 8;
    Args a;
    memset(&a, 0, sizeof a);
    a.n = n;
    hipError_t e = hipSuccess;
    auto rel = [&]() {
        for (int k = 0; k < kIn; k++) if (a.in[k]) (void)hipFree((void *)a.in[k]);
        for (int k = 0; k < kOut; k++) if (a.out[k]) (void)hipFree(a.out[k]);
    };
    for (int k = 0; k < kIn && e == hipSuccess; k++) {
        if (!in[k]) continue;
        void *p = nullptr;
        e = hipMalloc(&p, bytes);
        a.in[k] = (const uint64_t *)p;
        if (e == hipSuccess) e = hipMemcpy(p, in[k], bytes, hipMemcpyHostToDevice);
    }
    for (int k = 0; k < kOut && e == hipSuccess; k++) {
        if (!out[k]) continue;
        void *p = nullptr;
        e = hipMalloc(&p, bytes);
        a.out[k] = (uint64_t *)p;
        if (e == hipSuccess) e = hipMemset(p, 0, bytes);
    }
    if (e == hipSuccess) {
        launch(a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    for (int k = 0; k < kOut && e == hipSuccess; k++)
        if (out[k]) e = hipMemcpy(out[k], a.out[k], bytes, hipMemcpyDeviceToHost);
    rel();
    return (int)e;
}

template <int FAM, int INV>
int thread_launch(int64_t n, const uint64_t *const *in, uint64_t *const *out) {
    return run(n, in, out, [&](const Args &a) { k_thread<FAM, INV><<<(unsigned)((n + 255) / 256), 256>>>(a); });
}
template <int FAM, int INV>
int wave_launch(int64_t n, const uint64_t *const *in, uint64_t *const *out) {
    return run(n, in, out, [&](const Args &a) {
        k_wave<FAM, INV><<<(unsigned)((n + kWavesPerBlock - 1) / kWavesPerBlock), 64 * kWavesPerBlock>>>(a);
    });
}

}  // namespace

#define DA_INV(L, FAM)                                                      \
    switch (inv) {                                                          \
    case INV_RECIP: return L<FAM, INV_RECIP>(n, in, out);                   \
    case INV_RECIP_SMALL: return L<FAM, INV_RECIP_SMALL>(n, in, out);       \
    case INV_RECIP2_SMALL: return L<FAM, INV_RECIP2_SMALL>(n, in, out);     \
    case INV_IEEE: return L<FAM, INV_IEEE>(n, in, out);                     \
    default: return -1;                                                     \
    }

extern "C" {

// in: kIn pointers to n u64 each (null: zeros); out: kOut pointers (null: not wanted)
int da_thread(int fam, int inv, int64_t n, const uint64_t *const *in, uint64_t *const *out) {
    switch (fam) {
    case T_RECIP: return thread_launch<T_RECIP, 0>(n, in, out);
    case T_RECIP_SMALL: return thread_launch<T_RECIP_SMALL, 0>(n, in, out);
    case T_F64_SMALL: return thread_launch<T_F64_SMALL, 0>(n, in, out);
    case T_DIV_FLOOR: return thread_launch<T_DIV_FLOOR, 0>(n, in, out);
    case T_DIV_SMALL: DA_INV(thread_launch, T_DIV_SMALL)
    case T_DIV_NEAR: DA_INV(thread_launch, T_DIV_NEAR)
    case T_DIV_MID: DA_INV(thread_launch, T_DIV_MID)
    case T_FRAC: return thread_launch<T_FRAC, 0>(n, in, out);
    case T_RANGES: DA_INV(thread_launch, T_RANGES)
    case T_FUDGE: return thread_launch<T_FUDGE, 0>(n, in, out);
    case T_IS_FUDGED: return thread_launch<T_IS_FUDGED, 0>(n, in, out);
    case T_CR_RATIO: return thread_launch<T_CR_RATIO, 0>(n, in, out);
    case T_FIX: return thread_launch<T_FIX, 0>(n, in, out);
    default: return -1;
    }
}

int da_wave(int fam, int inv, int64_t n, const uint64_t *const *in, uint64_t *const *out) {
    switch (fam) {
    case W_SMALL_U: DA_INV(wave_launch, W_SMALL_U)
    case W_SMALL_U2: DA_INV(wave_launch, W_SMALL_U2)
    case W_NEAR_U: DA_INV(wave_launch, W_NEAR_U)
    case W_NEAR_U2: DA_INV(wave_launch, W_NEAR_U2)
    case W_MID_U2: DA_INV(wave_launch, W_MID_U2)
    case W_FRAC_UNI: return wave_launch<W_FRAC_UNI, 0>(n, in, out);
    case W_DIV_PAIR: DA_INV(wave_launch, W_DIV_PAIR)
    case W_FRAC_PAIR: return wave_launch<W_FRAC_PAIR, 0>(n, in, out);
    case W_FIX: return wave_launch<W_FIX, 0>(n, in, out);
    default: return -1;
    }
}

int da_limits(int *n_in, int *n_out) {
    *n_in = kIn;
    *n_out = kOut;
    return 0;
}

}  // extern "C"
