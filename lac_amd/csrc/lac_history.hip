// lac_history.hip -- match-history models (include/lac.h lac_hist_*; the reference's History
// predictor, arith_code.py:364-398): the table of step t is built from the longest recent
// matches in a ring of the last P symbols, so each row depends on every symbol before it -- and
// the kernels keep the ring and the match lengths in the wave, build each step's row from them,
// code, and move them: one launch each way for a job of any length.  The bit format, the
// registers and every per-stream error are those of the pmf path on the rows the ring produces
// (lac_history.h): the coder chains are lac_dev.h's coder_step and lac_dec_dev.h's divisions
// and renormalisation, as they are.
//
//   k_hist_encode  one wave per stream (one wave per workgroup), any number of steps: lane k owns
//                  lags k, k + 64, ... (<= 4): per step it reads p_i from the ring in LDS, takes
//                  r_i = min(P - i - 1, M_i) from its registers and loads L[i][r_i].  The row is 1
//                  everywhere but at the <= P symbols p_i, so lo, hi and T are three wave sums of
//                  the lanes' weights (below s, at s, all) and need no row; the smallest entry is
//                  pmf[0] == 1 always.  A u32 context adds the weights into a 64-bit LDS row
//                  (LDS adds), and each lane reads back the entries it added to for one >= 2^32;
//                  a step that fudges adds them too and writes the row out for the fudged scans.
//                  The lanes that added clear what they added.
//   k_hist_decode  the same pairs, always added into the LDS row; the search is the count
//                  kernels' in-register inclusive scan over the row read back from LDS
//
// Writer and reader of the LDS row and of the scratch row are the same wave: a workgroup barrier
// (one wave: it orders the compiler, the LDS queue is in order anyway) between the adds and the
// reads, __threadfence_block() behind the scratch row.
#include "lac_host.h"
#include "lac_dec_dev.h"

namespace {

constexpr int kHistLags = kHistMaxPast / 64;   // lags per lane

struct HistDev {                      // the model and the streams' state as the kernels take them
    const uint64_t *L;                // [P][P]
    int32_t *ring;                    // [B][P]
    int32_t *pasti;                   // [B]
    int32_t *M;                       // [B][P] derived: the match lengths of ring / pasti
    void *scratch;                    // [B][Vc] entries: the row of a step that fudges
    int64_t Vc;                       // V rounded up to 4: the LDS row's u64 entries, the scratch row's entries
    int P;
};

// A stream's model state in its wave: the ring in LDS, M and the step's pairs in registers.
struct HistWave {
    int32_t *ring;                    // LDS [P]
    uint64_t *row;                    // LDS [Vc]: the sums of the weights per symbol, 0 between steps
    int32_t M[kHistLags];
    int32_t p[kHistLags];             // the step's p_i (-1 for a lag >= P)
    uint64_t wt[kHistLags];           // the step's L[i][r_i], 0 where p_i gains no weight
    int pasti;                        // wave-uniform
};

__device__ inline bool hist_live(int32_t p, int64_t V) { return p > 0 && p < V; }

__device__ inline void hist_wave_load(HistWave &h, const HistDev &m, int64_t b, uint64_t *smem, int lane) {
    h.row = smem;
    h.ring = reinterpret_cast<int32_t *>(smem + m.Vc);
    for (int64_t e = lane; e < m.Vc; e += 64) h.row[e] = 0;
#pragma unroll
    for (int q = 0; q < kHistLags; q++) {
        const int i = lane + 64 * q;
        h.M[q] = 0;
        if (i < m.P) {
            h.ring[i] = m.ring[b * m.P + i];
            h.M[q] = m.M[b * m.P + i];
        }
    }
    h.pasti = __builtin_amdgcn_readfirstlane(m.pasti[b]);
    __syncthreads();
}
__device__ inline void hist_wave_store(const HistWave &h, const HistDev &m, int64_t b, int lane) {
#pragma unroll
    for (int q = 0; q < kHistLags; q++) {
        const int i = lane + 64 * q;
        if (i < m.P) {
            m.ring[b * m.P + i] = h.ring[i];
            m.M[b * m.P + i] = h.M[q];
        }
    }
    if (lane == 0) m.pasti[b] = h.pasti;
}
// the step's pairs (lac_history.h): the loads from L are per-lane addresses, vector loads
__device__ inline void hist_pairs(HistWave &h, const HistDev &m, int64_t V, int lane) {
#pragma unroll
    for (int q = 0; q < kHistLags; q++) {
        const int i = lane + 64 * q;
        h.p[q] = -1;
        h.wt[q] = 0;
        if (i < m.P) {
            int at = h.pasti - 1 - i;
            at += at < 0 ? m.P : 0;
            h.p[q] = h.ring[at];
            const int clamp = m.P - i - 1;
            const int r = h.M[q] < clamp ? h.M[q] : clamp;
            if (hist_live(h.p[q], V)) h.wt[q] = m.L[(int64_t)i * m.P + r];
        }
    }
}
// the weights into the LDS row / out of it again, by the lanes that own them
__device__ inline void hist_row_add(const HistWave &h, int64_t V) {
#pragma unroll
    for (int q = 0; q < kHistLags; q++)
        if (hist_live(h.p[q], V))
            __hip_atomic_fetch_add(&h.row[h.p[q]], h.wt[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
}
__device__ inline void hist_row_clear(const HistWave &h, int64_t V) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kHistLags; q++)
        if (hist_live(h.p[q], V)) h.row[h.p[q]] = 0;
    __syncthreads();
}
// accept(s): every lag's match length, then the ring
__device__ inline void hist_accept_wave(HistWave &h, const HistDev &m, int32_t s, int lane) {
#pragma unroll
    for (int q = 0; q < kHistLags; q++) h.M[q] = hist_m_next(h.M[q], h.p[q], s, m.P);
    if (lane == 0) h.ring[h.pasti] = s;
    h.pasti = h.pasti + 1 == m.P ? 0 : h.pasti + 1;
    __syncthreads();
}

// One pass of the row from LDS: this lane's VEC entries from entry e0 on (mine: e0 < Vc),
// x = 1 + the weights for the entries below V and 0 past them.
template <int VEC>
__device__ inline void hist_pass(const uint64_t *row, int64_t e0, bool mine, int64_t V, uint64_t (&x)[VEC]) {
    const int64_t ec = mine ? e0 : 0;
#pragma unroll
    for (int j = 0; j < VEC; j++) {
        const uint64_t y = 1 + row[ec + j];
        x[j] = (mine && e0 + j < V) ? y : 0;
    }
}

// The row of the current step (the weights are in the LDS row) into the stream's scratch row,
// zero-padded to whole vectors, for the fudged scans
template <typename E>
__device__ inline void hist_materialise(const HistWave &h, int64_t Vc, int64_t V, E *scr, int lane) {
    constexpr int VEC = 16 / sizeof(E);
    typedef typename VecT<E, VEC>::type VT;
    for (int64_t r0 = 0; r0 < Vc; r0 += 64 * VEC) {
        const int64_t e0 = r0 + (int64_t)lane * VEC;
        const bool mine = e0 < Vc;
        uint64_t x[VEC];
        hist_pass<VEC>(h.row, e0, mine, V, x);
        VT xv;
#pragma unroll
        for (int j = 0; j < VEC; j++) xv[j] = (E)x[j];
        if (mine) *reinterpret_cast<VT *>(scr + e0) = xv;
    }
    __threadfence_block();                                    // the same wave reads it back
}

// ------------------------------------------------------------------ encode
template <typename E>
__global__ __launch_bounds__(64) void k_hist_encode(const HistDev m, const int32_t *__restrict__ sym, int64_t B,
                                                    int64_t nsteps, int64_t V, int prec, EncState *states,
                                                    uint64_t *planeA, uint64_t *planeC, uint64_t cap_words,
                                                    uint64_t *trace, const int64_t *__restrict__ slen) {
    extern __shared__ uint64_t hist_smem[];
    const int lane = (int)lane_id();
    const int64_t b = (int64_t)blockIdx.x;
    if (b >= B) return;
    EncState st = states[b];
    if (slen) {
        nsteps = live_steps(slen, b, st.nsym, nsteps);
        if (nsteps == 0) return;
    }
    if (st.err || st.nflush >= 0) {                           // (k_encode's rule for a failed or finished stream)
        if (lane == 0 && !st.err && st.nflush >= 0) { st.err = LAC_E_STATE; st.err_step = st.nsym; states[b] = st; }
        return;
    }
    uint64_t *pa = planeA + (uint64_t)b * cap_words, *pc = planeC + (uint64_t)b * cap_words;
    // the registers and plane words wave-uniform (SGPRs): the chain runs on the scalar unit
    int64_t l = (int64_t)rfl_u64((uint64_t)st.l), h = (int64_t)rfl_u64((uint64_t)st.h);
    st.L = rfl_u64(st.L);
    st.wa = rfl_u64(st.wa);
    st.wc = rfl_u64(st.wc);
    st.nsym = (int64_t)rfl_u64((uint64_t)st.nsym);
    E *scr = (E *)m.scratch + b * m.Vc;
    HistWave hw;
    hist_wave_load(hw, m, b, hist_smem, lane);
    bool ok = true;
    for (int64_t g0 = 0; g0 < nsteps && ok; g0 += 64) {
        const int n = (int)((nsteps - g0) < 64 ? (nsteps - g0) : 64);
        const int32_t mys = sym[(g0 + (lane < n ? lane : n - 1)) * B + b];
        for (int i = 0; i < n; i++) {
            const int32_t s = __builtin_amdgcn_readlane(mys, i);
            const bool sym_ok = (uint32_t)s < (uint32_t)V;
            const int32_t sc = sym_ok ? s : 0;
            hist_pairs(hw, m, V, lane);
            // the row is 1 + the weights at the p_i: the sums below s, at s and of all of them
            uint64_t below = 0, at = 0, all = 0;
#pragma unroll
            for (int q = 0; q < kHistLags; q++) {
                below += hw.p[q] < sc ? hw.wt[q] : 0;         // (wt is 0 wherever p gains no weight)
                at += hw.p[q] == sc ? hw.wt[q] : 0;
                all += hw.wt[q];
            }
            const uint64_t lo = (uint64_t)sc + rfl_u64(wave_sum_u64(below));
            const uint64_t hi = lo + 1 + rfl_u64(wave_sum_u64(at));
            uint64_t T = (uint64_t)V + rfl_u64(wave_sum_u64(all));   // < 2^57 (lac_history.h)
            const uint64_t w = (uint64_t)(h - l + 1);
            bool added = false;
            if constexpr (sizeof(E) == 4) {                   // an entry that does not fit: LAC_E_TABLE
                hist_row_add(hw, V);
                added = true;
                bool bad = false;
#pragma unroll
                for (int q = 0; q < kHistLags; q++)
                    if (hist_live(hw.p[q], V)) bad |= ((1 + hw.row[hw.p[q]]) >> 32) != 0;
                if (__ballot(bad)) T = 0;
            }
            // the fudge test itself (T > w minp, minp = pmf[0] = 1), handed to coder_step as its threshold
            const bool fudged = T != 0 && is_fudged(T, w, 1);
            if (fudged && sym_ok) {
                if (!added) hist_row_add(hw, V);
                added = true;
                hist_materialise<E>(hw, m.Vc, V, scr, lane);
            }
            const bool stepped = coder_step<E, true>(st, l, h, lo, hi, T, 1, s, scr, V, prec, pa, pc, cap_words,
                                                     trace ? trace + 2 * ((g0 + i) * B + b) : nullptr, lane,
                                                     LAC_MAP_CEIL, 0.0, true, kNoFrac, kNoFrac,
                                                     fudged ? kFsmThrCap : 0);
            if (added) hist_row_clear(hw, V);
            if (!stepped) {
                ok = false;                                   // a failed step moves neither the ring nor M
                break;
            }
            hist_accept_wave(hw, m, s, lane);
        }
    }
    if (lane == 0) store_state(st, l, h, pa, pc, cap_words, &states[b]);
    hist_wave_store(hw, m, b, lane);
}

// ------------------------------------------------------------------ decode
// decode_symbol (lac_dec_dev.h) with the row read from the LDS sums and the search on its
// in-register scan: the targets, the ranges, the determined test, the stop and the
// renormalisation are its uniform forms.  (A deliberate copy of count_decode_symbol's frame,
// for the reason given at fsm_decode_symbol.)  The weights are in the LDS row when it is called.
template <typename E>
__device__ inline int hist_decode_symbol(DecState &st, const HistWave &hw, int64_t Vc, E *scr, int64_t V, int prec,
                                         const uint8_t *bits, uint64_t nbits, int64_t *s_out, bool stop_undet) {
    constexpr int VEC = 16 / sizeof(E);
    const int lane = (int)lane_id();
    const BitWin win = bit_window(bits, nbits, st.pos);
    const bool one = Vc <= 64 * VEC;                          // one pass: the row stays in registers
    uint64_t x[VEC];
    uint64_t T = 0;
    bool bad = false;
    for (int64_t r0 = 0; r0 < Vc; r0 += 64 * VEC) {
        const int64_t e0 = r0 + (int64_t)lane * VEC;
        const bool mine = e0 < Vc;
        hist_pass<VEC>(hw.row, e0, mine, V, x);
        uint64_t ls = 0;
#pragma unroll
        for (int j = 0; j < VEC; j++) {
            ls += x[j];
            if constexpr (sizeof(E) == 4) bad |= (x[j] >> 32) != 0;
        }
        T += wave_sum_u64(ls);                                // < 2^57 (lac_history.h)
    }
    if (__ballot(bad)) T = 0;
    if (T == 0) return LAC_E_TABLE;
    const uint64_t minp = 1;                                  // pmf[0]
    const int64_t l = st.l, h = st.h, xx = st.x;
    if (xx < l || xx > h) return LAC_E_DECODE_RANGE;          // corrupted state / bits
    const uint64_t w = (uint64_t)(h - l + 1), v = (uint64_t)(xx - l);
    int64_t s = -1;
    uint64_t a = 0, bb = 0;
    const uint64_t past = st.pos > nbits ? st.pos - nbits : 0;
    const int u = past < (uint64_t)prec ? (int)past : prec;
    const uint64_t vhi = v + ((1ull << u) - 1);
    bool det;
    if (!is_fudged(T, w, minp)) {                             // not fudged (arith_code.py:84)
        uint64_t tgt, thi;
        const bool small = T < kSmallQuot && prec <= 50;
        if (small) {
            const double iw = recip2_small(w);
            tgt = div_small_u(v, T, 0, w, iw);
            thi = vhi == v ? tgt : (vhi < w ? div_small_u(vhi, T, 0, w, iw) : 0);
        } else {
            div_pair(v, vhi < w ? vhi : 0, T, 0, w, recip(w), &tgt, &thi);   // tgt < T
        }
        // the first lane whose entries end past the target holds the crossing; its count of
        // entries <= tgt and the bracket c_{s-1}, c_s are read out of it
        uint64_t lo_c = 0, hi_c = 0, cb = 0;
        bool found = false;
        for (int64_t r0 = 0; r0 < Vc && !found; r0 += 64 * VEC) {
            const int64_t e0 = r0 + (int64_t)lane * VEC;
            const bool mine = e0 < Vc;
            if (!one) hist_pass<VEC>(hw.row, e0, mine, V, x);
            uint64_t loc[VEC], ls = 0;
#pragma unroll
            for (int j = 0; j < VEC; j++) { ls += x[j]; loc[j] = ls; }
            const uint64_t in = wave_incl_scan_u64(ls);
            const uint64_t ex = cb + in - ls;
            const uint64_t mask = __ballot(mine && ex + ls > tgt);
            if (mask) {
                const int Ln = __ffsll((unsigned long long)mask) - 1;
                int k = 0;
                uint64_t lo_in = ex, hi_in = ~0ull;
#pragma unroll
                for (int j = 0; j < VEC; j++) {
                    const uint64_t ce = ex + loc[j];
                    const bool le = ce <= tgt;
                    k += le ? 1 : 0;
                    lo_in = le ? ce : lo_in;
                    hi_in = (!le && ce < hi_in) ? ce : hi_in;
                }
                const int kL = __builtin_amdgcn_readlane(k, Ln);
                s = r0 + (int64_t)Ln * VEC + kL;
                lo_c = readlane_u64(lo_in, Ln);
                hi_c = readlane_u64(hi_in, Ln);
                found = true;
            } else {
                cb += readlane_u64(in, 63);
            }
        }
        if (!found || s >= V) return LAC_E_DECODE_RANGE;
        const uint64_t add = T - 1;
        if (small) div_small_u2(lo_c, hi_c, w, add, T, recip2_small(T), &a, &bb);
        else div_pair(lo_c, hi_c, w, add, T, recip(T), &a, &bb);
        det = vhi < w && thi < hi_c;                          // bisect_right(cdf, t_hi) == s
    } else {
        hist_materialise<E>(hw, Vc, V, scr, lane);
        const int e = decode_fudged<E>(scr, V, w, v, T, &s, &a, &bb);
        if (e) return e;
        a = rfl_u64(a);
        bb = rfl_u64(bb);
        s = (int64_t)rfl_u64((uint64_t)s);
        if ((uint64_t)s >= (uint64_t)V) return LAC_E_DECODE_RANGE;
        det = vhi < bb;                                       // f_s > v_hi
    }
    if (stop_undet && !det) return LAC_E_UNDETERMINED;        // LAC_OPT_DECODE_STOP
    if (st.det && det) st.ndet++;
    else st.det = 0;
    *s_out = s;
    return decode_advance_nb(st, a, bb, win, nbits, prec);
}

template <typename E>
__global__ __launch_bounds__(64) void k_hist_decode(const HistDev m, int64_t nsteps, int64_t V, int prec,
                                                    DecState *states, const uint8_t *bits, uint64_t stride,
                                                    const uint64_t *nbits, int32_t *sym_out, int64_t B,
                                                    int stop_undet, const int64_t *__restrict__ slen) {
    extern __shared__ uint64_t hist_smem[];
    const int lane = (int)lane_id();
    const int64_t b = (int64_t)blockIdx.x;
    if (b >= B) return;
    DecState st = states[b];
    dec_state_uniform(st);
    const uint8_t *mybits = bits + b * stride;
    const uint64_t mynbits = nbits[b];
    int64_t iend = nsteps;
    if (slen) {                                               // per-stream counts: -1 for the steps past them
        iend = live_steps(slen, b, st.nsym, iend);
        for (int64_t j = iend + lane; j < nsteps; j += 64) sym_out[j * B + b] = -1;
        if (iend == 0) return;
    }
    E *scr = (E *)m.scratch + b * m.Vc;
    HistWave hw;
    hist_wave_load(hw, m, b, hist_smem, lane);
    for (int64_t i = 0; i < iend; i++) {
        dec_state_uniform(st);                                // (the loop's phis are not seen as uniform)
        if (st.err) {                                         // failed or stopped: -1 for the rest, 64 at once
            for (int64_t j = i + lane; j < nsteps; j += 64) sym_out[j * B + b] = -1;
            break;
        }
        int64_t s = -1;
        hist_pairs(hw, m, V, lane);
        hist_row_add(hw, V);
        const int err = hist_decode_symbol<E>(st, hw, m.Vc, scr, V, prec, mybits, mynbits, &s, stop_undet != 0);
        hist_row_clear(hw, V);
        if (err) {
            st.err = err;                                     // a failed step moves neither the ring nor M
            st.err_step = st.nsym;
        } else {
            hist_accept_wave(hw, m, (int32_t)s, lane);
        }
        if (lane == 0) sym_out[i * B + b] = err ? -1 : (int32_t)s;
    }
    if (lane == 0) states[b] = st;
    hist_wave_store(hw, m, b, lane);
}

// ------------------------------------------------------------------ state
// whether a state lac_hist_set_state was handed is one (lac_history.h hist_state_ok): *flag != 0 if not
__global__ void k_hist_check(const int32_t *__restrict__ ring, const int32_t *__restrict__ pasti, int64_t B, int P,
                             int64_t V, int *flag) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * P) return;
    bool bad = ring && !hist_entry_ok(ring[t], V);
    if (pasti && t < B) bad |= pasti[t] < 0 || pasti[t] >= P;
    if (bad) atomicOr(flag, 1);
}
// M from ring and pasti by the literal rule, one thread per lag
__global__ void k_hist_rebuild(const int32_t *__restrict__ ring, const int32_t *__restrict__ pasti, int64_t B, int P,
                               int32_t *M) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * P) return;
    const int64_t b = t / P;
    const int i = (int)(t - b * P);
    const int32_t *r = ring + b * P;
    const int at = pasti[b];
    int run = 0;
    for (int j = 1; j < P - i; j++) {
        int x = at - 1 - i - j, y = at - j;
        x += x < 0 ? P : 0;                                   // (>= -P: i + j <= P - 1)
        y += y < 0 ? P : 0;
        if (r[x] != r[y]) break;
        run++;
    }
    M[t] = run;
}

HistDev hist_dev(const lac_ctx *c) {
    HistDev m;
    m.L = c->hist_L;
    m.ring = c->hist_ring;
    m.pasti = c->hist_pasti;
    m.M = c->hist_M;
    m.scratch = c->hist_row;
    m.Vc = (c->V + 3) / 4 * 4;
    m.P = c->hist_P;
    return m;
}
size_t hist_lds_bytes(const lac_ctx *c) { return sizeof(uint64_t) * (size_t)((c->V + 3) / 4 * 4) + sizeof(int32_t) * (size_t)c->hist_P; }

// what every call on a loaded model checks first
int hist_loaded(lac_ctx *c) {
    if (!c) return fail(LAC_E_ARG, "ctx is NULL");
    if (!c->hist_L) return fail(LAC_E_STATE, "no history model: call lac_hist_load first");
    return LAC_OK;
}
int hist_ready(lac_ctx *c, int64_t steps) {
    const int rc = hist_loaded(c);
    if (rc) return rc;
    if (c->mapping != LAC_MAP_CEIL)
        return fail(LAC_E_STATE, "history models use the ceil mapping (the reference's History is a CDFPredictor)");
    if (steps < 0) return fail(LAC_E_ARG, "negative steps");
    return LAC_OK;
}
int hist_rebuild_launch(lac_ctx *c, hipStream_t st) {
    const int64_t n = c->B * c->hist_P;
    k_hist_rebuild<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(c->hist_ring, c->hist_pasti, c->B, c->hist_P, c->hist_M);
    CHECK_LAUNCH();
    return LAC_OK;
}

}  // namespace

extern "C" {

int lac_hist_load(lac_ctx *c, int P, const uint64_t *weights_host, void *stream) {
    if (!c || !weights_host) return fail(LAC_E_ARG, "NULL argument");
    if (!hist_limits_ok(c->V, P))
        return fail(LAC_E_ARG, "history model of %d past symbols over %lld symbols: 1 <= P <= %d and V <= %lld", P,
                    (long long)c->V, kHistMaxPast, (long long)kHistMaxVocab);
    if (!hist_weights_ok(weights_host, P)) return fail(LAC_E_ARG, "a weight >= 2^48");
    if (c->mapping != LAC_MAP_CEIL)
        return fail(LAC_E_ARG, "history models use the ceil mapping (the reference's History is a CDFPredictor)");
    if ((c->mode == 0 && c->open) || (c->mode == 1 && c->fsm_busy))
        return fail(LAC_E_STATE, "a job is in progress: load a model between jobs");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = S(stream);
    const int64_t Vc = (c->V + 3) / 4 * 4;
    const size_t nl = sizeof(uint64_t) * (size_t)P * (size_t)P;
    const size_t nr = sizeof(int32_t) * (size_t)c->B * (size_t)P;
    const size_t np = sizeof(int32_t) * (size_t)c->B;
    const size_t ns = (size_t)(c->pmf_bits / 8) * (size_t)c->B * (size_t)Vc;
    uint64_t *L = nullptr;
    int32_t *ring = nullptr, *pasti = nullptr, *M = nullptr;
    void *row = nullptr;
    int *flag = nullptr;
    auto drop = [&](int rc) {
        (void)hipFree(L); (void)hipFree(ring); (void)hipFree(pasti); (void)hipFree(M); (void)hipFree(row);
        (void)hipFree(flag);
        return rc;
    };
    if (hipMalloc(&L, nl) != hipSuccess || hipMalloc(&ring, nr) != hipSuccess || hipMalloc(&pasti, np) != hipSuccess ||
        hipMalloc(&M, nr) != hipSuccess || hipMalloc(&row, ns) != hipSuccess || hipMalloc(&flag, sizeof(int)) != hipSuccess)
        return drop(fail(LAC_E_HIP, "hipMalloc of %zu bytes of history state", nl + 2 * nr + np + ns));
    if (hipMemcpyAsync(L, weights_host, nl, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(ring, 0xff, nr, st) != hipSuccess || hipMemsetAsync(pasti, 0, np, st) != hipSuccess ||
        hipMemsetAsync(row, 0, ns, st) != hipSuccess || hipMemsetAsync(flag, 0, sizeof(int), st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return drop(fail(LAC_E_HIP, "upload of the history model"));
    (void)hipFree((void *)c->hist_L);                         // (synchronised above: nothing reads the old model)
    (void)hipFree(c->hist_ring);
    (void)hipFree(c->hist_pasti);
    (void)hipFree(c->hist_M);
    (void)hipFree(c->hist_row);
    (void)hipFree(c->hist_flag);
    c->hist_L = L;
    c->hist_ring = ring;
    c->hist_pasti = pasti;
    c->hist_M = M;
    c->hist_row = row;
    c->hist_flag = flag;
    c->hist_P = P;
    return hist_rebuild_launch(c, st);
}

int lac_hist_set_state(lac_ctx *c, const int32_t *ring_dev, const int32_t *pasti_dev, void *stream) {
    const int rc = hist_loaded(c);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = S(stream);
    const size_t nr = sizeof(int32_t) * (size_t)c->B * (size_t)c->hist_P;
    const size_t np = sizeof(int32_t) * (size_t)c->B;
    if (ring_dev || pasti_dev) {                              // refused as a whole, before anything is set
        const int64_t n = c->B * c->hist_P;
        int bad = 0;
        HIPCHK(hipMemsetAsync(c->hist_flag, 0, sizeof(int), st));
        k_hist_check<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(ring_dev, pasti_dev, c->B, c->hist_P, c->V, c->hist_flag);
        CHECK_LAUNCH();
        HIPCHK(hipMemcpyAsync(&bad, c->hist_flag, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (bad) return fail(LAC_E_ARG, "a ring entry outside [-1, %lld) or a pasti outside [0, %d)", (long long)c->V, c->hist_P);
    }
    if (ring_dev) HIPCHK(hipMemcpyAsync(c->hist_ring, ring_dev, nr, hipMemcpyDeviceToDevice, st));
    else HIPCHK(hipMemsetAsync(c->hist_ring, 0xff, nr, st));
    if (pasti_dev) HIPCHK(hipMemcpyAsync(c->hist_pasti, pasti_dev, np, hipMemcpyDeviceToDevice, st));
    else HIPCHK(hipMemsetAsync(c->hist_pasti, 0, np, st));
    return hist_rebuild_launch(c, st);
}

int lac_hist_get_state(lac_ctx *c, int32_t *ring_dev_out, int32_t *pasti_dev_out, void *stream) {
    const int rc = hist_loaded(c);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    const size_t nr = sizeof(int32_t) * (size_t)c->B * (size_t)c->hist_P;
    const size_t np = sizeof(int32_t) * (size_t)c->B;
    if (ring_dev_out) HIPCHK(hipMemcpyAsync(ring_dev_out, c->hist_ring, nr, hipMemcpyDeviceToDevice, S(stream)));
    if (pasti_dev_out) HIPCHK(hipMemcpyAsync(pasti_dev_out, c->hist_pasti, np, hipMemcpyDeviceToDevice, S(stream)));
    return LAC_OK;
}

int lac_hist_encode(lac_ctx *c, const int32_t *sym_dev, int64_t steps, uint64_t *trace_dev, void *stream) {
    const int rc = hist_ready(c, steps);
    if (rc) return rc;
    if (c->mode != 0) return fail(LAC_E_STATE, "context is decoding; call lac_encode_reset first");
    if (steps == 0) return LAC_OK;
    if (!sym_dev) return fail(LAC_E_ARG, "sym_dev is NULL");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = S(stream);
    const HistDev m = hist_dev(c);
    const size_t lds = hist_lds_bytes(c);
    {
        ProfScope ps(c, KID_ENCODE, st);
        if (c->pmf_bits == 32)
            k_hist_encode<uint32_t><<<(unsigned)c->B, 64, lds, st>>>(m, sym_dev, c->B, steps, c->V, c->prec, c->enc,
                                                                     c->planeA, c->planeC, c->cap_words, trace_dev,
                                                                     stream_lengths(c));
        else
            k_hist_encode<uint64_t><<<(unsigned)c->B, 64, lds, st>>>(m, sym_dev, c->B, steps, c->V, c->prec, c->enc,
                                                                     c->planeA, c->planeC, c->cap_words, trace_dev,
                                                                     stream_lengths(c));
    }
    CHECK_LAUNCH();
    enc_mark_open(c);
    return LAC_OK;
}

int lac_hist_decode(lac_ctx *c, int64_t steps, int32_t *sym_out_dev, void *stream) {
    const int rc = hist_ready(c, steps);
    if (rc) return rc;
    if (c->mode != 1) return fail(LAC_E_STATE, "call lac_decode_open first");
    if (steps == 0) return LAC_OK;
    if (!sym_out_dev) return fail(LAC_E_ARG, "sym_out_dev is NULL");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = S(stream);
    const HistDev m = hist_dev(c);
    const size_t lds = hist_lds_bytes(c);
    {
        ProfScope ps(c, KID_DECODE, st);
        if (c->pmf_bits == 32)
            k_hist_decode<uint32_t><<<(unsigned)c->B, 64, lds, st>>>(m, steps, c->V, c->prec, c->dec, c->dbits,
                                                                     c->dstride, c->dnbits, sym_out_dev, c->B,
                                                                     c->dec_stop, stream_lengths(c));
        else
            k_hist_decode<uint64_t><<<(unsigned)c->B, 64, lds, st>>>(m, steps, c->V, c->prec, c->dec, c->dbits,
                                                                     c->dstride, c->dnbits, sym_out_dev, c->B,
                                                                     c->dec_stop, stream_lengths(c));
    }
    CHECK_LAUNCH();
    c->fsm_busy = 1;
    return LAC_OK;
}

}  // extern "C"
