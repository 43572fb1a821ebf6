// lac_count.hip -- adaptive n-gram count models (include/lac.h lac_count_*; the reference's
// Markov_up_to_n predictor, arith_code.py:443-464): the table of step t is built from counts
// that every accepted symbol updates, so each row depends on every symbol before it -- and the
// kernel keeps the counts in device memory, builds each step's row from them in registers,
// codes, and updates them: one launch each way for a job of any length.  The bit format, the
// registers and every per-stream error are those of the pmf path on the rows the counts
// produce (lac_count.h): the coder chains are lac_dev.h's coder_step and lac_dec_dev.h's
// divisions and renormalisation, as they are.
//
//   k_count_encode  one wave per stream, any number of steps: per step each lane loads its own
//                   entries of the <= k count rows (lane (e / VEC) % 64 owns entry e, in passes
//                   of 64 vectors), forms 1 + sum W c in u64, one wave scan gives lo, hi and T,
//                   one min-reduce minp, then coder_step on the scalar unit, then the owning
//                   lane increments the <= k counts
//   k_count_decode  one wave per stream, all steps: the same row, the search on the in-register
//                   inclusive scan (a ballot for the lane, a count inside it)
//
// The lane that loads a count is the lane that increments it: the same context may recur on the
// very next step, and with ownership fixed by the entry index the read after the write is a
// same-thread dependence through global memory -- no fence.  The fudged branches read the row
// from memory, so a step that fudges first writes its row, zero-padded to whole vectors, to a
// per-stream scratch row; writer and reader are the same wave, so __threadfence_block() between
// them is enough.
#include "lac_host.h"
#include "lac_dec_dev.h"

namespace {

struct CountDev {                     // the model and the streams' state as the kernels take them
    uint32_t *counts;                 // [B][stride]
    int32_t *past;                    // [B][order], most recent last, -1 absent
    void *scratch;                    // [B][Vc] entries: the row of a step that fudges
    int64_t stride, Vc, off[4];
    uint32_t W[4];
    int order;
};

// 0 in a VGPR the compiler cannot see through: added to a wave-uniform index it keeps the
// load a vector load (a scalar load's wait would sit on the chain)
__device__ inline int vzero_c() {
    int z = 0;
    asm volatile("" : "+v"(z));
    return z;
}

// A stream's history, wave-uniform: q[3] the most recent symbol, m of them valid.
struct CountHist {
    int32_t q[4];
    int m;
};

__device__ inline CountHist count_hist_load(const int32_t *past, int order, int64_t V, int vz) {
    CountHist h;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int at = j - (4 - order);                       // q[j] = past[order - (4 - j)]
        h.q[j] = at >= 0 ? __builtin_amdgcn_readfirstlane(past[at + vz]) : -1;
    }
    h.m = 0;
    bool run = true;
#pragma unroll
    for (int j = 3; j >= 0; j--) {
        run = run && (uint32_t)h.q[j] < (uint32_t)V && (3 - j) < order;
        h.m += run ? 1 : 0;
    }
    return h;
}
__device__ inline void count_hist_store(const CountHist &h, int32_t *past, int order) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int at = j - (4 - order);
        if (at >= 0) past[at] = (4 - j) <= h.m ? h.q[j] : -1;
    }
}
__device__ inline void count_hist_push(CountHist &h, int32_t s, int order) {
    h.q[0] = h.q[1];
    h.q[1] = h.q[2];
    h.q[2] = h.q[3];
    h.q[3] = s;
    h.m = h.m + 1 < order ? h.m + 1 : order;
}
// word of a stream's counts where the row of section i under the current history starts
// (lac_count.h: the last i symbols, oldest first, as base-V digits)
__device__ inline void count_rows(const CountDev &m, const CountHist &h, int64_t V, int64_t (&at)[4]) {
    const int64_t i1 = h.q[3], i2 = (int64_t)h.q[2] * V + h.q[3], i3 = ((int64_t)h.q[1] * V + h.q[2]) * V + h.q[3];
    at[0] = m.off[0];
    at[1] = m.off[1] + (h.m >= 1 ? i1 : 0) * m.Vc;
    at[2] = m.off[2] + (h.m >= 2 ? i2 : 0) * m.Vc;
    at[3] = m.off[3] + (h.m >= 3 ? i3 : 0) * m.Vc;
}

// One pass of a row: this lane's VEC entries from entry e0 on (mine: e0 < Vc), x = 1 + sum W c
// for the entries below V and 0 past them, and the counts they came from.
template <int VEC>
__device__ inline void count_pass(const CountDev &m, const uint32_t *cs, const CountHist &h, const int64_t (&at)[4],
                                  int64_t e0, bool mine, int64_t V, uint32_t (&c)[4][VEC], uint64_t (&x)[VEC]) {
    typedef uint32_t CV __attribute__((ext_vector_type(VEC)));
    const int64_t ec = mine ? e0 : 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (i < h.m) {                                        // (wave-uniform)
            const CV v = *reinterpret_cast<const CV *>(cs + at[i] + ec);
#pragma unroll
            for (int j = 0; j < VEC; j++) c[i][j] = v[j];
        } else {
#pragma unroll
            for (int j = 0; j < VEC; j++) c[i][j] = 0;
        }
    }
#pragma unroll
    for (int j = 0; j < VEC; j++) {
        uint64_t y = 1;
#pragma unroll
        for (int i = 0; i < 4; i++) y += (uint64_t)m.W[i] * c[i][j];
        x[j] = (mine && e0 + j < V) ? y : 0;
    }
}

// a[j] for a register array: an OR of masked entries (a chain of selects is turned back into
// an indexed access of the array, which then lives in scratch)
template <int VEC, typename T>
__device__ inline T vsel(const T (&a)[VEC], int j) {
    T r = 0;
#pragma unroll
    for (int i = 0; i < VEC; i++) r |= a[i] & (T)0 - (T)(j == i);
    return r;
}

// What a step needs of its row besides the search: the total (0: LAC_E_TABLE -- an entry that
// does not fit the entries' width, or a total >= 2^64) and the smallest entry.
template <typename E>
struct CountTotals {
    uint64_t base = 0, mn = ~0ull, hs = 0, lsum = 0;
    bool bad = false, big = false;
    template <int VEC>
    __device__ void take(const uint64_t (&x)[VEC], int64_t e0, bool mine, int64_t V) {
#pragma unroll
        for (int j = 0; j < VEC; j++) {
            if (mine && e0 + j < V) mn = x[j] < mn ? x[j] : mn;
            if constexpr (sizeof(E) == 4) {
                bad |= (x[j] >> 32) != 0;
            } else {
                big |= (x[j] >> 52) != 0;
                hs += x[j] >> 32;
                lsum += (uint32_t)x[j];
            }
        }
    }
    // T (wave-uniform) after every pass has been taken and `base` holds the wrapped total
    __device__ uint64_t total() {
        if constexpr (sizeof(E) == 4) {
            return __ballot(bad) ? 0 : base;
        } else {
            if (!__ballot(big)) return base;                  // 4096 entries below 2^52 cannot reach 2^64
            const u128 t = (u128)wave_sum_u64(lsum) + ((u128)wave_sum_u64(hs) << 32);
            return (t >> 64) ? 0 : (uint64_t)t;
        }
    }
};

// The combined row of the current step into the stream's scratch row, for the fudged scans
template <typename E>
__device__ inline void count_materialise(const CountDev &m, const uint32_t *cs, const CountHist &h,
                                         const int64_t (&at)[4], int64_t V, E *scr, int lane) {
    constexpr int VEC = 16 / sizeof(E);
    typedef typename VecT<E, VEC>::type VT;
    for (int64_t r0 = 0; r0 < m.Vc; r0 += 64 * VEC) {
        const int64_t e0 = r0 + (int64_t)lane * VEC;
        const bool mine = e0 < m.Vc;
        uint32_t c[4][VEC];
        uint64_t x[VEC];
        count_pass<VEC>(m, cs, h, at, e0, mine, V, c, x);
        VT xv;
#pragma unroll
        for (int j = 0; j < VEC; j++) xv[j] = (E)x[j];
        if (mine) *reinterpret_cast<VT *>(scr + e0) = xv;
    }
    __threadfence_block();                                    // the same wave reads it back
}

// ------------------------------------------------------------------ encode
template <typename E>
__global__ __launch_bounds__(256) void k_count_encode(const CountDev m, const int32_t *__restrict__ sym, int64_t B,
                                                      int64_t nsteps, int64_t V, int prec, EncState *states,
                                                      uint64_t *planeA, uint64_t *planeC, uint64_t cap_words,
                                                      uint64_t *trace, const int64_t *__restrict__ slen) {
    constexpr int VEC = 16 / sizeof(E);
    const int lane = (int)lane_id();
    const int64_t b = (int64_t)blockIdx.x * kWavesPerBlock + wave_in_block();
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
    // the registers, plane words and the history wave-uniform (SGPRs): the chain runs on the scalar unit
    int64_t l = (int64_t)rfl_u64((uint64_t)st.l), h = (int64_t)rfl_u64((uint64_t)st.h);
    st.L = rfl_u64(st.L);
    st.wa = rfl_u64(st.wa);
    st.wc = rfl_u64(st.wc);
    st.nsym = (int64_t)rfl_u64((uint64_t)st.nsym);
    const int vz = vzero_c();
    uint32_t *cs = m.counts + b * m.stride;
    E *scr = (E *)m.scratch + b * m.Vc;
    int32_t *mypast = m.past + b * m.order;
    CountHist hist = count_hist_load(mypast, m.order, V, vz);
    bool ok = true;
    for (int64_t g0 = 0; g0 < nsteps && ok; g0 += 64) {
        const int n = (int)((nsteps - g0) < 64 ? (nsteps - g0) : 64);
        const int32_t mys = sym[(g0 + (lane < n ? lane : n - 1)) * B + b];
        for (int i = 0; i < n; i++) {
            const int32_t s = __builtin_amdgcn_readlane(mys, i);
            const int64_t sc = (uint32_t)s < (uint32_t)V ? s : 0;
            const int64_t sv = sc / VEC;
            const int sr = (int)(sc - sv * VEC), sl = (int)(sv & 63);
            const int64_t sp0 = (sv >> 6) * (64 * VEC);       // first entry of the pass that holds the symbol
            int64_t at[4];
            count_rows(m, hist, V, at);
            CountTotals<E> tt;
            uint64_t lo = 0, hi = 0;
            uint32_t oc[4] = {0, 0, 0, 0};                    // the symbol's counts, from the lane that owns them
            for (int64_t r0 = 0; r0 < m.Vc; r0 += 64 * VEC) {
                const int64_t e0 = r0 + (int64_t)lane * VEC;
                const bool mine = e0 < m.Vc;
                uint32_t c[4][VEC];
                uint64_t x[VEC];
                count_pass<VEC>(m, cs, hist, at, e0, mine, V, c, x);
                tt.template take<VEC>(x, e0, mine, V);
                uint64_t ls = 0, pre = 0;
#pragma unroll
                for (int j = 0; j < VEC; j++) {
                    pre += j < sr ? x[j] : 0;
                    ls += x[j];
                }
                const uint64_t incl = wave_incl_scan_u64(ls);
                if (r0 == sp0) {                              // (wave-uniform)
                    lo = readlane_u64(tt.base + incl - ls + pre, sl);
                    hi = lo + readlane_u64(vsel<VEC>(x, sr), sl);
#pragma unroll
                    for (int k = 0; k < 4; k++) oc[k] = (uint32_t)__builtin_amdgcn_readlane((int)vsel<VEC>(c[k], sr), sl);
                }
                tt.base += readlane_u64(incl, 63);
            }
            uint64_t T = tt.total();
            const uint64_t minp = wave_min_u64(tt.mn);
            bool full = false;
#pragma unroll
            for (int k = 0; k < 4; k++) full |= k < hist.m && oc[k] == kCountFull;
            if (full) T = 0;                                  // a count that would pass 2^32 - 1: LAC_E_TABLE
            // the fudge test itself (T > w minp), handed to coder_step as its threshold: w < 2^62 always
            const uint64_t w = (uint64_t)(h - l + 1);
            const bool fudged = T != 0 && is_fudged(T, w, minp);
            if (fudged && (uint32_t)s < (uint32_t)V) count_materialise<E>(m, cs, hist, at, V, scr, lane);
            if (!coder_step<E, true>(st, l, h, lo, hi, T, minp, s, scr, V, prec, pa, pc, cap_words,
                                     trace ? trace + 2 * ((g0 + i) * B + b) : nullptr, lane, LAC_MAP_CEIL, 0.0, true,
                                     kNoFrac, kNoFrac, fudged ? kFsmThrCap : 0)) {
                ok = false;                                   // a failed step updates no count and does not move past
                break;
            }
            if (lane == sl) {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (k < hist.m) cs[at[k] + sc] = oc[k] + 1;
            }
            count_hist_push(hist, s, m.order);
        }
    }
    if (lane == 0) {
        store_state(st, l, h, pa, pc, cap_words, &states[b]);
        count_hist_store(hist, mypast, m.order);
    }
}

// ------------------------------------------------------------------ decode
// decode_symbol (lac_dec_dev.h) with the row built from the counts and the search on its
// in-register scan: the targets, the ranges, the determined test, the stop and the
// renormalisation are its uniform forms.  (A deliberate copy of fsm_decode_symbol's frame, for
// the reason given there.)  On success the counts of the symbol are incremented by the lane
// that owns them.
template <typename E>
__device__ inline int count_decode_symbol(DecState &st, const CountDev &m, uint32_t *cs, E *scr, const CountHist &hist,
                                          int64_t V, int prec, const uint8_t *bits, uint64_t nbits, int64_t *s_out,
                                          bool stop_undet) {
    constexpr int VEC = 16 / sizeof(E);
    const int lane = (int)lane_id();
    const BitWin win = bit_window(bits, nbits, st.pos);
    int64_t at[4];
    count_rows(m, hist, V, at);
    const bool one = m.Vc <= 64 * VEC;                        // one pass: the row stays in registers
    uint32_t c[4][VEC];
    uint64_t x[VEC];
    CountTotals<E> tt;
    for (int64_t r0 = 0; r0 < m.Vc; r0 += 64 * VEC) {
        const int64_t e0 = r0 + (int64_t)lane * VEC;
        const bool mine = e0 < m.Vc;
        count_pass<VEC>(m, cs, hist, at, e0, mine, V, c, x);
        tt.template take<VEC>(x, e0, mine, V);
        uint64_t ls = 0;
#pragma unroll
        for (int j = 0; j < VEC; j++) ls += x[j];
        tt.base += wave_sum_u64(ls);
    }
    const uint64_t T = tt.total(), minp = wave_min_u64(tt.mn);
    if (T == 0) return LAC_E_TABLE;
    const int64_t l = st.l, h = st.h, xx = st.x;
    if (xx < l || xx > h) return LAC_E_DECODE_RANGE;          // corrupted state / bits
    const uint64_t w = (uint64_t)(h - l + 1), v = (uint64_t)(xx - l);
    int64_t s = -1;
    uint64_t a = 0, bb = 0;
    const uint64_t past = st.pos > nbits ? st.pos - nbits : 0;
    const int u = past < (uint64_t)prec ? (int)past : prec;
    const uint64_t vhi = v + ((1ull << u) - 1);
    uint32_t oc[4] = {0, 0, 0, 0};
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
        for (int64_t r0 = 0; r0 < m.Vc && !found; r0 += 64 * VEC) {
            const int64_t e0 = r0 + (int64_t)lane * VEC;
            const bool mine = e0 < m.Vc;
            if (!one) count_pass<VEC>(m, cs, hist, at, e0, mine, V, c, x);
            uint64_t loc[VEC], ls = 0;
#pragma unroll
            for (int j = 0; j < VEC; j++) { ls += x[j]; loc[j] = ls; }
            const uint64_t in = wave_incl_scan_u64(ls);
            const uint64_t ex = cb + in - ls;
            const uint64_t mask = __ballot(mine && ex + ls > tgt);
            if (mask) {
                const int L = __ffsll((unsigned long long)mask) - 1;
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
                const int kL = __builtin_amdgcn_readlane(k, L);
                s = r0 + (int64_t)L * VEC + kL;
                lo_c = readlane_u64(lo_in, L);
                hi_c = readlane_u64(hi_in, L);
#pragma unroll
                for (int i = 0; i < 4; i++) oc[i] = (uint32_t)__builtin_amdgcn_readlane((int)vsel<VEC>(c[i], kL), L);
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
        count_materialise<E>(m, cs, hist, at, V, scr, lane);
        const int e = decode_fudged<E>(scr, V, w, v, T, &s, &a, &bb);
        if (e) return e;
        a = rfl_u64(a);
        bb = rfl_u64(bb);
        s = (int64_t)rfl_u64((uint64_t)s);
        if ((uint64_t)s >= (uint64_t)V) return LAC_E_DECODE_RANGE;
        det = vhi < bb;                                       // f_s > v_hi
        // the symbol's counts, by the lane that owns them
        const int own = (int)((s / VEC) & 63);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            uint32_t ci = 0;
            if (i < hist.m && lane == own) ci = cs[at[i] + s];
            oc[i] = (uint32_t)__builtin_amdgcn_readlane((int)ci, own);
        }
    }
    bool full = false;
#pragma unroll
    for (int i = 0; i < 4; i++) full |= i < hist.m && oc[i] == kCountFull;
    if (full) return LAC_E_TABLE;                             // a count that would pass 2^32 - 1
    if (stop_undet && !det) return LAC_E_UNDETERMINED;        // LAC_OPT_DECODE_STOP
    if (st.det && det) st.ndet++;
    else st.det = 0;
    *s_out = s;
    const int rc = decode_advance_nb(st, a, bb, win, nbits, prec);
    if (rc) return rc;
    if (lane == (int)((s / VEC) & 63)) {
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (i < hist.m) cs[at[i] + s] = oc[i] + 1;
    }
    return 0;
}

template <typename E>
__global__ __launch_bounds__(256) void k_count_decode(const CountDev m, int64_t nsteps, int64_t V, int prec,
                                                      DecState *states, const uint8_t *bits, uint64_t stride,
                                                      const uint64_t *nbits, int32_t *sym_out, int64_t B,
                                                      int stop_undet, const int64_t *__restrict__ slen) {
    const int lane = (int)lane_id();
    const int64_t b = (int64_t)blockIdx.x * kWavesPerBlock + wave_in_block();
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
    const int vz = vzero_c();
    uint32_t *cs = m.counts + b * m.stride;
    E *scr = (E *)m.scratch + b * m.Vc;
    int32_t *mypast = m.past + b * m.order;
    CountHist hist = count_hist_load(mypast, m.order, V, vz);
    for (int64_t i = 0; i < iend; i++) {
        dec_state_uniform(st);                                // (the loop's phis are not seen as uniform)
        if (st.err) {                                         // failed or stopped: -1 for the rest, 64 at once
            for (int64_t j = i + lane; j < nsteps; j += 64) sym_out[j * B + b] = -1;
            break;
        }
        int64_t s = -1;
        const int err = count_decode_symbol<E>(st, m, cs, scr, hist, V, prec, mybits, mynbits, &s, stop_undet != 0);
        if (err) {
            st.err = err;
            st.err_step = st.nsym;
        } else {
            count_hist_push(hist, (int32_t)s, m.order);
        }
        if (lane == 0) sym_out[i * B + b] = err ? -1 : (int32_t)s;
    }
    if (lane == 0) {
        states[b] = st;
        count_hist_store(hist, mypast, m.order);
    }
}

CountDev count_dev(const lac_ctx *c) {
    CountDev m;
    m.counts = c->cnt;
    m.past = c->cnt_past;
    m.scratch = c->cnt_row;
    m.stride = c->cnt_y.stride;
    m.Vc = c->cnt_y.Vc;
    for (int i = 0; i < 4; i++) {
        m.off[i] = c->cnt_y.off[i];
        m.W[i] = c->cnt_w[i];
    }
    m.order = c->cnt_y.order;
    return m;
}

// what every call on a loaded model checks first
int count_loaded(lac_ctx *c) {
    if (!c) return fail(LAC_E_ARG, "ctx is NULL");
    if (!c->cnt) return fail(LAC_E_STATE, "no count model: call lac_count_load first");
    return LAC_OK;
}
int count_ready(lac_ctx *c, int64_t steps) {
    const int rc = count_loaded(c);
    if (rc) return rc;
    if (c->mapping != LAC_MAP_CEIL)
        return fail(LAC_E_STATE, "count models use the ceil mapping (the reference's Markov_up_to_n is a CDFPredictor)");
    if (steps < 0) return fail(LAC_E_ARG, "negative steps");
    return LAC_OK;
}

}  // namespace

extern "C" {

int lac_count_load(lac_ctx *c, int order, const uint32_t *weights_host, void *stream) {
    if (!c || !weights_host) return fail(LAC_E_ARG, "NULL argument");
    if (!count_limits_ok(c->V, order))
        return fail(LAC_E_ARG, "count model of order %d over %lld symbols: 1 <= order <= %d, V <= %lld and "
                    "sum V^(i+1) <= %lld", order, (long long)c->V, kCountMaxOrder, (long long)kCountMaxVocab,
                    (long long)kCountMaxCounts);
    if (!count_weights_ok(weights_host, order)) return fail(LAC_E_ARG, "a weight >= 2^30");
    if (c->mapping != LAC_MAP_CEIL)
        return fail(LAC_E_ARG, "count models use the ceil mapping (the reference's Markov_up_to_n is a CDFPredictor)");
    if ((c->mode == 0 && c->open) || (c->mode == 1 && c->fsm_busy))
        return fail(LAC_E_STATE, "a job is in progress: load a model between jobs");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = S(stream);
    const CountLayout y = count_layout(c->V, order);
    const size_t nc = sizeof(uint32_t) * (size_t)c->B * (size_t)y.stride;
    const size_t np = sizeof(int32_t) * (size_t)c->B * (size_t)order;
    const size_t nr = (size_t)(c->pmf_bits / 8) * (size_t)c->B * (size_t)y.Vc;
    uint32_t *counts = nullptr;
    int32_t *past = nullptr;
    void *row = nullptr;
    auto drop = [&](int rc) { (void)hipFree(counts); (void)hipFree(past); (void)hipFree(row); return rc; };
    if (hipMalloc(&counts, nc) != hipSuccess || hipMalloc(&past, np) != hipSuccess ||
        hipMalloc(&row, nr) != hipSuccess)
        return drop(fail(LAC_E_HIP, "hipMalloc of %zu bytes of counts", nc));
    if (hipMemsetAsync(counts, 0, nc, st) != hipSuccess || hipMemsetAsync(past, 0xff, np, st) != hipSuccess ||
        hipMemsetAsync(row, 0, nr, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return drop(fail(LAC_E_HIP, "hipMemsetAsync"));
    (void)hipFree(c->cnt);                                    // (synchronised above: nothing reads the old model)
    (void)hipFree(c->cnt_past);
    (void)hipFree(c->cnt_row);
    c->cnt = counts;
    c->cnt_past = past;
    c->cnt_row = row;
    c->cnt_y = y;
    for (int i = 0; i < 4; i++) c->cnt_w[i] = i < order ? weights_host[i] : 0;
    return LAC_OK;
}

int lac_count_layout(lac_ctx *c, int64_t *out) {
    const int rc = count_loaded(c);
    if (rc) return rc;
    if (!out) return fail(LAC_E_ARG, "out is NULL");
    out[0] = c->cnt_y.Vc;
    out[1] = c->cnt_y.stride;
    for (int i = 0; i < 4; i++) out[2 + i] = c->cnt_y.off[i];
    return LAC_OK;
}

int lac_count_set_state(lac_ctx *c, const uint32_t *counts_dev, const int32_t *past_dev, void *stream) {
    const int rc = count_loaded(c);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    const size_t nc = sizeof(uint32_t) * (size_t)c->B * (size_t)c->cnt_y.stride;
    const size_t np = sizeof(int32_t) * (size_t)c->B * (size_t)c->cnt_y.order;
    if (counts_dev) HIPCHK(hipMemcpyAsync(c->cnt, counts_dev, nc, hipMemcpyDeviceToDevice, S(stream)));
    else HIPCHK(hipMemsetAsync(c->cnt, 0, nc, S(stream)));
    if (past_dev) HIPCHK(hipMemcpyAsync(c->cnt_past, past_dev, np, hipMemcpyDeviceToDevice, S(stream)));
    else HIPCHK(hipMemsetAsync(c->cnt_past, 0xff, np, S(stream)));
    return LAC_OK;
}

int lac_count_get_state(lac_ctx *c, uint32_t *counts_dev_out, int32_t *past_dev_out, void *stream) {
    const int rc = count_loaded(c);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    const size_t nc = sizeof(uint32_t) * (size_t)c->B * (size_t)c->cnt_y.stride;
    const size_t np = sizeof(int32_t) * (size_t)c->B * (size_t)c->cnt_y.order;
    if (counts_dev_out) HIPCHK(hipMemcpyAsync(counts_dev_out, c->cnt, nc, hipMemcpyDeviceToDevice, S(stream)));
    if (past_dev_out) HIPCHK(hipMemcpyAsync(past_dev_out, c->cnt_past, np, hipMemcpyDeviceToDevice, S(stream)));
    return LAC_OK;
}

int lac_count_encode(lac_ctx *c, const int32_t *sym_dev, int64_t steps, uint64_t *trace_dev, void *stream) {
    const int rc = count_ready(c, steps);
    if (rc) return rc;
    if (c->mode != 0) return fail(LAC_E_STATE, "context is decoding; call lac_encode_reset first");
    if (steps == 0) return LAC_OK;
    if (!sym_dev) return fail(LAC_E_ARG, "sym_dev is NULL");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = S(stream);
    const unsigned blocks = (unsigned)((c->B + kWavesPerBlock - 1) / kWavesPerBlock);
    const CountDev m = count_dev(c);
    {
        ProfScope ps(c, KID_ENCODE, st);
        if (c->pmf_bits == 32)
            k_count_encode<uint32_t><<<blocks, 64 * kWavesPerBlock, 0, st>>>(
                m, sym_dev, c->B, steps, c->V, c->prec, c->enc, c->planeA, c->planeC, c->cap_words, trace_dev,
                stream_lengths(c));
        else
            k_count_encode<uint64_t><<<blocks, 64 * kWavesPerBlock, 0, st>>>(
                m, sym_dev, c->B, steps, c->V, c->prec, c->enc, c->planeA, c->planeC, c->cap_words, trace_dev,
                stream_lengths(c));
    }
    CHECK_LAUNCH();
    enc_mark_open(c);
    return LAC_OK;
}

int lac_count_decode(lac_ctx *c, int64_t steps, int32_t *sym_out_dev, void *stream) {
    const int rc = count_ready(c, steps);
    if (rc) return rc;
    if (c->mode != 1) return fail(LAC_E_STATE, "call lac_decode_open first");
    if (steps == 0) return LAC_OK;
    if (!sym_out_dev) return fail(LAC_E_ARG, "sym_out_dev is NULL");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = S(stream);
    const unsigned blocks = (unsigned)((c->B + kWavesPerBlock - 1) / kWavesPerBlock);
    const CountDev m = count_dev(c);
    {
        ProfScope ps(c, KID_DECODE, st);
        if (c->pmf_bits == 32)
            k_count_decode<uint32_t><<<blocks, 64 * kWavesPerBlock, 0, st>>>(
                m, steps, c->V, c->prec, c->dec, c->dbits, c->dstride, c->dnbits, sym_out_dev, c->B, c->dec_stop,
                stream_lengths(c));
        else
            k_count_decode<uint64_t><<<blocks, 64 * kWavesPerBlock, 0, st>>>(
                m, steps, c->V, c->prec, c->dec, c->dbits, c->dstride, c->dnbits, sym_out_dev, c->B, c->dec_stop,
                stream_lengths(c));
    }
    CHECK_LAUNCH();
    c->fsm_busy = 1;
    return LAC_OK;
}

}  // extern "C"
