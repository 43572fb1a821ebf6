// lac_fsm.hip -- finite-state models (include/lac.h lac_fsm_*; the reference's NFA predictor,
// arith_code.py:423-434): the table of step t is pmf[q_t], q_{t+1} = next[q_t][sym_t], and the
// kernel itself advances q -- one launch each way for a model of any size.  The bit format,
// the registers and every per-stream error are those of the pmf path on the gathered rows
// pmf[q_t]: the coder chains are lac_dev.h's coder_step and lac_dec_dev.h's divisions and
// renormalisation, as they are.
//
//   k_fsm_prepare  once per lac_fsm_load, one wave per state row: the row's per-entry
//                  inclusive CDF, its total, smallest positive entry, fudge threshold
//                  ceil(T / minp) and 1 / T, a zero-padded copy of the row and, for rows of
//                  more than 64 16-B vectors, <= 64 chunk bounds (layout: lac_fsm.h)
//   k_fsm_encode   one wave per stream, any number of steps, in 64-step blocks: the block's
//                  state chain first (a pointer chase, the symbols are known), then lane i
//                  gathers step i's {lo, hi, T, ceil(T / minp)} -- an O(1) lookup where the pmf
//                  path scans a row --, then the scalar-unit chain codes the block
//   k_fsm_decode   one wave per stream, all steps: with the state known, the row's meta and
//                  CDF (or chunk bounds) load together; one ballot finds the symbol; the next
//                  state is one dependent load
#include "lac_host.h"
#include "lac_dec_dev.h"

namespace {

struct FsmDev {                       // the prepared model as the kernels take it
    const FsmMeta *meta;
    const void *cdf, *pmf, *bounds;
    const int32_t *next;              // null: the explicit-states form only
    int64_t K, Vp, G, nvec;
};

// 0 in a VGPR the compiler cannot see through: added to a wave-uniform index it keeps the
// load a vector load (a scalar load's wait would sit on the chain)
__device__ inline int vzero() {
    int z = 0;
    asm volatile("" : "+v"(z));
    return z;
}

template <typename E>
__device__ inline typename VecT<E, 16 / sizeof(E)>::type fsm_load_vec(const E *row, int64_t vi) {
    typedef typename VecT<E, 16 / sizeof(E)>::type V;
    return *(reinterpret_cast<const V *>(row) + vi);          // (cached: every step of every stream re-reads the model)
}

// ------------------------------------------------------------------ prepare
template <typename E>
__global__ __launch_bounds__(256) void k_fsm_prepare(const E *__restrict__ pmf, int64_t K, int64_t V, int64_t Vp,
                                                     int64_t G, int long_rows, FsmMeta *__restrict__ meta,
                                                     E *__restrict__ cdf, E *__restrict__ pad,
                                                     E *__restrict__ bounds) {
    constexpr int VEC = 16 / sizeof(E);
    typedef typename VecT<E, VEC>::type VT;
    const int lane = (int)lane_id();
    const int64_t q = (int64_t)blockIdx.x * kWavesPerBlock + wave_in_block();
    if (q >= K) return;
    const E *row = pmf + q * V;
    const RowSums rs = row_reduce<E, 1>(row, V, 0);           // (any alignment: the caller's rows are not padded)
    const uint64_t T = (rs.T >> 64) ? 0 : (uint64_t)rs.T;     // 0: an empty row or a total >= 2^64
    if (lane == 0) {
        FsmMeta m;
        m.T = T;
        m.minp = T ? rs.minp : 0;
        const uint64_t thr = T ? div_floor((u128)T + (rs.minp - 1), rs.minp) : 0;
        m.fthr = thr < kFsmThrCap ? thr : kFsmThrCap;
        m.inv_T = T ? 1.0 / (double)T : 0.0;
        meta[q] = m;
    }
    E *crow = cdf + q * Vp, *prow = pad + q * Vp;
    const int64_t CE = G * VEC;                               // entries per chunk
    uint64_t base = 0;
    for (int64_t r0 = 0; r0 < Vp; r0 += 64 * VEC) {
        const int64_t e0 = r0 + (int64_t)lane * VEC;
        E x[VEC];
        uint64_t ls = 0;
#pragma unroll
        for (int j = 0; j < VEC; j++) {
            const int64_t e = e0 + j;
            const E y = row[e < V ? e : V - 1];
            x[j] = e < V ? y : (E)0;
            ls += (uint64_t)x[j];
        }
        const uint64_t incl = wave_incl_scan_u64(ls);
        uint64_t c = base + incl - ls;
        VT cv, pv;
#pragma unroll
        for (int j = 0; j < VEC; j++) {
            const int64_t e = e0 + j;
            c += (uint64_t)x[j];
            const E ce = e < V ? (E)c : (E)T;
            cv[j] = ce;
            pv[j] = x[j];
            if (long_rows && e < Vp && ((e + 1) % CE == 0 || e == Vp - 1)) bounds[q * 64 + e / CE] = ce;
        }
        if (e0 < Vp) {                                        // (Vp is whole vectors)
            *reinterpret_cast<VT *>(crow + e0) = cv;
            *reinterpret_cast<VT *>(prow + e0) = pv;
        }
        base += readlane_u64(incl, 63);
    }
    if (long_rows && (int64_t)lane * CE >= Vp) bounds[q * 64 + lane] = (E)T;   // chunks past the row
}

__global__ __launch_bounds__(256) void k_fsm_check_next(const int32_t *__restrict__ next, int64_t n, int64_t K,
                                                        int *flag) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        bad |= (uint32_t)next[i] >= (uint32_t)K;
    if (bad) atomicOr(flag, 1);
}

// ------------------------------------------------------------------ encode
template <typename E>
__global__ __launch_bounds__(256) void k_fsm_encode(const FsmDev m, const int32_t *__restrict__ sym,
                                                    const int32_t *__restrict__ xstates, int64_t B, int64_t nsteps,
                                                    int64_t V, int prec, EncState *states, int32_t *fstate,
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
    // the registers, plane words and the state wave-uniform (SGPRs): the chains run on the scalar unit
    int64_t l = (int64_t)rfl_u64((uint64_t)st.l), h = (int64_t)rfl_u64((uint64_t)st.h);
    st.L = rfl_u64(st.L);
    st.wa = rfl_u64(st.wa);
    st.wc = rfl_u64(st.wc);
    st.nsym = (int64_t)rfl_u64((uint64_t)st.nsym);
    const int vz = vzero();
    const E *cdf = (const E *)m.cdf, *pmf = (const E *)m.pmf;
    int32_t q = xstates ? 0 : __builtin_amdgcn_readfirstlane(fstate[b]);
    bool ok = true;
    for (int64_t g0 = 0; g0 < nsteps && ok; g0 += 64) {
        const int n = (int)((nsteps - g0) < 64 ? (nsteps - g0) : 64);
        const int64_t at = (g0 + (lane < n ? lane : n - 1)) * B + b;
        const int32_t mys = sym[at];
        int32_t myq = 0, qend = q;
        if (xstates) {
            myq = xstates[at];
        } else {
            // the block's state chain, ahead of the coder: q <- next[q][sym], one dependent
            // load per step.  A step with a symbol or state out of range leaves q where it is:
            // the coder fails there, and the states after it are not used.
            for (int i = 0; i < n; i++) {
                myq = lane == i ? qend : myq;
                const int32_t s = __builtin_amdgcn_readlane(mys, i);
                const bool in = (uint32_t)qend < (uint32_t)m.K && (uint32_t)s < (uint32_t)V;
                const int32_t nq = m.next[(in ? (int64_t)qend * V + s : 0) + vz];
                qend = in ? __builtin_amdgcn_readfirstlane(nq) : qend;
            }
        }
        // lane i gathers step i's row values from the prepared model
        const bool qok = lane < n && (uint32_t)myq < (uint32_t)m.K;
        const int64_t qc = qok ? myq : 0;
        FsmMeta mm = m.meta[qc];
        if (!qok) { mm.T = 0; mm.minp = 0; mm.fthr = 0; mm.inv_T = 0.0; }   // LAC_E_TABLE at that step
        const int64_t sc = mys < 0 ? 0 : (mys >= V ? V - 1 : mys);
        const E *crow = cdf + qc * m.Vp;
        const E c1 = crow[sc], c0 = crow[sc > 0 ? sc - 1 : 0];
        uint64_t lo = sc > 0 ? (uint64_t)c0 : 0, hi = (uint64_t)c1;
        if constexpr (sizeof(E) == 4) {
            // wide rows (u32, T >= 2^32: the CDF does not fit its entries): the pmf path's row scan
            uint64_t wm = __ballot(lane < n && fsm_row_wide<E>(mm.T));
            while (wm) {
                const int i = __ffsll((unsigned long long)wm) - 1;
                wm &= wm - 1;
                const int64_t qi = __builtin_amdgcn_readlane(myq, i);
                const RowSums rs = row_reduce<E, VEC>(pmf + qi * m.Vp, m.Vp, (int64_t)__builtin_amdgcn_readlane((int)sc, i));
                if (lane == i) { lo = (uint64_t)rs.lo; hi = lo + rs.ps; }
            }
        }
        // the 64 steps' row fractions at once, one lane each, off the serial chain (k_encode)
        const bool frac_ok = lane < n && !(mm.T >> 62);
        const uint64_t flo = frac_ok ? row_frac(lo, mm.T) : kNoFrac;
        const uint64_t fhi = frac_ok ? row_frac(hi, mm.T) : kNoFrac;
        int i = 0;
        for (; i < n; i++) {
            const uint64_t slo = readlane_u64(lo, i), shi = readlane_u64(hi, i);
            const uint64_t T = readlane_u64(mm.T, i), minp = readlane_u64(mm.minp, i);
            const uint64_t invb = readlane_u64(__builtin_bit_cast(uint64_t, mm.inv_T), i);
            const uint64_t fl = readlane_u64(flo, i), fh = readlane_u64(fhi, i), ft = readlane_u64(mm.fthr, i);
            const int64_t s = __builtin_amdgcn_readlane(mys, i);
            const int64_t qi = __builtin_amdgcn_readlane((int)qc, i);
            if (!coder_step<E, true>(st, l, h, slo, shi, T, minp, s, pmf + qi * m.Vp, V, prec, pa, pc, cap_words,
                                     trace ? trace + 2 * ((g0 + i) * B + b) : nullptr, lane, LAC_MAP_CEIL, __builtin_bit_cast(double, invb), true, fl, fh,
                                     ft)) {
                ok = false;
                break;
            }
        }
        // a failed stream keeps the state of its failing step (nsym excludes that step too)
        if (!xstates) q = i == n ? qend : __builtin_amdgcn_readlane(myq, i);
    }
    if (lane == 0) {
        store_state(st, l, h, pa, pc, cap_words, &states[b]);
        if (!xstates) fstate[b] = q;
    }
}

// ------------------------------------------------------------------ decode
// decode_symbol (lac_dec_dev.h) with the row search on the prepared CDF: the targets, the
// ranges, the determined test, the stop and the renormalisation are its uniform forms.  (A
// deliberate copy: a search parameter in decode_symbol itself changes every pmf decoder.)
template <typename E, bool LONG>
__device__ inline int fsm_decode_symbol(DecState &st, const FsmDev &m, int64_t q, int64_t V, int prec,
                                        const uint8_t *bits, uint64_t nbits, int64_t *s_out, bool stop_undet) {
    constexpr int VEC = 16 / sizeof(E);
    typedef typename VecT<E, VEC>::type VT;
    const int lane = (int)lane_id();
    const BitWin win = bit_window(bits, nbits, st.pos);
    // the row's meta (lanes 0..3 one word each) and its first search level, issued together
    const uint64_t mw = reinterpret_cast<const uint64_t *>(m.meta + q)[lane & 3];
    const E *crow = (const E *)m.cdf + q * m.Vp, *prow = (const E *)m.pmf + q * m.Vp;
    VT x0 = (VT)0;
    E bnd = 0;
    if constexpr (LONG) bnd = ((const E *)m.bounds)[q * 64 + lane];
    else x0 = fsm_load_vec<E>(crow, lane < m.nvec ? lane : m.nvec - 1);
    const uint64_t T = readlane_u64(mw, 0), fthr = readlane_u64(mw, 2);
    const double inv_T = __builtin_bit_cast(double, readlane_u64(mw, 3));
    if (T == 0) return LAC_E_TABLE;
    const int64_t l = st.l, h = st.h, x = st.x;
    if (x < l || x > h) return LAC_E_DECODE_RANGE;            // corrupted state / bits
    const uint64_t w = (uint64_t)(h - l + 1), v = (uint64_t)(x - l);
    int64_t s = -1;
    uint64_t a = 0, bb = 0;
    const uint64_t past = st.pos > nbits ? st.pos - nbits : 0;
    const int u = past < (uint64_t)prec ? (int)past : prec;
    const uint64_t vhi = v + ((1ull << u) - 1);
    bool det;
    if (w >= fthr) {                                          // not fudged (arith_code.py:84)
        uint64_t tgt, thi;
        const bool small = T < kSmallQuot && prec <= 50;
        if (small) {
            const double iw = recip2_small(w);
            tgt = div_small_u(v, T, 0, w, iw);
            thi = vhi == v ? tgt : (vhi < w ? div_small_u(vhi, T, 0, w, iw) : 0);
        } else {
            div_pair(v, vhi < w ? vhi : 0, T, 0, w, recip(w), &tgt, &thi);   // tgt < T
        }
        uint64_t lo_c = 0, hi_c = 0;
        if (fsm_row_wide<E>(T)) {                             // the pmf path's scan of the whole row
            uint64_t cnt;
            if (!scan_chunk<E, VEC>(prow, m.nvec, 0, (int)m.G, 0, tgt, &cnt, &lo_c, &hi_c)) return LAC_E_DECODE_RANGE;
            s = (int64_t)cnt;
        } else {
            // one vector per lane: the CDF is nondecreasing, so the first lane whose last entry
            // exceeds the target holds the crossing; its count of entries <= tgt and the
            // bracket c_{s-1}, c_s are read out of it (c_{s-1} from the lane before when the
            // crossing is the lane's first entry)
            int64_t v0 = 0, nv = m.nvec;                      // the vectors searched: [v0, v0 + nv)
            uint64_t before = 0;                              // c just before vector v0
            if constexpr (LONG) {
                const uint64_t cm = __ballot((uint64_t)bnd > tgt);
                if (!cm) return LAC_E_DECODE_RANGE;
                const int ch = __ffsll((unsigned long long)cm) - 1;
                before = ch ? readlane_u64((uint64_t)bnd, ch - 1) : 0;
                v0 = (int64_t)ch * m.G;
                nv = m.G < m.nvec - v0 ? m.G : m.nvec - v0;
            }
            bool found = false;
            for (int64_t r = 0; r < nv && !found; r += 64) {
                const bool mine = r + lane < nv;
                VT xv;
                if constexpr (LONG) xv = fsm_load_vec<E>(crow, v0 + (mine ? r + lane : nv - 1));
                else xv = x0;
                int k = 0;
                uint64_t lo_in = 0, hi_in = ~0ull;
#pragma unroll
                for (int j = 0; j < VEC; j++) {
                    const uint64_t ce = (uint64_t)xv[j];
                    const bool le = ce <= tgt;
                    k += le ? 1 : 0;
                    lo_in = le ? ce : lo_in;
                    hi_in = (!le && ce < hi_in) ? ce : hi_in;
                }
                const uint64_t last = (uint64_t)xv[VEC - 1];
                const uint64_t mask = __ballot(mine && last > tgt);
                if (mask) {
                    const int L = __ffsll((unsigned long long)mask) - 1;
                    const int kL = __builtin_amdgcn_readlane(k, L);
                    s = (v0 + r + L) * VEC + kL;
                    hi_c = readlane_u64(hi_in, L);
                    lo_c = kL ? readlane_u64(lo_in, L) : (L ? readlane_u64(last, L - 1) : before);
                    found = true;
                } else {
                    before = readlane_u64(last, 63);
                }
            }
            if (!found) return LAC_E_DECODE_RANGE;
        }
        const uint64_t add = T - 1;
        if (small) div_small_u2(lo_c, hi_c, w, add, T, inv_T, &a, &bb);
        else div_pair(lo_c, hi_c, w, add, T, inv_T, &a, &bb);
        det = vhi < w && thi < hi_c;                          // bisect_right(cdf, t_hi) == s
    } else {
        const int e = decode_fudged<E>(prow, V, w, v, T, &s, &a, &bb);
        if (e) return e;
        a = rfl_u64(a);
        bb = rfl_u64(bb);
        s = (int64_t)rfl_u64((uint64_t)s);
        det = vhi < bb;                                       // f_s > v_hi
    }
    if (stop_undet && !det) return LAC_E_UNDETERMINED;        // LAC_OPT_DECODE_STOP
    if (st.det && det) st.ndet++;
    else st.det = 0;
    *s_out = s;
    return decode_advance_nb(st, a, bb, win, nbits, prec);
}

template <typename E, bool LONG>
__global__ __launch_bounds__(256) void k_fsm_decode(const FsmDev m, const int32_t *__restrict__ xstates,
                                                    int64_t nsteps, int64_t V, int prec, DecState *states,
                                                    int32_t *fstate, const uint8_t *bits, uint64_t stride,
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
    const int vz = vzero();
    int32_t q = xstates ? 0 : __builtin_amdgcn_readfirstlane(fstate[b]);
    int32_t nq = xstates ? xstates[b + vz] : 0;
    for (int64_t i = 0; i < iend; i++) {
        dec_state_uniform(st);                                // (the loop's phis are not seen as uniform)
        if (xstates) {
            q = __builtin_amdgcn_readfirstlane(nq);
            if (i + 1 < iend) nq = xstates[(i + 1) * B + b + vz];   // a step ahead: independent of the chain
        }
        if (st.err) {                                         // failed or stopped: -1 for the rest, 64 at once
            for (int64_t j = i + lane; j < nsteps; j += 64) sym_out[j * B + b] = -1;
            break;
        }
        int err = (uint32_t)q < (uint32_t)m.K ? 0 : LAC_E_TABLE;
        int64_t s = -1;
        if (!err) err = fsm_decode_symbol<E, LONG>(st, m, q, V, prec, mybits, mynbits, &s, stop_undet != 0);
        if (err) {
            st.err = err;
            st.err_step = st.nsym;
        } else if (!xstates) {
            q = __builtin_amdgcn_readfirstlane(m.next[(int64_t)q * V + s + vz]);   // the one dependent load
        }
        if (lane == 0) sym_out[i * B + b] = err ? -1 : (int32_t)s;
    }
    if (lane == 0) {
        states[b] = st;
        if (!xstates) fstate[b] = q;
    }
}

FsmDev fsm_dev(const lac_ctx *c) {
    const FsmLayout &y = c->fsm_y;
    const uint8_t *p = (const uint8_t *)c->fsm;
    return FsmDev{(const FsmMeta *)(p + y.off_meta), p + y.off_cdf, p + y.off_pmf, p + y.off_bounds,
                  c->fsm_has_next ? (const int32_t *)(p + y.off_next) : nullptr, y.K, y.Vp, y.G, y.nvec};
}

// what every coding call checks before it launches anything
int fsm_ready(lac_ctx *c, const int32_t *states_dev, int64_t steps) {
    if (!c) return fail(LAC_E_ARG, "ctx is NULL");
    if (!c->fsm) return fail(LAC_E_STATE, "no model: call lac_fsm_load first");
    if (c->mapping != LAC_MAP_CEIL)
        return fail(LAC_E_STATE, "finite-state models use the ceil mapping (the reference's NFA is a CDFPredictor)");
    if (steps < 0) return fail(LAC_E_ARG, "negative steps");
    if (!c->fsm_has_next && !states_dev)
        return fail(LAC_E_ARG, "the model was loaded without transitions: pass every step's state");
    return LAC_OK;
}

template <typename E>
int fsm_prepare_launch(lac_ctx *c, const FsmLayout &y, const void *pmf_dev, uint8_t *p, hipStream_t st) {
    k_fsm_prepare<E><<<(unsigned)((y.K + kWavesPerBlock - 1) / kWavesPerBlock), 64 * kWavesPerBlock, 0, st>>>(
        (const E *)pmf_dev, y.K, y.V, y.Vp, y.G, y.long_rows, (FsmMeta *)(p + y.off_meta), (E *)(p + y.off_cdf),
        (E *)(p + y.off_pmf), (E *)(p + y.off_bounds));
    CHECK_LAUNCH();
    return LAC_OK;
}

}  // namespace

extern "C" {

int lac_fsm_load(lac_ctx *c, const void *pmf_dev, const int32_t *next_dev, int64_t states, void *stream) {
    if (!c || !pmf_dev) return fail(LAC_E_ARG, "NULL argument");
    if (!fsm_limits_ok(states, c->V))
        return fail(LAC_E_ARG, "model of %lld states x %lld symbols: V <= %lld and K * V <= %lld", (long long)states,
                    (long long)c->V, (long long)kFsmMaxVocab, (long long)kFsmMaxEntries);
    if ((c->mode == 0 && c->open) || (c->mode == 1 && c->fsm_busy))
        return fail(LAC_E_STATE, "a job is in progress: load a model between jobs");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = S(stream);
    const FsmLayout y = fsm_layout(states, c->V, c->pmf_bits, next_dev != nullptr);
    uint8_t *p = nullptr;
    HIPCHK(hipMalloc(&p, y.bytes));
    auto drop = [&](int rc) { (void)hipFree(p); return rc; };
    if (!c->fsm_flag && hipMalloc(&c->fsm_flag, sizeof(int)) != hipSuccess) return drop(fail(LAC_E_HIP, "hipMalloc"));
    if (!c->fsm_state && hipMalloc(&c->fsm_state, sizeof(int32_t) * c->B) != hipSuccess)
        return drop(fail(LAC_E_HIP, "hipMalloc"));
    int rc = c->pmf_bits == 32 ? fsm_prepare_launch<uint32_t>(c, y, pmf_dev, p, st)
                               : fsm_prepare_launch<uint64_t>(c, y, pmf_dev, p, st);
    if (rc) return drop(rc);
    int bad = 0;
    if (next_dev) {
        const int64_t n = states * c->V;
        if (hipMemsetAsync(c->fsm_flag, 0, sizeof(int), st) != hipSuccess) return drop(fail(LAC_E_HIP, "hipMemsetAsync"));
        const int64_t blocks = (n + 255) / 256;
        k_fsm_check_next<<<(unsigned)(blocks < 1024 ? blocks : 1024), 256, 0, st>>>(next_dev, n, states, c->fsm_flag);
        if (hipGetLastError() != hipSuccess) return drop(fail(LAC_E_HIP, "k_fsm_check_next launch"));
        if (hipMemcpyAsync(p + y.off_next, next_dev, sizeof(int32_t) * n, hipMemcpyDeviceToDevice, st) != hipSuccess ||
            hipMemcpyAsync(&bad, c->fsm_flag, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess)
            return drop(fail(LAC_E_HIP, "hipMemcpyAsync"));
    }
    // the caller's buffers are free once the load returns
    if (hipStreamSynchronize(st) != hipSuccess) return drop(fail(LAC_E_HIP, "hipStreamSynchronize"));
    if (bad) return drop(fail(LAC_E_TABLE, "a transition leaves [0, %lld)", (long long)states));
    if (hipMemsetAsync(c->fsm_state, 0, sizeof(int32_t) * c->B, st) != hipSuccess)
        return drop(fail(LAC_E_HIP, "hipMemsetAsync"));
    (void)hipFree(c->fsm);                                    // (synchronised above: nothing reads the old model)
    c->fsm = p;
    c->fsm_y = y;
    c->fsm_has_next = next_dev != nullptr;
    return LAC_OK;
}

int lac_fsm_set_states(lac_ctx *c, const int32_t *state_dev, void *stream) {
    if (!c) return fail(LAC_E_ARG, "ctx is NULL");
    if (!c->fsm) return fail(LAC_E_STATE, "no model: call lac_fsm_load first");
    HIPCHK(hipSetDevice(c->device));
    if (state_dev)
        HIPCHK(hipMemcpyAsync(c->fsm_state, state_dev, sizeof(int32_t) * c->B, hipMemcpyDeviceToDevice, S(stream)));
    else
        HIPCHK(hipMemsetAsync(c->fsm_state, 0, sizeof(int32_t) * c->B, S(stream)));
    return LAC_OK;
}

int lac_fsm_get_states(lac_ctx *c, int32_t *state_dev_out, void *stream) {
    if (!c || !state_dev_out) return fail(LAC_E_ARG, "NULL argument");
    if (!c->fsm) return fail(LAC_E_STATE, "no model: call lac_fsm_load first");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(state_dev_out, c->fsm_state, sizeof(int32_t) * c->B, hipMemcpyDeviceToDevice, S(stream)));
    return LAC_OK;
}

int lac_fsm_encode(lac_ctx *c, const int32_t *sym_dev, const int32_t *states_dev, int64_t steps,
                   uint64_t *trace_dev, void *stream) {
    const int rc = fsm_ready(c, states_dev, steps);
    if (rc) return rc;
    if (c->mode != 0) return fail(LAC_E_STATE, "context is decoding; call lac_encode_reset first");
    if (steps == 0) return LAC_OK;
    if (!sym_dev) return fail(LAC_E_ARG, "sym_dev is NULL");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = S(stream);
    const unsigned blocks = (unsigned)((c->B + kWavesPerBlock - 1) / kWavesPerBlock);
    const FsmDev m = fsm_dev(c);
    {
        ProfScope ps(c, KID_ENCODE, st);
        if (c->pmf_bits == 32)
            k_fsm_encode<uint32_t><<<blocks, 64 * kWavesPerBlock, 0, st>>>(
                m, sym_dev, states_dev, c->B, steps, c->V, c->prec, c->enc, c->fsm_state, c->planeA, c->planeC,
                c->cap_words, trace_dev, stream_lengths(c));
        else
            k_fsm_encode<uint64_t><<<blocks, 64 * kWavesPerBlock, 0, st>>>(
                m, sym_dev, states_dev, c->B, steps, c->V, c->prec, c->enc, c->fsm_state, c->planeA, c->planeC,
                c->cap_words, trace_dev, stream_lengths(c));
    }
    CHECK_LAUNCH();
    enc_mark_open(c);
    return LAC_OK;
}

int lac_fsm_decode(lac_ctx *c, const int32_t *states_dev, int64_t steps, int32_t *sym_out_dev, void *stream) {
    const int rc = fsm_ready(c, states_dev, steps);
    if (rc) return rc;
    if (c->mode != 1) return fail(LAC_E_STATE, "call lac_decode_open first");
    if (steps == 0) return LAC_OK;
    if (!sym_out_dev) return fail(LAC_E_ARG, "sym_out_dev is NULL");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = S(stream);
    const unsigned blocks = (unsigned)((c->B + kWavesPerBlock - 1) / kWavesPerBlock);
    const FsmDev m = fsm_dev(c);
    auto launch = [&](auto kern) {
        ProfScope ps(c, KID_DECODE, st);
        kern<<<blocks, 64 * kWavesPerBlock, 0, st>>>(m, states_dev, steps, c->V, c->prec, c->dec, c->fsm_state,
                                                    c->dbits, c->dstride, c->dnbits, sym_out_dev, c->B, c->dec_stop,
                                                    stream_lengths(c));
    };
    if (c->pmf_bits == 32) {
        if (c->fsm_y.long_rows) launch(k_fsm_decode<uint32_t, true>);
        else launch(k_fsm_decode<uint32_t, false>);
    } else {
        if (c->fsm_y.long_rows) launch(k_fsm_decode<uint64_t, true>);
        else launch(k_fsm_decode<uint64_t, false>);
    }
    CHECK_LAUNCH();
    c->fsm_busy = 1;
    return LAC_OK;
}

}  // extern "C"
