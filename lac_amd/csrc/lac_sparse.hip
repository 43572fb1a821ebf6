// lac_sparse.hip -- sparse rows (include/lac.h lac_encode_sparse, lac_decode_sparse_steps): a row
// is at most K <= 256 (symbol, weight) pairs over a uniform floor `base`, the form top-k outputs,
// truncated samplers and the match model's rows have.  It stands for the dense table
// pmf[s] = base + (wt_j where s == idx_j), and per stream everything -- bytes, registers, planes,
// traces, errors -- is what the range step gives on that table's triple, which is the pmf path's
// result on the dense row (lac_sparse.h, where the rules live in both of their forms).  A step
// reads 8 K bytes whatever V is.
//
//   k_sparse_encode  one wave per stream (one wave per workgroup), any number of steps: lane j
//                    owns slots 4 j .. 4 j + 3, loaded as one 16-B vector of idx and one of wt
//                    (lanes past K / 4 hold pads); step t + 1's slots are loaded before step t's
//                    chain runs.  lo, hi and T are three wave sums of the lanes' weights below s,
//                    at s and in all; the order test takes each lane's last index against its
//                    neighbour's first (a DPP row shift).  Registers and plane words are
//                    wave-uniform, so the chain is the scalar-unit chain of k_hist_encode
//                    (coder_step<.., UNI>, never fudged).
//   k_sparse_decode  the same layout and prefetch: one inclusive wave scan of the lanes' sums, the
//                    count of B_j <= t as a ballot of the lanes that hold a slot not below t, one
//                    broadcast of the winning slot, then decode_symbol's frame (the determined
//                    test, the stop, the renormalisation).  The division by base runs only on a gap
//                    hit, and not at all for base = 1.
#include "lac_host.h"
#include "lac_dec_dev.h"
#include "lac_sparse.h"

namespace {

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct SparseDev {                    // the call's rows as the kernels take them
    const int32_t *idx;
    const uint32_t *wt;
    int64_t step_stride, stream_stride;   // in slots, multiples of 4
    uint64_t baseV;                   // base V (lac_sparse.h sparse_base_v)
    uint32_t base;
    int lanes;                        // K / 4: the lanes that own slots
};

// The slots of row (t, b) this lane owns, in flight until sparse_lane() reads them.  The load is
// unconditional (a lane past K / 4 reads lane 0's vector and drops it): no branch, no wait.
struct SparseVec {
    i32x4 idx;
    u32x4 wt;
};
__device__ inline SparseVec sparse_load(const SparseDev &m, int64_t t, int64_t b, int lane) {
    const int64_t e = t * m.step_stride + b * m.stream_stride + (lane < m.lanes ? 4 * lane : 0);
    SparseVec v;
    v.idx = *reinterpret_cast<const i32x4 *>(m.idx + e);
    v.wt = *reinterpret_cast<const u32x4 *>(m.wt + e);
    return v;
}
__device__ inline SparseLane sparse_lane(const SparseVec &v, const SparseDev &m, int lane) {
    SparseLane s;
    const bool mine = lane < m.lanes;
#pragma unroll
    for (int q = 0; q < kSparseLaneSlots; q++) {
        s.idx[q] = mine ? v.idx[q] : -1;
        s.wt[q] = mine ? v.wt[q] : 0;
    }
    return s;
}
// the last index of the lane before (kSparseNoPrev in lane 0), on DPP like the wave sums: row_shr:1
// inside each 16-lane row, the rows' first lanes from readlanes of lanes 15, 31 and 47
__device__ inline int32_t sparse_prev(const SparseLane &s, int lane) {
    const int32_t last = s.idx[kSparseLaneSlots - 1];
    int32_t up = (int32_t)dpp32<kDppShr1>((uint32_t)last);
    const int32_t r1 = __builtin_amdgcn_readlane(last, 15), r2 = __builtin_amdgcn_readlane(last, 31);
    const int32_t r3 = __builtin_amdgcn_readlane(last, 47);
    up = lane == 16 ? r1 : (lane == 32 ? r2 : (lane == 48 ? r3 : up));
    return lane == 0 ? kSparseNoPrev : up;
}

// ------------------------------------------------------------------ encode
__global__ __launch_bounds__(64) void k_sparse_encode(const SparseDev m, const int32_t *__restrict__ sym, int64_t B,
                                                      int64_t nsteps, int64_t V, int prec, EncState *states,
                                                      uint64_t *planeA, uint64_t *planeC, uint64_t cap_words,
                                                      uint64_t *trace, const int64_t *__restrict__ slen) {
    const int lane = (int)lane_id();
    const int64_t b = (int64_t)blockIdx.x;
    if (b >= B) return;
    EncState st = states[b];
    if (slen) {                                               // a stream past its count fetches nothing
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
    SparseVec nxt = sparse_load(m, 0, b, lane);
    bool ok = true;
    for (int64_t g0 = 0; g0 < nsteps && ok; g0 += 64) {
        const int n = (int)((nsteps - g0) < 64 ? (nsteps - g0) : 64);
        const int32_t mys = sym[(g0 + (lane < n ? lane : n - 1)) * B + b];
        for (int i = 0; i < n; i++) {
            const int64_t t = g0 + i;
            const SparseLane cur = sparse_lane(nxt, m, lane);
            nxt = sparse_load(m, t + 1 < nsteps ? t + 1 : t, b, lane);   // in flight during this step's chain
            const int32_t s = __builtin_amdgcn_readlane(mys, i);
            const bool sym_ok = (uint32_t)s < (uint32_t)V;
            const int32_t sc = sym_ok ? s : 0;
            const bool bad = __ballot(sparse_lane_bad(cur, sparse_prev(cur, lane), V)) != 0;
            uint64_t below, at, all;
            sparse_lane_sums(cur, sc, &below, &at, &all);
            uint64_t lo, hi, T;
            sparse_encode_triple(m.base, m.baseV, sc, rfl_u64(wave_sum_u64(below)), rfl_u64(wave_sum_u64(at)),
                                 rfl_u64(wave_sum_u64(all)), bad, prec, &lo, &hi, &T);
            // never fudged (T <= 2^(prec-1) < w, every entry >= 1): threshold 0, no row
            const bool stepped = coder_step<uint64_t, true>(st, l, h, lo, hi, T, 1, s, (const uint64_t *)nullptr, V, prec,
                                                            pa, pc, cap_words,
                                                            trace ? trace + 2 * (t * B + b) : nullptr, lane,
                                                            LAC_MAP_CEIL, 0.0, true, kNoFrac, kNoFrac, 0);
            if (!stepped) {
                ok = false;
                break;
            }
        }
    }
    if (lane == 0) store_state(st, l, h, pa, pc, cap_words, &states[b]);
}

// ------------------------------------------------------------------ decode
// decode_symbol (lac_dec_dev.h) with the search on the row's pairs: the targets, the determined
// test, the stop and the renormalisation are its uniform forms.  (A deliberate copy of
// hist_decode_symbol's frame, for the reason given at fsm_decode_symbol.)
__device__ inline int sparse_decode_symbol(DecState &st, const SparseLane &cur, const SparseDev &m, int64_t V, int prec,
                                           const uint8_t *bits, uint64_t nbits, int64_t *s_out, bool stop_undet,
                                           int lane) {
    const BitWin win = bit_window(bits, nbits, st.pos);
    // the row alone: its form, the lanes' sums and their scan, the total
    const int32_t prev = sparse_prev(cur, lane);
    const bool bad = __ballot(sparse_lane_bad(cur, prev, V)) != 0;
    const uint64_t ls = sparse_lane_weight(cur);
    const uint64_t in = wave_incl_scan_u64(ls);
    const uint64_t T = m.baseV + readlane_u64(in, 63);
    if (bad || !range_total_ok(T, prec)) return LAC_E_TABLE;
    const int64_t l = st.l, h = st.h, xx = st.x;
    if (xx < l || xx > h) return LAC_E_DECODE_RANGE;          // corrupted state / bits
    const uint64_t w = (uint64_t)(h - l + 1), v = (uint64_t)(xx - l);
    const uint64_t past = st.pos > nbits ? st.pos - nbits : 0;
    const int u = past < (uint64_t)prec ? (int)past : prec;
    const uint64_t vhi = v + ((1ull << u) - 1);
    uint64_t tgt, thi;
    div_pair(v, vhi < w ? vhi : 0, T, 0, w, recip(w), &tgt, &thi);   // tgt < T
    // j* = 4 L + count_L for the first lane L that holds a slot not below the target
    const uint64_t ex = in - ls;
    const int c = sparse_lane_count(cur, m.base, ex, tgt);
    const uint64_t mask = __ballot(c < kSparseLaneSlots);
    const int Ln = mask ? __ffsll((unsigned long long)mask) - 1 : 63;
    const SparsePick mine = sparse_lane_pick(cur, prev, ex, c);
    SparsePick p;
    p.idx = __builtin_amdgcn_readlane(mine.idx, Ln);
    p.before = __builtin_amdgcn_readlane(mine.before, Ln);
    p.wt = (uint32_t)__builtin_amdgcn_readlane((int)mine.wt, Ln);
    p.P = readlane_u64(mine.P, Ln);
    int64_t s;
    uint64_t lo_c, hi_c;
    sparse_resolve(p, m.base, tgt, &s, &lo_c, &hi_c);
    if ((uint64_t)s >= (uint64_t)V) return LAC_E_DECODE_RANGE;
    uint64_t a, bb;
    div_pair(lo_c, hi_c, w, T - 1, T, recip(T), &a, &bb);
    const bool det = vhi < w && thi < hi_c;                   // bisect_right(cdf, t_hi) == s
    if (stop_undet && !det) return LAC_E_UNDETERMINED;        // LAC_OPT_DECODE_STOP
    if (st.det && det) st.ndet++;
    else st.det = 0;
    *s_out = s;
    return decode_advance_nb(st, a, bb, win, nbits, prec);
}

__global__ __launch_bounds__(64) void k_sparse_decode(const SparseDev m, int64_t nsteps, int64_t V, int prec,
                                                      DecState *states, const uint8_t *bits, uint64_t stride,
                                                      const uint64_t *nbits, int32_t *sym_out, int64_t B,
                                                      int stop_undet, const int64_t *__restrict__ slen) {
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
    if (st.err) {                                             // failed or stopped before this call: no row is fetched
        for (int64_t j = lane; j < nsteps; j += 64) sym_out[j * B + b] = -1;
        return;
    }
    SparseVec nxt = sparse_load(m, 0, b, lane);
    for (int64_t i = 0; i < iend; i++) {
        dec_state_uniform(st);                                // (the loop's phis are not seen as uniform)
        if (st.err) {                                         // failed or stopped: -1 for the rest, 64 at once
            for (int64_t j = i + lane; j < nsteps; j += 64) sym_out[j * B + b] = -1;
            break;
        }
        const SparseLane cur = sparse_lane(nxt, m, lane);
        nxt = sparse_load(m, i + 1 < iend ? i + 1 : i, b, lane);   // in flight during this step's chain
        int64_t s = -1;
        const int err = sparse_decode_symbol(st, cur, m, V, prec, mybits, mynbits, &s, stop_undet != 0, lane);
        if (err) {
            st.err = err;
            st.err_step = st.nsym;
        }
        if (lane == 0) sym_out[i * B + b] = err ? -1 : (int32_t)s;
    }
    if (lane == 0) states[b] = st;
}

// ------------------------------------------------------------------ host
// what every sparse call checks before anything is launched
int sparse_ready(lac_ctx *c) {
    if (!c) return fail(LAC_E_ARG, "ctx is NULL");
    if (c->mapping != LAC_MAP_CEIL)
        return fail(LAC_E_STATE, "sparse rows use the ceil mapping (the floor-mapped decoder is no inverse)");
    if (c->term != LAC_TERM_FLUSH) return fail(LAC_E_STATE, "sparse rows use the flush termination");
    return LAC_OK;
}
int sparse_args(const int32_t *idx, const uint32_t *wt, int K, int64_t step_stride, int64_t stream_stride,
                uint32_t base, int64_t steps) {
    if (steps < 0) return fail(LAC_E_ARG, "negative steps");
    if (!sparse_slots_ok(K)) return fail(LAC_E_ARG, "K = %d: a multiple of 4 in [4, %d]", K, kSparseMaxSlots);
    if (base == 0) return fail(LAC_E_ARG, "base is 0: every entry of a row is at least 1");
    if (!sparse_stride_ok(step_stride) || !sparse_stride_ok(stream_stride))
        return fail(LAC_E_ARG, "strides are in slots, non-negative multiples of 4");
    if (!idx || !wt) return fail(LAC_E_ARG, "NULL argument");
    if (!sparse_ptr_ok(idx) || !sparse_ptr_ok(wt)) return fail(LAC_E_ARG, "idx_dev and wt_dev must be 16-byte aligned");
    return LAC_OK;
}
SparseDev sparse_dev(const lac_ctx *c, const int32_t *idx, const uint32_t *wt, int K, int64_t step_stride,
                     int64_t stream_stride, uint32_t base) {
    SparseDev m;
    m.idx = idx;
    m.wt = wt;
    m.step_stride = step_stride;
    m.stream_stride = stream_stride;
    m.baseV = sparse_base_v(base, c->V);
    m.base = base;
    m.lanes = K / kSparseLaneSlots;
    return m;
}

int sparse_encode(lac_ctx *c, const int32_t *idx, const uint32_t *wt, int K, int64_t step_stride, int64_t stream_stride,
                  uint32_t base, const int32_t *sym, int64_t steps, uint64_t *trace, void *stream, bool job) {
    int rc = sparse_ready(c);
    if (rc) return rc;
    if (!job && c->mode != 0) return fail(LAC_E_STATE, "context is decoding; call lac_encode_reset first");
    rc = sparse_args(idx, wt, K, step_stride, stream_stride, base, steps);
    if (rc) return rc;
    if (steps > 0 && !sym) return fail(LAC_E_ARG, "sym_dev is NULL");
    if (steps == 0 && !job) return LAC_OK;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = S(stream);
    if (job) {                                                // (lac_encode_reset's bookkeeping)
        c->mode = 0;
        c->finished = 0;
        c->open = 0;
        c->fsm_busy = 0;
        const int r = enc_reset_launch(c, st);
        if (r) return r;
    }
    if (steps > 0) {
        ProfScope ps(c, KID_ENCODE, st);
        k_sparse_encode<<<(unsigned)c->B, 64, 0, st>>>(sparse_dev(c, idx, wt, K, step_stride, stream_stride, base), sym,
                                                       c->B, steps, c->V, c->prec, c->enc, c->planeA, c->planeC,
                                                       c->cap_words, trace, stream_lengths(c));
    }
    CHECK_LAUNCH();
    if (job) {
        const int r = enc_finish_launch(c, c->term, st);
        if (r) return r;
        enc_mark_finished(c);
    } else {
        enc_mark_open(c);
    }
    return LAC_OK;
}

}  // namespace

extern "C" {

int lac_encode_sparse(lac_ctx *c, const int32_t *idx_dev, const uint32_t *wt_dev, int K, int64_t step_stride,
                      int64_t stream_stride, uint32_t base, const int32_t *sym_dev, int64_t steps, uint64_t *trace_dev,
                      void *stream) {
    return sparse_encode(c, idx_dev, wt_dev, K, step_stride, stream_stride, base, sym_dev, steps, trace_dev, stream,
                         false);
}

int lac_encode_sparse_job(lac_ctx *c, const int32_t *idx_dev, const uint32_t *wt_dev, int K, int64_t step_stride,
                          int64_t stream_stride, uint32_t base, const int32_t *sym_dev, int64_t steps,
                          uint64_t *trace_dev, void *stream) {
    return sparse_encode(c, idx_dev, wt_dev, K, step_stride, stream_stride, base, sym_dev, steps, trace_dev, stream,
                         true);
}

int lac_decode_sparse_steps(lac_ctx *c, const int32_t *idx_dev, const uint32_t *wt_dev, int K, int64_t step_stride,
                            int64_t stream_stride, uint32_t base, int64_t steps, int32_t *sym_out_dev, void *stream) {
    int rc = sparse_ready(c);
    if (rc) return rc;
    if (c->mode != 1) return fail(LAC_E_STATE, "call lac_decode_open first");
    rc = sparse_args(idx_dev, wt_dev, K, step_stride, stream_stride, base, steps);
    if (rc) return rc;
    if (steps == 0) return LAC_OK;
    if (!sym_out_dev) return fail(LAC_E_ARG, "sym_out_dev is NULL");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = S(stream);
    {
        ProfScope ps(c, KID_DECODE, st);
        k_sparse_decode<<<(unsigned)c->B, 64, 0, st>>>(sparse_dev(c, idx_dev, wt_dev, K, step_stride, stream_stride, base),
                                                       steps, c->V, c->prec, c->dec, c->dbits, c->dstride, c->dnbits,
                                                       sym_out_dev, c->B, c->dec_stop, stream_lengths(c));
    }
    CHECK_LAUNCH();
    return LAC_OK;
}

}  // extern "C"
