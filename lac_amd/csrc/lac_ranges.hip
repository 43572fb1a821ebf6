// lac_ranges.hip -- range-level coding (include/lac.h lac_encode_ranges, lac_decode_ranges_step):
// the coder is handed lo = c_{s-1}, hi = c_s and T per symbol instead of a table, which is all
// symbol_to_range reads (arith_code.py:98-110).  A model whose distribution is a formula, or
// whose alphabet is too large to write out per step, codes through these calls.  The bit format,
// the registers and every per-stream error are the pmf path's on the three-entry table
// [lo, hi - lo, T - hi] with symbol 1 (lac_ranges.h, where the step itself lives).
//
//   k_ranges_encode  one LANE per stream, 256-thread workgroups, any number of steps in one
//                    launch.  No row is scanned, so the lanes' work is the coder chain itself:
//                    two 128-bit mul-divs, the renormalisation and the plane append, all per lane
//                    on the vector unit.  lo[t][b .. b + 63] are coalesced loads; step t + 1's
//                    triple is loaded before step t's chain runs, and recip(T) depends on the
//                    triple alone, so neither sits on the chain.  Some lane of a wave crosses a
//                    plane word at almost every step, so the append is straight-line
//                    (range_append) with only its store under a branch.  Lanes whose stream has
//                    failed, ended its count or lies past the last stream are masked; the loop
//                    bound is the wave's longest live count, a wave-uniform value.
//   k_ranges_decode  the same layout, one step: advance by the previous symbol's range
//                    (decode_symbol's frame without find_chunk / scan_chunk), then peek the next
//                    target floor((x - l) T' / w).
#include "lac_host.h"
#include "lac_dec_dev.h"
#include "lac_ranges.h"

namespace {

__global__ __launch_bounds__(kRangeThreads) void k_ranges_encode(
    const uint64_t *__restrict__ lo, const uint64_t *__restrict__ hi, const uint64_t *__restrict__ tot,
    int64_t tot_step, int64_t tot_stream, int64_t B, int64_t nsteps, int prec, EncState *states, uint64_t *planeA,
    uint64_t *planeC, uint64_t cap_words, uint64_t *trace, const int64_t *__restrict__ slen) {
    const int64_t b0 = (int64_t)blockIdx.x * kRangeThreads + threadIdx.x;
    const bool inb = b0 < B;
    const int64_t b = inb ? b0 : B - 1;                       // masked lanes read the last stream, write nothing
    EncState st = states[b];
    // the stream's live steps of this launch (lac_set_stream_lengths): 0 for a masked lane
    int64_t mine = nsteps;
    if (slen) {
        const int64_t n = slen[b];
        mine = n <= st.nsym ? 0 : (n - st.nsym < nsteps ? n - st.nsym : nsteps);
    }
    if (!inb) mine = 0;
    if (mine > 0 && !st.err && st.nflush >= 0) {              // (k_encode's rule for a finished stream)
        st.err = LAC_E_STATE;
        st.err_step = st.nsym;
        states[b] = st;
    }
    const bool entered = mine > 0 && !st.err;
    if (!entered) mine = 0;
    uint64_t *pa = planeA + (uint64_t)b * cap_words, *pc = planeC + (uint64_t)b * cap_words;
    int64_t l = st.l, h = st.h;
    const int64_t wave_steps = (int64_t)wave_max_u64((uint64_t)mine);   // wave-uniform loop bound
    auto store = [&](uint64_t idx, uint64_t wa, uint64_t wc) {
        pa[idx] = wa;
        pc[idx] = wc;
    };
    const int64_t toff = b * tot_stream;
    uint64_t nlo = lo[b], nhi = hi[b], nT = tot[toff];
    for (int64_t t = 0; t < wave_steps; t++) {
        const uint64_t clo = nlo, chi = nhi, cT = nT;
        const int64_t tn = t + 1 < nsteps ? t + 1 : t;        // the next step's triple, in flight during this chain
        nlo = lo[tn * B + b];
        nhi = hi[tn * B + b];
        nT = tot[tn * tot_step + toff];
        const double inv = recip(cT ? cT : 1);                // off the chain: the triple alone
        if (t < mine) {
            int k;
            uint64_t E;
            const int rc = range_encode_step(st, l, h, clo, chi, cT, inv, prec, cap_words, store, &k, &E);
            if (trace && k >= 0) {
                uint64_t *slot = trace + 2 * (t * B + b);
                slot[0] = E;
                slot[1] = (uint64_t)k;
            }
            if (rc) {
                st.err = rc;
                st.err_step = st.nsym;
                mine = 0;                                     // frozen from here on
            }
        }
    }
    if (entered) {                                            // (store_state, lac_dev.h)
        if (st.L > 0 && ((st.L - 1) >> 6) < cap_words) {
            pa[(st.L - 1) >> 6] = st.wa;
            pc[(st.L - 1) >> 6] = st.wc;
        }
        st.l = l;
        st.h = h;
        states[b] = st;
    }
}

__global__ __launch_bounds__(kRangeThreads) void k_ranges_decode(
    const uint64_t *__restrict__ lo, const uint64_t *__restrict__ hi, const uint64_t *__restrict__ tot,
    const uint64_t *__restrict__ next_tot, uint64_t *target_out, int64_t B, int prec, DecState *states,
    const uint8_t *bits, uint64_t stride, const uint64_t *__restrict__ nbits, int stop,
    const int64_t *__restrict__ slen) {
    const int64_t b = (int64_t)blockIdx.x * kRangeThreads + threadIdx.x;
    if (b >= B) return;                                       // (one step: no loop whose bound a masked lane could change)
    DecState st = states[b];
    const int64_t count = slen ? slen[b] : INT64_MAX;
    if (lo && !st.err && st.nsym < count) {
        const uint64_t nb = nbits[b], pos = st.pos;
        const BitWin win = bit_window(bits + (uint64_t)b * stride, nb, pos);   // in flight during the tests
        const uint64_t T = tot[b];
        const int rc = range_decode_step(st, lo[b], hi[b], T, recip(T ? T : 1), prec, pos > nb ? pos - nb : 0,
                                         stop != 0, [&](int k) { return window_bits(win, nb, pos, k); });
        if (rc) {
            st.err = rc;
            st.err_step = st.nsym;
        }
        states[b] = st;
    }
    if (next_tot) target_out[b] = (st.err || st.nsym >= count) ? kRangeNoTarget : range_peek(st, next_tot[b], prec);
}

// what every range-level call checks before anything is launched
int ranges_ready(lac_ctx *c) {
    if (!c) return fail(LAC_E_ARG, "ctx is NULL");
    if (c->mapping != LAC_MAP_CEIL)
        return fail(LAC_E_STATE, "range-level coding uses the ceil mapping (the floor-mapped decoder is no inverse)");
    if (c->term != LAC_TERM_FLUSH) return fail(LAC_E_STATE, "range-level coding uses the flush termination");
    return LAC_OK;
}

int ranges_encode(lac_ctx *c, const uint64_t *lo, const uint64_t *hi, const uint64_t *tot, int64_t tot_step,
                  int64_t tot_stream, int64_t steps, uint64_t *trace, void *stream, bool job) {
    const int rc = ranges_ready(c);
    if (rc) return rc;
    if (!job && c->mode != 0) return fail(LAC_E_STATE, "context is decoding; call lac_encode_reset first");
    if (steps < 0 || tot_step < 0 || tot_stream < 0) return fail(LAC_E_ARG, "negative size/stride");
    if (steps > 0 && (!lo || !hi || !tot)) return fail(LAC_E_ARG, "NULL argument");
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
        k_ranges_encode<<<range_blocks(c->B), kRangeThreads, 0, st>>>(lo, hi, tot, tot_step, tot_stream, c->B, steps,
                                                                      c->prec, c->enc, c->planeA, c->planeC,
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

int lac_encode_ranges(lac_ctx *c, const uint64_t *lo_dev, const uint64_t *hi_dev, const uint64_t *tot_dev,
                      int64_t tot_step_stride, int64_t tot_stream_stride, int64_t steps, uint64_t *trace_dev,
                      void *stream) {
    return ranges_encode(c, lo_dev, hi_dev, tot_dev, tot_step_stride, tot_stream_stride, steps, trace_dev, stream,
                         false);
}

int lac_encode_ranges_job(lac_ctx *c, const uint64_t *lo_dev, const uint64_t *hi_dev, const uint64_t *tot_dev,
                          int64_t tot_step_stride, int64_t tot_stream_stride, int64_t steps, uint64_t *trace_dev,
                          void *stream) {
    return ranges_encode(c, lo_dev, hi_dev, tot_dev, tot_step_stride, tot_stream_stride, steps, trace_dev, stream,
                         true);
}

int lac_decode_ranges_step(lac_ctx *c, const uint64_t *lo_dev, const uint64_t *hi_dev, const uint64_t *tot_dev,
                           const uint64_t *next_tot_dev, uint64_t *target_out_dev, void *stream) {
    const int rc = ranges_ready(c);
    if (rc) return rc;
    if (c->mode != 1) return fail(LAC_E_STATE, "call lac_decode_open first");
    if (!lo_dev && !next_tot_dev) return fail(LAC_E_ARG, "neither an advance nor a peek: lo_dev and next_tot_dev are NULL");
    if (lo_dev && (!hi_dev || !tot_dev)) return fail(LAC_E_ARG, "an advance needs lo_dev, hi_dev and tot_dev");
    if (next_tot_dev && !target_out_dev) return fail(LAC_E_ARG, "a peek needs target_out_dev");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = S(stream);
    {
        ProfScope ps(c, KID_DECODE, st);
        k_ranges_decode<<<range_blocks(c->B), kRangeThreads, 0, st>>>(lo_dev, hi_dev, tot_dev, next_tot_dev,
                                                                      target_out_dev, c->B, c->prec, c->dec, c->dbits,
                                                                      c->dstride, c->dnbits, c->dec_stop,
                                                                      stream_lengths(c));
    }
    CHECK_LAUNCH();
    return LAC_OK;
}

}  // extern "C"
