// Host-side check of lac_amd/csrc/lac_select.h -- test infrastructure.
//
// C wrappers over the kernel selection (q1_plan, decode_plan and the helpers they rank
// forms with), flattened to int64 arrays for ctypes (tests/test_select_host.py) and for
// the sanitizer program (sanitize_main.cpp).  Plain C++: nothing else is linked.
#include <stdint.h>

#include "lac_select.h"

extern "C" {

// o[18]: shape, family, rw, r, multi, pf, nwb, rep, lastn, nt, wide_slots, k, split, nrb, rep16, repair,
// groups_per_chunk, the shape of the tiled form (rw .. nwb)
int sc_q1_plan(int cus, int64_t V, int type_bytes, int dec, int forced_shape, int64_t *o) {
    Q1Plan p;
    const int rc = q1_plan(cus, V, type_bytes, dec != 0, forced_shape, &p);
    if (rc) return rc;
    static const int none[6] = {0, 0, 0, 0, 0, 0};
    const int *t = p.tiled >= 0 ? kQ1Tiled[p.tiled] : none;     // (shape, RW, R, MULTI, PF, NWB)
    const int64_t v[18] = {p.shape, p.family, t[1],         t[2],          t[3],        t[4],
                           t[5],    p.rep,    p.lastn,      p.nt,          p.wide_slots, p.group.k,
                           p.group.split, p.group.nrb, p.group.rep16, p.repair, p.groups_per_chunk, t[0]};
    for (int i = 0; i < 18; i++) o[i] = v[i];
    return rc;
}

// q1_group's best slot form for a row (nrb 0: over all forms); o[4]: k, split, nrb, rep16
int sc_q1_group(int cus, int64_t nvec, int dec, int bf16, int nrb, int64_t *o) {
    Q1Group g;
    if (!q1_group(cus, nvec, dec != 0, bf16 != 0, nrb, &g)) return 0;
    o[0] = g.k, o[1] = g.split, o[2] = g.nrb, o[3] = g.rep16;
    return 1;
}

int64_t sc_q1_slot_cap(int nrb, int rep16) { return q1_slot_cap(nrb, rep16 != 0); }
int sc_q1_shape_live(int sh) { return q1_shape_live(sh); }

// o[12]: kRLRep, kRLLastTrim, kRLTrimMaxVec, kQ1WideMaxVec, kQ1WideSlotMaxVec, kQ1MaxSeg, kLeanMaxStreams,
// kLeanHelpMaxStreams, kLeanHelpers, kLeanBytes, kLeanRounds, LeanCW<uint32_t>
void sc_consts(int64_t *o) {
    const int64_t v[12] = {kRLRep,          kRLLastTrim,         kRLTrimMaxVec, kQ1WideMaxVec, kQ1WideSlotMaxVec, kQ1MaxSeg,
                           kLeanMaxStreams, kLeanHelpMaxStreams, kLeanHelpers,  kLeanBytes,    kLeanRounds,
                           LeanCW<uint32_t>};
    for (int i = 0; i < 12; i++) o[i] = v[i];
}

// Where the kernels' position-dependent arithmetic changes (tests/positions.py).
// o[6]: kRLRegVec, kRLSlots, kQ1WideThreads, kQ1WideMaxVec, kQ1WideSlotMaxVec, kQ1StepMaxVec
void sc_layout_consts(int64_t *o) {
    const int64_t v[6] = {kRLRegVec, kRLSlots, kQ1WideThreads, kQ1WideMaxVec, kQ1WideSlotMaxVec, kQ1StepMaxVec};
    for (int i = 0; i < 6; i++) o[i] = v[i];
}

// o[4]: fused, rc, threads, R of the one-position step
void sc_q1_step_plan(int cus, int64_t V, int type_bytes, int64_t streams, int mode, int64_t *o) {
    const Q1StepPlan p = q1_step_plan(cus, V, type_bytes, streams, mode);
    o[0] = p.fused, o[1] = p.rc, o[2] = p.threads, o[3] = p.R;
}

// k_decode_lean's chunks of a row of pmf_bits entries, vec per 16-byte load; o[2]: iterations per chunk, chunks
void sc_lean_chunks(int64_t V, int vec, int pmf_bits, int64_t *o) {
    lean_chunk_layout_n(V, vec, pmf_bits == 64 ? LeanCW<uint64_t> : LeanCW<uint32_t>, &o[0], &o[1]);
}

// kn[10]: dpath, wave_decode_min_streams, block_decode_min_streams, block_window_lo, block_window_hi,
// block_waves, fine_decode, dec_stop, has_len, chunk_steps
// o[12]: rc, path, vec, fine_nr, block_nw, G, step_waves, lean, CI, cs, help, static_rows
void sc_decode_plan(const int64_t *kn, int64_t B, int64_t V, int pmf_bits, int prec, int aligned16,
                    int64_t step_stride, int64_t stream_stride, int64_t steps, int64_t *o) {
    DecodeKnobs k;
    k.dpath = (int)kn[0];
    k.wave_decode_min_streams = kn[1];
    k.block_decode_min_streams = kn[2];
    k.block_window_lo = kn[3];
    k.block_window_hi = kn[4];
    k.block_waves = (int)kn[5];
    k.fine_decode = (int)kn[6];
    k.dec_stop = (int)kn[7];
    k.has_len = kn[8] != 0;
    k.chunk_steps = kn[9];
    const DecodePlan p = decode_plan(k, B, V, pmf_bits, prec, aligned16 != 0, step_stride, stream_stride, steps);
    const int64_t v[12] = {p.rc, p.path, p.vec, p.fine_nr, p.block_nw, p.G, p.step_waves, p.lean, p.CI, p.cs, p.help,
                           p.static_rows};
    for (int i = 0; i < 12; i++) o[i] = v[i];
}

}  // extern "C"
