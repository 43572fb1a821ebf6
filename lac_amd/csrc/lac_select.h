// lac_select.h -- which kernel runs for a job, as plain host functions: the logits path's
// row-statistics shape (q1_plan) and the pmf decode path (decode_plan), with the capacity
// constants the kernels share with them.  No HIP, no lac_ctx, no allocation: plain C++, so
// tests/test_select_host.py checks every rule without a GPU.  The launchers (q1_launch in
// lac_logits.hip, decode_dispatch in lac_decode.hip) take a plan and launch it.
#pragma once
#include <stdint.h>

#include "lac.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LAC_SEL_HD __host__ __device__
#else
#define LAC_SEL_HD
#endif

// ============================================================ logits row statistics (q1)
// k_q1_stats_rl: 8 table copies beside all 8 LDS slots, or 16 where the row needs only
// kRLLastTrim threads' worth of the last slot
constexpr int kRLRep = 8;
constexpr int kRLRegVec = 8, kRLSlots = 8;       // 16-B vectors per thread in registers, then in LDS slots
constexpr int kRLLastTrim = 704;                 // last-slot threads of the 16-copy form
constexpr int kRLTrimMaxVec = 15 * 1024 + kRLLastTrim;   // rows it holds: 16064 vectors
// k_q1_stats_wide: vectors per thread of a 512-thread block
constexpr int kQ1WideR = 40;
constexpr int kQ1WideThreads = 512;
constexpr int kQ1WideMaxVec = kQ1WideThreads * kQ1WideR;       // registers only
constexpr int kQ1WideL = 11;                                   // + LDS slots (the 32-copy table beside them)
constexpr int kQ1WideSlotMaxVec = kQ1WideThreads * (kQ1WideR + kQ1WideL);
constexpr int kQ1MaxSeg = 16;                    // segments per row (lanes polling partners)

// Row-group shapes (waves per row RW, 16-B vectors per thread R, rolling
// prefetch) of k_q1_stats.  AUTO takes the first listed shape that holds the row
// in registers (measured on MI355X, c3 shape: encode bf16 (8,8,y) 0.75 ms vs
// (8,8,n) 0.79 ms; decode (8,8,n) 70 M sym/s vs 46 M for the spilling (8,8,y)),
// else tiles of (8, 8); LAC_OPT_Q1_SHAPE forces one for both directions (tuning;
// identical results).  10 = tiles of a 16-wave (16,16,n) block per CU, 14 = tiles of
// (16,8) with a rolling prefetch that walks the tiles (pass 1 up, pass 2 down, then
// the next row's first tile).
//
// Round 4 retired the shapes AUTO never reaches (5, 7, 9, 11, 12, 13, 16): each vocabulary
// range resolves to one of 1..4 / 6 (rows <= 4096 vectors), 17 / 18 (<= 8192), 15
// (<= 16384), 22 (<= 26112), 19..21 / 23 (longer) or the tiled fallbacks 8 / 10 / 14,
// and a forced retired number is refused (LAC_E_ARG) instead of running a form no
// default configuration exercises.  Their measurements stay in DESIGN.md section 5b.
constexpr int kQ1Shapes[][3] = {{1, 4, 0}, {2, 8, 0}, {4, 8, 0}, {8, 8, 0}, {8, 16, 0}, {8, 8, 1}, {8, 4, 1}};
// the live tiled forms: shape, then k_q1_stats<RW, R, MULTI, PF, NWB> (MULTI: tiles, rows of any length)
constexpr int kQ1Tiled[][6] = {{1, 1, 4, 0, 0, 8}, {2, 2, 8, 0, 0, 8},  {3, 4, 8, 0, 0, 8},     {4, 8, 8, 0, 0, 8},
                               {6, 8, 8, 0, 1, 8}, {8, 8, 8, 1, 0, 8}, {10, 16, 16, 1, 0, 16}, {14, 16, 8, 1, 1, 16}};
constexpr int kQ1TiledForms = sizeof(kQ1Tiled) / sizeof(kQ1Tiled[0]);
inline bool q1_shape_live(int sh) {
    return sh >= 0 && sh <= 23 && sh != 5 && sh != 7 && sh != 9 && sh != 11 && sh != 12 && sh != 13 && sh != 16;
}

inline int64_t q1_groups_per_chunk(int64_t nvec) {                // 64-vector groups per decode chunk
    const int64_t groups = (nvec + 63) / 64;
    return groups <= 64 ? 1 : (groups + 63) / 64;
}

// Grouped row stats (shapes 19 / 20 / 21): a row in kg segments of `split` vectors
// (a multiple of 64; the last one the rest), one per row slot of the rl kernel
// with NRB = 1 / 2 / 4 rows per block; every segment must fit its slot -- the
// 16-copy form (16064 / 8000 / 4032 vectors) or the 8-copy form (16384 / 8192 /
// 4096).  Decode has no 16-copy form at NRB = 4 (LDS: its group totals).
struct Q1Group {
    int k = 0, split = 0, nrb = 1;
    bool rep16 = false;
    double score = 0;
};
inline int q1_rl_lastn(int nrb, bool rep16) {                     // threads' worth of a row slot's last LDS slot
    const int nt = 1024 / nrb;
    return !rep16 ? nt : nrb == 1 ? kRLLastTrim : nrb == 2 ? 320 : 192;
}
// vectors a row slot holds: 8 in registers + 7 full LDS slots per thread, and the last slot
inline int64_t q1_slot_cap(int nrb, bool rep16) {
    return (int64_t)(kRLRegVec + kRLSlots - 1) * (1024 / nrb) + q1_rl_lastn(nrb, rep16);
}
// the fewest segments, kmin (at least 2) .. kmax, of whole 64-vector groups, each within lim vectors
inline bool q1_split(int64_t nvec, int64_t kmin, int64_t kmax, int64_t lim, Q1Group *g) {
    const int64_t ngrp = (nvec + 63) / 64;
    for (int64_t k = kmin < 2 ? 2 : kmin; k <= kQ1MaxSeg && k <= kmax; k++) {
        const int64_t sp = 64 * ((ngrp + k - 1) / k), last = nvec - (k - 1) * sp;
        if (last > 0 && sp <= lim && last <= lim) {
            g->k = (int)k;
            g->split = (int)sp;
            return true;
        }
    }
    return false;
}
// the fewest segments of this form; score = the row's share of its slots' capacity
// (the bytes a CU keeps in flight) x the share of the XCD's slots in use
inline bool q1_group_form(int cus, int64_t nvec, int nrb, bool rep16, Q1Group *g) {
    const int64_t spx = (int64_t)(cus / 8) * nrb;
    if (!q1_split(nvec, 2, spx, q1_slot_cap(nrb, rep16), g)) return false;
    g->nrb = nrb;
    g->rep16 = rep16;
    g->score = (double)nvec / (g->k * (16384.0 / nrb)) * (double)((spx / g->k) * g->k) / (double)spx;
    return true;
}
// nrb = 0: the best-scoring form (ties: the first, i.e. fewer rows per block and the
// 16-copy form); decode's 8-copy forms score 5 % lower (q1_rl_rep16: its lookups
// are the bound there; encode measured the same either way), and bf16 encode's
// 25 % lower: with the group logic they spill 29-32 VGPRs at the 128 cap (the
// 16-copy ones none), and the round-2 pair form at V = 262144 ran at 59 % of peak
// against 78 % for V = 256000's 16-copy halves
inline bool q1_group(int cus, int64_t nvec, bool dec, bool bf16, int nrb, Q1Group *best) {
    bool any = false;
    for (int n = 1; n <= 4; n *= 2) {
        if (nrb && n != nrb) continue;
        for (int rep16 = 1; rep16 >= 0; rep16--) {
            if (dec && n == 4 && rep16) continue;
            Q1Group g;
            if (!q1_group_form(cus, nvec, n, rep16 != 0, &g)) continue;
            if (!rep16) g.score *= dec ? 0.95 : bf16 ? 0.75 : 1.0;
            if (!any || g.score > best->score + 1e-9) *best = g;
            any = true;
        }
    }
    return any;
}
// Shape 23: rows of > 20480 vectors in kg = ceil(vectors / 20480) segments of one
// 8-wave block each (k_q1_stats_wide's GROUP form); false when the row would need
// more segments than an XCD's CUs.
inline bool q1_wide_group(int cus, int64_t nvec, Q1Group *g) {
    g->nrb = 1;
    return q1_split(nvec, (nvec + kQ1WideMaxVec - 1) / kQ1WideMaxVec, cus / 8, kQ1WideMaxVec, g);
}

// What q1_launch needs to pick a template instance.
enum { Q1_TILED, Q1_RL, Q1_WIDE, Q1_RL_GROUP, Q1_WIDE_GROUP };
struct Q1Plan {
    int shape = 0;                   // 1..23 (a group AUTO chose: 19 / 20 / 21 by rows per block, or 23)
    int family = Q1_TILED;
    int tiled = -1;                  // kQ1Tiled's row: the tiled kernel, or the group forms' repair launch
    int rep = 0, lastn = 0, nt = 0;  // k_q1_stats_rl<REP, LASTN, NT> (rl, rl group)
    bool wide_slots = false;         // k_q1_stats_wide with its LDS slots (rows past kQ1WideMaxVec)
    Q1Group group;                   // the group forms' segments
    int repair = 0;                  // the group forms' gated tiled shape: 10 / 14 / 8
    int64_t groups_per_chunk = 1;
};

inline int q1_tiled_form(int sh) {
    for (int i = 0; i < kQ1TiledForms; i++)
        if (kQ1Tiled[i][0] == sh) return i;
    return -1;
}

// The row-statistics kernel for rows of V logits of type_bytes (2 bf16, 4 f32) on `cus`
// compute units; forced_shape 0 = AUTO, else LAC_OPT_Q1_SHAPE's number.  LAC_E_ARG: a
// forced shape that is retired or does not hold the row.
inline int q1_plan(int cus, int64_t V, int type_bytes, bool dec, int forced_shape, Q1Plan *out) {
    const bool bf16 = type_bytes == 2;
    const int64_t nvec = V / (bf16 ? 8 : 4);
    auto holds = [&](int i) { return nvec <= 64 * kQ1Shapes[i - 1][0] * kQ1Shapes[i - 1][1]; };
    Q1Plan p;
    p.groups_per_chunk = q1_groups_per_chunk(nvec);
    int sh = forced_shape;
    bool grouped = false;
    if (sh == 0) {
        // both directions take the prefetching (8,8) form 6 at 2049..4096 vectors: its decode
        // form spilled around the 8-way multi-sum (4 instead, no prefetch) until round 5
        // streamed the butterfly (127 VGPRs, no spills; profiles/r05/q1dec_pf/)
        static const int order[] = {1, 2, 3, 6};
        // several rows per 16-wave block in registers + LDS slots (shapes 17 / 18; same-box,
        // profiles/r02/q1_rl_rows/): rows of 4097..8192 vectors in both directions (bf16
        // V = 65536 encode 1.48 -> 1.31 ms, f32 c3 1.241 -> 1.200 ms = 87 % of peak, decode
        // stats 2-3 % faster), f32 rows of 2049..4096 vectors in encode (V = 16384: 0.678 ->
        // 0.621 ms).  bf16 c3 keeps shape 6 in both directions (encode 0.651 vs 0.660 ms).
        if (nvec > 4096 && nvec <= 8192) sh = 18;
        else if (!dec && !bf16 && nvec > 2048 && nvec <= 4096) sh = 17;
        for (int i : order) {
            if (sh) break;
            if (holds(i)) sh = i;
        }
        // rows of 8193..16384 vectors: registers + LDS slots (shape 15; same-box, bf16
        // V = 128256 encode 3.23 -> 2.49 ms = 84 % of peak, f32 V = 65536 encode 2.73 ->
        // 2.43 ms, decode 21.5 -> 24.0 M sym/s, profiles/r02/q1_rl/; bf16 decode, once its
        // spills were removed (streamed butterfly, per-group LDS totals, fresh lane index),
        // 220 -> 210 us per step of 4096 rows vs shape 9, profiles/r02/q1_rl_dec/)
        if (sh == 0 && nvec <= 16384) sh = 15;
        // rows of 16385..20480 vectors: one row per CU in the registers of an 8-wave
        // block with a rolling prefetch (shape 22; same-box vs row groups,
        // profiles/r03/wide/prefetch/: bf16 V = 151936 (Qwen2) 70.8 -> 85.6 % of peak,
        // decode stats 270 -> 184-216 us per step; bf16 131080 63 -> 73 %; f32 65540
        // 71.7 -> 80.5 %)
        // Rows of 20481..26112 vectors add 11 vectors per thread in LDS slots (same box,
        // profiles/r03/vocabs/: bf16 V = 202048 (Llama-4) 66.9 -> 81.1 %, bf16 200024
        // (o200k) 65.8 -> 76.0 %, f32 100280 (cl100k) 72.4 -> 80.4 %, f32 102400
        // (DeepSeek) 78.5 -> 86.7 %; f32 decode stats 8-11 % faster).  The bf16 decode form
        // spilled 21 VGPRs there until round 4 (hoisted LDS-DMA offsets and per-batch bin
        // addresses, now recomputed where used): spill-free, bf16 V = 202048 decode stats
        // 313 -> 269 us per step (65.9 -> 76.9 % of peak), 200024 317 -> 275 us
        // (profiles/r04/ab_dec/), so AUTO takes it in both directions
        if (sh == 0 && nvec <= kQ1WideSlotMaxVec) sh = 22;
        // longer rows: row groups (shapes 19 / 20 / 21: segments in row slots of 1 / 2 / 4
        // rows per block), the form that keeps the most bytes in flight (q1_group).
        // Round 2 had whole blocks per segment (kg = 2..4 blocks of 1 or 2 rows): bf16
        // V = 256000 48 -> 78 % of peak (profiles/r02/q1_pair_bf16/), Qwen2 bf16 57 -> 65 %
        // (profiles/r02/q1_groups2/); row slots at any kg: profiles/r03/q1_slots/
        if (sh == 0 && q1_group(cus, nvec, dec, bf16, 0, &p.group)) {
            // where the best slot form has several rows per block, rows go to groups of
            // 8-wave blocks instead (shape 23; same box, profiles/r03/wide/group/: bf16
            // V = 262144 68.6 -> 80.1 % of peak (slots of the 4-row form before), f32
            // 151936 79.6 -> 85.2 % (2-row form); one-row forms stay: bf16 256000 79.3 vs
            // 77.8 %, f32 128256 83.7 vs 82.5 %, f32 262144 82.2 vs 82.1 %)
            // ... and only where those blocks are well filled: segments of ~12500 vectors
            // (f32 V = 100280 / 102400, bf16 200024 / 202048: 61-63 % of a block) ran at
            // 58-70 % against 66-79 % in the slot forms (profiles/r03/vocabs/)
            Q1Group wg;
            grouped = true;
            sh = p.group.nrb == 1 ? 19 : p.group.nrb == 2 ? 20 : 21;
            if (p.group.nrb > 1 && q1_wide_group(cus, nvec, &wg) && nvec >= 0.75 * wg.k * kQ1WideMaxVec) {
                p.group = wg;
                sh = 23;
            }
        }
        // measured at V = 128256 f32: encode tiles of (16,8) with the tile-rolling
        // prefetch 1.98 ms vs 2.18 for tiles of (8,8) (shape 13, its (8,8) form: 2.20)
        // (rows of > 16384 vectors that no group form takes)
        if (sh == 0) sh = dec ? 10 : (!bf16 ? 14 : 8);
    } else if (sh >= 19 && sh <= 21) {
        grouped = q1_group(cus, nvec, dec, bf16, sh == 19 ? 1 : sh == 20 ? 2 : 4, &p.group);
    } else if (sh == 23) {
        grouped = q1_wide_group(cus, nvec, &p.group);
    }
    p.shape = sh;
    // The register + LDS-slot shapes (k_q1_stats_rl), by rows per block:
    //   15 = one row of <= 16384 vectors (16 table copies when <= 16064: trimmed last slot, else 8),
    //   17 = four rows of <= 4096 vectors (4 waves each), 18 = two rows of <= 8192 (8 waves each);
    //   19 / 20 / 21 = their row slots holding a group's segments.  A trimmed last slot (whole waves
    // only) makes room for 16 table copies where the LDS allows it: 17 decodes with 8.
    const int nrb = sh == 15 || sh == 19 ? 1 : sh == 18 || sh == 20 ? 2 : 4;
    if (sh == 15 || (sh >= 17 && sh <= 21)) {
        if (sh >= 19 ? !grouped : nvec > q1_slot_cap(nrb, false)) return LAC_E_ARG;
        const bool trim = sh >= 19 ? p.group.rep16 : nvec <= q1_slot_cap(nrb, true);
        p.family = sh >= 19 ? Q1_RL_GROUP : Q1_RL;
        p.rep = trim && !(sh == 17 && dec) ? 16 : kRLRep;
        p.lastn = q1_rl_lastn(nrb, trim);
        p.nt = 1024 / nrb;
    } else if (sh == 22 || sh == 23) {
        if (sh == 23 ? !grouped : nvec > kQ1WideSlotMaxVec) return LAC_E_ARG;
        p.family = sh == 23 ? Q1_WIDE_GROUP : Q1_WIDE;
        p.wide_slots = sh == 22 && nvec > kQ1WideMaxVec;         // rows past the registers: + LDS slots
    } else {
        // tiles (8, 10, 14) hold any row, 1..4 / 6 a short one (kQ1Shapes: 1..7 only); no retired shape
        if (sh != 8 && sh != 10 && sh != 14 && (sh > 7 || !q1_shape_live(sh) || !holds(sh))) return LAC_E_ARG;
        p.tiled = q1_tiled_form(sh);
    }
    // the group forms' repair: the tiled two-pass shape over the same rows (q1_group_repair)
    if (grouped) p.tiled = q1_tiled_form(p.repair = dec ? 10 : (!bf16 ? 14 : 8));
    *out = p;
    return LAC_OK;
}

// ============================================================ logits one-position step (q1)
// k_q1_step_dec / k_q1_step_enc (lac_logits.hip): one workgroup per stream codes one position
// in one launch, the row held once in registers -- R 16-B vectors per thread of a block of up
// to 16 waves, wave w owning the R * 64 consecutive vectors from w * 64 * R (register j of lane l:
// vector w * 64 * R + 64 j + l, so every load instruction of a wave reads 1 KB in a piece).
constexpr int kQ1StepMaxThreads = 1024;
constexpr int kQ1StepMaxR = 16;
constexpr int kQ1StepMaxVec = kQ1StepMaxThreads * kQ1StepMaxR;   // 16384: bf16 V <= 131072, f32 V <= 65536
// AUTO takes the fused step up to this many streams, beyond them the two-launch path (row
// statistics + k_q1_decode / k_encode): one resident workgroup per compute unit at most.
// Measured on MI355X at V = 32000 bf16 (profiles/r07/step/, us per position, fused / two
// launches): decode 8.94 / 12.02 at 1 stream, 9.15 / 11.96 at 4, 9.60 / 12.79 at 16, 9.52 /
// 12.76 at 64, 10.47 / 12.56 at 256; encode 9.09 / 12.14 .. 9.87 / 14.59 -- the fused step
// wins at every measured count up to one workgroup per CU, so the cap is the CU count.
#ifndef LAC_Q1_STEP_MAX_STREAMS
#define LAC_Q1_STEP_MAX_STREAMS 256
#endif
constexpr int64_t kQ1StepMaxStreams = LAC_Q1_STEP_MAX_STREAMS;
enum { Q1_STEP_AUTO = 0, Q1_STEP_FUSED = 1, Q1_STEP_SPLIT = 2 };   // LAC_OPT_Q1_STEP
struct Q1StepPlan {
    bool fused = false;
    int rc = LAC_OK;                 // LAC_E_ARG: mode 1 on a shape the fused step cannot take
    int threads = 0, R = 0;          // the block, and 16-B vectors per thread (4, 8 or 16)
};
// The fewest vectors per thread whose full block holds the row (the most threads share the
// row: at one stream nothing else hides the loads' latency), then the fewest whole waves.
inline Q1StepPlan q1_step_plan(int cus, int64_t V, int type_bytes, int64_t streams, int mode) {
    Q1StepPlan p;
    const int64_t nvec = V / (type_bytes == 2 ? 8 : 4);
    const int64_t cap = kQ1StepMaxStreams < cus ? kQ1StepMaxStreams : cus;
    const bool fits = nvec >= 1 && nvec <= kQ1StepMaxVec && streams >= 1 && streams <= cap;
    if (mode == Q1_STEP_SPLIT) return p;
    if (!fits) {
        if (mode == Q1_STEP_FUSED) p.rc = LAC_E_ARG;
        return p;
    }
    p.fused = true;
    p.R = nvec <= 4 * kQ1StepMaxThreads ? 4 : nvec <= 8 * kQ1StepMaxThreads ? 8 : 16;
    const int64_t thr = ((nvec + p.R - 1) / p.R + 63) / 64 * 64;
    p.threads = (int)(thr < kQ1StepMaxThreads ? thr : kQ1StepMaxThreads);
    return p;
}

// ================================================================== pmf decode path
#ifndef LAC_LEAN
#define LAC_LEAN 1         // few-stream decode: k_decode_lean ahead of k_decode_seq (probe builds set 0)
#endif
// The lean step's chunks: up to 64 * LeanCW<E> of them, LeanCW bounds per lane -- u64 rows
// two (V = 32000: 125 chunks of 2 iterations, two 16-B loads per lane and step instead of
// four), u32 rows one (dec_chunk_layout's layout).
#ifndef LAC_LEAN_CW32
#define LAC_LEAN_CW32 1          // (2 for u32 rows too: c2 0.849-0.851 vs 0.848-0.850 us, profiles/r06/lean3/cw32/)
#endif
template <typename E> constexpr int LeanCW = sizeof(E) == 8 ? 2 : LAC_LEAN_CW32;
LAC_SEL_HD inline void lean_chunk_layout_n(int64_t V, int vec, int cw, int64_t *CI, int64_t *nch) {
    const int64_t nvec = V / vec, nit = (nvec + 63) / 64, per = 64 * cw;
    const int64_t ci = nit ? (nit + per - 1) / per : 1;
    *CI = ci;
    *nch = (nit + ci - 1) / ci;
}
template <typename E, int VEC>
LAC_SEL_HD inline void lean_chunk_layout(int64_t V, int64_t *CI, int64_t *nch) {
    lean_chunk_layout_n(V, VEC, LeanCW<E>, CI, nch);
}
#ifndef LAC_LEAN_HELPERS
#define LAC_LEAN_HELPERS 16
#endif
constexpr int kLeanHelpers = LAC_LEAN_HELPERS;  // helper waves per stream
// Up to 44 streams: the stats pass of the lean step writes a full CDF copy of every row, so
// its per-step cost grows with the streams, and k_decode_seq's read-only pass overtakes it
// between 32 and 64 (V=32000 u32, decode us per step lean / seq: 8 streams 1.17 / 2.75,
// 16 1.76 / 2.90, 32 2.75 / 3.25, 64 4.52 / 3.91; profiles/r06/lean3/fewstreams/)
#ifndef LAC_LEAN_MAX_STREAMS
#define LAC_LEAN_MAX_STREAMS 44
#endif
constexpr int64_t kLeanMaxStreams = LAC_LEAN_MAX_STREAMS;   // k_decode_lean up to this many streams
constexpr int kLeanHelpMaxStreams = 16;         // above: no helpers (L2: ~2.6 MB ahead per stream)
#ifndef LAC_LEAN_BYTES
#define LAC_LEAN_BYTES (512ll << 20)   // (256 MB: c2 u64 1.47 us per step, 512 MB 1.44: more stats waves per CU)
#endif
constexpr int64_t kLeanBytes = LAC_LEAN_BYTES;  // CDF rows per launch: at most this many bytes
#ifndef LAC_LEAN_ROUNDS
#define LAC_LEAN_ROUNDS 3
#endif
constexpr int kLeanRounds = LAC_LEAN_ROUNDS;    // k_decode_seq one step + lean again, per launch group

// The lac_ctx fields the decode path depends on, in lac_ctx's words (lac_host.h describes each).
struct DecodeKnobs {
    int dpath;
    int64_t wave_decode_min_streams, block_decode_min_streams, block_window_lo, block_window_hi;
    int block_waves, fine_decode, dec_stop;
    bool has_len;
    int64_t chunk_steps;
};
enum { DEC_PER_STEP, DEC_WAVE, DEC_BLOCK, DEC_STATS };
struct DecodePlan {
    int rc = LAC_OK;             // LAC_E_ARG: the per-step path's chunk table would not fit the LDS
    int path = DEC_PER_STEP;
    int vec = 1;                 // entries per 16-byte load (4 u32 / 2 u64), or 1: unaligned rows
    int fine_nr = 0;             // wave: k_decode_wave_fine's NR (2, 4, 8), 0 = k_decode_wave
    int block_nw = 0;            // block: waves per stream (4, 8, 16)
    int G = 0, step_waves = 0;   // per-step: loads per lane and chunk, waves per workgroup (16 or 4)
    bool lean = false, help = false;   // stats: k_decode_lean ahead of k_decode_seq; its prefetching helpers;
    int64_t CI = 0, cs = 0;            //   its iterations per chunk (1..4); steps per launch group;
    bool static_rows = false;          //   stride-0 steps: one row per stream, statistics computed once
};

inline DecodePlan decode_plan(const DecodeKnobs &k, int64_t B, int64_t V, int pmf_bits, int prec, bool aligned16,
                              int64_t step_stride, int64_t stream_stride, int64_t steps) {
    DecodePlan p;
    const int vw = pmf_bits == 32 ? 4 : 2, esize = pmf_bits / 8;
    const bool vec = aligned16 && V % vw == 0 && step_stride % vw == 0 && stream_stride % vw == 0;
    p.vec = vec ? vw : 1;
    const int64_t nit = (V / p.vec + 63) / 64;                  // 64-vector iterations per row
    const bool wave = k.dpath == LAC_PATH_FUSED || (k.dpath == LAC_PATH_AUTO && B >= k.wave_decode_min_streams);
    const bool blockable = vec && nit <= 512;                   // per-iteration totals fit LDS
    if (k.dec_stop) {                       // LAC_OPT_DECODE_STOP: the stats path's kernels implement it
        p.path = DEC_STATS;
    } else if (blockable && (k.dpath == LAC_PATH_BLOCK ||
                             (k.dpath == LAC_PATH_AUTO && !wave &&
                              ((B >= k.block_window_lo && B <= k.block_window_hi) || B >= k.block_decode_min_streams)))) {
        p.path = DEC_BLOCK;
        const int nw = k.block_waves ? k.block_waves : (B >= 1024 ? 4 : B >= 512 ? 8 : 16);
        p.block_nw = nw == 4 || nw == 8 ? nw : 16;
    } else if (k.dpath == LAC_PATH_STATS || k.dpath == LAC_PATH_BLOCK || (k.dpath == LAC_PATH_AUTO && !wave)) {
        p.path = DEC_STATS;
    } else if (wave) {
        p.path = DEC_WAVE;
        if (vec && k.fine_decode && nit <= 512) p.fine_nr = nit <= 128 ? 2 : nit <= 256 ? 4 : 8;
    } else {
        // few streams: 16 waves per stream keep the whole row in flight, 8 loads/lane per chunk
        const bool few = B <= 256;
        p.G = !vec || few ? 8 : pmf_bits == 32 ? 2 : 4;
        p.step_waves = few ? 16 : 4;
        if ((V + 64 * p.vec * p.G - 1) / (64 * p.vec * p.G) * 8 > 64 * 1024) p.rc = LAC_E_ARG;
    }
    if (p.path != DEC_STATS) return p;
    // A static model (stride-0 steps): every step reads the same row per stream, so the
    // statistics are computed once per stream and one launch pair covers any number of steps.
    p.static_rows = step_stride == 0;
    // k_decode_lean: prec <= 50, chunks of at most 4 iterations (V <= 65536 entries: 64 chunk
    // bounds per u32 row, 128 per u64 row), totals lean_total_ok<E> (checked per row).
    // Only for the fewest streams: the stats pass writes as many bytes more as it reads (the
    // CDF), which costs more than the shorter chain saves once enough streams run side by
    // side (round 4, per-vector CDF, V=32000: B=4 1.36 vs 2.66 us/step, 64 3.41 vs 3.96, 128
    // 5.39 vs 5.26; profiles/r04/lean/fewstreams/)
    // Per-stream counts (lac_set_stream_lengths) take k_decode_seq, as LAC_OPT_DECODE_STOP takes
    // this path: the lean step and its prefetching helpers stay unaware of counts, so no
    // helper waits on a decoder that has left at its count.
    int64_t lnch;
    lean_chunk_layout_n(V, p.vec, esize == 8 ? 2 : LAC_LEAN_CW32, &p.CI, &lnch);
    p.lean = LAC_LEAN && vec && prec <= 50 && p.CI <= 4 && V / p.vec > 0 && B <= kLeanMaxStreams && !k.has_len;
    p.cs = p.static_rows ? steps : k.chunk_steps;
    if (p.lean && !p.static_rows) {
        // its CDF buffer holds up to kLeanBytes, so a launch takes at most that many steps' rows
        const int64_t fit = kLeanBytes / (V * esize) / B;
        const int64_t ls = fit < 64 ? 64 : fit / 64 * 64;
        p.cs = ls < p.cs ? ls : p.cs;
    }
    // prefetching helper workgroups for the fewest streams (kLeanHelpers per stream, dealt
    // to the stream's XCD); a static model's rows stay in L2 without them
    p.help = p.lean && !p.static_rows && B <= kLeanHelpMaxStreams;
    return p;
}
