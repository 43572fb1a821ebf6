// lac_host.h -- the host side shared by liblac.so's translation units: the context
// (lac_ctx, include/lac.h), live kernel timing (ProfScope, lac_profile_*), error
// reporting, and the few host entry points one family calls in another.
#pragma once
#include <stdarg.h>
#include <stddef.h>
#include <string>
#include <vector>

#include "lac_dev.h"
#include "lac_select.h"
#include "lac_fsm.h"
#include "lac_count.h"
#include "lac_history.h"

// ====================================================================== C-ABI
struct lac_ctx {
    int device = 0, prec = 0, pmf_bits = 32;
    int64_t V = 0, B = 0;
    uint64_t cap_bits = 0, cap_words = 0;
    RowStats *stats = nullptr;
    EncState *enc = nullptr;
    DecState *dec = nullptr;
    TailState *tail = nullptr;          // decoder tail in the reference frame (lac_decode_tail_*)
    uint64_t *planeA = nullptr, *planeC = nullptr, *nbits = nullptr;
    uint64_t *own_planeA = nullptr, *own_nbits = nullptr;   // planeA / nbits unless lac_set_output redirects them
    const uint8_t *dbits = nullptr;
    uint64_t dstride = 0;
    const uint64_t *dnbits = nullptr;
    uint8_t *ubits = nullptr;           // lac_decode_open_packed: [B][cap_words * 8] unpacked slots and
    uint64_t *unbits = nullptr;         //                         [B] bit counts, allocated on first use
    // lac_decode_open_window: ubits / unbits are the window and its counts (one open decode at a time)
    const uint8_t *wsrc = nullptr;      //   the borrowed source k_dec_refill reads; null: the open decode has no window
    uint64_t wsrc_stride = 0;
    const uint64_t *wsrc_nbits = nullptr;
    uint64_t *wbase = nullptr;          //   [B] source word that window word 0 holds, allocated on first use
    int mode = 0;                       // 0 encode, 1 decode
    int finished = 0;                   // nbits / planeA hold finished streams (a job, lac_encode_finish)
    int open = 0;                       // streams hold coded symbols since the last reset and are not
                                        // finished: their output is split between calls (lac_set_output refuses)
    const uint64_t *fin_planeA = nullptr, *fin_nbits = nullptr;   // where the last finished job was written
    int path = LAC_PATH_AUTO;           // encode kernel path (lac_set_option)
    int64_t fused_min_streams = 2048;   // AUTO: fused kernel from this many streams
    int64_t chunk_steps = 64;           // split path: steps per row-stats launch
    int dpath = LAC_PATH_AUTO;          // decode kernel path
    int64_t wave_decode_min_streams = 2048;   // measured: the stats path wins at 1024 streams
    int fine_decode = 1;                // one-wave decode: per-iteration totals (k_decode_wave_fine)
    int dec_stop = 0;                   // LAC_OPT_DECODE_STOP: stop before the first undetermined symbol
    int64_t block_decode_min_streams = 1536;  // AUTO below wave_decode_min_streams: block path from here
                                              // (measured after the serial-step rework: the stats path wins
                                              // at 4-128 and 288-1024 streams, block at 160-256 -- its
                                              // 16-wave groups fill the chip in one round up to 256
                                              // streams -- and at 1536; profiles/r01/decode_paths_v2/)
    int64_t block_window_lo = 160, block_window_hi = 256;   // AUTO: block path inside this window too --
                                              // one 16-wave group per stream fills the chip in one round
                                              // while streams <= CUs; set from the CU count at open
    int block_waves = 0;                // block path waves per stream (0 = by stream count)
    int mapping = LAC_MAP_CEIL;         // symbol_to_range flavour (lac_set_option)
    int term = LAC_TERM_FLUSH;          // stream termination flavour
    int cus = 256;                      // compute units (persistent grids)
    int q1_shape = 0;                   // logits stats block shape (0 auto; lac_set_option tuning)
    int q1_step = 0;                    // LAC_OPT_Q1_STEP: the one-position logits calls (0 auto, 1 fused, 2 two launches)
    int topk_form = 0;                  // LAC_OPT_TOPK_FORM: lac_topk_logits' kernel form (0 auto, 1 registers, 2 streamed)
    uint64_t *q1chunks = nullptr;       // logits / stats-path decode: [chunk_steps * B][64] chunk totals
    void *dmeta = nullptr;              // stats-path decode: [chunk_steps * B] DecRowMeta
    int64_t *dresume = nullptr;         //                    [B] first step k_decode_lean left
    void *lcdf = nullptr;               // lean decode: [lean_rows][V] per-entry CDF (entry width)
    uint64_t *lchunk = nullptr;         //              [lean_rows][64] chunk exclusive bounds
    void *lmeta = nullptr;              //              [lean_rows] LeanMeta
    int64_t lean_rows = 0;              //              rows the buffers hold
    int lean_esize = 0;                 //              their entry width (4 / 8 bytes)
    int32_t *dprogress = nullptr;       //              [B] decoder progress for the prefetch helpers
    uint64_t *lwin = nullptr;           //              [B][lwin_stride] the bit streams as big-endian words, zero-padded
    int64_t lwin_words = 0;             //              words lwin holds
    float *q1m = nullptr;               //                [chunk_steps * B] row maxima
    uint64_t *pxch = nullptr;           // row-group stats (shapes 19..21, 23): [8 * cus + 1] words -- a pair of
                                        // maximum words per row slot (<= 4 per CU), then the abort word
    int64_t xch_abort = -1;             // word of pxch holding the last row-group launch's abort flag
    int64_t *slen = nullptr;            // lac_set_stream_lengths: [B] per-stream symbol counts (the context's copy)
    bool has_len = false;               //                         counts are set (kernels get slen, else nullptr)
    // finite-state models (lac_fsm_load, lac_fsm.hip): the prepared model (lac_fsm.h), one allocation
    void *fsm = nullptr;
    FsmLayout fsm_y = {};
    bool fsm_has_next = false;
    int32_t *fsm_state = nullptr;       //   [B] every stream's current state, kept across calls
    int *fsm_flag = nullptr;            //   the load's verdict on `next` (an entry outside [0, K))
    int fsm_busy = 0;                   //   an lac_fsm_decode / lac_count_decode / lac_hist_decode ran since the last lac_decode_open: mid-job
    // adaptive count models (lac_count_load, lac_count.hip): every stream's counts (lac_count.h)
    uint32_t *cnt = nullptr;            //   [B][cnt_y.stride]
    int32_t *cnt_past = nullptr;        //   [B][order] the last symbols, most recent last, -1 absent
    void *cnt_row = nullptr;            //   [B][cnt_y.Vc] entries: the row of a step that fudges
    CountLayout cnt_y = {};
    uint32_t cnt_w[4] = {0, 0, 0, 0};
    // match-history models (lac_hist_load, lac_history.hip): the weights and every stream's ring (lac_history.h)
    const uint64_t *hist_L = nullptr;   //   [P][P] L[i * P + r], shared by all streams
    int32_t *hist_ring = nullptr;       //   [B][P] the last P symbols, -1 unset
    int32_t *hist_pasti = nullptr;      //   [B] the ring's write index
    int32_t *hist_M = nullptr;          //   [B][P] derived: the match lengths of ring / pasti, rebuilt when they are set
    void *hist_row = nullptr;           //   [B][4 ceil(V / 4)] entries: the row of a step that fudges
    int *hist_flag = nullptr;           //   lac_hist_set_state's verdict on the state it was handed
    int hist_P = 0;
    // live kernel timing (lac_profile_enable): hipEvent pairs around launches
    bool prof = false;
    std::vector<hipEvent_t> ev_pool;
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> ev_used;   // kernel id, (start, stop)
    size_t ev_next = 0;
};

enum { KID_ROW_STATS = 0, KID_ENCODE = 1, KID_FINISH = 2, KID_DECODE = 3, KID_FUSED = 4, KID_DECODE_WAVE = 5,
       KID_Q1_STATS = 6, KID_Q1_DECODE = 7, KID_COUNT = 8 };
// the stats-path decode (k_dec_stats + k_decode_seq) reports under KID_DECODE

static inline hipEvent_t ev_get(lac_ctx *c) {
    if (c->ev_next == c->ev_pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        c->ev_pool.push_back(e);
    }
    return c->ev_pool[c->ev_next++];
}

// Brackets one launch with events on its stream when profiling is on.
struct ProfScope {
    lac_ctx *c;
    int kid;
    hipStream_t st;
    hipEvent_t a = nullptr, b = nullptr;
    ProfScope(lac_ctx *c_, int kid_, hipStream_t st_) : c(c_), kid(kid_), st(st_) {
        if (c->prof && kid >= 0) {
            a = ev_get(c);
            b = ev_get(c);
            if (a && b) (void)hipEventRecord(a, st);
        }
    }
    ~ProfScope() {
        if (c->prof && a && b) {
            (void)hipEventRecord(b, st);
            c->ev_used.push_back({kid, {a, b}});
        }
    }
};

// Error reporting (lac_last_error): the message of the last failing call on this thread.
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIPCHK(x)                                                                          \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) return fail(LAC_E_HIP, "%s: %s", #x, hipGetErrorString(e_)); \
    } while (0)

#define CHECK_LAUNCH() HIPCHK(hipGetLastError())

static inline hipStream_t S(void *s) { return reinterpret_cast<hipStream_t>(s); }

// The per-stream symbol counts as the kernels take them: null while none are set, so every
// kernel then computes what it did before counts existed.
static inline const int64_t *stream_lengths(const lac_ctx *c) { return c->has_len ? c->slen : nullptr; }

// Encode bookkeeping for lac_set_output / lac_pack_bits: a call that coded symbols leaves the
// streams open; a job or finish closes them and records which buffers hold the result.
static inline void enc_mark_open(lac_ctx *c) {
    c->open = 1;
    c->finished = 0;
}
static inline void enc_mark_finished(lac_ctx *c) {
    c->open = 0;
    c->finished = 1;
    c->fin_planeA = c->planeA;
    c->fin_nbits = c->nbits;
}

// encode family (lac_encode.hip), for the logits path's encode (q1_encode)
int enc_reset_launch(lac_ctx *c, hipStream_t st);
int enc_stats_launch(lac_ctx *c, const int32_t *sym, int64_t t0, int64_t n, uint64_t *trace, hipStream_t st);
int enc_finish_launch(lac_ctx *c, int term, hipStream_t st);
// decode family (lac_decode.hip): the per-chunk-of-steps buffers the stats path and the
// logits decode share
int ensure_chunk_buffers(lac_ctx *c);
