/*
 * lac.h -- C-ABI of liblac.so, the MI355X (gfx950) arithmetic coder.
 *
 * Plain pointers and sizes only; HIP streams are passed as `void *`
 * (a hipStream_t, NULL = the default stream).  Device pointers are
 * caller-owned and borrowed for the duration of the call (decode: for the
 * decode session).  One handle <-> one device; a handle is not thread-safe,
 * independent handles are.
 *
 * Each entry point replaces a piece of the reference's predictor->coder call
 * surface (/root/reference):
 *
 *   lac_open / lac_encode_reset   A_to_bin.__init__ state l=0, h=2^prec-1
 *                                 (arith_code.py:157-164); AC(pred, prec) (:144-155)
 *   lac_encode                    A_to_bin.step/run per symbol (:187-192, :207-211):
 *                                 receive_symbol (:169-175) with
 *                                 CDFPredictor.symbol_to_range/fudged_dist
 *                                 (:83-110) + decide_bit/emit_bit (:176-186),
 *                                 for B independent streams, T steps per call
 *   lac_encode_finish             A_to_bin.flush (:193-202) + bits() carry
 *                                 resolution (:227-246) + group_bits (:336-347)
 *   lac_encoded_lengths /         bytes(group_bits(bits(...))) of measure_compress
 *   lac_copy_bits                 (:401-420): L bits, MSB first, zero padded
 *   lac_flush_digits              the raw digits flush() yields (:193-202)
 *   lac_decode_open               A_from_bin.__init__ (:248-256) over a bitstream
 *   lac_decode_step(s)            A_from_bin.step/run (:264-299, :322-326) with
 *                                 CDFPredictor.val_to_symbol (:94-97); n symbols
 *                                 out per stream (the reference stores no n)
 *
 * Status codes: 0 = OK, negative = error; lac_last_error() describes the last
 * failure on the calling thread.  Per-stream coder errors are sticky and are
 * reported by lac_stream_status (the reference raises AssertionError or hangs):
 *   LAC_E_SYMBOL_RANGE  symbol not in [0, V)       arith_code.py:100-101
 *   LAC_E_ZERO_WIDTH    zero-probability symbol on the unfudged path
 *                       (the reference loops forever)
 *   LAC_E_TABLE         all-zero row, or row total >= 2^64
 *   LAC_E_DECODE_RANGE  decoded range misses the value  arith_code.py:277-278
 *   LAC_E_CAPACITY      stream exceeded capacity_bits
 *   LAC_E_PREC          prec outside [2, 61] or 2^(prec-1) < V
 *   LAC_E_FLUSH_ZERO_WIDTH  A_from_bin.flush met a zero-width candidate symbol
 *                       (the reference raises ZeroDivisionError, arith_code.py:307)
 *   LAC_E_FLUSH_LOOP    A_from_bin.flush emits symbols that leave [l, h]
 *                       unchanged (the reference loops forever, :308-313)
 *
 * The per-stream contract, the same on every encode and decode kernel form (path, straight or
 * general block, job or separate calls, fused or split, windowed or not):
 *   Precedence.  An encode step tests, in this order, the symbol's range (LAC_E_SYMBOL_RANGE),
 *     the table (LAC_E_TABLE), a zero width at the symbol (LAC_E_ZERO_WIDTH) and, after the
 *     narrowing, the output capacity (LAC_E_CAPACITY: a stream holds whole words,
 *     ceil(capacity_bits / 64) + 1 of them, and fails at the first step whose digits pass them);
 *     a step with several defects reports the first.  A decode step tests the table
 *     (LAC_E_TABLE), then the registers (x outside [l, h]) and the decoded range
 *     (LAC_E_DECODE_RANGE).
 *   err_step is the stream's nsym at the failing symbol: symbols coded since the last
 *     lac_encode_reset / lac_decode_open, whatever calls they came in -- a job cut into several
 *     lac_encode or lac_decode_steps calls reports the step one call reports.  It is -1 while the
 *     status is 0.  A stream whose flush does not fit (lac_encode_finish, or a job's finish) gets
 *     LAC_E_CAPACITY with err_step = the symbols it holds; a stream refused at lac_decode_open
 *     (LAC_E_ARG) has err_step 0.
 *   Frozen.  A symbol, table or zero-width error, and every decode error, leaves the stream
 *     exactly as it was before the failing step: registers, counters (nsym, L, pos, det / ndet),
 *     plane words and trace entries (the failing step's and all later ones are not written).  A
 *     capacity error happens after the narrowing: l, h and the plane registers are those of the
 *     failing step, the same on every form, and nsym still excludes it.  From then on every
 *     step is a no-op for the stream -- nothing of it depends on the symbols and rows it is given,
 *     decode writes -1 to its sym_out entry, in this call and every later one --, lac_encode_finish
 *     gives it 0 bits, and only lac_encode_reset (a job's included) / lac_decode_open clears the
 *     status.  The other streams of the batch are not affected in any way.
 */
#ifndef LAC_H
#define LAC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lac_ctx lac_ctx;

enum {
    LAC_OK = 0,
    LAC_E_ARG = -1,
    LAC_E_PREC = -2,
    LAC_E_SYMBOL_RANGE = -3,
    LAC_E_ZERO_WIDTH = -4,
    LAC_E_TABLE = -5,
    LAC_E_DECODE_RANGE = -6,
    LAC_E_CAPACITY = -7,
    LAC_E_HIP = -8,
    LAC_E_STATE = -9,
    LAC_E_FLUSH_ZERO_WIDTH = -10,
    LAC_E_FLUSH_LOOP = -11,
    LAC_E_UNDETERMINED = -12      /* not a failure: with LAC_OPT_DECODE_STOP a stream stopped before
                                     the first symbol its bits do not determine, registers and
                                     counters as they were before that symbol (lac_decode_get_state) */
};

enum {                       /* lac_set_option */
    LAC_OPT_ENCODE_PATH = 1,       /* LAC_PATH_*: which encode kernels run */
    LAC_OPT_FUSED_MIN_STREAMS = 2, /* AUTO picks the fused kernel from this many streams (2048) */
    LAC_OPT_MAPPING = 3,           /* LAC_MAP_*: how a symbol's CDF range maps onto [l, h] */
    LAC_OPT_TERMINATION = 4,       /* LAC_TERM_*: how a stream is closed */
    LAC_OPT_DECODE_PATH = 5,       /* LAC_PATH_*: SPLIT = one 4-wave workgroup per stream and step,
                                      FUSED = one wave per stream, all steps of a call in one launch;
                                      STATS, BLOCK = see LAC_PATH_STATS / LAC_PATH_BLOCK;
                                      AUTO = FUSED from 2048 streams, BLOCK at 5/8 CUs .. CUs streams
                                      (160-256 on MI355X) and from 1536, else STATS */
    LAC_OPT_Q1_SHAPE = 6,          /* logits path row-stats shape: 0 = auto (default), 1..4 / 6 = (waves per
                                      row, vectors/thread, rolling prefetch) (1,4,n) (2,8,n) (4,8,n)
                                      (8,8,n) / (8,8,y), 8 = tiles of (8,8,n), 10 = tiles of a
                                      16-wave (16,16,n) block, 14 = tiles of (16,8) with a
                                      tile-walking prefetch, 15 = 16-wave, 8 vectors/thread in
                                      registers + 8 in LDS (rows <= 16384 vectors; 16 table copies
                                      when the row fits a trimmed last slot, <= 16064 vectors),
                                      17 / 18 = the same register + LDS form with 4 rows of
                                      <= 4096 / 2 rows of <= 8192 vectors per 16-wave block,
                                      19 / 20 / 21 = row groups: a row of > 16384 vectors in
                                      2..16 segments, one per row slot of 1 / 2 / 4 rows per
                                      16-wave block (the forms of 15 / 18 / 17; slots are
                                      numbered across the blocks of an XCD, so a segment count
                                      need not divide the blocks); AUTO picks the form that
                                      fills its slots best (f32 V = 128256: 2 slots of 1 row
                                      per block), 22 = one row of <= 20480 vectors per 8-wave
                                      block, whole in registers (+ LDS slots up to 26112),
                                      23 = groups of such blocks (AUTO where the slot form has
                                      several rows per block: bf16 V = 262144, f32 V = 151936);
                                      5, 7, 9, 11, 12, 13 and 16 are retired (AUTO never took
                                      them) and refused with LAC_E_ARG; identical results,
                                      only speed differs */
    LAC_OPT_DECODE_FINE = 7,       /* one-wave decode (FUSED path): 1 = one total per 64 vectors of
                                      the row, so only 1 KB is re-read after the search (default,
                                      rows <= 131072 u32 / 65536 u64 entries); 0 = <= 64 chunk totals */
    LAC_OPT_BLOCK_WAVES = 8,       /* BLOCK decode path: waves per stream (4, 8, 16; 0 = by stream
                                      count, the default) */
    LAC_OPT_DECODE_STOP = 9,       /* 1: a decoding stream stops before the first symbol its bits do
                                      not determine (decide_symbol's ls != hs, arith_code.py:268-273)
                                      with LAC_E_UNDETERMINED, registers unchanged, instead of decoding
                                      on over zero padding; decodes then take the STATS path.  0 =
                                      off (default).  For decoders that stop where the reference's
                                      run(bits, stop=0) stops (lac_amd.coder.A_from_bin) */
    LAC_OPT_Q1_STEP = 10,          /* lac_decode_logits_step / lac_encode_logits_step: 0 = auto (default):
                                      the fused one-launch step where it holds the job -- rows of
                                      <= 16384 vectors (bf16 vocab <= 131072, f32 <= 65536) and few
                                      enough streams --, else the two launches of the `steps = 1`
                                      calls; 1 = fused (a shape it cannot take: LAC_E_ARG from the step
                                      call, nothing launched, no state changed); 2 = the two-launch
                                      path.  Identical results, only speed differs */
    LAC_OPT_TOPK_FORM = 11         /* lac_topk_logits: 0 = auto (default): the registers form where a row is
                                      <= 16384 vectors (bf16 vocab <= 131072, f32 <= 65536), else the
                                      streamed form; 1 = registers (a longer row: LAC_E_ARG from the call,
                                      nothing launched or written); 2 = streamed (any row).  Identical
                                      results, only speed differs */
};
enum {
    LAC_MAP_CEIL = 0,              /* CDFPredictor.symbol_to_range + fudged_dist (arith_code.py:83-110) */
    LAC_MAP_FLOOR = 1              /* Predictor.symbol_to_range (arith_code.py:69-70) and
                                      ACSampler's Region.map (arithmetic_coding.py:160-168) */
};
enum {
    LAC_TERM_FLUSH = 0,            /* A_to_bin.flush (arith_code.py:193-202) */
    LAC_TERM_ACSAMPLER = 1         /* ACSampler.flush_compress: step(1,2,3) + carry flush
                                      (arithmetic_coding.py:50-56) */
};
enum {
    LAC_PATH_AUTO = 0,             /* fused if streams >= fused_min_streams, else split */
    LAC_PATH_SPLIT = 1,            /* row-stats kernel over all (step, stream) rows + coder kernel */
    LAC_PATH_FUSED = 2,            /* one wave per stream: row scan + coder in one kernel */
    LAC_PATH_STATS = 3,            /* decode only: chunk totals of every (step, stream) row in one
                                      full-chip kernel, then a per-stream sequential kernel that
                                      re-reads one chunk per step */
    LAC_PATH_BLOCK = 4             /* decode only: one 4/8/16-wave workgroup per stream, all steps in
                                      one launch; the other waves stream row t+1 while wave 0 decodes
                                      step t (AUTO at 5/8 CUs .. CUs and 1536-2047 streams; rows <= 512 iterations of
                                      64 16-B vectors, 16-B aligned, else STATS) */
};

/* Library identification and the last error message of this thread. */
const char *lac_version(void);
const char *lac_last_error(void);

/* Create a coder for `streams` independent streams over a `vocab`-symbol
 * alphabet at `prec` bits (arith_code.py:157-162), tables of `pmf_bits` = 32
 * (uint32) or 64 (uint64) entries, each stream holding up to
 * `capacity_bits` output bits.  Allocates all device state on `device`. */
int lac_open(int device, int prec, int64_t vocab, int64_t streams, int pmf_bits,
             uint64_t capacity_bits, lac_ctx **out);
int lac_close(lac_ctx *ctx);

/* Tune a context (LAC_OPT_*); results are identical on every path. */
int lac_set_option(lac_ctx *ctx, int option, int64_t value);

/* Per-stream symbol counts: streams of different lengths in one batch.  len_dev: int64[streams]
 * in device memory, copied into the context on `stream` (the caller's buffer is not borrowed);
 * NULL clears.  While set, stream b takes part in a step only while the symbols it has coded
 * since the last reset / lac_decode_open (EncState.nsym / DecState.nsym) number fewer than
 * len[b] -- the base is that count, not the step index of a call, so encoding in calls of 50 +
 * 80 steps equals one call of 130.  For a stream that has reached its count a step is a no-op:
 * its state, planes, status and nsym do not change and it raises no error; encode does not
 * inspect its sym entry or write its trace entry; decode writes -1 to its sym_out entry.  The
 * memory of its table or logits row must be addressable, but the row's contents are never
 * observable: not in any stream's bits, outputs, status or registers.  A count <= 0 ends the
 * stream from the start (its finish is the flush of a fresh state, as a zero-symbol job's); a
 * count larger than the steps given is simply not reached.  Counts persist across
 * lac_encode_reset, the jobs' implicit reset and lac_decode_open, and are no part of
 * lac_enc_state / lac_dec_state.  With LAC_OPT_DECODE_STOP a stream stops at whichever comes
 * first; reaching the count leaves status 0.  With no counts set every result is what it was.
 *
 * Which kernels skip a dead row (never fetch it) and which merely ignore it:
 *   skip    k_encode_fused (loop and prefetch bound), k_row_stats, k_encode; k_decode_wave,
 *           k_decode_wave_fine, k_decode_block, k_decode_step, k_dec_stats, k_decode_seq; the
 *           coder kernels of the logits path (k_encode over the q1 statistics, k_q1_decode)
 *   ignore  the q1 row-statistics kernels of the logits path (k_q1_stats, _rl, _wide, single
 *           block and row group forms): a dead logits row is read and quantised like any other
 *           -- whatever it holds (zeros, NaN) raises nothing -- and its statistics are never
 *           consumed.  No participant of a row group's exchange leaves early.  So on the
 *           logits path counts save the coder kernels' work but no row traffic: every padded
 *           row is still fetched once by these kernels, and their encode form also loads the
 *           dead step's sym entry (clamped into [0, V], used for nothing that is consumed).
 *           Skipping dead rows in their single-block forms is open work.
 *   route   few-stream decodes take k_decode_seq instead of the lean step (k_decode_lean and its
 *           prefetching helpers know no counts), as LAC_OPT_DECODE_STOP takes the stats path.
 * lac_decode_tail_begin / lac_decode_tail_step (one stream's tail in the reference frame)
 * return LAC_E_STATE while counts are set; lac_quantize_logits materialises tables and ignores
 * counts. */
int lac_set_stream_lengths(lac_ctx *ctx, const int64_t *len_dev, void *stream);

/* Reset every stream to l = 0, h = 2^prec - 1 with an empty output. */
int lac_encode_reset(lac_ctx *ctx, void *stream);

/* Encode `steps` symbols per stream.  Row (t, b) of the integer pmf starts at
 * element t*step_stride + b*stream_stride of pmf_dev (a stride of 0 re-uses
 * one row: a static model); sym_dev is int32 [steps][streams].  trace_dev,
 * when not NULL, receives per (t, b) two uint64 {E, k}: the k >= 0 digits the
 * symbol emitted, as the integer E = sum d_i 2^(k-1-i) (first digit 0..3,
 * the rest 0/1).  Asynchronous on `stream`. */
int lac_encode(lac_ctx *ctx, const void *pmf_dev, int64_t step_stride, int64_t stream_stride,
               const int32_t *sym_dev, int64_t steps, uint64_t *trace_dev, void *stream);

/* One whole job in one call: reset every stream, encode `steps` symbols (as
 * lac_encode), flush and pack (as lac_encode_finish).  The batched counterpart
 * of bytes(group_bits(AC(...).to_bin.bits(symbols))) (arith_code.py:207-246,
 * :401-420).  At >= 2048 streams this is a single kernel launch. */
int lac_encode_job(lac_ctx *ctx, const void *pmf_dev, int64_t step_stride, int64_t stream_stride,
                   const int32_t *sym_dev, int64_t steps, uint64_t *trace_dev, void *stream);

/* Keep each stream's registers but drop its completed output words, so the
 * stream continues in at most 64 bits of its capacity.  For callers that read
 * every symbol's digits from trace_dev (A_to_bin.step/run, arith_code.py:
 * 187-211, which yield digits as they go): after a rebase the packed output of
 * lac_encode_finish holds only the tail, while lac_flush_digits stays exact.
 * Asynchronous on `stream`. */
int lac_encode_rebase(lac_ctx *ctx, void *stream);

/* Drain settled output mid-job, so that capacity_bits bounds the bits coded between two drains
 * and not the stream: each stream's settled prefix -- whole 64-bit words, resolved to their final
 * bytes -- is appended to the caller's slot b at dst_dev + b * dst_stride_bytes + fill_dev[b],
 * fill_dev[b] (uint64 [streams], in/out: bytes already in each slot) grows by the 8 g bytes
 * written, and the stream goes on coding in the words that remain (L shrinks by 64 g).  One
 * launch (k_enc_drain, one wave per stream) that reads only the words a stream holds;
 * asynchronous on `stream`, no host synchronisation, no allocation.  Every encode call, the
 * logits calls, lac_encode_get_state / set_state (they describe the remaining words with the
 * smaller L) and lac_set_output buffers work on the drained context as on any other.
 *   What a drain holds back (lac_amd/csrc/lac_drain.h):
 *   1. without a certain state, everything from the last word below the active one whose resolved
 *      value is neither 0 nor 2^64 - 1 (the guard word: a later carry of +-1 cannot pass it);
 *   2. in a certain state (0 <= l and h < 2^prec: no later digit carries) only the active word.
 *   The kept first word is stored resolved (plane C zero).
 * Contract, per stream: the bytes drained over all calls followed by the bytes of the final
 * lac_encode_finish are the bytes of the same symbols coded with no drain, and 8 * (drained
 * bytes) + nbits is that job's bit count.  The caller owns the drained bytes and their count:
 * they are no part of lac_enc_state, and lac_encode_reset does not touch fill_dev.  Registers,
 * nsym, status and err_step, traces, lac_flush_digits and per-stream counts mean what they did.
 *   All or nothing per stream: a stream whose 8 g bytes do not fit dst_stride_bytes - fill_dev[b]
 *   (or whose fill_dev[b] is no multiple of 8) drains nothing and changes nothing -- not an error;
 *   a later call with room takes it.  No byte at or past dst_stride_bytes of a slot is written.
 *   A stream with a sticky error, a finished stream and one of at most 64 bits do nothing.
 * Refused before anything is launched, nothing changed: LAC_E_STATE while a decode is open, or
 * after lac_encode_finish / a job with no lac_encode_reset since (plane A holds packed bytes
 * then); LAC_E_ARG for a NULL dst_dev or fill_dev, or dst_dev, fill_dev or dst_stride_bytes not
 * a multiple of 8. */
int lac_encode_drain(lac_ctx *ctx, uint8_t *dst_dev, uint64_t dst_stride_bytes, uint64_t *fill_dev, void *stream);

/* Flush every stream and resolve carries into packed bytes (asynchronous). */
int lac_encode_finish(lac_ctx *ctx, void *stream);

/* Synchronise `stream`; err_host[streams] / err_step_host[streams] (either may
 * be NULL) receive each stream's sticky status and the step it failed at.
 * Returns the first non-zero stream status, or LAC_OK. */
int lac_stream_status(lac_ctx *ctx, int32_t *err_host, int64_t *err_step_host, void *stream);

/* After lac_encode_finish: synchronise and copy the bit length of each stream. */
int lac_encoded_lengths(lac_ctx *ctx, uint64_t *nbits_host, void *stream);

/* Device view of the encoded streams: stream b's bytes start at
 * bits_dev + b*stride_bytes, nbits_dev[b] bits, MSB first, zero padded. */
int lac_encoded_device(lac_ctx *ctx, const uint8_t **bits_dev, uint64_t *stride_bytes,
                       const uint64_t **nbits_dev);

/* Synchronise and copy stream b's packed bytes to dst_host + b*dst_stride. */
int lac_copy_bits(lac_ctx *ctx, uint8_t *dst_host, uint64_t dst_stride, void *stream);

/* Same, device to device (asynchronous on `stream`). */
int lac_copy_bits_dev(lac_ctx *ctx, uint8_t *dst_dev, uint64_t dst_stride, void *stream);

/* Per-stream bit counts (uint64 [streams]) copied device to device (async). */
int lac_copy_nbits_dev(lac_ctx *ctx, uint64_t *dst_dev, void *stream);

/* The encoded streams packed back to back for the wire (after lac_encode_finish): a
 * header of every stream's bit count in `hdr_bytes` = 2 or 4 bytes each (little
 * endian), then stream b's ceil(nbits_b / 8) bytes (measure_compress's
 * bytes(group_bits(bits())), arith_code.py:401-420) for b = 0, 1, ...; *len_dev
 * (device uint64) receives the total length.  dst_dev holds at least
 * streams * (hdr_bytes + 8 * ceil(capacity_bits / 64)) bytes.  Two small launches,
 * asynchronous on `stream`: the multi-GPU gather's payload (lac_amd.dist).
 * LAC_E_ARG for hdr_bytes = 2 when the context's streams can hold 65536 bits or more
 * (8 * 8 * ceil(capacity_bits / 64) >= 65536: the count would not fit); LAC_E_STATE
 * unless the last encode call finished the streams (lac_encode_job,
 * lac_encode_logits_job, lac_encode_finish) and no decode is open. */
int lac_pack_bits(lac_ctx *ctx, uint8_t *dst_dev, int hdr_bytes, uint64_t *len_dev, void *stream);

/* lac_pack_bits appending to a buffer of several jobs (the gatherer's per-batch
 * outbox, lac_amd.dist.BitstreamGatherer): the packed job is written at byte offset
 * *base_dev of dst_dev (0 when base_dev is NULL; device memory, read by the kernel,
 * so jobs chain without a host round trip), *end_dev (device) receives base + the
 * packed length, and *len_out, when not NULL, the packed length -- len_out may be
 * host memory from lac_host_alloc (its device address), which the host reads once
 * the launch has completed, with no copy.  A job that would pass dst_bytes writes
 * nothing: *end_dev = base and *len_out = UINT64_MAX.  Same refusals as
 * lac_pack_bits. */
int lac_pack_bits_at(lac_ctx *ctx, uint8_t *dst_dev, uint64_t dst_bytes, int hdr_bytes, const uint64_t *base_dev,
                     uint64_t *end_dev, uint64_t *len_out, void *stream);

/* The packing kernel of lac_pack_bits_at over `jobs` finished jobs at once, no
 * context: job j's plane A at planeA_dev + j * plane_stride uint64 words (streams
 * slots of cap_words each: a context's plane A after its job, e.g. buffers
 * lac_set_output gave it) and its bit counts at nbits_dev + j * streams.  The jobs are
 * packed back to back from byte *base_dev (0 when NULL) of dst_dev; ends_dev[j]
 * (device) receives the end of job j and lens_out[j] (when not NULL; host memory from
 * lac_host_alloc allowed) its packed length.  One launch on `device`, asynchronous on
 * `stream`; same header rule and fit test as lac_pack_bits_at, per job. */
int lac_pack_jobs(int device, const uint64_t *planeA_dev, uint64_t plane_stride, const uint64_t *nbits_dev,
                  int64_t jobs, int64_t streams, uint64_t cap_words, uint8_t *dst_dev, uint64_t dst_bytes,
                  int hdr_bytes, const uint64_t *base_dev, uint64_t *ends_dev, uint64_t *lens_out, void *stream);

/* The inverse of lac_pack_jobs, for the receiving side: one launch on `device`, asynchronous
 * on `stream`, no context.  `jobs` packed jobs lie back to back from byte *base_dev (0 when
 * NULL; device memory) of src_dev, each exactly as lac_pack_jobs writes it: a header of
 * `streams` bit counts of hdr_bytes = 2 or 4 bytes each, then each stream's ceil(nbits / 8)
 * bytes.  hdr_bytes = 0: the payload carries no header and job j's counts are
 * counts_dev[j * streams + b] (required then, ignored otherwise): the body of a LAC1
 * container (lac_amd.container), whose counts travel in its own header.  src_dev may have
 * any alignment.  Stream b of job j is written at bits_dev + j * job_stride_bytes +
 * b * stride_bytes in the form lac_decode_open takes -- the stream's bytes in memory order,
 * then zeros: all stride_bytes of the slot are written -- and its bit count to
 * nbits_dev[j * streams + b]; ends_dev[j] (may be NULL) receives the byte offset just past
 * job j and status_dev[j] (may be NULL) the job's verdict.  Bytes between slots
 * (stride_bytes * streams < job_stride_bytes) and everything outside the `jobs` regions are
 * never written.  Source and destination must not overlap.
 * The payload is untrusted: no load touches a byte outside [src_dev, src_dev + src_bytes)
 * and no store falls outside a slot, whatever the counts claim (sums saturate).
 *   A job whose header or payload would pass src_bytes: status LAC_E_ARG, ends_dev[j] = the
 *   job's start, every stream's count UINT64_MAX and every slot zero; so for every later job
 *   of the call (their start is unknown; ends_dev = that same start).  Earlier jobs are
 *   unaffected.
 *   A stream whose count exceeds 8 * stride_bytes: its slot is zero and its count the
 *   claimed one (lac_decode_open then fails that stream with its sticky LAC_E_ARG), status
 *   LAC_E_CAPACITY unless LAC_E_ARG applies; the job's other streams are unpacked.
 * Refused with LAC_E_ARG before anything is launched: hdr_bytes not 0, 2 or 4; hdr_bytes = 0
 * with counts_dev NULL; jobs < 0 (or > 65535) or streams <= 0; bits_dev, stride_bytes or
 * job_stride_bytes not a multiple of 8; job_stride_bytes < streams * stride_bytes while
 * jobs > 1; src_dev, bits_dev or nbits_dev NULL.  jobs = 0 is LAC_OK with no launch. */
int lac_unpack_jobs(int device, const uint8_t *src_dev, uint64_t src_bytes, int hdr_bytes,
                    const uint64_t *counts_dev, const uint64_t *base_dev,
                    int64_t jobs, int64_t streams,
                    uint8_t *bits_dev, uint64_t stride_bytes, uint64_t job_stride_bytes,
                    uint64_t *nbits_dev, uint64_t *ends_dev, int32_t *status_dev, void *stream);

/* Redirect where the context's encodes write their output: plane A (streams *
 * cap_words + 1 uint64, the packed bytes after the job) and the bit counts (streams
 * uint64), caller-owned device buffers that must outlive their use; NULL, NULL
 * restores the context's own.  Every later call that reads or writes the output
 * (encode, finish, lac_copy_bits*, lac_encoded_*, lac_pack_bits*, lac_decode_open
 * with no bits) uses them, so consecutive jobs can leave their output in separate
 * buffers with no copy (lac_amd.dist.BitstreamGatherer packs a batch of them at once,
 * off the encode's stream).
 * Only between jobs: LAC_E_STATE (nothing changed) while a decode is open, or while the
 * streams hold coded symbols that are not finished -- an lac_encode / lac_encode_logits
 * call (or an lac_encode_set_state with symbols) since the last lac_encode_reset, not yet
 * followed by lac_encode_finish: those streams have written part of their planes to the
 * current buffers, and the finish would carry-add over the new ones.  Redirect before a
 * job's first call (lac_encode_job does its own reset) or after it finished.
 * Afterwards the context counts as finished (lac_pack_bits*) exactly when the new
 * buffers are the ones its last finished job was written to (showing that job again);
 * any other buffers need the next finished job first. */
int lac_set_output(lac_ctx *ctx, uint64_t *planeA_dev, uint64_t *nbits_dev);

/* Pinned host memory mapped into the device's address space, coherent (kernels'
 * stores are visible to the host when the launch completes), zero-filled:
 * *host_out is the host address, *dev_out the address kernels use.  For the few
 * words the host reads back per job (lac_pack_bits_at's len_out). */
int lac_host_alloc(uint64_t bytes, void **host_out, void **dev_out);
int lac_host_free(void *host);

/* Synchronise and copy each stream's coder registers l, h (A_to_bin.l/.h,
 * arith_code.py:161-162); either pointer may be NULL. */
int lac_encoder_registers(lac_ctx *ctx, int64_t *l_host, int64_t *h_host, void *stream);

/* The digits flush() emitted per stream (at most 8): digits_host[streams][8],
 * count_host[streams].  Synchronises. */
int lac_flush_digits(lac_ctx *ctx, int8_t *digits_host, int32_t *count_host, void *stream);

/* Encoder checkpoint / resume.  Everything an encoder holds per stream: its registers
 * and counters (A_to_bin's l, h and emitted bits, arith_code.py:157-163, in the O(1)
 * renormalisation's plane form) and the output words written so far.  get copies
 * them to the host; set restores them into a context of the same prec, vocab,
 * streams and capacity, so a job can stop after any lac_encode call and continue
 * later -- in this process or another -- bit for bit.  planes_host, when not NULL, is
 * [2][streams][cap_words] uint64 (plane A, then plane C; cap_words =
 * ceil(capacity_bits / 64) + 1, lac_encoded_device's stride_bytes / 8).  set refuses
 * (LAC_E_ARG, nothing copied) register sets no encoder reaches: l outside
 * [0, 2^(prec+1)), h < l, h - l >= 2^prec, L beyond the capacity, nflush outside
 * [-1, 8] (streams with err set are copied as they are), and
 * planes_host == NULL while a stream has bits written (L > 0: its output words would
 * be whatever the context held); get and set refuse a decoding context (LAC_E_STATE;
 * lac_encode_reset first).  A restored context is not finished: lac_pack_bits needs a
 * lac_encode_finish first.
 * Synchronise `stream`. */
typedef struct lac_enc_state {
    int64_t l, h;
    uint64_t L, wa, wc;
    int64_t nsym;
    int32_t err, nflush;
    int64_t err_step;
    int8_t flush[8];
} lac_enc_state;
int lac_encode_get_state(lac_ctx *ctx, lac_enc_state *host_out, uint64_t *planes_host, void *stream);
int lac_encode_set_state(lac_ctx *ctx, const lac_enc_state *host_in, const uint64_t *planes_host, void *stream);

/* Start decoding: stream b reads nbits_dev[b] bits at bits_dev + b*stride_bytes
 * (bits_dev == NULL: this context's own encoded streams).  The buffers are
 * borrowed until the next lac_decode_open / lac_close.  stride_bytes must be a
 * multiple of 8 and every stream's region readable up to it; a stream with
 * nbits_dev[b] > 8 * stride_bytes fails with a sticky LAC_E_ARG (lac_stream_status)
 * and reads nothing. */
int lac_decode_open(lac_ctx *ctx, const uint8_t *bits_dev, uint64_t stride_bytes,
                    const uint64_t *nbits_dev, void *stream);

/* lac_decode_open straight from the wire: unpack one packed job (lac_unpack_jobs with
 * jobs = 1 and the context's streams; src_dev, src_bytes, hdr_bytes, counts_dev, base_dev as
 * there) into a buffer the context owns and open the decoder on it, both queued on `stream`
 * with no host synchronisation.  The buffer -- streams slots of 8 * (ceil(capacity_bits / 64)
 * + 1) bytes and streams counts -- is allocated on first use, freed by lac_close, and is not
 * plane A: a pending encode output or an lac_set_output redirection is not disturbed.
 * *end_dev (device memory, may be NULL) receives the offset past the job, so a receiver
 * walks a payload of several jobs by passing it as the next base_dev.  The source is not
 * borrowed: once the queued work has run the caller may overwrite it.  A job that does not
 * fit src_bytes leaves every stream with the sticky LAC_E_ARG (lac_stream_status), a stream
 * longer than the context's slots gets it alone.  Everything after the open -- every decode
 * path, lac_set_stream_lengths, LAC_OPT_DECODE_STOP, the logits decode, lac_decode_get_state /
 * lac_decode_set_state -- is what it is after lac_decode_open. */
int lac_decode_open_packed(lac_ctx *ctx, const uint8_t *src_dev, uint64_t src_bytes, int hdr_bytes,
                           const uint64_t *counts_dev, const uint64_t *base_dev, uint64_t *end_dev,
                           void *stream);

/* Windowed decode, the mirror of lac_encode_drain: decode streams of any length through a
 * window of W = ceil(capacity_bits / 64) + 1 words per stream that the context owns, so that
 * capacity_bits bounds the bits decoded between two refills and not the stream.
 *   lac_decode_open_window takes lac_decode_open's source (bits_dev, stride_bytes, nbits_dev:
 * the same alignment rules; bits_dev == NULL is LAC_E_ARG) and borrows it until the next open or
 * lac_close.  Only k_dec_refill ever reads the source, so it may be device memory or
 * lac_host_alloc memory passed by its device address: the compressed data can stay on the host.
 * The window -- [streams][8 W] bytes, streams counts and streams bases, allocated on first use,
 * freed by lac_close, shared with lac_decode_open_packed's slots -- is filled from source word
 * base_words_dev[b] on (uint64 [streams], device memory; NULL: 0 for every stream) and the
 * decoder is opened on it: every decode path (split, fused, stats, block, lean), the logits
 * decode and its one-position step, the tail, lac_decode_determined, lac_set_stream_lengths,
 * LAC_OPT_DECODE_STOP and lac_decode_get_state / set_state read the window as they read any
 * opened buffer.  A stream with nbits_dev[b] > 8 * stride_bytes or 64 * base > nbits_dev[b]
 * fails with the sticky LAC_E_ARG and nothing of it is read.
 *   lac_decode_refill slides every stream's window: the whole words below bit pos - prec are
 * dropped (g = (pos - prec) >> 6), the kept words move to the front, g words come from the
 * source, and pos shrinks by 64 g, base grows by g.  One launch (k_dec_refill, one wave per
 * stream), asynchronous on `stream`, no host synchronisation, no allocation.  A window that
 * reaches its stream's end stays where it is, as does a stream with a sticky error or one
 * stopped at its count.  LAC_E_STATE unless the open decode is a windowed one.
 *   lac_decode_window_base copies every stream's base to the host (synchronises).
 * Contract, per stream: symbols, -1 fills, status and err_step, nsym, l / h / x, det / ndet and
 * pos + 64 * base are those of lac_decode_open on the whole stream followed by the same decode
 * calls (lac_amd/csrc/lac_refill.h: a decoder never reads below pos - prec, a step pulls at most
 * prec bits, and everything derived from the stream's end uses pos - nbits only).
 * lac_dec_state.pos is relative to the window; per-stream counts and LAC_OPT_DECODE_STOP mean
 * what they did.  Resume: lac_decode_open_window with the saved bases, then
 * lac_decode_set_state with the saved registers.
 *   Sizing: after a refill pos <= prec + 63 and N steps add at most N * prec, so N steps between
 * two refills are safe when 64 W >= (N + 1) * prec + 63; the encode side's
 * capacity_bits = N * (prec + 2) + 256 satisfies it for every prec.
 *   A stream whose steps read past the bits its window held while more of the stream lay outside
 * it (a dry stream) is detected by the next refill, not by the steps: it gets the sticky
 * LAC_E_CAPACITY with err_step = its nsym, and its symbols since the previous refill are void.
 * Refill once after the last step before trusting lac_stream_status. */
int lac_decode_open_window(lac_ctx *ctx, const uint8_t *bits_dev, uint64_t stride_bytes,
                           const uint64_t *nbits_dev, const uint64_t *base_words_dev, void *stream);
int lac_decode_refill(lac_ctx *ctx, void *stream);
int lac_decode_window_base(lac_ctx *ctx, uint64_t *base_words_host, void *stream);

/* Decode one symbol per stream from row b at pmf_dev + b*stream_stride. */
int lac_decode_step(lac_ctx *ctx, const void *pmf_dev, int64_t stream_stride,
                    int32_t *sym_out_dev, void *stream);

/* Decode `steps` symbols per stream (rows as in lac_encode); sym_out_dev is
 * int32 [steps][streams]. */
int lac_decode_steps(lac_ctx *ctx, const void *pmf_dev, int64_t step_stride, int64_t stream_stride,
                     int64_t steps, int32_t *sym_out_dev, void *stream);

/* ---- finite-state models (the reference's NFA predictor, arith_code.py:423-434) ----------
 * A model has K states over the context's V symbols: integer tables pmf[K][V] in the context's
 * pmf_bits and transitions next[K][V] (int32).  Stream b starts in state q_0 = its current state
 * (lac_fsm_set_states); step t codes sym_t with row pmf[q_t] exactly as lac_encode /
 * lac_decode_steps code that row -- ceil mapping, fudged rows included -- and then
 * q_{t+1} = next[q_t][sym_t] (NFA.calc_dist / NFA.accept, :427-432).  In the explicit-states form
 * the caller passes states[steps][streams] and q_t = states[t][b]; next is not consulted and the
 * context's current states do not move.  Per stream everything -- output bytes and nbits,
 * registers, decoded symbols, lac_stream_status codes and err_step, what a failed stream
 * freezes -- is what the pmf path gives on the gathered tables pmf[q_t], so either path decodes
 * the other's streams.  One kernel launch per call whatever the steps; the launches report under
 * lac_profile_read's slots 1 (encode) and 3 (decode_step).
 *
 * lac_fsm_load  (NFA.__init__, :424-426) copies the model into a prepared device form the context
 *   owns (per state row: the per-entry CDF, T, ceil(T / minp), 1 / T; lac_amd/csrc/lac_fsm.h); the
 *   caller's buffers are free when it returns (it synchronises `stream`), lac_close frees the
 *   prepared form, and every stream's current state becomes 0.  pmf_dev: [states][V] contiguous,
 *   any alignment; next_dev: [states][V] int32 or NULL (explicit-states form only).
 *   Limits: V <= 65536 and states * V <= 2^24 entries (an order-2 byte model fits); beyond
 *   either, LAC_E_ARG.  A next entry outside [0, states): LAC_E_TABLE, the model in place stays.
 *   A load replaces the model only between jobs: LAC_E_STATE after an lac_encode / lac_fsm_encode
 *   that is not finished, or after an lac_fsm_decode with no lac_decode_open* since.  A bad row
 *   (empty, total >= 2^64) is no load error: it raises the pmf path's sticky LAC_E_TABLE for the
 *   stream whose step reaches it.
 * lac_fsm_set_states / lac_fsm_get_states  (NFA.s, :426) the current state of every stream (int32
 *   [streams], device memory, copied on `stream`; NULL sets all to 0).  A state outside
 *   [0, states) is LAC_E_TABLE for its stream at the step that uses it, in both forms.
 * lac_fsm_encode  (A_to_bin.step with NFA.calc_dist + accept, :187-192, :427-432) continues the
 *   open encode like lac_encode: sym_dev int32 [steps][streams], states_dev int32
 *   [steps][streams] or NULL, trace_dev as lac_encode's (per (t, b) the symbol's digits {E, k}) or NULL.  lac_encode_reset, _drain, _rebase, _finish, the checkpoint calls and
 *   lac_set_output work around it unchanged.  A failed stream keeps the state of its failing step.
 * lac_fsm_decode  (A_from_bin.step, :264-299) after any lac_decode_open*: sym_out_dev int32
 *   [steps][streams] (-1 after an error); it reads the opened buffer like every decode path, so
 *   lac_decode_refill works between calls, and honours LAC_OPT_DECODE_STOP (LAC_E_UNDETERMINED,
 *   registers and state unchanged) and lac_decode_determined.
 * Both coding calls honour lac_set_stream_lengths.  Refused before anything is launched:
 * LAC_E_STATE with no model loaded, under LAC_MAP_FLOOR (the reference's NFA is a CDFPredictor)
 * or in the wrong mode (lac_encode's / lac_decode_steps' rule); LAC_E_ARG for states_dev NULL on a
 * model loaded without next. */
int lac_fsm_load(lac_ctx *ctx, const void *pmf_dev, const int32_t *next_dev, int64_t states, void *stream);
int lac_fsm_set_states(lac_ctx *ctx, const int32_t *state_dev, void *stream);
int lac_fsm_get_states(lac_ctx *ctx, int32_t *state_dev_out, void *stream);
int lac_fsm_encode(lac_ctx *ctx, const int32_t *sym_dev, const int32_t *states_dev, int64_t steps,
                   uint64_t *trace_dev, void *stream);
int lac_fsm_decode(lac_ctx *ctx, const int32_t *states_dev, int64_t steps, int32_t *sym_out_dev, void *stream);

/* ---- adaptive n-gram count models (the reference's Markov_up_to_n, arith_code.py:443-464) ----
 * A model that learns while it codes: V symbols (the context's), an order k in [1, 4] and integer
 * weights W[0..k-1] < 2^30.  Stream b keeps `past`, its last <= k accepted symbols, and one u32
 * count per n-gram of length i + 1 (i < k), all 0 at the start.  With m = len(past) the table of a
 * step is  pmf[s] = 1 + sum_{i<m} W[i] * C_i[(last i symbols of past), s]  (Markov_up_to_n.prob,
 * :460-462, with lfunc(c, o, n, order) == c * W[o]), and accepting s adds 1 to those m counts and
 * appends s to past (accept, :454-459).  Step t codes with that row exactly as lac_encode /
 * lac_decode_steps code it -- ceil mapping, fudged rows included -- so per stream everything
 * (bytes, nbits, registers, decoded symbols, status codes and err_step) is what the pmf path gives
 * on the rows the counts produce.  One kernel launch per call whatever the steps; the launches
 * report under lac_profile_read's slots 1 (encode) and 3 (decode_step).
 *
 * lac_count_load  (Markov_up_to_n.__init__, :444-449) allocates streams x stride counts, zeroed,
 *   and empties every past; weights_host: `order` host integers.  LAC_E_ARG: V > 4096, order
 *   outside [1, 4], sum_{i<order} V^(i+1) > 2^25 counts per stream (an order-3 byte model fits), a
 *   weight >= 2^30, LAC_MAP_FLOOR.  Only between jobs (LAC_E_STATE, lac_fsm_load's rule).  A
 *   context holds a finite-state model and a count model independently; lac_close frees both.
 * lac_count_layout  (:447, the dict `table` as a dense array) out[6] = {Vc, stride_words, off[4]}:
 *   stream b's counts are words [b * stride, (b + 1) * stride); section i (i < order) starts at
 *   word off[i] and holds V^i rows of Vc = 4 ceil(V / 4) counts; the row of a context is its i
 *   symbols read oldest first as base-V digits (lac_amd/csrc/lac_count.h).
 * lac_count_set_state / lac_count_get_state  (:447-448, `table` and `past`) every stream's counts
 *   (uint32 [streams][stride], device; NULL sets all to 0) and past (int32 [streams][order],
 *   most recent last, -1 absent; NULL: empty), copied on `stream`.  A stream's valid history is
 *   its trailing run of entries in [0, V).  Either output of get_state may be NULL.
 * lac_count_encode  (A_to_bin.step with prob + accept, :187-192, :454-462) continues the open encode
 *   like lac_encode: sym_dev int32 [steps][streams], trace_dev as lac_encode's or NULL.
 * lac_count_decode  (A_from_bin.step, :264-299, :454-462) after any lac_decode_open*: sym_out_dev
 *   int32 [steps][streams] (-1 after an error); honours lac_decode_refill between calls,
 *   LAC_OPT_DECODE_STOP and lac_decode_determined.
 * Sticky errors are the pmf path's on the row the counts produce, with its precedence: an entry
 * that does not fit pmf_bits or a total >= 2^64 is LAC_E_TABLE at that step (u32 rows whose total
 * passes 2^32 are legal), as is a count that would pass 2^32 - 1.  That last verdict needs the
 * symbol, so a decode step reaches it after the register and range tests (LAC_E_DECODE_RANGE), an
 * encode step after the symbol's range test.  A failed step updates no count and does not move past.  Both coding calls honour lac_set_stream_lengths.  Refused before
 * anything is launched: LAC_E_STATE with no count model loaded, under LAC_MAP_FLOOR or in the
 * wrong mode. */
int lac_count_load(lac_ctx *ctx, int order, const uint32_t *weights_host, void *stream);
int lac_count_layout(lac_ctx *ctx, int64_t *out);
int lac_count_set_state(lac_ctx *ctx, const uint32_t *counts_dev, const int32_t *past_dev, void *stream);
int lac_count_get_state(lac_ctx *ctx, uint32_t *counts_dev_out, int32_t *past_dev_out, void *stream);
int lac_count_encode(lac_ctx *ctx, const int32_t *sym_dev, int64_t steps, uint64_t *trace_dev, void *stream);
int lac_count_decode(lac_ctx *ctx, int64_t steps, int32_t *sym_out_dev, void *stream);

/* ---- match-history models (the reference's History, arith_code.py:364-398) ----
 * A model that predicts from the longest recent matches: V symbols (the context's), a ring of the
 * last P in [1, 256] symbols per stream and a table of weights L[i][r] < 2^48 (lag i, run r).
 * Stream b keeps `ring`, int32 [P], all -1 at the start, and the write index `pasti`, 0 at the
 * start.  With  p_i = ring[(pasti - 1 - i) mod P]  and  r_i  the number of j = 1, 2, ... < P - i,
 * taken while they hold, with  ring[(pasti - 1 - i - j) mod P] == ring[(pasti - j) mod P]
 * (History.runs, :371-380), the table of a step is
 *   pmf[s] = 1 + sum_{i : p_i == s and p_i > 0} L[i][r_i]      (calc_dist, :381-389, with
 * lfunc(r, i, n, P) == L[i][r]), and accepting s does ring[pasti] = s, pasti = (pasti + 1) mod P
 * (accept, :390-393).  The model's quirks are kept: symbol 0, like the -1 filler, never gains
 * weight (the test is p > 0), and -1 equals -1 in the comparisons, so an empty ring matches
 * itself.  Step t codes with that row exactly as lac_encode / lac_decode_steps code it -- ceil
 * mapping, fudged rows included -- so per stream everything (bytes, nbits, registers, decoded
 * symbols, status codes and err_step) is what the pmf path gives on the rows the ring produces.
 * One kernel launch per call whatever the steps; the launches report under lac_profile_read's
 * slots 1 (encode) and 3 (decode_step).
 *
 * lac_hist_load  (History.__init__, :365-370) uploads weights_host, uint64 [P][P] with
 *   L[i * P + r] = lfunc(r, i, V, P), and gives every stream the initial state.  LAC_E_ARG:
 *   V > 4096, P outside [1, 256], a weight >= 2^48 (so a total stays below 4096 + 256 * 2^48 <
 *   2^57 and never reaches 2^64), LAC_MAP_FLOOR.  Only between jobs (LAC_E_STATE, lac_fsm_load's
 *   rule).  A context holds a finite-state, a count and a history model independently; lac_close
 *   frees all.
 * lac_hist_set_state / lac_hist_get_state  (:367-368, `past` and `pasti`) every stream's ring
 *   (int32 [streams][P], device; NULL sets all to -1) and write index (int32 [streams], device;
 *   NULL: 0), copied on `stream`.  set_state refuses, as a whole and before anything is set, a
 *   ring entry outside [-1, V) or a pasti outside [0, P) (LAC_E_ARG; it waits for `stream` to
 *   learn that).  The match lengths the kernels carry from step to step are derived state: they
 *   are rebuilt from ring and pasti whenever those are set and are no part of what is saved.
 *   Either output of get_state may be NULL.
 * lac_hist_encode  (A_to_bin.step with calc_dist + accept, :187-192, :381-393) continues the open
 *   encode like lac_encode: sym_dev int32 [steps][streams], trace_dev as lac_encode's or NULL.
 * lac_hist_decode  (A_from_bin.step, :264-299, :381-393) after any lac_decode_open*: sym_out_dev
 *   int32 [steps][streams] (-1 after an error); honours lac_decode_refill between calls,
 *   LAC_OPT_DECODE_STOP and lac_decode_determined.
 * Sticky errors are the pmf path's on the row the ring produces, with its precedence: under a u32
 * context an entry >= 2^32 is LAC_E_TABLE at that step (u32 rows whose total passes 2^32 are
 * legal).  A failed step moves neither the ring nor the match lengths.  Both coding calls honour
 * lac_set_stream_lengths.  Refused before anything is launched: LAC_E_STATE with no history model
 * loaded, under LAC_MAP_FLOOR or in the wrong mode. */
int lac_hist_load(lac_ctx *ctx, int P, const uint64_t *weights_host, void *stream);
int lac_hist_set_state(lac_ctx *ctx, const int32_t *ring_dev, const int32_t *pasti_dev, void *stream);
int lac_hist_get_state(lac_ctx *ctx, int32_t *ring_dev_out, int32_t *pasti_dev_out, void *stream);
int lac_hist_encode(lac_ctx *ctx, const int32_t *sym_dev, int64_t steps, uint64_t *trace_dev, void *stream);
int lac_hist_decode(lac_ctx *ctx, int64_t steps, int32_t *sym_out_dev, void *stream);

/* ---- range-level coding (symbol_to_range / val_to_symbol, arith_code.py:94-110) ----
 * The coder itself needs three integers per symbol: lo = c_{s-1}, hi = c_s and the total T
 * (symbol_to_range reads dist[s-1], dist[s] and dist[-1] only).  These calls take them instead of
 * a table, for models whose distribution is a formula (a discretised Gaussian, a uniform law over
 * 10^12 values) or whose alphabet is too large to write out per step.  Triples are always uint64,
 * whatever the context's pmf_bits; the context's vocab plays no part.  A triple is valid when
 * 0 < T <= 2^(prec-1) and lo < hi <= T.  It codes exactly as the table [lo, hi - lo, T - hi] codes
 * its symbol 1: with T <= 2^(prec-1) no width can fudge (T <= w minp for every w > 2^(prec-1)),
 * whatever the other two entries are, so per stream everything -- bytes and nbits, lac_enc_state /
 * lac_dec_state, planes, trace_dev {E, k}, lac_flush_digits, capacity failures with their registers
 * and what a failed stream freezes -- is what lac_encode / lac_decode_steps give on that table
 * (lac_amd/csrc/lac_ranges.h).  Totals above 2^(prec-1) are refused: fudging needs the whole table.
 *
 * lac_encode_ranges  continues the open encode like lac_encode and mixes with it, the logits calls
 *   and the model families in one session; lac_set_stream_lengths, lac_encode_drain, _rebase,
 *   _finish, lac_encode_get_state / _set_state and lac_set_output work around it unchanged.
 *   lo_dev, hi_dev: [steps][streams]; the total of step t, stream b is
 *   tot_dev[t * tot_step_stride + b * tot_stream_stride], strides in elements, 0 re-uses the value
 *   (a per-stream total, or one total for the whole job).  Step t of stream b narrows by
 *   a = ceil(lo w / T), b = ceil(hi w / T) and renormalises.  Sticky errors, in this precedence:
 *   LAC_E_TABLE (T = 0, T > 2^(prec-1), hi > T or lo > hi), LAC_E_ZERO_WIDTH (lo == hi),
 *   LAC_E_CAPACITY (after the narrowing); err_step is the stream's nsym.  One kernel launch per
 *   call whatever the steps (one lane per stream); it reports under lac_profile_read's slot 1.
 * lac_encode_ranges_job  reset + lac_encode_ranges + finish (the reset and finish launches are the
 *   existing ones).
 * lac_decode_ranges_step  after any lac_decode_open*; one call is "advance by the previous symbol's
 *   range, then peek the next target", in one launch (slot 3):
 *   - advance (lo_dev != NULL; lo_dev, hi_dev, tot_dev: [streams]): a live stream with no sticky
 *     error tests, in order, the triple (LAC_E_TABLE), the registers (x outside [l, h]:
 *     LAC_E_DECODE_RANGE), lo <= floor((x - l) T / w) < hi (LAC_E_DECODE_RANGE otherwise: the
 *     range misses the target, as lo == hi always does), then decode_symbol's determined test,
 *     det = vhi < w && floor(vhi T / w) < hi (with LAC_OPT_DECODE_STOP an undetermined symbol is
 *     LAC_E_UNDETERMINED; det / ndet count as on the pmf path), then narrows, renormalises, pulls
 *     bits and counts the symbol.  Where the target lies in [lo, hi) everything equals
 *     lac_decode_steps on the three-entry table decoding symbol 1.  Every error leaves the stream
 *     frozen as before the step.
 *   - peek (next_tot_dev != NULL, [streams]), after the advance: target_out_dev[b] =
 *     floor((x - l) T' / w), no state changes (twice gives the same values).  UINT64_MAX for a
 *     stream with a sticky error or at its count, and for a T' that is not valid (the error itself
 *     is raised by the advance that uses it).
 *   The caller's model turns targets into symbols and ranges (val_to_symbol) between calls.  The
 *   call reads the opened buffer like every decode path: lac_decode_open_packed, _open_window,
 *   lac_decode_refill and lac_set_stream_lengths work between calls.
 * Refused before anything is launched: LAC_E_STATE under LAC_MAP_FLOOR or LAC_TERM_ACSAMPLER (the
 * reference's floor-mapped decoder is not an inverse of its encoder) and in the wrong mode
 * (lac_encode's / lac_decode_steps' rule); LAC_E_ARG for NULL lo / hi / tot on encode, negative
 * steps or strides, and a decode call with both halves NULL. */
int lac_encode_ranges(lac_ctx *ctx, const uint64_t *lo_dev, const uint64_t *hi_dev, const uint64_t *tot_dev,
                      int64_t tot_step_stride, int64_t tot_stream_stride, int64_t steps, uint64_t *trace_dev,
                      void *stream);
int lac_encode_ranges_job(lac_ctx *ctx, const uint64_t *lo_dev, const uint64_t *hi_dev, const uint64_t *tot_dev,
                          int64_t tot_step_stride, int64_t tot_stream_stride, int64_t steps, uint64_t *trace_dev,
                          void *stream);
int lac_decode_ranges_step(lac_ctx *ctx, const uint64_t *lo_dev, const uint64_t *hi_dev, const uint64_t *tot_dev,
                           const uint64_t *next_tot_dev, uint64_t *target_out_dev, void *stream);

/* ---- sparse rows: top-k pairs over a uniform floor ----
 * A row given as at most K (symbol, weight) pairs plus one integer: the form top-k logprob outputs,
 * truncated samplers and the match model's rows have.  A call names a base weight `base` (>= 1, one
 * per call), a slot count K (a multiple of 4, 4 <= K <= 256) and two device arrays, idx (int32) and
 * wt (uint32); row (t, b) is the K slots at element t * step_stride + b * stream_stride of both
 * (strides in slots; a step stride of 0 re-uses the rows, as in lac_encode).  With n the number of
 * leading slots with idx >= 0 the row stands for the dense table over the context's vocab V
 *     pmf[s] = base + (wt_j if s == idx_j for some j < n, else 0),   T = base V + sum_{j<n} wt_j
 * A row is valid when every pair has idx_j in [0, V), the pairs are strictly ascending in idx, every
 * slot j >= n has idx == -1 (its weight is ignored) and T <= 2^(prec-1); wt_j = 0 is legal.  Any
 * other row -- a pair after a pad, an equal or descending index, an idx < -1 or >= V, a total that
 * is too large -- is LAC_E_TABLE for the stream whose step reaches it.  As with ranges, totals above
 * 2^(prec-1) are refused rather than fudged: every entry is at least 1, so T <= 2^(prec-1) < w minp
 * at every coder state and no row can fudge.
 *
 * Equivalence, which is the contract: per stream a valid sparse row codes exactly as
 * lac_encode_ranges / lac_decode_ranges_step code the triple of the dense row, which is what a
 * pmf_bits = 64 context's lac_encode / lac_decode_steps give on the dense row -- bytes and nbits,
 * lac_enc_state / lac_dec_state, planes and trace_dev {E, k}, lac_flush_digits, decoded symbols and
 * det / ndet, capacity failures with their registers, and what a failed stream freezes.  The
 * context's own pmf_bits plays no part.  The rules, as whole-row rules and as the per-lane
 * partials the kernels run, are lac_amd/csrc/lac_sparse.h.
 *
 * lac_encode_sparse  continues the open encode like lac_encode and mixes with it, the logits calls,
 *   the ranges calls and the model families in one session; sym_dev: [steps][streams].  For symbol
 *   s: lo = base s + sum_{idx_j < s} wt_j, hi = lo + base + sum_{idx_j == s} wt_j, then the range
 *   step.  Sticky errors, in this precedence: LAC_E_SYMBOL_RANGE (s not in [0, V)), LAC_E_TABLE
 *   (the row), LAC_E_CAPACITY (after the narrowing); zero width cannot occur.  One wave per stream,
 *   one kernel launch per call whatever the steps (lac_profile_read's slot 1); streams ended by
 *   lac_set_stream_lengths fetch nothing.
 * lac_encode_sparse_job  reset + lac_encode_sparse + finish (the existing reset and finish launches).
 * lac_decode_sparse_steps  after any lac_decode_open*; one launch (slot 3) for `steps` positions.
 *   A step computes the target t = floor((x - l) T / w) and finds its symbol among the pairs and the
 *   plain entries between them (a wave scan of the weights, no walk over V), then runs the range
 *   decode frame: registers test, determined test with LAC_OPT_DECODE_STOP, narrow, renormalise,
 *   pull.  Errors: the row first (LAC_E_TABLE), then the registers (LAC_E_DECODE_RANGE), then
 *   LAC_E_UNDETERMINED.  sym_out_dev: [steps][streams], -1 where a stream decoded nothing.  The
 *   opened buffer is read like on every decode path: lac_decode_open_packed, _open_window,
 *   lac_decode_refill, lac_decode_determined and lac_set_stream_lengths work around it unchanged.
 * Refused before anything is launched: LAC_E_STATE under LAC_MAP_FLOOR or LAC_TERM_ACSAMPLER and in
 * the wrong mode (lac_encode's / lac_decode_steps' rule); LAC_E_ARG for K not a multiple of 4 in
 * [4, 256], base = 0, a stride that is negative or no multiple of 4, an array that is NULL or not
 * 16-byte aligned, negative steps, and a NULL sym_dev / sym_out_dev with steps > 0. */
int lac_encode_sparse(lac_ctx *ctx, const int32_t *idx_dev, const uint32_t *wt_dev, int K, int64_t step_stride,
                      int64_t stream_stride, uint32_t base, const int32_t *sym_dev, int64_t steps,
                      uint64_t *trace_dev, void *stream);
int lac_encode_sparse_job(lac_ctx *ctx, const int32_t *idx_dev, const uint32_t *wt_dev, int K, int64_t step_stride,
                          int64_t stream_stride, uint32_t base, const int32_t *sym_dev, int64_t steps,
                          uint64_t *trace_dev, void *stream);
int lac_decode_sparse_steps(lac_ctx *ctx, const int32_t *idx_dev, const uint32_t *wt_dev, int K, int64_t step_stride,
                            int64_t stream_stride, uint32_t base, int64_t steps, int32_t *sym_out_dev, void *stream);

/* ---- logits path --------------------------------
 * Tables are computed in-kernel from raw logits with the integer-exact "q1"
 * quantiser instead of being read from a pmf in HBM: for each row
 *   m = max_i x_i (NaN ignored),  c = RNE_f32(544 - 32 m),
 *   j_i = sat_u32(fmaf(x_i, 32, c)) capped at 544 (NaN, -inf, negatives -> 0),
 *   q_i = max(1, TAB[544 - j_i] >> (24 - k)),  TAB[i] = round(2^24 e^(-i/32))
 * i.e. softmax to 1/32-nat resolution, gaps clamped at 17 nats
 * (include/lac_q1_table.h; DESIGN.md "logits path"), with
 * k = lac_q1_k(prec, vocab) = min(24, prec - 1 - ceil(log2 vocab)) so that
 * T <= 2^(prec-1) and no row is ever fudged.  It replaces the float64 numpy
 * quantiser of llama_compress.py:24-30 (whose output is platform-dependent)
 * with a rule both the GPU and the C oracle reproduce bit for bit; the coder
 * semantics are those of CDFPredictor + A_to_bin / A_from_bin
 * (arith_code.py:76-110, 156-334).  Logit rows: bf16 (uint16 bit patterns) or
 * f32, 16-byte aligned, vocab and strides (in elements) multiples of 8 (bf16)
 * or 4 (f32); a stride of 0 re-uses the row.  Any other layout -- a base off 16
 * bytes, an odd row padding -- is refused with LAC_E_ARG by all four entry points
 * below, before anything is launched or any stream's state changes (the integer
 * pmf path takes such tables with its scalar kernels; this path has none).
 * Requires the CEIL mapping and FLUSH termination. */
#define LAC_LOGITS_BF16 1
#define LAC_LOGITS_F32 2

int lac_q1_k(int prec, int64_t vocab);

/* reset + encode `steps` symbols per stream from logits + finish
 * (logits[t*step_stride + b*stream_stride + i], sym_dev[t*streams + b]). */
int lac_encode_logits_job(lac_ctx *ctx, const void *logits_dev, int logit_type, int64_t step_stride,
                          int64_t stream_stride, const int32_t *sym_dev, int64_t steps, uint64_t *trace_dev,
                          void *stream);

/* Incremental form: encode `steps` more symbols per stream from logits,
 * continuing each stream where the last call (lac_encode_reset, lac_encode or
 * lac_encode_logits) left it; close with lac_encode_finish.  Streams may mix
 * pmf and logits steps (each step's table is exact either way). */
int lac_encode_logits(lac_ctx *ctx, const void *logits_dev, int logit_type, int64_t step_stride,
                      int64_t stream_stride, const int32_t *sym_dev, int64_t steps, uint64_t *trace_dev,
                      void *stream);

/* Decode `steps` symbols per stream (after lac_decode_open) with the tables
 * computed from logits; sym_out_dev[t*streams + b] (-1 after an error). */
int lac_decode_logits_steps(lac_ctx *ctx, const void *logits_dev, int logit_type, int64_t step_stride,
                            int64_t stream_stride, int64_t steps, int32_t *sym_out_dev, void *stream);

/* One position for a model in the loop: logits [streams][vocab] in (row b at logits_dev +
 * b*stream_stride), one symbol per stream decoded or encoded.  Every observable equals the
 * `steps = 1` call of lac_decode_logits_steps / lac_encode_logits (step_stride 0): symbols
 * and -1 fills, lac_dec_state / lac_enc_state, planes, traces (trace_dev[2 b], may be NULL),
 * sticky status and err_step, per-stream counts, and the same refusals before anything is
 * launched; LAC_OPT_DECODE_STOP is ignored as the logits decode ignores it.  The calls mix
 * freely with every other encode / decode call of a session.  Where the job fits
 * (LAC_OPT_Q1_STEP) a position is one launch instead of two: one workgroup per stream holds
 * the row in registers, computes its maximum, quantises it, scans it and runs the coder's
 * step, with no row statistics written to memory in between.  Under lac_profile_read the
 * fused decode step counts in slot 7 (q1_decode), the fused encode step in slot 1 (encode),
 * and slot 6 (q1_stats) gets nothing. */
int lac_decode_logits_step(lac_ctx *ctx, const void *logits_dev, int logit_type, int64_t stream_stride,
                           int32_t *sym_out_dev /* [streams] */, void *stream);
int lac_encode_logits_step(lac_ctx *ctx, const void *logits_dev, int logit_type, int64_t stream_stride,
                           const int32_t *sym_dev /* [streams] */, uint64_t *trace_dev, void *stream);

/* Rows longer than a CU holds (LAC_OPT_Q1_SHAPE 19 / 20 / 21 / 23, AUTO for e.g. f32 V =
 * 128256) are split over 2..16 row slots of workgroups that exchange each row's
 * maximum, which needs every member resident.  When a member is not (another
 * kernel holds CUs) the waiting ones give up after ~0.1 s, raise the launch's
 * abort flag, and a tiled two-pass launch queued behind it recomputes every row:
 * results are identical either way.  Synchronises `stream`; *aborted = 1 if the
 * last such launch of this context took that path. */
int lac_q1_group_aborted(lac_ctx *ctx, int64_t *aborted, void *stream);

/* Materialise the q1 tables: pmf_out_dev[(t*streams + b)*vocab + i] (uint32). */
int lac_quantize_logits(lac_ctx *ctx, const void *logits_dev, int logit_type, int64_t step_stride,
                        int64_t stream_stride, int64_t steps, uint32_t *pmf_out_dev, void *stream);

/* ---- top-k rows straight from logits -------------------------------------
 * One kernel reads each logits row once and writes its sparse form -- the rows lac_encode_sparse /
 * lac_decode_sparse_steps take -- by an integer-exact rule both sides of a codec reproduce (the
 * rules in both of their forms: lac_amd/csrc/lac_topk.h).  For one row x[0..V), bf16 or f32 with
 * the logits path's layout rules above:
 *   1. weights    g_i = TAB[544 - j_i] with j_i exactly q1's level (m, c and j_i as above): the q1
 *                 table at k = 24 whatever the context's prec -- what lac_quantize_logits writes on
 *                 a context whose lac_q1_k is 24.
 *   2. selection  the k entries largest by g survive; among equal g the lower symbol wins.  The key
 *                 is g, not j: TAB has 453 distinct values over its 545 levels (the first equal
 *                 pair is TAB[423] = TAB[424] = 30), so adjacent levels can form one tie class.
 *                 Flat rows, all -inf rows and rows containing +inf are all-tie rows: symbols
 *                 0..k-1.
 *   3. output     K slots, K a multiple of 4 with k <= K <= 256.  Slots 0..k-1: the survivors in
 *                 ascending symbol order, idx_j (int32) and wt_j = g >> (24 - weight_bits) (uint32,
 *                 may be 0).  Slots k..K-1: idx -1, wt 0.  A valid lac_encode_sparse row by
 *                 construction (base >= 1 is the caller's, as is T <= 2^(prec-1):
 *                 base V + k 2^weight_bits bounds it).
 * Row (t, b) is read at logits_dev + t*step_stride + b*stream_stride (elements) and written at
 * element (t*streams + b)*K of idx_out_dev and wt_out_dev (contiguous).  Like lac_quantize_logits
 * the call touches no stream state, works in any mode, mapping and termination, has no sticky
 * errors and computes every row (lac_set_stream_lengths is ignored).  One launch whatever the
 * steps, one workgroup per row (LAC_OPT_TOPK_FORM); it reports under lac_profile_read's slot 6.
 * LAC_E_ARG before anything is launched or written: a bad logit type, negative steps or strides,
 * k outside [1, min(V, 256)], K not a multiple of 4 or outside [k, 256], weight_bits outside
 * [0, 24]; with steps > 0 also NULL arrays, a logits layout the logits path refuses, outputs not
 * 16-byte aligned, a forced form that cannot hold the row, steps x streams >= 2^31.  steps == 0
 * is LAC_OK with no launch.
 * lac_topk_form: the form (1 registers, 2 streamed) the next such call runs for this logit type. */
int lac_topk_logits(lac_ctx *ctx, const void *logits_dev, int logit_type, int64_t step_stride, int64_t stream_stride,
                    int64_t steps, int k, int weight_bits, int K,
                    int32_t *idx_out_dev, uint32_t *wt_out_dev, /* [steps][streams][K], contiguous */
                    void *stream);
int lac_topk_form(lac_ctx *ctx, int logit_type);

/* Synchronise; ndet_host[streams] = how many leading decoded symbols the
 * available bits determine, i.e. how many symbols the reference's bit-serial
 * A_from_bin.run(bits, stop=0) emits (arith_code.py:268-299, :322-326). */
int lac_decode_determined(lac_ctx *ctx, int64_t *ndet_host, void *stream);

/* Decoder registers of one stream, A_from_bin's state (arith_code.py:248-256) in
 * the value form: l, h, the prec-bit value window x (bits at or past the stream's
 * nbits read as 0), pos = index of the next bit to read, symbols decoded, the
 * sticky error, and the determined flag / count of lac_decode_determined. */
typedef struct lac_dec_state {
    int64_t l, h, x;
    uint64_t pos;
    int64_t nsym;
    int32_t err, det;
    int64_t err_step, ndet;
} lac_dec_state;

/* Copy every stream's decoder registers to / from the host (synchronise).  With
 * lac_decode_open (which binds a longer bit buffer) and a host-side update of x
 * for the bits that arrived since, this resumes a decoder: the bit-serial
 * A_from_bin.step(bit) of the reference (arith_code.py:291-298) is built on it
 * (lac_amd.coder).  set_state refuses (LAC_E_ARG, nothing copied) register sets
 * no decoder reaches: l outside [0, 2^(prec+1)), h < l, h - l >= 2^prec, pos < prec
 * (streams with err set are copied as they are).  Not thread-safe with launches
 * on the same context. */
int lac_decode_get_state(lac_ctx *ctx, lac_dec_state *host_out, void *stream);
int lac_decode_set_state(lac_ctx *ctx, const lac_dec_state *host_in, void *stream);

/* ---- decoder tail in the reference's register frame (arith_code.py:248-334) ----
 * A_from_bin holds l, h and the received window [lb, hb] (the bits so far read
 * with 0s / 1s past the end).  lac_decode_tail_begin converts every stream's
 * value-form registers (after its determined symbols: lac_decode_determined ==
 * symbols decoded, else the stream gets LAC_E_STATE) into that frame; then each
 * lac_decode_tail_step runs one step per stream:
 *   LAC_TAIL_DECIDE  decide_symbol + emit_symbol + emit_bit (:268-291) on the
 *                    window: emits the symbol both window ends map to, or
 *                    nothing (undetermined).  Where the window leaves [l, h]
 *                    (foreign or corrupt bits) it reproduces the reference:
 *                    LAC_E_SYMBOL_RANGE naming V for tables (AssertionError
 *                    'unknown symbol'), out-of-range symbols for LAC_MAP_FLOOR
 *                    (the uniform Predictor(n) has no range check).
 *   LAC_TAIL_FLUSH   one iteration of A_from_bin.flush (:300-317): while [l, h]
 *                    is not inside [lb, hb], the candidate of largest overlap
 *                    ratio (CPython float ranking, first maximum kept), emitted
 *                    without renormalisation; once inside, the registers reset
 *                    and the stream reports idle.
 * sym_out_dev[b] (int64: uniform symbols can be negative) and code_out_dev[b]:
 * 0 = a symbol, 1 = nothing (undetermined / flushed), < 0 = the stream's sticky
 * error (LAC_E_SYMBOL_RANGE with sym_out = the symbol named, LAC_E_DECODE_RANGE
 * for emit_symbol's AssertionError :277-278, LAC_E_FLUSH_*).  Row b of the
 * stream's current table at pmf_dev + b*stream_stride (LAC_MAP_CEIL; ignored,
 * may be NULL, for LAC_MAP_FLOOR, whose alphabet is the context's vocab).
 * Asynchronous on `stream`. */
#define LAC_TAIL_DECIDE 0
#define LAC_TAIL_FLUSH 1
typedef struct lac_tail_state {
    int64_t l, h, lb, hb;
    int32_t err, done;
    int64_t still, nsym;      /* flush emits with [l, h] unchanged; symbols emitted */
} lac_tail_state;

int lac_decode_tail_begin(lac_ctx *ctx, void *stream);
int lac_decode_tail_step(lac_ctx *ctx, const void *pmf_dev, int64_t stream_stride, int mode,
                         int64_t *sym_out_dev, int32_t *code_out_dev, void *stream);
/* Copy the tail registers to / from the host (synchronise).  set_state refuses
 * (LAC_E_ARG) h < l, hb < lb or values beyond +-2^62; receive_bit (:264-267) is a
 * host-side update of lb, hb between steps. */
int lac_decode_tail_get_state(lac_ctx *ctx, lac_tail_state *host_out, void *stream);
int lac_decode_tail_set_state(lac_ctx *ctx, const lac_tail_state *host_in, void *stream);

/* ---- predictor-mapped coding (host, no device work) ----------------------------
 * A predictor whose symbol_to_range / val_to_symbol are its own code (the
 * reference's toy Predictor subclasses, e.g. ModifiedMarkov arith_code.py:468-522)
 * has no table for the GPU: its caller evaluates the mapping and these functions
 * do the coder's register arithmetic.  Registers stay within +-2^62 (LAC_E_ARG
 * otherwise); prec in [2, 61].
 *   lac_hc_encode_symbol  receive_symbol's narrowing to [l+lo, l+hi-1] plus the
 *                         decide_bit / emit_bit loop (arith_code.py:169-186):
 *                         the digits emitted (<= 64, int8); lo >= hi is
 *                         LAC_E_ZERO_WIDTH (the reference loops forever)
 *   lac_hc_encode_flush   A_to_bin.flush (:193-202): its digits
 *   lac_hc_decode_emit    emit_symbol (:274-283) on regs = {l, h, lb, hb}
 *                         (LAC_E_DECODE_RANGE when the range misses [lb, hb]),
 *                         then, if renormalise, the emit_bit loop (:284-291) */
int lac_hc_encode_symbol(int prec, int64_t *l, int64_t *h, int64_t lo, int64_t hi, int8_t *digits,
                         int32_t *ndigits);
int lac_hc_encode_flush(int prec, int64_t l, int64_t h, int8_t *digits, int32_t *ndigits);
int lac_hc_decode_emit(int prec, int64_t *regs, int64_t lo, int64_t hi, int renormalise);

/* Live kernel timing: with profiling on, every kernel launch is bracketed by
 * hipEvents recorded on its own stream.  lac_profile_read synchronises and
 * returns, per kernel id (0 row_stats, 1 encode, 2 finish, 3 decode_step,
 * 4 encode_fused, 5 decode_wave, 6 q1_stats, 7 q1_decode; 8 slots), the summed device milliseconds and the launch
 * count; reset != 0 clears.  The fused one-position logits step (lac_decode_logits_step /
 * lac_encode_logits_step) is one launch: its decode reports under 7, its encode under 1,
 * and 6 gets nothing. */
int lac_profile_enable(lac_ctx *ctx, int on);
int lac_profile_read(lac_ctx *ctx, double *ms_total /*[8]*/, int64_t *launches /*[8]*/, int reset);

#ifdef __cplusplus
}
#endif
#endif /* LAC_H */
