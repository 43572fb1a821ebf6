// lac_count.h -- plain host rules of the adaptive n-gram count models (include/lac.h
// lac_count_*): the limits a model must keep, the layout of a stream's counts the kernels of
// lac_count.hip read and write, the context indices, and how a step's row is built from the
// counts and how accept updates them -- checked without a GPU (tests/native/count_check.cpp).
//
// A model has V symbols, an order k in [1, 4] and integer weights W[0..k-1] < 2^30.  A stream
// keeps `past`, its last <= k accepted symbols, and one count per n-gram of length i + 1 for
// i < k, all 0 at the start.  With m = len(past) the row of a step is
//     pmf[s] = 1 + sum_{i < m} W[i] * C_i[(last i symbols of past), s]
// and accept(s) adds 1 to those m counts, then appends s to past (keeping the last k).  The
// reference ships the family as Markov_up_to_n(n, order, lfunc) (arith_code.py:443-464); this is
// that model whenever lfunc(c, o, n, order) == c * W[o].
//
// A stream's counts are one block of `stride` u32 words:
//   section i (i < k) at word off[i]: V^i rows of Vc = 4 * ceil(V / 4) counts, so every row
//   starts on a 16-B vector; the row of a context is the i context symbols read oldest first as
//   base-V digits (section 0 has the one row 0); entries V .. Vc - 1 of a row stay 0
//   stride = the sections' words rounded up to 256 B
#pragma once
#include <stdint.h>

namespace lac {

constexpr int kCountMaxOrder = 4;
constexpr int64_t kCountMaxVocab = 4096;
constexpr int64_t kCountMaxCounts = (int64_t)1 << 25;   // sum_{i<k} V^(i+1): an order-3 byte model fits
constexpr uint32_t kCountMaxWeight = (uint32_t)1 << 30; // W[i] < 2^30: 1 + 4 (2^30 - 1)(2^32 - 1) < 2^64
constexpr uint32_t kCountFull = 0xffffffffu;            // a count here cannot be incremented

// n-gram counts of one stream, sum_{i<k} V^(i+1); -1 past the limit
inline int64_t count_ngrams(int64_t V, int order) {
    int64_t n = 0, p = 1;
    for (int i = 0; i < order; i++) {
        if (p > kCountMaxCounts / V) return -1;
        p *= V;
        n += p;
        if (n > kCountMaxCounts) return -1;
    }
    return n;
}

// LAC_E_ARG beyond any limit
inline bool count_limits_ok(int64_t V, int order) {
    return V >= 1 && V <= kCountMaxVocab && order >= 1 && order <= kCountMaxOrder && count_ngrams(V, order) >= 0;
}
inline bool count_weights_ok(const uint32_t *W, int order) {
    for (int i = 0; i < order; i++)
        if (W[i] >= kCountMaxWeight) return false;
    return true;
}

struct CountLayout {
    int64_t V, Vc;             // symbols, padded row length in counts
    int order;
    int64_t off[4];            // first word of section i (0 for i >= order)
    int64_t words;             // words the sections hold
    int64_t stride;            // words per stream: `words` rounded up to 64 (256 B)
};

inline CountLayout count_layout(int64_t V, int order) {
    CountLayout y;
    y.V = V;
    y.Vc = (V + 3) / 4 * 4;
    y.order = order;
    int64_t o = 0, rows = 1;
    for (int i = 0; i < 4; i++) {
        y.off[i] = i < order ? o : 0;
        if (i < order) {
            o += rows * y.Vc;
            rows *= V;
        }
    }
    y.words = o;
    y.stride = (o + 63) / 64 * 64;
    return y;
}

// A stream's history as the coders hold it: m symbols, and for i <= m the row index of the last
// i symbols (idx[0] = 0).
struct CountCtx {
    int m;
    int64_t idx[4];
};

// past[order], most recent last, anything outside [0, V) absent: the valid history is the
// trailing run of symbols
inline CountCtx count_ctx(const int32_t *past, int order, int64_t V) {
    CountCtx c;
    c.m = 0;
    while (c.m < order && past[order - 1 - c.m] >= 0 && past[order - 1 - c.m] < V) c.m++;
    for (int i = 0; i < 4; i++) {
        c.idx[i] = 0;
        if (i <= c.m && i < order)
            for (int j = i; j >= 1; j--) c.idx[i] = c.idx[i] * V + past[order - j];
    }
    return c;
}

// the context after accepting s: the last i symbols of past + [s] are the last i - 1 of past,
// then s
inline void count_ctx_push(CountCtx &c, int64_t s, int64_t V, int order) {
    const int m1 = c.m + 1 < order ? c.m + 1 : order;
    for (int i = (m1 < order - 1 ? m1 : order - 1); i >= 1; i--) c.idx[i] = c.idx[i - 1] * V + s;
    c.m = m1;
}

inline const uint32_t *count_row_ptr(const uint32_t *cs, const CountLayout &y, int i, int64_t idx) {
    return cs + y.off[i] + idx * y.Vc;
}

// The row of a step from a stream's counts `cs`: row[s] = 1 + sum_{i<m} W[i] C_i[ctx_i, s], V
// entries.  Returns the row's status for entries of pmf_bits: false for an entry that does not
// fit or a total >= 2^64 (LAC_E_TABLE at that step); *T_out and *minp_out its total and
// smallest entry otherwise.
inline bool count_row(const uint32_t *cs, const CountLayout &y, const uint32_t *W, const CountCtx &c, int pmf_bits,
                      uint64_t *row, uint64_t *T_out, uint64_t *minp_out) {
    typedef unsigned __int128 u128;
    u128 T = 0;
    uint64_t minp = ~(uint64_t)0;
    bool ok = true;
    for (int64_t s = 0; s < y.V; s++) {
        uint64_t x = 1;
        for (int i = 0; i < c.m; i++) x += (uint64_t)W[i] * count_row_ptr(cs, y, i, c.idx[i])[s];
        row[s] = x;
        T += x;
        if (x < minp) minp = x;
        if (pmf_bits == 32 && (x >> 32)) ok = false;
    }
    if (T >> 64) ok = false;
    *T_out = ok ? (uint64_t)T : 0;
    *minp_out = ok ? minp : 0;
    return ok;
}

// accept(s): the m counts of s under the current contexts + 1, then the context moves.  false,
// and nothing changes, when one of them is full (LAC_E_TABLE at that step).
inline bool count_accept(uint32_t *cs, const CountLayout &y, CountCtx &c, int64_t s) {
    for (int i = 0; i < c.m; i++)
        if (count_row_ptr(cs, y, i, c.idx[i])[s] == kCountFull) return false;
    for (int i = 0; i < c.m; i++) cs[y.off[i] + c.idx[i] * y.Vc + s] += 1;
    count_ctx_push(c, s, y.V, y.order);
    return true;
}

}  // namespace lac
