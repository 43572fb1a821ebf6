// lac_history.h -- plain host rules of the match-history models (include/lac.h lac_hist_*; the
// reference's History predictor, arith_code.py:364-398): the limits a model must keep, what a
// stream's state is, how a step's row is built from it and how accept moves it -- the literal
// rule, and the incremental rule the kernels of lac_history.hip run, held to the literal one
// without a GPU (tests/native/history_check.cpp).
//
// A model has V symbols, a ring of P in [1, 256] past symbols and a table of weights
// L[i][r] < 2^48 (i the lag, r the run), stored L[i * P + r].  A stream keeps `ring`, int32 [P],
// all -1 at the start, and the write index `pasti`, 0 at the start.  With
//     p_i = ring[(pasti - 1 - i) mod P]                              the symbol i + 1 steps back
//     r_i = the number of j = 1, 2, ... < P - i, taken while they hold, with
//           ring[(pasti - 1 - i - j) mod P] == ring[(pasti - j) mod P]
// the row of a step is
//     pmf[s] = 1 + sum_{i < P : p_i == s and p_i > 0} L[i][r_i]
// and accept(s) does ring[pasti] = s, pasti = (pasti + 1) mod P.  The test is p_i > 0: symbol 0,
// like the -1 filler, never gains weight, so pmf[0] == 1 and 1 is every row's smallest entry; and
// -1 == -1 in the comparisons, so an empty ring matches itself (History.runs, :371-380).
//
// Incremental form.  M_i is lag i's match length before the clamp at P - i - 1, saturating at P:
//     r_i = min(P - i - 1, M_i)
//     accept(s):  M_i <- (p_i == s) ? min(P, M_i + 1) : 0     for every i, p_i before the write
// A match of lag i that reaches back j symbols becomes one of j + 1 when the next symbol equals
// the one i + 1 before it, and is lost otherwise; the clamp is what keeps the literal loop off
// the ring's oldest slot.  M is derived state: it is rebuilt from ring and pasti by the literal
// rule (M_i = r_i, which the recurrence continues exactly: a run at its clamp stays there on a
// match) whenever they are set, and is never part of what a caller saves.
#pragma once
#include <stdint.h>

#ifdef __HIP__
#define LAC_HIST_HD __host__ __device__      // the two rules the kernels call as they are
#else
#define LAC_HIST_HD
#endif

namespace lac {

constexpr int kHistMaxPast = 256;
constexpr int64_t kHistMaxVocab = 4096;
constexpr uint64_t kHistMaxWeight = (uint64_t)1 << 48;   // L < 2^48: T <= 4096 + 256 (2^48 - 1) < 2^57

// LAC_E_ARG beyond any limit
inline bool hist_limits_ok(int64_t V, int64_t P) {
    return V >= 1 && V <= kHistMaxVocab && P >= 1 && P <= kHistMaxPast;
}
inline bool hist_weights_ok(const uint64_t *L, int P) {
    for (int64_t k = 0; k < (int64_t)P * P; k++)
        if (L[k] >= kHistMaxWeight) return false;
    return true;
}
// a state lac_hist_set_state takes: ring entries in [-1, V), pasti in [0, P)
LAC_HIST_HD inline bool hist_entry_ok(int32_t x, int64_t V) { return x >= -1 && x < V; }
inline bool hist_state_ok(const int32_t *ring, int32_t pasti, int64_t V, int P) {
    if (pasti < 0 || pasti >= P) return false;
    for (int i = 0; i < P; i++)
        if (!hist_entry_ok(ring[i], V)) return false;
    return true;
}

// ring[x mod P] for x in [-2 P, P)
inline int32_t hist_at(const int32_t *ring, int x, int P) {
    while (x < 0) x += P;
    return ring[x];
}
// p_i and the literal r_i
inline int32_t hist_sym(const int32_t *ring, int pasti, int P, int i) { return hist_at(ring, pasti - 1 - i, P); }
inline int hist_run_literal(const int32_t *ring, int pasti, int P, int i) {
    int r = 0;
    for (int j = 1; j < P - i; j++) {
        if (hist_at(ring, pasti - 1 - i - j, P) != hist_at(ring, pasti - j, P)) break;
        r++;
    }
    return r;
}

// the incremental state: M of the initial ring, M rebuilt from a ring that was set
inline void hist_m_init(int32_t *M, int P) {
    for (int i = 0; i < P; i++) M[i] = P;
}
inline void hist_m_rebuild(const int32_t *ring, int pasti, int P, int32_t *M) {
    for (int i = 0; i < P; i++) M[i] = hist_run_literal(ring, pasti, P, i);
}
inline int hist_run(const int32_t *M, int P, int i) { return M[i] < P - i - 1 ? M[i] : P - i - 1; }
// one lag's move on accepting s (p: p_i before the write)
LAC_HIST_HD inline int32_t hist_m_next(int32_t Mi, int32_t p, int32_t s, int P) { return p == s ? (Mi + 1 < P ? Mi + 1 : P) : 0; }

// accept(s): M moves by the incremental rule (when kept), then the ring
inline void hist_accept(int32_t *ring, int32_t *pasti, int P, int32_t *M, int32_t s) {
    if (M)
        for (int i = 0; i < P; i++) M[i] = hist_m_next(M[i], hist_sym(ring, *pasti, P, i), s, P);
    ring[*pasti] = s;
    *pasti = *pasti + 1 == P ? 0 : *pasti + 1;
}

// The row of a step, V entries: with M the incremental runs, with M == nullptr the literal ones.
// Returns the row's status for entries of pmf_bits: false for an entry that does not fit
// (LAC_E_TABLE at that step; totals cannot reach 2^64 under the weight limit); *T_out its total.
inline bool hist_row(const int32_t *ring, int pasti, int P, const int32_t *M, const uint64_t *L, int64_t V,
                     int pmf_bits, uint64_t *row, uint64_t *T_out) {
    for (int64_t s = 0; s < V; s++) row[s] = 1;
    for (int i = 0; i < P; i++) {
        const int32_t p = hist_sym(ring, pasti, P, i);
        const int r = M ? hist_run(M, P, i) : hist_run_literal(ring, pasti, P, i);
        if (p > 0 && p < V) row[p] += L[(int64_t)i * P + r];
    }
    uint64_t T = 0;
    bool ok = true;
    for (int64_t s = 0; s < V; s++) {
        T += row[s];
        if (pmf_bits == 32 && (row[s] >> 32)) ok = false;
    }
    *T_out = ok ? T : 0;
    return ok;
}

}  // namespace lac
