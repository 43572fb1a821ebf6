// fsm_check.cpp -- host checks of lac_amd/csrc/lac_fsm.h, the plain host rules of the finite-state
// models: the limits, the prepared layout and what a prepared row holds against a plain scan of
// the row.  tests/test_fsm_host.py builds it as a shared library and, with -DFSM_CHECK_MAIN, as a
// stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer: every buffer of the
// sweep is a heap block of exactly the size the layout names.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "lac_fsm.h"

using namespace lac;
typedef unsigned __int128 u128;

namespace {

struct Rng {
    uint64_t s;
    uint64_t next() {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return s;
    }
    uint64_t below(uint64_t n) { return n ? next() % n : 0; }
};

int g_fail = 0;
#define EXPECT(cond, ...)                      \
    do {                                       \
        if (!(cond)) {                         \
            if (g_fail < 20) {                 \
                fprintf(stderr, "fsm_check: %s:%d: ", __FILE__, __LINE__); \
                fprintf(stderr, __VA_ARGS__);  \
                fprintf(stderr, "\n");         \
            }                                  \
            g_fail++;                          \
        }                                      \
    } while (0)

// V entries of type E summing to `target` exactly (target below 2^64, and within E's range), some zero
template <typename E>
std::vector<E> row_with_total(Rng &r, int64_t V, uint64_t target) {
    std::vector<E> row((size_t)V, (E)0);
    const uint64_t base = target / (uint64_t)V;
    uint64_t sum = 0;
    for (int64_t i = 0; i + 1 < V; i++) {
        uint64_t e = r.below(4) == 0 ? 0 : base - r.below(base / 2 + 1);
        row[(size_t)i] = (E)e;
        sum += e;
    }
    row[(size_t)V - 1] = (E)(target - sum);
    return row;
}

// every_bound: the search is probed at c_i - 1, c_i and T - 1 for every positive entry too
template <typename E>
void check_row(Rng &r, const std::vector<E> &row, int64_t V, bool every_bound = false) {
    const FsmLayout y = fsm_layout(1, V, 8 * (int)sizeof(E), false);
    EXPECT(y.Vp >= V && y.Vp < V + y.vec && y.Vp % y.vec == 0 && y.nvec * y.vec == y.Vp, "padding V=%lld", (long long)V);
    EXPECT(y.G * 64 >= y.nvec && (y.G - 1) * 64 < y.nvec, "chunking V=%lld", (long long)V);
    std::vector<E> cdf((size_t)y.Vp), pad((size_t)y.Vp), bounds(y.long_rows ? 64 : 0);
    FsmMeta m;
    fsm_prepare_row<E>(row.data(), y, cdf.data(), pad.data(), y.long_rows ? bounds.data() : nullptr, &m);
    // the plain scan
    u128 T = 0;
    uint64_t minp = 0;
    for (int64_t i = 0; i < V; i++) {
        T += row[(size_t)i];
        if (row[(size_t)i] && (!minp || row[(size_t)i] < minp)) minp = row[(size_t)i];
    }
    const bool bad = T == 0 || (T >> 64);
    EXPECT(m.T == (bad ? 0 : (uint64_t)T), "total V=%lld", (long long)V);
    for (int64_t i = 0; i < y.Vp; i++) EXPECT(pad[(size_t)i] == (i < V ? row[(size_t)i] : (E)0), "padded row");
    if (bad) {
        EXPECT(m.minp == 0 && m.fthr == 0 && m.inv_T == 0.0, "bad row's meta");
        return;
    }
    EXPECT(m.minp == minp, "minp");
    const u128 thr = (T + (minp - 1)) / minp;
    EXPECT(m.fthr == (thr < kFsmThrCap ? (uint64_t)thr : kFsmThrCap), "ceil(T / minp)");
    EXPECT(m.inv_T == 1.0 / (double)(uint64_t)T, "1 / T");
    for (int k = 0; k < 8; k++) {                              // fudged iff T > w minp, for every width a coder has
        const uint64_t w = k == 0 ? 1 : (k == 1 ? (uint64_t)1 << 61 : 1 + r.below((uint64_t)1 << (1 + r.below(61))));
        EXPECT((w < m.fthr) == (T > (u128)w * minp), "fudge threshold at w=%llu", (unsigned long long)w);
    }
    if (fsm_row_wide<E>((uint64_t)T)) return;                  // a wide row's CDF is not read
    uint64_t c = 0;
    for (int64_t s = 0; s < V; s++) {                          // the O(1) lookup against the scan
        uint64_t lo, hi;
        fsm_lookup<E>(cdf.data(), s, &lo, &hi);
        EXPECT(lo == c && hi == c + row[(size_t)s], "lookup s=%lld V=%lld", (long long)s, (long long)V);
        c += row[(size_t)s];
    }
    for (int64_t i = V; i < y.Vp; i++) EXPECT((uint64_t)cdf[(size_t)i] == (uint64_t)T, "CDF padding");
    std::vector<uint64_t> targets;
    for (int k = 0; k < 24; k++) targets.push_back(k == 0 ? 0 : (k == 1 ? (uint64_t)T - 1 : r.below((uint64_t)T)));
    if (every_bound) {
        c = 0;
        for (int64_t i = 0; i < V; i++) {
            if (!row[(size_t)i]) continue;
            c += row[(size_t)i];                               // c_i: the first target past entry i
            targets.push_back(c - 1);
            if (c < (uint64_t)T) targets.push_back(c);
        }
    }
    for (const uint64_t tgt : targets) {                       // the decoder's search against bisect_right
        int64_t want = 0;
        uint64_t cc = 0;
        for (int64_t i = 0; i < V; i++) {
            cc += row[(size_t)i];
            if (cc <= tgt) want = i + 1;
        }
        const int64_t got = fsm_search<E>(cdf.data(), y.long_rows ? bounds.data() : nullptr, y, tgt);
        EXPECT(got == want && got < V, "search tgt=%llu V=%lld: %lld, want %lld", (unsigned long long)tgt, (long long)V,
               (long long)got, (long long)want);
    }
}

// A sparse row of a long-row layout: at most 8 positive entries, on both sides of a chunk bound,
// of a second chunk bound at least two whole zero chunks on, and of a 16-B vector bound inside a
// chunk, plus entries 0 and V - 1; `drop` (a bit per position) leaves some out, so a zero run
// crosses a bound, starts the row or reaches its end.
template <typename E>
void check_sparse_row(Rng &r, int64_t V, unsigned drop) {
    const FsmLayout y = fsm_layout(1, V, 8 * (int)sizeof(E), false);
    const int64_t CE = y.G * y.vec, chunks = (y.Vp + CE - 1) / CE;
    EXPECT(y.long_rows && chunks >= 6, "sparse rows need a long-row layout, V=%lld", (long long)V);
    if (!y.long_rows || chunks < 6) return;
    const int64_t c1 = 1 + (int64_t)r.below((uint64_t)(chunks - 5)), c2 = c1 + 3;   // chunks c1 + 1, c1 + 2: all zero
    const int64_t vb = (chunks - 1) * CE + y.vec;              // a vector bound inside the last chunk, if it has one
    int64_t at[8] = {0, c1 * CE - 1, c1 * CE, c2 * CE - 1, c2 * CE, vb - 1, vb, V - 1};
    if (y.G < 2 || vb >= V - 1) at[5] = at[6] = (c2 + 1) * CE - 1 < V ? c2 * CE + y.vec : V - 1;
    std::vector<E> row((size_t)V, (E)0);
    int n = 0;
    for (int k = 0; k < 8; k++)
        if (!((drop >> k) & 1) && at[k] >= 0 && at[k] < V) {
            row[(size_t)at[k]] = (E)(1 + r.below(k & 1 ? 1 : 1 << 12));
            n++;
        }
    if (!n) row[(size_t)(c1 * CE)] = 1;
    int64_t run = 0, longest = 0;                              // (the zero run of two chunks is there)
    for (int64_t i = 0; i < V; i++) {
        run = row[(size_t)i] ? 0 : run + 1;
        longest = run > longest ? run : longest;
    }
    EXPECT(longest >= 2 * CE, "zero run of %lld entries, a chunk has %lld", (long long)longest, (long long)CE);
    check_row<E>(r, row, V, true);
}

int64_t pick_vocab(Rng &r, int i) {
    static const int64_t edge[] = {1, 2, 3, 4, 5, 127, 128, 129, 255, 256, 257, 260, 511, 512, 513, 4097};
    if (i % 3 == 0) return edge[r.below(sizeof edge / sizeof *edge)];
    return i % 50 == 7 ? 65536 : 1 + (int64_t)r.below(700);
}

}  // namespace

extern "C" {

int fc_limits_ok(int64_t K, int64_t V) { return fsm_limits_ok(K, V); }

// out: Vp, nvec, long_rows, G, off_meta, off_cdf, off_pmf, off_bounds, off_next, bytes, sizeof(FsmMeta)
void fc_layout(int64_t K, int64_t V, int pmf_bits, int has_next, uint64_t *out) {
    const FsmLayout y = fsm_layout(K, V, pmf_bits, has_next != 0);
    const uint64_t v[] = {(uint64_t)y.Vp, (uint64_t)y.nvec, (uint64_t)y.long_rows, (uint64_t)y.G, y.off_meta, y.off_cdf,
                          y.off_pmf, y.off_bounds, y.off_next, y.bytes, sizeof(FsmMeta)};
    for (size_t i = 0; i < sizeof v / sizeof *v; i++) out[i] = v[i];
}

// `rows` random rows (a third u32, the rest u64 with the totals the divisions care about);
// returns the number of failed expectations
int fc_sweep(int rows, uint64_t seed) {
    Rng r{seed | 1};
    g_fail = 0;
    const uint64_t p32 = ((uint64_t)1 << 32) - 1, p50 = (uint64_t)1 << 50, p60 = (uint64_t)1 << 60,
                   p63 = (uint64_t)1 << 63;
    for (int i = 0; i < rows; i++) {
        const int64_t V = pick_vocab(r, i);
        switch (i % 12) {
        case 0: check_row<uint32_t>(r, row_with_total<uint32_t>(r, V, p32), V); break;
        case 1: check_row<uint32_t>(r, row_with_total<uint32_t>(r, V, 1 + r.below(p32)), V); break;
        case 2: check_row<uint32_t>(r, row_with_total<uint32_t>(r, V, 1 + r.below(1 << 16)), V); break;
        case 3: {                                             // a wide u32 row: every entry near 2^31
            const int64_t Vw = V < 3 ? 3 : V;
            std::vector<uint32_t> row((size_t)Vw);
            for (auto &e : row) e = (uint32_t)(((uint64_t)1 << 31) + r.below(1 << 20));
            check_row<uint32_t>(r, row, Vw);
            break;
        }
        case 4: check_row<uint64_t>(r, row_with_total<uint64_t>(r, V, p32), V); break;
        case 5: check_row<uint64_t>(r, row_with_total<uint64_t>(r, V, p50 - 1), V); break;
        case 6: check_row<uint64_t>(r, row_with_total<uint64_t>(r, V, p50 + 1), V); break;
        case 7: check_row<uint64_t>(r, row_with_total<uint64_t>(r, V, p60 - r.below(1 << 20)), V); break;
        case 8: check_row<uint64_t>(r, row_with_total<uint64_t>(r, V, p63 + r.below(p63)), V); break;
        case 9: check_row<uint64_t>(r, row_with_total<uint64_t>(r, V, 1 + r.below(p60)), V); break;
        case 10: {                                            // bad rows: empty, and a total of 2^64 and more
            std::vector<uint64_t> row((size_t)(V < 2 ? 2 : V), 0);
            if (i % 24 == 10) { row[0] = p63; row[row.size() - 1] = p63 + r.below(1000); }
            check_row<uint64_t>(r, row, (int64_t)row.size());
            break;
        }
        default: check_row<uint64_t>(r, row_with_total<uint64_t>(r, V, ~(uint64_t)0), V); break;   // 2^64 - 1
        }
    }
    // sparse rows of long-row layouts: every position kept, one side of a bound dropped, a row that
    // ends in a zero run, a row of its first entry alone, then random subsets
    static const int64_t V32[] = {260, 1000, 4100, 65536}, V64[] = {129, 1000, 65536};
    static const unsigned drops[] = {0x00, 0x02, 0x04, 0x08, 0x10, 0x80, 0xe0, 0x01, 0xfe, 0x7d, 0xfb, 0x06};
    for (int i = 0; i < rows / 25; i++) {
        const unsigned drop = i < 12 ? drops[i] : (unsigned)r.below(256);
        check_sparse_row<uint32_t>(r, V32[i % 4], drop);
        check_sparse_row<uint64_t>(r, V64[i % 3], drop);
    }
    return g_fail;
}

}  // extern "C"

#ifdef FSM_CHECK_MAIN
int main() {
    const int bad = fc_sweep(1000, 20261020);
    if (bad) {
        fprintf(stderr, "fsm_check: %d failed expectations\n", bad);
        return 1;
    }
    printf("fsm_check: ok\n");
    return 0;
}
#endif
