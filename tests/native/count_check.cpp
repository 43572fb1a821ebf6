// count_check.cpp -- host checks of lac_amd/csrc/lac_count.h, the plain host rules of the adaptive
// n-gram count models: the limits, the per-stream layout, the context indices, and the row and
// accept against a sparse n-gram map.  tests/test_counts_host.py builds it as a shared library and,
// with -DCOUNT_CHECK_MAIN, as a stand-alone program under AddressSanitizer +
// UndefinedBehaviorSanitizer: every buffer of the sweep is a heap block of exactly the size the
// layout names.
#include <stdint.h>
#include <stdio.h>

#include <map>
#include <vector>

#include "lac_count.h"

using namespace lac;

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
                fprintf(stderr, "count_check: %s:%d: ", __FILE__, __LINE__); \
                fprintf(stderr, __VA_ARGS__);  \
                fprintf(stderr, "\n");         \
            }                                  \
            g_fail++;                          \
        }                                      \
    } while (0)

// One random model and history: the dense rules against a map from n-gram to count.
void check_model(Rng &r, int64_t V, int order, int steps, int pmf_bits) {
    const CountLayout y = count_layout(V, order);
    std::vector<uint32_t> W((size_t)order);
    for (auto &w : W) w = r.below(3) == 0 ? 0 : (uint32_t)r.below(r.below(2) ? 50 : kCountMaxWeight);
    std::vector<uint32_t> cs((size_t)y.stride, 0);                // exactly one stream's block
    std::vector<int32_t> past((size_t)order, -1);
    std::map<std::vector<int32_t>, uint32_t> sparse;
    std::vector<int32_t> hist;
    std::vector<uint64_t> row((size_t)V);
    CountCtx c = count_ctx(past.data(), order, V);
    EXPECT(c.m == 0, "fresh history");
    for (int t = 0; t < steps; t++) {
        // the context, two ways: pushed step by step, and from the stored past
        for (int j = 0; j < order; j++)
            past[(size_t)j] = (int)hist.size() >= order - j ? hist[hist.size() - (size_t)(order - j)] : -1;
        const CountCtx d = count_ctx(past.data(), order, V);
        EXPECT(d.m == c.m && d.m == (int)(hist.size() < (size_t)order ? hist.size() : (size_t)order), "m at %d", t);
        for (int i = 0; i < order && i <= c.m; i++) EXPECT(d.idx[i] == c.idx[i], "idx[%d] at %d", i, t);
        uint64_t T = 0, minp = 0;
        const bool ok = count_row(cs.data(), y, W.data(), c, pmf_bits, row.data(), &T, &minp);
        unsigned __int128 sum = 0;
        uint64_t mn = ~(uint64_t)0;
        bool fits = true;
        for (int64_t s = 0; s < V; s++) {
            uint64_t x = 1;
            for (int i = 0; i < c.m; i++) {
                std::vector<int32_t> key(hist.end() - i, hist.end());
                key.push_back((int32_t)s);
                auto it = sparse.find(key);
                if (it != sparse.end()) x += (uint64_t)W[(size_t)i] * it->second;
            }
            EXPECT(row[(size_t)s] == x, "row[%lld] at %d", (long long)s, t);
            sum += x;
            mn = x < mn ? x : mn;
            fits = fits && (pmf_bits == 64 || !(x >> 32));
        }
        fits = fits && !(sum >> 64);
        EXPECT(ok == fits, "row status at %d", t);
        if (ok) EXPECT(T == (uint64_t)sum && minp == mn, "T / minp at %d", t);
        else EXPECT(T == 0 && minp == 0, "bad row's T at %d", t);
        // accept: a recurring symbol half the time
        const int32_t s = (hist.size() >= 2 && r.below(2)) ? hist[hist.size() - 2] : (int32_t)r.below((uint64_t)V);
        EXPECT(count_accept(cs.data(), y, c, s), "accept at %d", t);
        for (int i = 0; i < (int)(hist.size() < (size_t)order ? hist.size() : (size_t)order); i++) {
            std::vector<int32_t> key(hist.end() - i, hist.end());
            key.push_back(s);
            sparse[key] += 1;
        }
        hist.push_back(s);
    }
    // the padding of every row stays 0, and the counts are the map's
    uint64_t total = 0, want = 0;
    for (int i = 0; i < order; i++) {
        int64_t rows = 1;
        for (int j = 0; j < i; j++) rows *= V;
        for (int64_t q = 0; q < rows; q++)
            for (int64_t s = 0; s < y.Vc; s++) {
                const uint32_t x = cs[(size_t)(y.off[i] + q * y.Vc + s)];
                if (s >= V) EXPECT(x == 0, "padding of section %d", i);
                total += x;
            }
    }
    for (auto &kv : sparse) want += kv.second;
    EXPECT(total == want, "sum of the counts");
    // a full count refuses the step and changes nothing
    if (c.m > 0) {
        const int32_t s = (int32_t)r.below((uint64_t)V);
        uint32_t *slot = &cs[(size_t)(y.off[c.m - 1] + c.idx[c.m - 1] * y.Vc + s)];
        const uint32_t keep = *slot;
        *slot = kCountFull;
        const std::vector<uint32_t> before = cs;
        const CountCtx cb = c;
        EXPECT(!count_accept(cs.data(), y, c, s), "a full count is refused");
        EXPECT(cs == before && c.m == cb.m, "a refused step changes nothing");
        *slot = keep;
    }
}

}  // namespace

extern "C" {

int cc_limits_ok(int64_t V, int order) { return count_limits_ok(V, order) ? 1 : 0; }
int cc_weights_ok(const uint32_t *W, int order) { return count_weights_ok(W, order) ? 1 : 0; }
int64_t cc_ngrams(int64_t V, int order) { return count_ngrams(V, order); }

// out[7] = {Vc, stride, words, off[4]}
void cc_layout(int64_t V, int order, int64_t *out) {
    const CountLayout y = count_layout(V, order);
    out[0] = y.Vc;
    out[1] = y.stride;
    out[2] = y.words;
    for (int i = 0; i < 4; i++) out[3 + i] = y.off[i];
}

// One stream's walk: counts [stride] and past [order] in and out, rows_out [n][V], ok_out [n] the
// row's status, acc_out [n] whether the step was accepted (a bad row or symbol ends the walk).
void cc_walk(int64_t V, int order, const uint32_t *W, int pmf_bits, const int32_t *syms, int64_t n, uint32_t *counts,
             int32_t *past, uint64_t *rows_out, int32_t *ok_out, int32_t *acc_out) {
    const CountLayout y = count_layout(V, order);
    CountCtx c = count_ctx(past, order, V);
    std::vector<int32_t> hist;
    for (int j = order - c.m; j < order; j++) hist.push_back(past[j]);
    bool dead = false;
    for (int64_t t = 0; t < n; t++) {
        uint64_t T, minp;
        ok_out[t] = count_row(counts, y, W, c, pmf_bits, rows_out + t * V, &T, &minp) ? 1 : 0;
        const bool go = !dead && ok_out[t] && syms[t] >= 0 && syms[t] < V && count_accept(counts, y, c, syms[t]);
        acc_out[t] = go ? 1 : 0;
        if (go) hist.push_back(syms[t]);
        else dead = true;
    }
    for (int j = 0; j < order; j++)
        past[j] = (int)hist.size() >= order - j ? hist[hist.size() - (size_t)(order - j)] : -1;
}

int cc_sweep(int n, uint64_t seed) {
    Rng r{seed ? seed : 1};
    g_fail = 0;
    static const int64_t Vs[] = {1, 2, 3, 4, 5, 7, 8, 17, 64, 255, 256, 257, 300};
    for (int k = 0; k < n; k++) {
        const int64_t V = Vs[r.below(sizeof(Vs) / sizeof(Vs[0]))];
        int order = 1 + (int)r.below(4);
        while (!count_limits_ok(V, order)) order--;
        check_model(r, V, order, 20 + (int)r.below(60), r.below(2) ? 32 : 64);
    }
    return g_fail;
}

}  // extern "C"

#ifdef COUNT_CHECK_MAIN
int main() {
    const int bad = cc_sweep(120, 4242);
    if (bad) {
        fprintf(stderr, "count_check: %d failures\n", bad);
        return 1;
    }
    printf("count_check: ok\n");
    return 0;
}
#endif
