// topk_check.cpp -- lac_amd/csrc/lac_topk.h (the rules of lac_topk_logits) as a host library for
// tests/test_topk_host.py: the argument rules, the form selection and its seams, the level ->
// class rule, the threshold search in its literal and its lane form, and whole rows by the literal
// rule and by the kernels' histogram / threshold / ordered-rank form walked over emulated tiles,
// waves, register rounds and lanes.  tk_sweep holds the forms to each other on random and tie-heavy
// rows; with -DTOPK_CHECK_MAIN it is a stand-alone program for AddressSanitizer +
// UndefinedBehaviorSanitizer (host code only).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "lac_topk.h"

using namespace lac;

namespace {

const uint32_t kTab[LAC_Q1_TAB_SIZE] = LAC_Q1_TAB_INIT;

struct Rng {                                                  // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    uint64_t below(uint64_t n) { return next() % n; }
    float unit() { return (float)(next() >> 40) / (float)(1 << 24); }
};

uint16_t to_bf16(float f) {                                   // truncation: any bf16 will do
    uint32_t u;
    memcpy(&u, &f, 4);
    return (uint16_t)(u >> 16);
}

// a row of `kind`: 0 random over 30 nats, 1 flat, 2 two values near the threshold classes, 3 with
// specials, 4 many entries at the maximum
void make_row(Rng &g, int kind, int tb, int64_t V, std::vector<uint8_t> &buf) {
    buf.assign((size_t)(V * tb), 0);
    const float top = (float)((int)g.below(41) - 20);
    for (int64_t i = 0; i < V; i++) {
        float x;
        switch (kind) {
        case 0: x = top - 30.0f * g.unit(); break;
        case 1: x = top; break;
        case 2: x = top - 13.3f - 3.7f * g.unit(); break;
        case 3: {
            const uint64_t q = g.below(12);
            x = q == 0 ? -INFINITY : q == 1 ? NAN : top - 20.0f * g.unit();
            break;
        }
        default: x = g.below(3) ? top : top - 18.0f * g.unit(); break;
        }
        if (tb == 2) ((uint16_t *)buf.data())[i] = to_bf16(x);
        else ((float *)buf.data())[i] = x;
    }
    if (kind == 2) {                                          // (the maximum itself somewhere)
        if (tb == 2) ((uint16_t *)buf.data())[g.below((uint64_t)V)] = to_bf16(top);
        else ((float *)buf.data())[g.below((uint64_t)V)] = top;
    }
}

}  // namespace

extern "C" {

int tk_args_ok(uint64_t lg, int type, int64_t V, int64_t ss, int64_t bs, int64_t k, int64_t wb, int64_t K, uint64_t idx,
               uint64_t wt) {
    return topk_args_ok((uintptr_t)lg, type, V, ss, bs, k, wb, K, (uintptr_t)idx, (uintptr_t)wt) ? 1 : 0;
}

// out: form, R, threads, tiles
int tk_plan(int64_t V, int type_bytes, int forced, int *out) {
    const TopkPlan p = topk_plan(V, type_bytes, forced);
    out[0] = p.form;
    out[1] = p.R;
    out[2] = p.threads;
    out[3] = p.tiles;
    return p.rc;
}

// out: the first symbol after a thread, register-round, wave and tile seam
int tk_seams(int64_t V, int type_bytes, int forced, int64_t *out) {
    const TopkPlan p = topk_plan(V, type_bytes, forced);
    if (p.rc) return p.rc;
    topk_seams(p, type_bytes, out);
    return 0;
}

void tk_class(int j, int *lo, int *hi) {
    *lo = topk_class_lo(kTab, j);
    *hi = topk_class_hi(kTab, j);
}

uint32_t tk_level(float x, float m) { return topk_level(x, topk_c(m)); }

// out: jlo, jhi, above, r, ties;  which 0: the literal search, 1: the lanes
void tk_threshold(int which, const uint32_t *hist, int k, int64_t *out) {
    const TopkCut c = which ? topk_threshold_lanes(hist, kTab, k) : topk_threshold(hist, kTab, k);
    out[0] = c.jlo;
    out[1] = c.jhi;
    out[2] = c.above;
    out[3] = c.r;
    out[4] = c.ties;
}

// one row: which 0 the literal rule, 1 the kernels' form under topk_plan(V, type_bytes, forced)
int tk_row(int which, const void *row, int type_bytes, int64_t V, int k, int weight_bits, int K, int forced,
           int32_t *idx_out, uint32_t *wt_out) {
    if (!which) {
        topk_row_literal(row, type_bytes, V, kTab, k, weight_bits, K, idx_out, wt_out);
        return 0;
    }
    const TopkPlan p = topk_plan(V, type_bytes, forced);
    if (p.rc) return p.rc;
    topk_row_lanes(row, type_bytes, V, kTab, p, k, weight_bits, K, idx_out, wt_out);
    return 0;
}

// Random and tie-heavy rows: the literal rule against the kernels' form under both plans (outputs
// pre-filled with a sentinel: every slot must be written), and the literal threshold against the lanes'.
int tk_sweep(uint64_t seed, int64_t *count) {
    Rng g{seed};
    int bad = 0;
    int64_t n = 0;
    std::vector<uint8_t> buf;
    for (int it = 0; it < 600; it++) {
        const int tb = g.below(2) ? 2 : 4, per = 16 / tb;
        const int64_t V = per * (1 + (int64_t)g.below(it % 10 == 0 ? 1100 : 140));
        const int kind = (int)g.below(5);
        make_row(g, kind, tb, V, buf);
        const int kmax = (int)(V < kTopkMaxK ? V : kTopkMaxK);
        const int ks[] = {1, 2, 63, 64, 255, 256, kmax, 1 + (int)g.below((uint64_t)kmax)};
        for (int k : ks) {
            if (k > kmax) continue;
            const int K = g.below(2) ? (k + 3) / 4 * 4 : kTopkMaxK, wb = (int)g.below(25);
            int32_t ia[kTopkMaxK], ib[kTopkMaxK];
            uint32_t wa[kTopkMaxK], wbuf[kTopkMaxK];
            topk_row_literal(buf.data(), tb, V, kTab, k, wb, K, ia, wa);
            for (int s = 0; s < K; s++) {                     // a valid sparse row
                if (s < k ? (ia[s] < 0 || ia[s] >= V || (s && ia[s - 1] >= ia[s])) : (ia[s] != -1 || wa[s] != 0)) bad++;
            }
            for (int forced = 1; forced <= 2; forced++) {
                for (int s = 0; s < kTopkMaxK; s++) {
                    ib[s] = -7;
                    wbuf[s] = 0xDEADBEEFu;
                }
                if (tk_row(1, buf.data(), tb, V, k, wb, K, forced, ib, wbuf)) bad++;
                if (memcmp(ia, ib, sizeof(int32_t) * (size_t)K) || memcmp(wa, wbuf, sizeof(uint32_t) * (size_t)K)) bad++;
                n++;
            }
        }
        // thresholds on the row's own histogram, at every k
        uint32_t hist[kTopkLevels] = {0};
        const float c = topk_row_c(buf.data(), tb, V);
        for (int64_t i = 0; i < V; i++) hist[topk_level(topk_load(buf.data(), tb, i), c)]++;
        for (int k = 1; k <= kmax; k++) {
            const TopkCut a = topk_threshold(hist, kTab, k), b = topk_threshold_lanes(hist, kTab, k);
            if (a.jlo != b.jlo || a.jhi != b.jhi || a.above != b.above || a.r != b.r || a.ties != b.ties) bad++;
            if (a.above >= (uint32_t)k || a.r < 1 || a.r > a.ties) bad++;
            n++;
        }
    }
    *count = n;
    return bad;
}

}  // extern "C"

#ifdef TOPK_CHECK_MAIN
int main() {
    int64_t n = 0;
    const int bad = tk_sweep(12345, &n);
    printf("topk_check: %lld checks, %d bad\n", (long long)n, bad);
    if (bad) return 1;
    printf("topk_check: ok\n");
    return 0;
}
#endif
