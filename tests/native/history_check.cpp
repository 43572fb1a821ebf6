// history_check.cpp -- host checks of lac_amd/csrc/lac_history.h, the plain host rules of the
// match-history models: the limits, the states lac_hist_set_state takes, and the incremental rule
// the kernels run (M_i, r_i = min(P - i - 1, M_i)) against the literal loops of the reference's
// History.runs, step by step, with the ring wrapping, M saturating, and the state set in
// mid-sequence.  tests/test_history_host.py builds it as a shared library and, with
// -DHISTORY_CHECK_MAIN, as a stand-alone program under AddressSanitizer +
// UndefinedBehaviorSanitizer: every buffer of the sweep is a heap block of exactly P (or V) entries.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "lac_history.h"

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
int64_t g_steps = 0;
#define EXPECT(cond, ...)                      \
    do {                                       \
        if (!(cond)) {                         \
            if (g_fail < 20) {                 \
                fprintf(stderr, "history_check: %s:%d: ", __FILE__, __LINE__); \
                fprintf(stderr, __VA_ARGS__);  \
                fprintf(stderr, "\n");         \
            }                                  \
            g_fail++;                          \
        }                                      \
    } while (0)

// every lag's run, incremental against literal
void same_runs(const std::vector<int32_t> &ring, int pasti, int P, const std::vector<int32_t> &M, const char *what,
               int t) {
    for (int i = 0; i < P; i++) {
        const int lit = hist_run_literal(ring.data(), pasti, P, i), inc = hist_run(M.data(), P, i);
        EXPECT(lit == inc, "%s: P %d step %d lag %d: literal %d, incremental %d", what, P, t, i, lit, inc);
        EXPECT(M[(size_t)i] >= 0 && M[(size_t)i] <= P, "%s: M out of [0, P]", what);
    }
    g_steps++;
}

// One model: phases of random, period-3 and constant symbols, more than 3 P steps each; the rows
// both ways; then the state is set (M rebuilt) in mid-sequence and the walk goes on.
void check_model(Rng &r, int64_t V, int P) {
    std::vector<uint64_t> L((size_t)P * (size_t)P);
    for (auto &w : L) w = r.below(4) == 0 ? 0 : r.below(r.below(2) ? 50 : kHistMaxWeight);
    std::vector<int32_t> ring((size_t)P, -1), M((size_t)P);
    int32_t pasti = 0;
    hist_m_init(M.data(), P);
    std::vector<uint64_t> row_a((size_t)V), row_b((size_t)V);
    const int per = 3 * P + 4;
    int t = 0;
    auto step = [&](int32_t s, const char *what) {
        same_runs(ring, pasti, P, M, what, t);
        if (P <= 5 || t % 7 == 0) {                            // (the rows follow from the runs: a sample of them)
            uint64_t Ta, Tb;
            const bool oa = hist_row(ring.data(), pasti, P, M.data(), L.data(), V, 64, row_a.data(), &Ta);
            const bool ob = hist_row(ring.data(), pasti, P, nullptr, L.data(), V, 64, row_b.data(), &Tb);
            EXPECT(oa && ob && Ta == Tb && row_a == row_b, "%s: rows at step %d", what, t);
            EXPECT(row_a[0] == 1, "symbol 0 gains no weight");
            uint64_t Tc;
            const bool oc = hist_row(ring.data(), pasti, P, M.data(), L.data(), V, 32, row_b.data(), &Tc);
            bool fits = true;
            for (uint64_t x : row_a) fits = fits && !(x >> 32);
            EXPECT(oc == fits && Tc == (fits ? Ta : 0), "%s: u32 status at step %d", what, t);
        }
        hist_accept(ring.data(), &pasti, P, M.data(), s);
        EXPECT(pasti >= 0 && pasti < P, "pasti");
        t++;
    };
    for (int k = 0; k < per; k++) step((int32_t)r.below((uint64_t)V), "random");
    for (int k = 0; k < per; k++) step((int32_t)((k % 3) % V), "period 3");
    for (int k = 0; k < per; k++) step((int32_t)(V - 1), "constant");
    for (int k = 0; k < per; k++) step(0, "symbol 0");
    // the state is set: M rebuilt from ring and pasti alone continues the same walk ...
    std::vector<int32_t> M2((size_t)P);
    hist_m_rebuild(ring.data(), pasti, P, M2.data());
    M = M2;
    for (int k = 0; k < per; k++) step(k % 5 == 4 ? (int32_t)r.below((uint64_t)V) : (int32_t)(V - 1), "after a rebuild");
    // ... and so does M of a ring no walk produced (any entries in [-1, V), any pasti)
    for (auto &x : ring) x = (int32_t)r.below((uint64_t)V + 1) - 1;
    pasti = (int32_t)r.below((uint64_t)P);
    EXPECT(hist_state_ok(ring.data(), pasti, V, P), "a state in range");
    hist_m_rebuild(ring.data(), pasti, P, M.data());
    for (int k = 0; k < per; k++) step((int32_t)((k % 2) * (V - 1)), "after a set state");
    // the initial M is the rebuilt M of the initial ring, as far as the runs go
    std::vector<int32_t> fresh((size_t)P, -1), Mi((size_t)P), Mr((size_t)P);
    hist_m_init(Mi.data(), P);
    hist_m_rebuild(fresh.data(), 0, P, Mr.data());
    for (int i = 0; i < P; i++) EXPECT(hist_run(Mi.data(), P, i) == hist_run(Mr.data(), P, i) && Mr[(size_t)i] == P - i - 1, "initial M");
}

}  // namespace

extern "C" {

int hc_limits_ok(int64_t V, int64_t P) { return hist_limits_ok(V, P) ? 1 : 0; }
int hc_weights_ok(const uint64_t *L, int P) { return hist_weights_ok(L, P) ? 1 : 0; }
int hc_state_ok(const int32_t *ring, int32_t pasti, int64_t V, int P) { return hist_state_ok(ring, pasti, V, P) ? 1 : 0; }

// One stream's walk by the incremental rule (M rebuilt from the state handed in): ring [P] and
// *pasti in and out, rows_out [n][V], ok_out [n] the row's status, acc_out [n] whether the step
// was accepted (a bad row or symbol ends the walk).
void hc_walk(int64_t V, int P, const uint64_t *L, int pmf_bits, const int32_t *syms, int64_t n, int32_t *ring,
             int32_t *pasti, uint64_t *rows_out, int32_t *ok_out, int32_t *acc_out) {
    std::vector<int32_t> M((size_t)P);
    hist_m_rebuild(ring, *pasti, P, M.data());
    bool dead = false;
    for (int64_t t = 0; t < n; t++) {
        uint64_t T;
        ok_out[t] = hist_row(ring, *pasti, P, M.data(), L, V, pmf_bits, rows_out + t * V, &T) ? 1 : 0;
        const bool go = !dead && ok_out[t] && syms[t] >= 0 && syms[t] < V;
        acc_out[t] = go ? 1 : 0;
        if (go) hist_accept(ring, pasti, P, M.data(), syms[t]);
        else dead = true;
    }
}

// -> failures; *steps_out the steps at which every lag was compared
int hc_sweep(uint64_t seed, int64_t *steps_out) {
    Rng r{seed ? seed : 1};
    g_fail = 0;
    g_steps = 0;
    static const int Ps[] = {1, 2, 3, 5, 64, 256};
    static const int64_t Vs[] = {2, 3, 256};
    for (int P : Ps)
        for (int64_t V : Vs) check_model(r, V, P);
    if (steps_out) *steps_out = g_steps;
    return g_fail;
}

}  // extern "C"

#ifdef HISTORY_CHECK_MAIN
int main() {
    int64_t steps = 0;
    const int bad = hc_sweep(4242, &steps);
    if (bad) {
        fprintf(stderr, "history_check: %d failures\n", bad);
        return 1;
    }
    printf("history_check: ok (%lld steps)\n", (long long)steps);
    return 0;
}
#endif
