// drain_check.cpp -- test infrastructure: the drain rules of lac_amd/csrc/lac_drain.h on the host.
// Built two ways by tests/test_drain_host.py: as a shared library whose dc_* functions the test
// drives from reference traces (oracle/restate.py), and with -DDRAIN_CHECK_MAIN as a stand-alone
// program under AddressSanitizer + UndefinedBehaviorSanitizer that codes seeded random streams
// with and without drains and compares them.  Planes, slots and outputs live in heap blocks of
// exactly the declared size, so a word or byte out of bounds is a sanitizer report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "lac_core.h"
#include "lac_drain.h"
#include "lac.h"

using namespace lac;

namespace {

// finish_stream's flush + backward add (lac_dev.h, LAC_TERM_FLUSH) over host planes: the packed
// big-endian bytes into out (8 * cap_words bytes) -> bit count, or a negative status.
int64_t finish_host(int64_t l, int64_t h, int prec, uint64_t L, uint64_t wa, uint64_t wc, uint64_t *pa, uint64_t *pc,
                    uint64_t cap_words, uint8_t *out, int8_t *fd, int *nfd) {
    if (L > 0) {
        if (((L - 1) >> 6) >= cap_words) return LAC_E_CAPACITY;
        pa[(L - 1) >> 6] = wa;
        pc[(L - 1) >> 6] = wc;
    }
    const int m = flush_digits(l, h, prec, fd);
    if (m < 0) return LAC_E_CAPACITY;
    *nfd = m;
    int64_t F = 0;
    for (int i = 0; i < m; i++) F = F * 2 + fd[i];
    const uint64_t Lf = L + (uint64_t)m, nwords = (Lf + 63) >> 6;
    if (nwords > cap_words) return LAC_E_CAPACITY;
    const int pad = (int)(nwords * 64 - Lf);
    i128 carry = (i128)F * ((i128)1 << pad);
    const int64_t last = L ? (int64_t)((L - 1) >> 6) : -1;
    for (int64_t i = (int64_t)nwords - 1; i >= 0; i--) {
        const uint64_t a = i <= last ? pa[i] : 0, c = i <= last ? pc[i] : 0;
        const i128 sm = (i128)(u128)a + (i128)(u128)c + carry;
        const uint64_t w = bswap64((uint64_t)sm);
        memcpy(out + 8 * i, &w, 8);
        carry = sm >> 64;
    }
    if (carry != 0) return LAC_E_ARG;
    return (int64_t)Lf;
}

struct Stream {
    int prec;
    uint64_t cap_words;
    int64_t l, h;
    uint64_t L = 0, wa = 0, wc = 0;
    uint64_t *pa, *pc;
    Stream(int prec_, uint64_t cap) : prec(prec_), cap_words(cap), l(0), h(((int64_t)1 << prec_) - 1) {
        pa = (uint64_t *)calloc(cap, 8);
        pc = (uint64_t *)calloc(cap, 8);
    }
    ~Stream() { free(pa); free(pc); }
    bool append(int k, uint64_t E, int64_t l2, int64_t h2) {
        auto store = [&](uint64_t idx, uint64_t a, uint64_t c) { pa[idx] = a; pc[idx] = c; };
        if (!plane_append(L, wa, wc, k, E, cap_words, store)) return false;
        l = l2;
        h = h2;
        if (L > 0) { pa[(L - 1) >> 6] = wa; pc[(L - 1) >> 6] = wc; }      // store_state's mirror
        return true;
    }
};

}  // namespace

extern "C" {

int dc_is_guard(uint64_t a, uint64_t c) { return drain::is_guard(a, c); }
int dc_is_certain(int64_t l, int64_t h, int prec) { return drain::is_certain(l, h, prec); }
int dc_slot_fits(uint64_t g, uint64_t fill, uint64_t stride) { return drain::slot_fits(g, fill, stride); }
uint64_t dc_block_carries(uint64_t gen, uint64_t prop, uint64_t cin, uint64_t *cout) {
    return drain::block_carries(gen, prop, cin, cout);
}
int dc_flush_digits(int64_t l, int64_t h, int prec, int8_t *out8) { return flush_digits(l, h, prec, out8); }

// One stream from a trace: symbol i appends the k[i] digits of value E[i] and leaves the registers
// l[i], h[i]; a drain follows it when dr[i] != 0, into a fresh slot of stage_bytes.  out receives
// the drained bytes, then the finished tail.  stats: [0] most words kept by a drain, [1] drains
// that moved words, [2] the smallest flush digit + 8, [3] the most words resident before a drain.
int dc_run(int prec, int64_t n, const uint64_t *E, const int32_t *k, const int64_t *l, const int64_t *h,
           const uint8_t *dr, uint64_t cap_words, uint64_t stage_bytes, uint8_t *out, uint64_t out_cap,
           uint64_t *out_bytes, uint64_t *nbits, uint64_t *stats) {
    Stream s(prec, cap_words);
    uint64_t pos = 0;
    stats[0] = stats[1] = stats[3] = 0;
    stats[2] = 8;
    uint8_t *slot = (uint8_t *)malloc(stage_bytes ? stage_bytes : 1);
    for (int64_t i = 0; i < n; i++) {
        if (!s.append(k[i], E[i], l[i], h[i])) { free(slot); return LAC_E_CAPACITY; }
        if (!dr[i]) continue;
        const uint64_t before = s.L ? ((s.L - 1) >> 6) + 1 : 0;
        stats[3] = before > stats[3] ? before : stats[3];
        uint64_t fill = 0;
        const uint64_t g = drain::drain_stream_host(s.l, s.h, prec, 0, -1, s.L, s.wa, s.wc, s.pa, s.pc, slot,
                                                    stage_bytes, fill);
        if (fill != 8 * g || pos + fill > out_cap) { free(slot); return LAC_E_ARG; }
        memcpy(out + pos, slot, fill);
        pos += fill;
        if (g) {
            stats[1]++;
            const uint64_t kept = ((s.L - 1) >> 6) + 1;
            stats[0] = kept > stats[0] ? kept : stats[0];
        }
    }
    free(slot);
    uint8_t *tail = (uint8_t *)malloc(8 * cap_words);
    int8_t fd[8];
    int nfd = 0;
    const int64_t Lf = finish_host(s.l, s.h, prec, s.L, s.wa, s.wc, s.pa, s.pc, cap_words, tail, fd, &nfd);
    if (Lf < 0) { free(tail); return (int)Lf; }
    for (int i = 0; i < nfd; i++) stats[2] = (uint64_t)(fd[i] + 8) < stats[2] ? (uint64_t)(fd[i] + 8) : stats[2];
    const uint64_t nb = ((uint64_t)Lf + 7) >> 3;
    if (pos + nb > out_cap) { free(tail); return LAC_E_ARG; }
    memcpy(out + pos, tail, nb);
    free(tail);
    *out_bytes = pos + nb;
    *nbits = 8 * pos + (uint64_t)Lf;
    return LAC_OK;
}

// drain_stream_host on planes given by the caller (crafted cases): lw = {L, wa, wc} in/out, the
// planes [cap_words] in/out, slot [stride_bytes] and *fill in/out -> g.
uint64_t dc_drain(int64_t l, int64_t h, int prec, int32_t err, int32_t nflush, uint64_t *lw, uint64_t *pa,
                  uint64_t *pc, uint8_t *slot, uint64_t stride_bytes, uint64_t *fill) {
    return drain::drain_stream_host(l, h, prec, err, nflush, lw[0], lw[1], lw[2], pa, pc, slot, stride_bytes, *fill);
}

// The finish of given planes (copied first): out [8 * cap_words] -> bit count or a negative status.
int64_t dc_finish(int64_t l, int64_t h, int prec, const uint64_t *lw, const uint64_t *pa, const uint64_t *pc,
                  uint64_t cap_words, uint8_t *out, int8_t *fd8, int32_t *nfd) {
    std::vector<uint64_t> a(pa, pa + cap_words), c(pc, pc + cap_words);
    int m = 0;
    const int64_t r = finish_host(l, h, prec, lw[0], lw[1], lw[2], a.data(), c.data(), cap_words, out, fd8, &m);
    *nfd = m;
    return r;
}

}  // extern "C"

#ifdef DRAIN_CHECK_MAIN
// Seeded random streams coded twice -- once into planes that hold the whole stream, once into a
// few words with drains at random points -- through the same renorm() / plane_append as the
// kernels: the drained bytes followed by the finished tail must be the undrained bytes.
static uint64_t sd = 0x2545F4914F6CDD1Dull;
static uint64_t rnd() {
    uint64_t z = (sd += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }
static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); if (++fails > 20) exit(1); } } while (0)

int main() {
    // block_carries against a ripple over 64 positions
    for (int it = 0; it < 200000; it++) {
        uint64_t gen = rnd() & rnd(), prop = rnd() & ~gen;
        if (below(4) == 0) prop = ~gen;
        if (below(8) == 0) { gen = 0; prop = ~0ull; }
        const uint64_t cin = below(2);
        uint64_t want = 0, c = cin;
        for (int j = 0; j < 64; j++) {
            want |= c << j;
            c = ((gen >> j) & 1) | (((prop >> j) & 1) & c);
        }
        uint64_t cout = 7;
        CHECK(drain::block_carries(gen, prop, cin, &cout) == want && cout == c, "block_carries");
    }
    // crafted planes (random streams rarely hold them): runs of all-ones and zero words between a
    // random prefix and an active word with a pending carry, open and certain registers -- the drain
    // stops at the last word that is neither, and the finish is the undrained one
    for (int it = 0; it < 20000; it++) {
        const int prec = 48;
        const uint64_t nw = 2 + below(70), cap = nw + 2;        // words below the active one
        const int off = 1 + (int)below(64);
        const uint64_t L = nw * 64 + (uint64_t)off;
        std::vector<uint64_t> a(cap, 0), c(cap, 0);
        uint64_t want_g = 0;
        a[0] = 1 + below(1000);                                   // word 0 never overflows
        for (uint64_t i = 1; i < nw; i++) {
            const int kind = (int)below(4);
            a[i] = kind == 0 ? ~0ull : kind == 1 ? 0 : kind == 2 ? ~0ull - 7 : rnd();
            c[i] = kind == 2 ? 7 : 0;                            // (kind 2: all-ones only as a sum)
        }
        for (uint64_t i = 0; i < nw; i++) if (drain::is_guard(a[i], c[i])) want_g = i;
        const uint64_t top = off == 64 ? ~0ull : ~0ull << (64 - off);
        const uint64_t wa = below(2) ? top : rnd() & top, wc = below(2) ? 1ull << (64 - off) : 0;
        const bool cert = below(3) == 0;
        const int64_t D = (int64_t)1 << prec;
        const int64_t l = cert ? (int64_t)below(100) : D - 10, h = cert ? l + D / 2 + (int64_t)below((uint64_t)(D / 2 - 200)) : l + D / 2 + 5;
        a[nw] = wa; c[nw] = wc;
        uint64_t lw[3] = {L, wa, wc};
        std::vector<uint8_t> ref(8 * cap), tail(8 * cap), slot(8 * cap);
        int8_t fd[8];
        int32_t nfd;
        const int64_t Lr = dc_finish(l, h, prec, lw, a.data(), c.data(), cap, ref.data(), fd, &nfd);
        uint64_t fill = 0;
        const uint64_t g = dc_drain(l, h, prec, 0, -1, lw, a.data(), c.data(), slot.data(), 8 * cap, &fill);
        const int64_t Lt = dc_finish(l, h, prec, lw, a.data(), c.data(), cap, tail.data(), fd, &nfd);
        CHECK(Lr >= 0 && Lt >= 0 && g == (cert ? nw : want_g) && fill == 8 * g && (uint64_t)Lt + 64 * g == (uint64_t)Lr,
              "crafted: g %llu want %llu", (unsigned long long)g, (unsigned long long)(cert ? nw : want_g));
        CHECK(memcmp(ref.data(), slot.data(), (size_t)fill) == 0 &&
                  memcmp(ref.data() + fill, tail.data(), (size_t)(((uint64_t)(Lt > 0 ? Lt : 0) + 7) / 8)) == 0,
              "crafted: bytes differ (nw %llu off %d cert %d)", (unsigned long long)nw, off, (int)cert);
    }
    uint64_t neg_flush = 0, drains = 0, max_kept = 0;
    for (int it = 0; it < 4000; it++) {
        const int prec = 16 + (int)below(46);
        const int mode = (int)below(4);                      // 0 random, 1 peaky, 2 / 3 nearly constant low / high
        const int64_t n = 1 + (int64_t)below(mode >= 2 ? 1500 : 300);
        const int every = (int)(below(3) == 0 ? 1 : 1 + below(70));
        std::vector<uint64_t> E((size_t)n);
        std::vector<int32_t> k((size_t)n);
        std::vector<int64_t> l((size_t)n), h((size_t)n);
        std::vector<uint8_t> dr((size_t)n);
        int64_t cl = 0, ch = ((int64_t)1 << prec) - 1;
        for (int64_t i = 0; i < n; i++) {
            const uint64_t w = (uint64_t)(ch - cl + 1), T = 2 + below(((uint64_t)1 << (prec - 1)) - 1);
            uint64_t lo, hi;
            if (mode == 0) { lo = below(T); hi = lo + 1 + below(T - lo); }
            else if (mode == 1) { lo = below(8) ? 0 : below(T); hi = below(8) ? T - below(T - lo) / 64 : lo + 1 + below(T - lo); }
            else { const bool common = below(33) != 0; const bool low = (mode == 2) == common; lo = low ? 0 : T / 2; hi = low ? T / 2 : T; }
            if (hi <= lo) hi = lo + 1;
            const uint64_t a = (uint64_t)(((u128)lo * w + T - 1) / T), b = (uint64_t)(((u128)hi * w + T - 1) / T);
            if (a >= b) { i--; continue; }
            ch = cl + (int64_t)b - 1;
            cl = cl + (int64_t)a;
            int kk;
            uint64_t Ev;
            renorm(cl, ch, prec, &kk, &Ev);
            E[(size_t)i] = Ev; k[(size_t)i] = kk; l[(size_t)i] = cl; h[(size_t)i] = ch;
            dr[(size_t)i] = (uint8_t)((i + 1) % every == 0 || below((uint64_t)every) == 0);   // gaps <= every
        }
        const uint64_t big = (uint64_t)(n * (prec + 2) + 256) / 64 + 2;
        std::vector<uint8_t> none((size_t)n, 0);
        uint8_t *ref = (uint8_t *)malloc(8 * big), *got = (uint8_t *)malloc(8 * big);
        uint64_t nr = 0, br = 0, ng = 0, bg = 0, st0[4], st1[4];
        const int r0 = dc_run(prec, n, E.data(), k.data(), l.data(), h.data(), none.data(), big, 8, ref, 8 * big, &nr, &br, st0);
        // small planes: what `every` symbols can add, plus the words a drain keeps
        const uint64_t small = (uint64_t)(every * (prec + 2) + 256) / 64 + 40;
        const int r1 = dc_run(prec, n, E.data(), k.data(), l.data(), h.data(), dr.data(), small < big ? small : big,
                              8 * big, got, 8 * big, &ng, &bg, st1);
        CHECK(r0 == LAC_OK, "undrained run fails: %d", r0);
        CHECK(r1 == LAC_OK, "drained run fails: %d (prec %d mode %d n %lld every %d)", r1, prec, mode, (long long)n, every);
        if (r0 == LAC_OK && r1 == LAC_OK)
            CHECK(nr == ng && br == bg && memcmp(ref, got, (size_t)nr) == 0, "bytes differ (prec %d mode %d n %lld every %d)",
                  prec, mode, (long long)n, every);
        neg_flush += st0[2] < 8;
        drains += st1[1];
        max_kept = st1[0] > max_kept ? st1[0] : max_kept;
        free(ref);
        free(got);
    }
    CHECK(drains > 1000, "too few drains moved anything: %llu", (unsigned long long)drains);
    CHECK(neg_flush > 0, "no stream with a negative flush digit");
    printf("drain_check: %s (%llu drains, %llu streams with a -1 flush digit, <= %llu words kept)\n",
           fails ? "FAILED" : "ok", (unsigned long long)drains, (unsigned long long)neg_flush, (unsigned long long)max_kept);
    return fails ? 1 : 0;
}
#endif
