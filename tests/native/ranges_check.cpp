// ranges_check.cpp -- host checks of lac_amd/csrc/lac_ranges.h, the plain host/device rules of
// range-level coding: triple validation and its precedence, the launch geometry, the mapping, and
// the whole encode and decode step one lane of the kernels runs.  tests/test_ranges_host.py builds
// it as a shared library (the yardsticks there are Python integers and the C oracle on three-entry
// rows) and, with -DRANGES_CHECK_MAIN, as a stand-alone program under AddressSanitizer +
// UndefinedBehaviorSanitizer whose sweep holds the rules to 128-bit integer division and to
// plane_append, every buffer a heap block of exactly the size the step may touch.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "lac_ranges.h"

using namespace lac;

namespace {

// bits [pos, pos + k) of a big-endian byte stream of nbits bits, zeros past the end
uint64_t host_bits(const uint8_t *bytes, uint64_t nbits, uint64_t pos, int k) {
    uint64_t v = 0;
    for (int i = 0; i < k; i++) {
        const uint64_t p = pos + (uint64_t)i;
        const uint64_t bit = p < nbits ? (bytes[p >> 3] >> (7 - (p & 7))) & 1 : 0;
        v = (v << 1) | bit;
    }
    return v;
}

}  // namespace

extern "C" {

int rc_check(uint64_t lo, uint64_t hi, uint64_t T, int prec) { return range_check(lo, hi, T, prec); }
unsigned rc_blocks(int64_t B) { return range_blocks(B); }
int rc_threads() { return kRangeThreads; }
void rc_table(uint64_t lo, uint64_t hi, uint64_t T, uint64_t *row) { range_table(lo, hi, T, row); }
void rc_map(uint64_t lo, uint64_t hi, uint64_t T, uint64_t w, uint64_t *a, uint64_t *b) {
    range_map(lo, hi, T, recip(T), w, a, b);
}
uint64_t rc_target(uint64_t v, uint64_t T, uint64_t w) { return range_target(v, T, w, recip(w)); }

// One stream from the fresh state: n steps of range_encode_step, then store_state's last word.
// ek[2 t] = E, ek[2 t + 1] = k (k = -1 as 2^64 - 1 where the step did not narrow); planes: [2][cap_words];
// regs = {l, h, L, nsym}.  Returns the sticky status, *err_step the failing step's nsym.
int rc_encode(int64_t n, const uint64_t *lo, const uint64_t *hi, const uint64_t *T, int prec, uint64_t cap_words,
              uint64_t *ek, uint64_t *planes, int64_t *regs, int64_t *err_step) {
    EncState st;
    memset(&st, 0, sizeof(st));
    st.nflush = -1;
    int64_t l = 0, h = ((int64_t)1 << prec) - 1;
    uint64_t *pa = planes, *pc = planes + cap_words;
    auto store = [&](uint64_t idx, uint64_t wa, uint64_t wc) {
        pa[idx] = wa;
        pc[idx] = wc;
    };
    int rc = LAC_OK;
    *err_step = -1;
    for (int64_t t = 0; t < n && !rc; t++) {
        int k;
        uint64_t E;
        rc = range_encode_step(st, l, h, lo[t], hi[t], T[t], recip(T[t] ? T[t] : 1), prec, cap_words, store, &k, &E);
        ek[2 * t] = E;
        ek[2 * t + 1] = (uint64_t)(int64_t)k;
        if (rc) *err_step = st.nsym;
    }
    if (st.L > 0 && ((st.L - 1) >> 6) < cap_words) {
        pa[(st.L - 1) >> 6] = st.wa;
        pc[(st.L - 1) >> 6] = st.wc;
    }
    regs[0] = l;
    regs[1] = h;
    regs[2] = (int64_t)st.L;
    regs[3] = st.nsym;
    return rc;
}

int rc_flush(int64_t l, int64_t h, int prec, int8_t *digits) { return flush_digits(l, h, prec, digits); }

// One stream's decode from the opened state: per step the peek under T[t] (targets[t]), then the
// advance by triple t.  regs = {l, h, x, pos, nsym, det, ndet}.  Returns the sticky status.
int rc_decode(int64_t n, const uint64_t *lo, const uint64_t *hi, const uint64_t *T, int prec, const uint8_t *bytes,
              uint64_t nbits, int stop, uint64_t *targets, int64_t *regs) {
    DecState st;
    memset(&st, 0, sizeof(st));
    st.h = ((int64_t)1 << prec) - 1;
    st.pos = (uint64_t)prec;
    st.det = 1;
    st.err_step = -1;
    st.x = (int64_t)host_bits(bytes, nbits, 0, prec);
    int rc = LAC_OK;
    for (int64_t t = 0; t < n && !rc; t++) {
        targets[t] = range_peek(st, T[t], prec);
        const uint64_t pos = st.pos;
        rc = range_decode_step(st, lo[t], hi[t], T[t], recip(T[t] ? T[t] : 1), prec, pos > nbits ? pos - nbits : 0,
                               stop != 0, [&](int k) { return host_bits(bytes, nbits, pos, k); });
    }
    regs[0] = st.l;
    regs[1] = st.h;
    regs[2] = st.x;
    regs[3] = (int64_t)st.pos;
    regs[4] = st.nsym;
    regs[5] = st.det;
    regs[6] = st.ndet;
    return rc;
}

// The sweep: random valid triples (totals to 2^60, widths to 2^61) against 128-bit division;
// range_append against plane_append word for word over random digit runs, capacity failures
// included.  Returns the number of failures; *count the checks made.
int rc_sweep(uint64_t seed, int64_t *count) {
    struct Rng {
        uint64_t s;
        uint64_t next() {
            s ^= s << 13;
            s ^= s >> 7;
            s ^= s << 17;
            return s;
        }
    } r{seed ? seed : 1};
    int bad = 0;
    int64_t n = 0;
    for (int i = 0; i < 1000; i++) {
        const int prec = 2 + (int)(r.next() % 60);                          // 2 .. 61
        const uint64_t half = 1ull << (prec - 1);
        const uint64_t T = (i % 7 == 0) ? half : 1 + r.next() % half;
        const uint64_t hi = (i % 5 == 0) ? T : 1 + r.next() % T;
        const uint64_t lo = (i % 3 == 0) ? 0 : r.next() % hi;
        const uint64_t w = (i % 11 == 0) ? 2 * half : half + 1 + r.next() % half;   // (2^(prec-1), 2^prec]
        if (range_check(lo, hi, T, prec) != LAC_OK) bad++;
        uint64_t a, b;
        range_map(lo, hi, T, recip(T), w, &a, &b);
        const u128 na = (u128)lo * w + (T - 1), nb = (u128)hi * w + (T - 1);
        if (a != (uint64_t)(na / T) || b != (uint64_t)(nb / T) || a >= b || b > w) bad++;
        // every value of [a, b) maps back into [lo, hi): the ends
        if (range_target(a, T, w, recip(w)) < lo || range_target(b - 1, T, w, recip(w)) >= hi) bad++;
        if (a > 0 && range_target(a - 1, T, w, recip(w)) >= lo) bad++;
        if (b < w && range_target(b, T, w, recip(w)) < hi) bad++;
        n++;
    }
    for (int run = 0; run < 200; run++) {
        const uint64_t cap_words = 1 + r.next() % 40;
        std::vector<uint64_t> p1(2 * cap_words, 0), p2(2 * cap_words, 0);   // exactly the planes
        uint64_t L1 = 0, wa1 = 0, wc1 = 0, L2 = 0, wa2 = 0, wc2 = 0;
        auto s1 = [&](uint64_t idx, uint64_t wa, uint64_t wc) { p1[idx] = wa; p1[cap_words + idx] = wc; };
        auto s2 = [&](uint64_t idx, uint64_t wa, uint64_t wc) { p2[idx] = wa; p2[cap_words + idx] = wc; };
        for (int t = 0; t < 80; t++) {
            const int k = (int)(r.next() % 62);                             // 0 .. 61
            uint64_t E = k ? r.next() & ((1ull << k) - 1) : 0;
            if (k && L1 > 0 && r.next() % 4 == 0) E |= 1ull << k;          // a carry onto bit L-1
            const bool ok1 = plane_append(L1, wa1, wc1, k, E, cap_words, s1);
            const bool ok2 = range_append(L2, wa2, wc2, k, E, cap_words, s2);
            n++;
            if (ok1 != ok2 || L1 != L2 || wa1 != wa2 || wc1 != wc2 || p1 != p2) bad++;
            if (!ok1) break;
        }
    }
    *count = n;
    return bad;
}

}  // extern "C"

#ifdef RANGES_CHECK_MAIN
int main() {
    int64_t n = 0;
    int bad = rc_sweep(12345, &n);
    // whole steps, round trip: jobs of 1 .. 286 symbols coded, finished by hand (the digits as one number), decoded
    for (int job = 0; job < 20 && !bad; job++) {
        const int prec = job % 2 ? 61 : 16 + job;
        const int64_t steps = 1 + 15 * job;
        const uint64_t half = 1ull << (prec - 1);
        std::vector<uint64_t> lo((size_t)steps), hi((size_t)steps), T((size_t)steps), ek(2 * (size_t)steps), tg((size_t)steps);
        uint64_t s = 99 + (uint64_t)job;
        auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
        for (int64_t t = 0; t < steps; t++) {
            T[(size_t)t] = t % 9 == 0 ? half : 1 + next() % half;
            hi[(size_t)t] = 1 + next() % T[(size_t)t];
            lo[(size_t)t] = next() % hi[(size_t)t];
        }
        const uint64_t cap_words = ((uint64_t)steps * (uint64_t)(prec + 2) + 64 + 63) / 64;
        std::vector<uint64_t> planes(2 * cap_words, 0);
        int64_t regs[7], es = 0;
        if (rc_encode(steps, lo.data(), hi.data(), T.data(), prec, cap_words, ek.data(), planes.data(), regs, &es)) bad++;
        // the digits as one big number, carries resolved from the end: one digit per byte
        std::vector<int> dg;
        for (int64_t t = 0; t < steps; t++) {
            const int k = (int)(int64_t)ek[2 * (size_t)t + 1];
            const uint64_t E = ek[2 * (size_t)t];
            for (int i = 0; i < k; i++) dg.push_back(i == 0 ? (int)(E >> (k - 1)) : (int)((E >> (k - 1 - i)) & 1));
        }
        int8_t fd[8];
        const int m = rc_flush(regs[0], regs[1], prec, fd);
        for (int i = 0; i < m; i++) dg.push_back(fd[i]);
        int carry = 0;
        for (size_t i = dg.size(); i-- > 0;) {
            const int d = dg[i] + carry;
            dg[i] = ((d % 2) + 2) % 2;
            carry = (d - dg[i]) / 2;
        }
        if (carry) bad++;
        std::vector<uint8_t> bytes((dg.size() + 7) / 8 + 1, 0);
        for (size_t i = 0; i < dg.size(); i++) bytes[i >> 3] |= (uint8_t)(dg[i] << (7 - (i & 7)));
        if (rc_decode(steps, lo.data(), hi.data(), T.data(), prec, bytes.data(), dg.size(), 0, tg.data(), regs)) bad++;
        for (int64_t t = 0; t < steps; t++)
            if (tg[(size_t)t] < lo[(size_t)t] || tg[(size_t)t] >= hi[(size_t)t]) bad++;
        if (regs[4] != steps) bad++;
        n += steps;
    }
    if (bad) {
        fprintf(stderr, "ranges_check: %d failures in %lld checks\n", bad, (long long)n);
        return 1;
    }
    printf("ranges_check: ok (%lld checks)\n", (long long)n);
    return 0;
}
#endif
