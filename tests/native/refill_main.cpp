// refill_main.cpp -- test infrastructure: a reader model over lac_amd/csrc/lac_refill.h as a
// stand-alone program, built by tests/test_refill_host.py under AddressSanitizer +
// UndefinedBehaviorSanitizer (host code only).  A reader pulls k <= prec bits per step from a
// window that refill_stream_host slides every N steps; every value must be the one the whole
// string gives at pos + 64 * base.  The source lives in a heap block of exactly nw words and the
// window in one of exactly W words, so a word out of bounds is a sanitizer report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lac_refill.h"

using namespace lac;

static uint64_t sd = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    uint64_t z = (sd += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }
static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); if (++fails > 20) exit(1); } } while (0)

// Bits [pos, pos + k) of `words` big-endian words read one by one, zeros at or past nbits; no
// byte at or past ceil(nbits / 8) is touched.
static uint64_t read_bits(const uint64_t *words, uint64_t nbits, uint64_t pos, int k) {
    const uint8_t *p = reinterpret_cast<const uint8_t *>(words);
    uint64_t v = 0;
    for (int i = 0; i < k; i++) {
        const uint64_t q = pos + (uint64_t)i;
        v = v << 1 | (q < nbits ? (uint64_t)((p[q >> 3] >> (7 - (q & 7))) & 1) : 0);
    }
    return v;
}

static uint64_t bound_words(int N, int prec) { return ((uint64_t)(N + 1) * (uint64_t)prec + 63 + 63) / 64; }

int main() {
    static const int precs[] = {16, 24, 36, 48, 61}, everys[] = {1, 7, 64};
    uint64_t moved = 0, steps = 0, dry = 0;
    for (int it = 0; it < 3000; it++) {
        const int prec = precs[below(5)], N = everys[below(3)];
        const uint64_t nw = below(41), W = bound_words(N, prec) + below(3);
        const uint64_t nbits = nw ? 64 * (nw - 1) + 1 + below(64) : 0;
        uint64_t *src = (uint64_t *)malloc(nw ? 8 * nw : 1), *win = (uint64_t *)malloc(8 * W);
        for (uint64_t i = 0; i < nw; i++) src[i] = rnd();
        uint64_t base = 0, held = 0, pos = (uint64_t)prec;
        CHECK(refill::open_stream_host(src, 8 * nw, nbits, 0, W, win, &held), "open refused");
        CHECK(read_bits(win, held, 0, prec) == read_bits(src, nbits, 0, prec), "x differs at the open");
        const int total = (int)(nbits / (uint64_t)(prec / 2 + 1)) + 3 * N + 8;
        for (int t = 0; t < total; t++) {
            const int k = below(4) == 0 ? prec : (int)below((uint64_t)prec + 1);
            const uint64_t got = read_bits(win, held, pos, k), want = read_bits(src, nbits, pos + 64 * base, k);
            CHECK(got == want, "read differs: prec %d N %d nw %llu step %d", prec, N, (unsigned long long)nw, t);
            pos += (uint64_t)k;
            steps++;
            if ((t + 1) % N == 0) {
                const uint64_t abs0 = pos + 64 * base;
                const int r = refill::refill_stream_host(src, 8 * nw, nbits, prec, 0, W, win, base, held, pos);
                CHECK(r != refill::REFILL_DRY, "dry with W from the bound: prec %d N %d", prec, N);
                CHECK(pos + 64 * base == abs0 && pos >= (uint64_t)prec, "position moved");
                CHECK(r != refill::REFILL_MOVED || pos <= (uint64_t)prec + 63, "pos past prec + 63 after a refill");
                moved += r == refill::REFILL_MOVED;
            }
        }
        free(src);
        free(win);
    }
    // one word below the bound, k = prec every step from the worst position prec + 63: dry at the
    // refill, nothing changed; at the bound the same steps are safe
    for (int pi = 0; pi < 5; pi++)
        for (int ni = 0; ni < 3; ni++)
            for (int shrink = 0; shrink < 2; shrink++) {
                const int prec = precs[pi], N = everys[ni];
                const uint64_t W = bound_words(N, prec) - (uint64_t)shrink, nw = W + 80, nbits = 64 * nw - 5;
                uint64_t *src = (uint64_t *)malloc(8 * nw), *win = (uint64_t *)malloc(8 * W), *keep = (uint64_t *)malloc(8 * W);
                for (uint64_t i = 0; i < nw; i++) src[i] = rnd();
                uint64_t base = 0, held = 0, pos = (uint64_t)prec;
                CHECK(refill::open_stream_host(src, 8 * nw, nbits, 0, W, win, &held), "open refused");
                // a refill that checks: dry changes nothing, anything else keeps the absolute position
                auto step_refill = [&]() {
                    memcpy(keep, win, 8 * W);
                    const uint64_t b0 = base, h0 = held, p0 = pos;
                    const int r = refill::refill_stream_host(src, 8 * nw, nbits, prec, 0, W, win, base, held, pos);
                    if (r == refill::REFILL_DRY)
                        CHECK(base == b0 && held == h0 && pos == p0 && memcmp(keep, win, 8 * W) == 0, "a dry refill changed something");
                    else
                        CHECK(pos + 64 * base == p0 + 64 * b0, "position moved");
                    return r;
                };
                int r = refill::REFILL_IDLE;
                for (int rem = 63; rem > 0 && r != refill::REFILL_DRY;) {   // lead-in: (pos - prec) mod 64 = 63
                    const int k = rem < prec ? rem : prec;
                    pos += (uint64_t)k;
                    rem -= k;
                    r = step_refill();
                }
                if (r != refill::REFILL_DRY) {
                    CHECK(pos == (uint64_t)prec + 63, "lead-in position");
                    for (int t = 0; t < N; t++) pos += (uint64_t)prec;
                    r = step_refill();
                }
                if (shrink) {
                    CHECK(r == refill::REFILL_DRY, "not dry below the bound: prec %d N %d", prec, N);
                    dry++;
                } else {
                    CHECK(r == refill::REFILL_MOVED, "the bound's window is not safe: prec %d N %d", prec, N);
                }
                // a failed stream is left alone
                memcpy(keep, win, 8 * W);
                const uint64_t b1 = base, h1 = held, p1 = pos;
                CHECK(refill::refill_stream_host(src, 8 * nw, nbits, prec, -7, W, win, base, held, pos) == refill::REFILL_IDLE &&
                          base == b1 && held == h1 && pos == p1 && memcmp(keep, win, 8 * W) == 0, "err != 0 not left alone");
                free(src);
                free(win);
                free(keep);
            }
    CHECK(moved > 1000, "too few refills moved anything: %llu", (unsigned long long)moved);
    printf("refill_check: %s (%llu steps, %llu refills moved words, %llu dry)\n", fails ? "FAILED" : "ok",
           (unsigned long long)steps, (unsigned long long)moved, (unsigned long long)dry);
    return fails ? 1 : 0;
}
