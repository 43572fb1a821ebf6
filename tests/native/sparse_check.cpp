// sparse_check.cpp -- host checks of lac_amd/csrc/lac_sparse.h, the plain host/device rules of
// sparse-row coding, in both of their forms: the literal whole-row rules over arrays, and the
// per-lane partials with their combination that the kernels of lac_sparse.hip run -- here over 64
// emulated lanes, lane j owning slots 4 j .. 4 j + 3.  tests/test_sparse_host.py builds it as a
// shared library (the yardsticks there are Python integers on the dense row and the C oracle) and,
// with -DSPARSE_CHECK_MAIN, as a stand-alone program under AddressSanitizer +
// UndefinedBehaviorSanitizer whose sweep holds the two forms to each other and to a dense row
// walked entry by entry, every row a heap block of exactly K slots.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "lac_sparse.h"

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

// ------------------------------------------------------------------ 64 emulated lanes
struct Wave {
    SparseLane lane[64];
    int32_t prev[64];
};
void wave_load(const int32_t *idx, const uint32_t *wt, int K, Wave &w) {
    for (int j = 0; j < 64; j++) {
        w.lane[j] = sparse_lane_pads();
        if (j < K / kSparseLaneSlots)
            for (int q = 0; q < kSparseLaneSlots; q++) {
                w.lane[j].idx[q] = idx[4 * j + q];
                w.lane[j].wt[q] = wt[4 * j + q];
            }
        w.prev[j] = j == 0 ? kSparseNoPrev : w.lane[j - 1].idx[kSparseLaneSlots - 1];
    }
}
bool wave_bad(const Wave &w, int64_t V) {
    bool bad = false;
    for (int j = 0; j < 64; j++) bad |= sparse_lane_bad(w.lane[j], w.prev[j], V);   // the ballot
    return bad;
}
// the encode triple: three sums over lanes; T = 0 for a row that is LAC_E_TABLE
void wave_triple(const Wave &w, uint32_t base, int64_t V, int32_t s, int prec, uint64_t *lo, uint64_t *hi, uint64_t *T) {
    uint64_t below = 0, at = 0, all = 0;
    for (int j = 0; j < 64; j++) {
        uint64_t b, a, t;
        sparse_lane_sums(w.lane[j], s, &b, &a, &t);
        below += b;
        at += a;
        all += t;
    }
    sparse_encode_triple(base, sparse_base_v(base, V), s, below, at, all, wave_bad(w, V), prec, lo, hi, T);
}
// the row's total by the decode kernel's scan (0 for a row that is LAC_E_TABLE), and the scan
uint64_t wave_total(const Wave &w, uint32_t base, int64_t V, int prec, uint64_t in[64]) {
    uint64_t run = 0;
    for (int j = 0; j < 64; j++) {
        run += sparse_lane_weight(w.lane[j]);
        in[j] = run;
    }
    const uint64_t T = sparse_base_v(base, V) + in[63];
    return (wave_bad(w, V) || !range_total_ok(T, prec)) ? 0 : T;
}
void wave_search(const Wave &w, const uint64_t in[64], uint32_t base, uint64_t t, int64_t *s, uint64_t *lo, uint64_t *hi) {
    int L = 63, c[64];
    uint64_t ex[64];
    for (int j = 63; j >= 0; j--) {
        ex[j] = in[j] - sparse_lane_weight(w.lane[j]);
        c[j] = sparse_lane_count(w.lane[j], base, ex[j], t);
        if (c[j] < kSparseLaneSlots) L = j;                                  // the ballot's first lane
    }
    sparse_resolve(sparse_lane_pick(w.lane[L], w.prev[L], ex[L], c[L]), base, t, s, lo, hi);
}

}  // namespace

extern "C" {

int sc_args_ok(uint64_t idx_addr, uint64_t wt_addr, int64_t K, int64_t step_stride, int64_t stream_stride, uint32_t base) {
    return sparse_args_ok((const void *)(uintptr_t)idx_addr, (const void *)(uintptr_t)wt_addr, K, step_stride,
                          stream_stride, base)
               ? 1
               : 0;
}
uint64_t sc_base_v(uint32_t base, int64_t V) { return sparse_base_v(base, V); }

// the row's verdict and total: form 0 the literal rule, form 1 the lanes'
int sc_row_check(int form, const int32_t *idx, const uint32_t *wt, int K, uint32_t base, int64_t V, int prec, uint64_t *T) {
    if (!form) return sparse_row_check(idx, wt, K, sparse_base_v(base, V), V, prec, T);
    Wave w;
    wave_load(idx, wt, K, w);
    uint64_t in[64], lo, hi, T2;
    *T = wave_total(w, base, V, prec, in);
    wave_triple(w, base, V, 0, prec, &lo, &hi, &T2);                         // the encode kernel's total: the same
    if (T2 != *T) return LAC_E_ARG;
    return *T ? LAC_OK : LAC_E_TABLE;
}
// the encode triple of symbol s on a valid row
void sc_range(int form, const int32_t *idx, const uint32_t *wt, int K, uint32_t base, int64_t V, int prec, int64_t s,
              uint64_t *lo, uint64_t *hi) {
    if (!form) {
        sparse_row_range(idx, wt, K, base, s, lo, hi);
        return;
    }
    Wave w;
    wave_load(idx, wt, K, w);
    uint64_t T;
    wave_triple(w, base, V, (int32_t)s, prec, lo, hi, &T);
}
// the decode search for every target of ts[n] on a valid row
void sc_search(int form, const int32_t *idx, const uint32_t *wt, int K, uint32_t base, int64_t V, int prec, int64_t n,
               const uint64_t *ts, int64_t *s, uint64_t *lo, uint64_t *hi) {
    Wave w;
    uint64_t in[64];
    if (form) {
        wave_load(idx, wt, K, w);
        wave_total(w, base, V, prec, in);
    }
    for (int64_t i = 0; i < n; i++) {
        if (form) wave_search(w, in, base, ts[i], &s[i], &lo[i], &hi[i]);
        else sparse_row_search(idx, wt, K, base, ts[i], &s[i], &lo[i], &hi[i]);
    }
}

// One stream from the fresh state: n steps over rows idx[t * K ..], then store_state's last word.
// ek[2 t] = E, ek[2 t + 1] = k (-1 where the step did not narrow); planes: [2][cap_words];
// regs = {l, h, L, nsym}.  Returns the sticky status, *err_step the failing step's nsym.
int sc_encode(int form, int64_t n, const int32_t *idx, const uint32_t *wt, int K, uint32_t base, int64_t V,
              const int32_t *syms, int prec, uint64_t cap_words, uint64_t *ek, uint64_t *planes, int64_t *regs,
              int64_t *err_step) {
    EncState st;
    memset(&st, 0, sizeof(st));
    st.nflush = -1;
    int64_t l = 0, h = ((int64_t)1 << prec) - 1;
    uint64_t *pa = planes, *pc = planes + cap_words;
    auto store = [&](uint64_t i, uint64_t wa, uint64_t wc) {
        pa[i] = wa;
        pc[i] = wc;
    };
    int rc = LAC_OK;
    *err_step = -1;
    for (int64_t t = 0; t < n && !rc; t++) {
        int k = -1;
        uint64_t E = 0;
        const int32_t *ri = idx + t * K;
        const uint32_t *rw = wt + t * K;
        if (!form) {
            rc = sparse_encode_step(st, l, h, ri, rw, K, base, V, syms[t], prec, cap_words, store, &k, &E);
        } else {                                                             // the kernel's order: symbol, row, step
            Wave w;
            wave_load(ri, rw, K, w);
            const bool sym_ok = (uint32_t)syms[t] < (uint32_t)V;
            uint64_t lo, hi, T;
            wave_triple(w, base, V, sym_ok ? syms[t] : 0, prec, &lo, &hi, &T);
            if (!sym_ok) rc = LAC_E_SYMBOL_RANGE;
            else if (T == 0) rc = LAC_E_TABLE;
            else rc = range_encode_step(st, l, h, lo, hi, T, recip(T), prec, cap_words, store, &k, &E);
        }
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

int sc_flush(int64_t l, int64_t h, int prec, int8_t *digits) { return flush_digits(l, h, prec, digits); }

// One stream's decode from the opened state.  regs = {l, h, x, pos, nsym, det, ndet}; syms_out[t]
// = -1 from the failing step on.  Returns the sticky status.
int sc_decode(int form, int64_t n, const int32_t *idx, const uint32_t *wt, int K, uint32_t base, int64_t V, int prec,
              const uint8_t *bytes, uint64_t nbits, int stop, int32_t *syms_out, int64_t *regs) {
    DecState st;
    memset(&st, 0, sizeof(st));
    st.h = ((int64_t)1 << prec) - 1;
    st.pos = (uint64_t)prec;
    st.det = 1;
    st.err_step = -1;
    st.x = (int64_t)host_bits(bytes, nbits, 0, prec);
    int rc = LAC_OK;
    for (int64_t t = 0; t < n; t++) {
        syms_out[t] = -1;
        if (rc) continue;
        const int32_t *ri = idx + t * K;
        const uint32_t *rw = wt + t * K;
        const uint64_t pos = st.pos, past = pos > nbits ? pos - nbits : 0;
        auto pull = [&](int k) { return host_bits(bytes, nbits, pos, k); };
        int64_t s = -1;
        if (!form) {
            rc = sparse_decode_step(st, ri, rw, K, base, V, prec, past, stop != 0, pull, &s);
        } else {                                                             // the kernel's order: row, registers, search, frame
            Wave w;
            wave_load(ri, rw, K, w);
            uint64_t in[64];
            const uint64_t T = wave_total(w, base, V, prec, in);
            if (T == 0) rc = LAC_E_TABLE;
            else if (st.x < st.l || st.x > st.h) rc = LAC_E_DECODE_RANGE;
            else {
                const uint64_t wd = (uint64_t)(st.h - st.l + 1);
                const uint64_t tg = range_target((uint64_t)(st.x - st.l), T, wd, recip(wd));
                uint64_t lo, hi;
                wave_search(w, in, base, tg, &s, &lo, &hi);
                rc = s >= V ? LAC_E_DECODE_RANGE : range_decode_step(st, lo, hi, T, recip(T), prec, past, stop != 0, pull);
            }
        }
        if (!rc) syms_out[t] = (int32_t)s;
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

// The sweep: random rows (valid and malformed), every row a heap block of exactly K slots.  The
// lanes' verdict and total against the literal rule's; on valid rows the triple of every symbol
// of interest and the search at t = 0, T - 1 and every A_j - 1, A_j, B_j - 1, B_j, lanes against
// literal, and both against a dense row walked entry by entry where V <= 400.  Returns the number
// of failures; *count the checks made.
int sc_sweep(uint64_t seed, int64_t *count) {
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
    static const int precs[] = {16, 34, 48, 61};
    static const int Ks[] = {4, 8, 12, 64, 252, 256};
    for (int i = 0; i < 1500; i++) {
        const int prec = precs[r.next() % 4];
        const int K = Ks[r.next() % 6];
        const int64_t V = (i % 5 == 0) ? ((int64_t)1 << 18) : (i % 7 == 0 ? 5 : 1 + (int64_t)(r.next() % 400));
        uint32_t base = (i % 3 == 0) ? 1 : (i % 3 == 1 ? 3 : 65536 + (uint32_t)(r.next() % 100000));
        if ((u128)base * (u128)V > ((u128)1 << (prec - 1))) base = 1;
        if ((uint64_t)V > (1ull << (prec - 1))) continue;
        const uint64_t room = (1ull << (prec - 1)) - (uint64_t)base * (uint64_t)V;
        int np = (int)(r.next() % (uint64_t)(K + 1));
        if (i % 4 == 0) np = K;
        if (i % 9 == 0) np = 0;
        if ((int64_t)np > V) np = (int)V;
        std::vector<int32_t> idx((size_t)K, -1);                             // exactly the row
        std::vector<uint32_t> wt((size_t)K, 0);
        // ascending indices: np of V by a stride walk
        int64_t at = 0;
        for (int j = 0; j < np; j++) {
            const int64_t left = V - at - (np - j);                          // slack to spend
            const int64_t skip = left > 0 ? (int64_t)(r.next() % (uint64_t)(1 + (j % 3 == 0 ? 0 : (left < 8 ? left : left / (np - j))))) : 0;
            at += skip;
            idx[(size_t)j] = (int32_t)at;
            at += 1;
        }
        uint64_t left_w = room;
        for (int j = 0; j < np; j++) {
            uint64_t w = r.next() % 4 == 0 ? 0 : r.next() & 0xFFFFFFFFull;
            if (np) w = w < left_w / (uint64_t)np ? w : left_w / (uint64_t)np;
            if (w > 0xFFFFFFFFull) w = 0xFFFFFFFFull;
            wt[(size_t)j] = (uint32_t)w;
        }
        for (int j = np; j < K; j++) wt[(size_t)j] = (uint32_t)r.next();   // a pad's weight is ignored
        // every fifth row is broken one way
        const int defect = i % 5 == 2 ? 1 + (int)(r.next() % 6) : 0;
        if (defect == 1 && np < K) idx[(size_t)(K - 1)] = (int32_t)(r.next() % (uint64_t)V);   // a pair after a pad
        if (defect == 2 && np >= 2) idx[(size_t)(np - 1)] = idx[(size_t)(np - 2)];   // equal
        if (defect == 3 && np >= 2) { const int j = (int)(r.next() % (uint64_t)(np - 1)); const int32_t x = idx[(size_t)j]; idx[(size_t)j] = idx[(size_t)j + 1]; idx[(size_t)j + 1] = x; }
        if (defect == 4) idx[(size_t)(r.next() % (uint64_t)K)] = -2 - (int32_t)(r.next() % 5);   // idx < -1
        if (defect == 5 && np >= 1 && V < ((int64_t)1 << 30)) idx[(size_t)(np - 1)] = (int32_t)V;   // idx >= V
        if (defect == 6 && np >= 1 && room < 0xFFFFFFFFull * (uint64_t)np) {      // the total one too large
            uint64_t sum = 0;
            for (int j = 0; j < np; j++) sum += wt[(size_t)j];
            uint64_t need = room + 1 - sum;
            for (int j = 0; j < np && need; j++) {
                const uint64_t add = 0xFFFFFFFFull - wt[(size_t)j] < need ? 0xFFFFFFFFull - wt[(size_t)j] : need;
                wt[(size_t)j] += (uint32_t)add;
                need -= add;
            }
        }
        uint64_t T0, T1;
        const int rc0 = sc_row_check(0, idx.data(), wt.data(), K, base, V, prec, &T0);
        const int rc1 = sc_row_check(1, idx.data(), wt.data(), K, base, V, prec, &T1);
        n++;
        if (rc0 != rc1 || T0 != T1) { bad++; continue; }
        if (rc0) continue;
        np = sparse_row_pairs(idx.data(), K);                                // (a defect that left the row valid)
        // a dense row, where it can be written
        std::vector<uint64_t> dense;
        if (V <= 400) {
            dense.assign((size_t)V, base);
            for (int j = 0; j < np; j++) dense[(size_t)idx[(size_t)j]] += wt[(size_t)j];
        }
        // symbols of interest: at a pair, around it, 0, V - 1
        std::vector<int64_t> ss = {0, V - 1, (int64_t)(r.next() % (uint64_t)V)};
        for (int j = 0; j < np; j++)
            for (int d = -1; d <= 1; d++)
                if (idx[(size_t)j] + d >= 0 && idx[(size_t)j] + d < V) ss.push_back(idx[(size_t)j] + d);
        std::vector<uint64_t> ts = {0, T0 - 1};
        for (int64_t s : ss) {
            uint64_t lo0, hi0, lo1, hi1;
            sc_range(0, idx.data(), wt.data(), K, base, V, prec, s, &lo0, &hi0);
            sc_range(1, idx.data(), wt.data(), K, base, V, prec, s, &lo1, &hi1);
            n++;
            if (lo0 != lo1 || hi0 != hi1 || lo0 >= hi0 || hi0 > T0) bad++;
            if (!dense.empty()) {
                uint64_t c = 0;
                for (int64_t e = 0; e < s; e++) c += dense[(size_t)e];
                if (c != lo0 || c + dense[(size_t)s] != hi0) bad++;
            }
            ts.push_back(lo0);
            ts.push_back(hi0 - 1);
            if (lo0 > 0) ts.push_back(lo0 - 1);
            if (hi0 < T0) ts.push_back(hi0);
        }
        const int64_t nt = (int64_t)ts.size();
        std::vector<int64_t> s0((size_t)nt), s1((size_t)nt);
        std::vector<uint64_t> l0((size_t)nt), h0((size_t)nt), l1((size_t)nt), h1((size_t)nt);
        sc_search(0, idx.data(), wt.data(), K, base, V, prec, nt, ts.data(), s0.data(), l0.data(), h0.data());
        sc_search(1, idx.data(), wt.data(), K, base, V, prec, nt, ts.data(), s1.data(), l1.data(), h1.data());
        for (int64_t q = 0; q < nt; q++) {
            n++;
            const size_t u = (size_t)q;
            if (s0[u] != s1[u] || l0[u] != l1[u] || h0[u] != h1[u]) bad++;
            if (!(l0[u] <= ts[u] && ts[u] < h0[u]) || s0[u] < 0 || s0[u] >= V) bad++;
            uint64_t lo, hi;                                                 // the search inverts the triple
            sc_range(0, idx.data(), wt.data(), K, base, V, prec, s0[u], &lo, &hi);
            if (lo != l0[u] || hi != h0[u]) bad++;
            if (!dense.empty()) {
                uint64_t c = 0;
                int64_t e = 0;
                while (e < V && c + dense[(size_t)e] <= ts[u]) c += dense[(size_t)e++];
                if (e != s0[u] || c != l0[u]) bad++;
            }
        }
    }
    *count = n;
    return bad;
}

}  // extern "C"

#ifdef SPARSE_CHECK_MAIN
int main() {
    int64_t n = 0;
    int bad = sc_sweep(12345, &n);
    // whole jobs, round trip, both forms: coded, finished by hand (the digits as one number), decoded
    for (int job = 0; job < 16 && !bad; job++) {
        const int form = job & 1;
        const int prec = job % 4 == 3 ? 61 : 16 + 2 * job;
        const int K = job % 3 == 0 ? 4 : (job % 3 == 1 ? 64 : 256);
        const int64_t V = job % 5 == 0 ? 5 : 300, steps = 1 + 9 * job;
        const uint32_t base = job % 2 ? 3 : 1;
        std::vector<int32_t> idx((size_t)(steps * K), -1), syms((size_t)steps), got((size_t)steps);
        std::vector<uint32_t> wt((size_t)(steps * K), 0);
        uint64_t s = 77 + (uint64_t)job;
        auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
        const uint64_t room = (1ull << (prec - 1)) - (uint64_t)base * (uint64_t)V;
        for (int64_t t = 0; t < steps; t++) {
            int np = (int)(next() % (uint64_t)(K + 1));
            if ((int64_t)np > V) np = (int)V;
            int64_t at = 0;
            for (int j = 0; j < np; j++) {
                const int64_t slack = V - at - (np - j);
                at += slack > 0 ? (int64_t)(next() % (uint64_t)(1 + slack / (np - j))) : 0;
                idx[(size_t)(t * K + j)] = (int32_t)at++;
                const uint64_t w = next() & 0xFFFFFFFFull, cap = room / (uint64_t)np;
                wt[(size_t)(t * K + j)] = (uint32_t)(w < cap ? w : cap);
            }
            syms[(size_t)t] = (int32_t)(next() % (uint64_t)V);
        }
        const uint64_t cap_words = ((uint64_t)steps * (uint64_t)(prec + 2) + 64 + 63) / 64;
        std::vector<uint64_t> planes(2 * cap_words, 0), ek(2 * (size_t)steps);
        int64_t regs[7], es = 0;
        if (sc_encode(form, steps, idx.data(), wt.data(), K, base, V, syms.data(), prec, cap_words, ek.data(),
                      planes.data(), regs, &es))
            bad++;
        std::vector<int> dg;
        for (int64_t t = 0; t < steps; t++) {
            const int k = (int)(int64_t)ek[2 * (size_t)t + 1];
            const uint64_t E = ek[2 * (size_t)t];
            for (int i = 0; i < k; i++) dg.push_back(i == 0 ? (int)(E >> (k - 1)) : (int)((E >> (k - 1 - i)) & 1));
        }
        int8_t fd[8];
        const int m = sc_flush(regs[0], regs[1], prec, fd);
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
        if (sc_decode(1 - form, steps, idx.data(), wt.data(), K, base, V, prec, bytes.data(), dg.size(), 0, got.data(), regs))
            bad++;
        if (got != syms || regs[4] != steps) bad++;
        n += steps;
    }
    if (bad) {
        fprintf(stderr, "sparse_check: %d failures in %lld checks\n", bad, (long long)n);
        return 1;
    }
    printf("sparse_check: ok (%lld checks)\n", (long long)n);
    return 0;
}
#endif
