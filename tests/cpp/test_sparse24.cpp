// tests/cpp/test_sparse24.cpp -- minimal-sdr_amd/csrc/msdr_sparse24.h on the CPU: the first and last tap block of a FIR run merged into one
// 2:4-sparse operand, expanded again by the header's documented encoding, must be the K-stacked pair exactly, in the hi and in the lo piece.
// Stand-alone (own main, no GPU, no library):
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o test_sparse24 test_sparse24.cpp && ./test_sparse24
// Built with -DMSDR_MUTATE=1 / =2 (`make mutants`) the same checks run against the mutated split: the mutations act on the merged pieces.
#include "../../minimal-sdr_amd/csrc/msdr_sparse24.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#ifndef MSDR_MUTATE
#define MSDR_MUTATE 0
#endif

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { if (failures < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } failures++; } } while (0)

static unsigned rng_state = 2463534242u;
static unsigned rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }
static double rnd_tap() { double v; do { v = ((double)(rnd() >> 8) / (double)(1 << 24)) * 2.0 - 1.0; } while (v == 0.0); return v; }

// the fp16 value nearest to v (ties to the even mantissa), found by walking the fp16 values themselves: independent of the header's rounding
static double nearest_half(double v)
{
    const double a = std::fabs(v);
    unsigned lo = 0, hi = 0x7bff;                     // bit patterns of the non-negative finite fp16 values, increasing
    while (hi - lo > 1) { const unsigned mid = (lo + hi) / 2; if (msdr::sparse24_half_value((uint16_t)mid) <= a) lo = mid; else hi = mid; }
    const double dl = a - msdr::sparse24_half_value((uint16_t)lo), dh = msdr::sparse24_half_value((uint16_t)hi) - a;
    const unsigned pick = (dl < dh) ? lo : (dh < dl) ? hi : ((lo & 1u) ? hi : lo);
    const double r = msdr::sparse24_half_value((uint16_t)pick);
#ifdef __FLT16_MANT_DIG__
    if ((double)(_Float16)a != r) { printf("FAIL: nearest_half(%a) = %a, the compiler's conversion gives %a\n", a, r, (double)(_Float16)a); exit(1); }
#endif
    return v < 0 ? -r : r;
}

// what a table entry must hold, written out independently of the header: scaled, (mutant 2: 16 significant bits), hi = fp16, lo = fp16 of the
// remainder (mutant 1: none)
static void expected_split(double m, double scale, double *hi, double *lo)
{
    double val = m * scale;
    if (MSDR_MUTATE == 2 && val != 0.0) { int e; const double f = std::frexp(val, &e); val = std::ldexp(std::nearbyint(std::ldexp(f, 16)), e - 16); }
    *hi = nearest_half(val);
    *lo = (MSDR_MUTATE == 1) ? 0.0 : nearest_half(val - *hi);
}

// the scale msdr_chain_create gives a table: max |entry| * scale in [2^13, 2^14)
static double table_scale(const std::vector<double> &a, const std::vector<double> &b)
{
    double maxabs = 0.0;
    for (double v : a) maxabs = std::max(maxabs, std::fabs(v));
    for (double v : b) maxabs = std::max(maxabs, std::fabs(v));
    int ex = 0;
    if (maxabs > 0) { std::frexp(maxabs, &ex); ex = 14 - ex; }
    return std::ldexp(1.0, ex);
}

static void check_pair(const char *what, const std::vector<double> &first, const std::vector<double> &last, int stride)
{
    const double scale = table_scale(first, last);
    std::vector<uint16_t> hi(msdr::kSp24FragHalfs), lo(msdr::kSp24FragHalfs);
    std::vector<uint32_t> idx(64);
    const bool ok = msdr::sparse24_merge(first.data(), last.data(), stride, scale, hi.data(), lo.data(), idx.data());
    EXPECT(ok, "%s: complementary blocks refused", what);
    if (!ok) return;
    for (int l = 0; l < 64; l++) {
        EXPECT((idx[l] >> 16) == 0, "%s: lane %d index word 0x%x uses the high half", what, l, idx[l]);
        for (int g = 0; g < 4; g++) {
            const unsigned nib = (idx[l] >> (4 * g)) & 15u;
            EXPECT((nib & 3u) < (nib >> 2), "%s: lane %d group %d index pair (%u, %u) not strictly increasing", what, l, g, nib & 3u, nib >> 2);
        }
    }
    std::vector<double> eh(32 * 32), el(32 * 32);
    msdr::sparse24_expand(hi.data(), idx.data(), eh.data());
    msdr::sparse24_expand(lo.data(), idx.data(), el.data());
    double lo_sum = 0.0;
    for (int m = 0; m < 32; m++)
        for (int b = 0; b < 32; b++) {
            const double tap = (m < 16) ? first[m * stride + b] : last[(m - 16) * stride + b];
            double xh, xl;
            expected_split(tap, scale, &xh, &xl);
            EXPECT(eh[m * 32 + b] == xh, "%s: hi piece at K-stacked row %d column %d is %g, expected %g", what, m, b, eh[m * 32 + b], xh);
            EXPECT(el[m * 32 + b] == xl, "%s: lo piece at K-stacked row %d column %d is %g, expected %g", what, m, b, el[m * 32 + b], xl);
            lo_sum += std::fabs(el[m * 32 + b]);
        }
    if (MSDR_MUTATE == 1) EXPECT(lo_sum == 0.0, "%s: mutant 1 left lo pieces", what);
    else EXPECT(lo_sum > 0.0, "%s: no lo pieces at all", what);
}

// the first and last chunk of a run over one parity array: column b meets the array's samples m0(b) .. m0(b) + band - 1 with the taps
// t[m - m0(b)] (Toeplitz); odd: m0 = ceil(b / 2), else m0 = floor(b / 2) + 1
static void toeplitz_case(int band, bool odd, int stride)
{
    std::vector<double> taps(band);
    for (auto &t : taps) t = rnd_tap() * 0.01;
    auto m0 = [&](int b) { return odd ? (b + 1) / 2 : b / 2 + 1; };
    const int jlast = (m0(31) + band - 1) / 16;
    std::vector<double> first((size_t)16 * stride, 0.0), last((size_t)16 * stride, 0.0);
    for (int m = 0; m < 16; m++)
        for (int b = 0; b < 32; b++) {
            const int d0 = m - m0(b), d1 = 16 * jlast + m - m0(b);
            if (d0 >= 0 && d0 < band) first[m * stride + b] = taps[d0];
            if (d1 >= 0 && d1 < band) last[m * stride + b] = taps[d1];
        }
    char what[96];
    snprintf(what, sizeof what, "Toeplitz band %d, %s samples, stride %d, %d steps", band, odd ? "odd" : "even", stride, jlast + 1);
    EXPECT(jlast >= 1, "%s: not a run of two steps", what);
    check_pair(what, first, last, stride);
}

int main()
{
    for (int band : {8, 52, 128, 256})
        for (int odd = 0; odd < 2; odd++) {
            toeplitz_case(band, odd != 0, 32);
            toeplitz_case(band, odd != 0, 64);       // (msdr_chain_create's matrix interleaves the two parities: row stride 64)
        }
    for (int rep = 0; rep < 50; rep++) {             // random complementary blocks: every (m, b) in the first block, in the last, or in neither
        std::vector<double> first(16 * 32, 0.0), last(16 * 32, 0.0);
        for (int k = 0; k < 16 * 32; k++) {
            const unsigned w = rnd() % 3;
            if (w == 0) first[k] = rnd_tap(); else if (w == 1) last[k] = rnd_tap();
        }
        check_pair("random complementary blocks", first, last, 32);
        // one entry in both: refused
        const int k = (int)(rnd() % (16 * 32));
        first[k] = rnd_tap(); last[k] = rnd_tap();
        std::vector<uint16_t> hi(msdr::kSp24FragHalfs), lo(msdr::kSp24FragHalfs);
        std::vector<uint32_t> idx(64);
        EXPECT(!msdr::sparse24_merge(first.data(), last.data(), 32, 1024.0, hi.data(), lo.data(), idx.data()), "overlap at entry %d accepted", k);
    }
    {   // empty blocks: explicit zeros with a valid index
        std::vector<double> z(16 * 32, 0.0);
        std::vector<uint16_t> hi(msdr::kSp24FragHalfs), lo(msdr::kSp24FragHalfs);
        std::vector<uint32_t> idx(64);
        EXPECT(msdr::sparse24_merge(z.data(), z.data(), 32, 1.0, hi.data(), lo.data(), idx.data()), "empty blocks refused");
        for (int l = 0; l < 64; l++) EXPECT(idx[l] == 0x4444u, "empty blocks: index word 0x%x", idx[l]);
    }
    printf("test_sparse24 (MSDR_MUTATE %d): %d failures\n", MSDR_MUTATE, failures);
    return failures ? 1 : 0;
}
