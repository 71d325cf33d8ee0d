// kstack_check -- host-only check of the K-stacked A operands of the folded cascade's sparse products (minimal-sdr_amd/csrc/msdr_kstack.h,
// included as it is; nothing is launched).  Random responses X (R: scale 2^14, one and two sections; Rd: scale 2^13) meet random vectors v
// (sigma / delta), split into fp16 pieces as the kernels split them (hi = toward zero, lo = the remainder toward zero).  The 16-row K sum
// of one v_mfma_f32_32x32x16_f16 is formed in double -- fp16 x fp16 is exact there -- for
//     two instructions:  stack . [0 ; v_hi v_lo]  +  lo . [0 ; v_hi v_lo]
//     one instruction :  stack . [v_hi 0 ; v_hi v_lo]
// and must equal  X_hi v_hi + X_hi v_lo + X_lo v_hi  to double rounding.
//   kstack_check          the product's tables
//   kstack_check mutant   built with -DMSDR_MUTATE=5: the X_lo v_hi term is gone and nothing else changes
// Prints "hi-checksum <n>" (the entries that hold X_hi: the same number from both builds) and "kstack_check: <n> failures".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "../../minimal-sdr_amd/csrc/msdr_kstack.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } failures++; } } while (0)

// v_cvt_pkrtz_f16_f32: toward zero
static _Float16 half_rtz(float f)
{
    _Float16 h = (_Float16)f;
    if (std::fabs((double)h) > std::fabs((double)f)) {
        uint16_t b;
        memcpy(&b, &h, 2);
        b -= 1;                                 // one step toward zero (sign-magnitude)
        memcpy(&h, &b, 2);
    }
    return h;
}

// element k (0 .. 15) of row m of an A operand: lane (m, h = k >> 3), entry k & 7
static double a_at(const _Float16 *frag, int m, int k) { return (double)frag[(m + 32 * (k >> 3)) * 8 + (k & 7)]; }

int main(int argc, char **argv)
{
    const bool mutant = argc > 1 && strcmp(argv[1], "mutant") == 0;
    std::mt19937_64 rng(20261);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    uint64_t hisum = 1469598103934665603ull;
    bool lo_term_seen = false;
    for (int trial = 0; trial < 300; trial++) {
        const int kind = trial % 3;                         // R with one section, R with two, Rd
        const int ncomp = kind == 0 ? 2 : 4;
        const double scale = std::ldexp(1.0, kind == 2 ? 13 : 14);
        const double mag = std::ldexp(1.0, -(int)(rng() % 12));          // responses from ~1 down to 2^-11 (the lo pieces reach fp16's subnormals)
        double X[32][4] = {{0}};
        for (int m = 0; m < 32; m++) for (int j = 0; j < ncomp; j++) X[m][j] = u(rng) * mag * 3.5;
        _Float16 stack[msdr::kKstackHalves], lo[msdr::kKstackHalves];
        memset(stack, 0x7f, sizeof stack); memset(lo, 0x7f, sizeof lo);            // (NaN patterns: the filler writes every entry)
        msdr::kstack_fill(X, scale, stack, lo);
        // the pieces, split here independently of the filler
        double xh[32][4], xl[32][4];
        for (int m = 0; m < 32; m++) for (int j = 0; j < 4; j++) {
            const double val = X[m][j] * scale;
            const _Float16 h = (_Float16)val;
            xh[m][j] = (double)h; xl[m][j] = (double)(_Float16)(val - (double)h);
        }
        // layout: what sits where, and zeros (finite) everywhere else
        for (int m = 0; m < 32; m++) for (int k = 0; k < 16; k++) {
            const double ws = k >= 8 ? xh[m][k & 3] : (k < 4 ? (mutant ? 0.0 : xl[m][k]) : 0.0);
            const double wl = (k >= 8 && k < 12) ? (mutant ? 0.0 : xl[m][k - 8]) : 0.0;
            CHECK(a_at(stack, m, k) == ws, "stack trial %d m %d k %d: %g != %g", trial, m, k, a_at(stack, m, k), ws);
            CHECK(a_at(lo, m, k) == wl, "lo trial %d m %d k %d: %g != %g", trial, m, k, a_at(lo, m, k), wl);
            if (k >= 8) { uint16_t b; memcpy(&b, &stack[(m + 32) * 8 + (k & 7)], 2); hisum = (hisum ^ b) * 1099511628211ull; }
        }
        for (int col = 0; col < 8; col++) {
            double vh[4] = {0, 0, 0, 0}, vl[4] = {0, 0, 0, 0};
            for (int j = 0; j < ncomp; j++) {
                const float f = (float)(u(rng) * 3.0 * std::ldexp(1.0, -(int)(rng() % 10)));
                const _Float16 h = half_rtz(f);
                vh[j] = (double)h; vl[j] = (double)half_rtz(f - (float)h);
            }
            double b2[16] = {0}, b1[16] = {0};               // B operand of the column, K 0 .. 15: two-instruction form, one-instruction form
            for (int j = 0; j < 4; j++) { b2[8 + j] = vh[j]; b2[12 + j] = vl[j]; b1[8 + j] = vh[j]; b1[12 + j] = vl[j]; b1[j] = vh[j]; }
            for (int m = 0; m < 32; m++) {
                double two = 0.0, one = 0.0, want = 0.0, mass = 0.0, loterm = 0.0;
                for (int k = 0; k < 16; k++) two += a_at(stack, m, k) * b2[k];
                for (int k = 0; k < 16; k++) two += a_at(lo, m, k) * b2[k];
                for (int k = 0; k < 16; k++) one += a_at(stack, m, k) * b1[k];
                for (int j = 0; j < 4; j++) { want += xh[m][j] * vh[j]; mass += std::fabs(xh[m][j] * vh[j]); }
                for (int j = 0; j < 4; j++) { want += xh[m][j] * vl[j]; mass += std::fabs(xh[m][j] * vl[j]); }
                for (int j = 0; j < 4; j++) { loterm += xl[m][j] * vh[j]; mass += std::fabs(xl[m][j] * vh[j]); }
                if (!mutant) want += loterm;
                if (loterm != 0.0) lo_term_seen = true;
                const double tol = 8 * 2.220446049250313e-16 * mass;           // 12 exact products, summed in double in another order
                CHECK(std::fabs(two - want) <= tol, "two instructions, trial %d col %d m %d: %.17g != %.17g", trial, col, m, two, want);
                CHECK(std::fabs(one - want) <= tol, "one instruction, trial %d col %d m %d: %.17g != %.17g", trial, col, m, one, want);
            }
        }
    }
    CHECK(lo_term_seen, "no draw had a lo piece: the check would not see it missing");
    printf("hi-checksum %llu\n", (unsigned long long)hisum);
    printf("kstack_check%s: %d failures\n", mutant ? " (mutant 5)" : "", failures);
    return failures ? 1 : 0;
}
