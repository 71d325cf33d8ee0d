// nco_host_check.cpp -- the phase-accumulator oscillator's host definition (minimal-sdr_amd/csrc/msdr_nco.h) checked exhaustively by a
// stand-alone program: tests/test_nco_host.py compiles it with -fsanitize=address,undefined and runs it.  No library, no GPU.
//   1. every (i, f) pair of the interpolation, 1024 x 65536: the value lies in -32767 .. 32767 and within 1.16 LSB of 32767 sin; the packed
//      table (what the kernels read) gives the same value; cos is sin a quarter turn on
//   2. the rebase identity of a phase-continuous retune: for seeded (base0, T, step_old, step_new), T up to 2^40, the phase at T is unchanged
//      and the phase at T + m advances by m * step_new; an explicit phase is met at T
//   3. msdr_nco_step's rule on the issue's examples
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
#include "msdr_nco.h"

using namespace msdr;

int main()
{
    std::vector<int16_t> T(kNcoTabLen + 1);
    std::vector<uint32_t> P(kNcoTabLen);
    nco_table_build(T.data());
    nco_pack(T.data(), P.data());
    if (T[0] != 0 || T[256] != 32767 || T[768] != -32767 || T[1024] != 0) { printf("FAIL table corners\n"); return 1; }
    int maxd = 0;
    for (int i = 0; i < kNcoTabLen; i++) maxd = std::max(maxd, std::abs(T[i + 1] - T[i]));
    if (maxd > 201) { printf("FAIL table difference %d\n", maxd); return 1; }

    const double w = 6.283185307179586476925286766559 / 4294967296.0;
    double worst = 0.0;
    for (uint32_t i = 0; i < (uint32_t)kNcoTabLen; i++)
        for (uint32_t f = 0; f < 65536u; f++) {
            const uint32_t phi = (i << 22) | (f << 6) | ((i * 7u + f) & 63u);          // (the low 6 bits take no part)
            const int s = nco_sinq(T.data(), phi);
            if (s < -32767 || s > 32767) { printf("FAIL range: phi %08x -> %d\n", phi, s); return 1; }
            if (s != nco_sinq_packed(P[phi >> 22], phi)) { printf("FAIL packed: phi %08x\n", phi); return 1; }
            const double e = std::fabs((double)s - 32767.0 * std::sin(w * (double)(phi & ~63u)));
            if (e > worst) worst = e;
            if (e > 1.16) { printf("FAIL error: phi %08x -> %d, %.4f LSB off\n", phi, s, e); return 1; }
            if ((f & 1023u) == 0 && nco_cosq(T.data(), phi) != nco_sinq(T.data(), phi + 0x40000000u)) { printf("FAIL cos: phi %08x\n", phi); return 1; }
        }

    std::mt19937_64 rng(20240607);
    for (int k = 0; k < 200000; k++) {
        const uint32_t base0 = (uint32_t)rng(), so = (uint32_t)rng(), sn = (uint32_t)rng(), want = (uint32_t)rng();
        const uint64_t Tm = rng() & ((1ull << 40) - 1), m = rng() & 0xFFFFFull;
        const uint32_t b1 = nco_rebase(base0, Tm, so, sn);
        if (nco_phase(b1, sn, (uint32_t)Tm) != nco_phase(base0, so, (uint32_t)Tm)) { printf("FAIL rebase at T (case %d)\n", k); return 1; }
        if (nco_phase(b1, sn, (uint32_t)(Tm + m)) != (uint32_t)(nco_phase(base0, so, (uint32_t)Tm) + (uint32_t)m * sn)) { printf("FAIL rebase at T + m (case %d)\n", k); return 1; }
        const uint32_t b2 = nco_base_for(want, sn, Tm);
        if (nco_phase(b2, sn, (uint32_t)Tm) != want || nco_phase(b2, sn, (uint32_t)(Tm + m)) != (uint32_t)(want + (uint32_t)m * sn)) { printf("FAIL explicit phase (case %d)\n", k); return 1; }
    }

    if (nco_step_of(6000.0, 24000.0) != 0x40000000u || nco_step_of(-6000.0, 24000.0) != 0xC0000000u || nco_step_of(0.0, 24000.0) != 0u) { printf("FAIL step\n"); return 1; }
    for (uint32_t k = 0; k < 128; k++)
        if (nco_step_of(k * 24000.0 / 128.0, 24000.0) != (k << 25)) { printf("FAIL step on the 128 grid, k = %u\n", k); return 1; }

    printf("OK worst %.4f LSB\n", worst);
    return 0;
}
