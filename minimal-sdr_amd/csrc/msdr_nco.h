// msdr_nco.h -- the phase-accumulator oscillator of the per-receiver chains (msdr_chain_set_nco_channels): plain functions that the host
// and the kernels share, no device state; includes nothing of HIP, so that a host compiler can test every function on its own
// (tests/cpp/nco_host_check.cpp).
//
// tune() of the reference (Minimal-SDR.ino:328-368) sets the local oscillator to ANY frequency.  Here a receiver keeps one 32-bit phase
// and one 32-bit step; the phase of the sample at chain time T (samples since msdr_chain_reset, low 32 bits) is
//     phi(T) = base0 + (uint32) T * step                                   (wrapping)
// and the oscillator pair is {cos, sin} = {sinq(phi + 2^30), sinq(phi)}:
//     table   T[i] = (int16) lround(32767 sin(2 pi i / 1024)), i = 0 .. 1024, T[1024] = 0
//     sinq    i = phi >> 22, f = (phi >> 6) & 0xFFFF, sinq = T[i] + (((T[i + 1] - T[i]) * f + 32768) >> 16)         (arithmetic shift)
// |T[i + 1] - T[i]| <= 201, so every product fits 32 bits; the result lies in -32767 .. 32767 and is within
// 0.5 (table rounding) + 0.5 (interpolation rounding) + 32767 (2 pi / 1024)^2 / 8 (chord) = 1.154 LSB of 32767 sin.  For step = k 2^25 the
// values equal round(32767 sin(2 pi k n / 128)): a 128-entry table chain is a special case.
// The kernels read the table as one dword per entry, T[i] | (T[i + 1] - T[i]) << 16 (nco_pack): a sine is one LDS read.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MSDR_NCO_HD __host__ __device__ inline
#else
#define MSDR_NCO_HD inline
#endif

namespace msdr {

constexpr int kNcoTabLen = 1024;                        // entries of a period; the table itself has one more (T[1024] = T[0] = 0)
constexpr uint32_t kNcoQuarter = 0x40000000u;           // cos(phi) = sin(phi + a quarter turn)

// the table, computed once on the host in double (no entry is closer than 1.2e-3 to a rounding boundary: any libm gives the same integers)
inline void nco_table_build(int16_t table[kNcoTabLen + 1])
{
    const double w = 6.283185307179586476925286766559 / kNcoTabLen;
    for (int i = 0; i < kNcoTabLen; i++) table[i] = (int16_t)std::lround(32767.0 * std::sin(w * i));
    table[kNcoTabLen] = 0;
}
// the kernels' form: entry i = T[i] (low half) | T[i + 1] - T[i] (high half), i < 1024
inline void nco_pack(const int16_t table[kNcoTabLen + 1], uint32_t packed[kNcoTabLen])
{
    for (int i = 0; i < kNcoTabLen; i++) packed[i] = (uint32_t)(uint16_t)table[i] | ((uint32_t)(table[i + 1] - table[i]) << 16);
}

MSDR_NCO_HD int nco_interp(int t0, int d, uint32_t phi) { return t0 + ((d * (int)((phi >> 6) & 0xFFFFu) + 32768) >> 16); }
MSDR_NCO_HD int nco_sinq(const int16_t *table, uint32_t phi) { const uint32_t i = phi >> 22; return nco_interp(table[i], table[i + 1] - table[i], phi); }
MSDR_NCO_HD int nco_cosq(const int16_t *table, uint32_t phi) { return nco_sinq(table, phi + kNcoQuarter); }
// ... from a packed entry (the caller read packed[phi >> 22])
MSDR_NCO_HD int nco_sinq_packed(uint32_t entry, uint32_t phi) { return nco_interp((int16_t)(entry & 0xFFFFu), (int)entry >> 16, phi); }

// phase of the sample at chain time t32 (the low 32 bits of the sample count since msdr_chain_reset)
MSDR_NCO_HD uint32_t nco_phase(uint32_t base0, uint32_t step, uint32_t t32) { return base0 + t32 * step; }
// a retune at chain time T: the base that gives the next sample (time T) the phase `phi`
MSDR_NCO_HD uint32_t nco_base_for(uint32_t phi, uint32_t step, uint64_t T) { return phi - (uint32_t)T * step; }
// ... and the phase-continuous one: the phase at T is what the old step had reached
MSDR_NCO_HD uint32_t nco_rebase(uint32_t base0, uint64_t T, uint32_t step_old, uint32_t step_new) { return base0 + (uint32_t)T * step_old - (uint32_t)T * step_new; }

// llround(f / fs * 2^32) mod 2^32; a negative frequency wraps (-6000 at 24000: 0xC0000000).  0 where the ratio is not a usable number.
inline uint32_t nco_step_of(double f_hz, double fs_hz)
{
    const double r = f_hz / fs_hz * 4294967296.0;
    if (!(std::fabs(r) < 4.0e18)) return 0;
    return (uint32_t)(uint64_t)std::llround(r);
}

}  // namespace msdr
