// msdr_bank_post.hip -- the PLL demodulator behind the per-receiver down-converter bank and its launcher (a translation unit of its own).
#include "msdr_bank_post.hiph"

namespace msdr {

__global__ __launch_bounds__(64) void bank_pll_q15_kernel(BankPllParams p) { bank_pll_body<false>(p); }
__global__ __launch_bounds__(64) void bank_pll_f32_kernel(BankPllParams p) { bank_pll_body<true>(p); }

hipError_t launch_bank_pll(hipStream_t stream, bool f32, const BankPllParams &p)
{
    if (!p.pairs || !p.audio || !p.state || !p.chan_mode || p.channels <= 0 || p.n <= 0 || p.n > p.pair_pitch) return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(p.pairs) & (f32 ? 7 : 3)) return hipErrorInvalidValue;
    const dim3 grid(((unsigned)p.channels + 63u) / 64u), block(64);
    if (f32) hipLaunchKernelGGL(bank_pll_f32_kernel, grid, block, 0, stream, p);
    else hipLaunchKernelGGL(bank_pll_q15_kernel, grid, block, 0, stream, p);
    return hipGetLastError();
}

}  // namespace msdr
