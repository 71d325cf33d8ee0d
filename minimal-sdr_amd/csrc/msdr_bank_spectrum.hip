// msdr_bank_spectrum.hip -- the batched 64-point complex FFT behind msdr_cfft64_* and msdr_chain_set_spectrum, and its launcher (a translation
// unit of its own).
#include "msdr_bank_spectrum.hiph"

namespace msdr {

__global__ __launch_bounds__(256) void bank_cfft64_q15_kernel(BankSpecParams p) { bank_cfft64_q15_body(p); }
__global__ __launch_bounds__(256) void bank_cfft64_f32_kernel(BankSpecParams p) { bank_cfft64_f32_body(p); }

hipError_t launch_bank_cfft64(hipStream_t stream, bool f32, const BankSpecParams &p)
{
    const uintptr_t pair_mask = f32 ? 7 : 3;
    if (!p.pairs || !p.tw || p.nfft <= 0 || p.n_new <= 0 || p.n_new > p.pitch) return hipErrorInvalidValue;
    if (!p.tail && p.n_new != kCfftBins) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(p.pairs) & pair_mask) || (reinterpret_cast<uintptr_t>(p.tail) & 15) ||
        (reinterpret_cast<uintptr_t>(p.bins) & 15) || (reinterpret_cast<uintptr_t>(p.power) & 15)) return hipErrorInvalidValue;
    BankSpecParams q = p;
    // whole 16-byte slots: no pair of the window comes from the tail, and every row's window starts on a slot boundary
    const long long pair_bytes = f32 ? 8 : 4, first = p.n_new - kCfftBins;
    q.vec = first >= 0 && ((reinterpret_cast<uintptr_t>(p.pairs) + (uintptr_t)(first * pair_bytes)) & 15) == 0 && ((p.pitch * pair_bytes) & 15) == 0;
    const dim3 grid((unsigned)std::min<long long>((p.nfft + kCfftPerBlock - 1) / kCfftPerBlock, 256LL * 32)), block(256);
    if (f32) hipLaunchKernelGGL(bank_cfft64_f32_kernel, grid, block, 0, stream, q);
    else hipLaunchKernelGGL(bank_cfft64_q15_kernel, grid, block, 0, stream, q);
    return hipGetLastError();
}

}  // namespace msdr
