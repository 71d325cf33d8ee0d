// msdr_biquad_pc.hip -- the AudioFilterBiquad node kernel with per-channel coefficients and its launcher (a translation unit of its own).
#include "msdr_biquad_pc.hiph"
#include "msdr_block.h"

namespace msdr {

hipError_t launch_biquad_teensy_pc(hipStream_t stream, int nodes, short *data, int *defs0, int *defs1, int channels, long long n)
{
    const dim3 grid((unsigned)((channels + 63) / 64)), block(64);
    switch (nodes) {
    case 1: hipLaunchKernelGGL((biquad_teensy_pc_kernel<1>), grid, block, 0, stream, data, defs0, (int *)nullptr, channels, n); break;
    case 2: hipLaunchKernelGGL((biquad_teensy_pc_kernel<2>), grid, block, 0, stream, data, defs0, defs1, channels, n); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace msdr
