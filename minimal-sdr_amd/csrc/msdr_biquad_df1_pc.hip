// msdr_biquad_df1_pc.hip -- the CMSIS-order fp32 cascade kernel with per-channel coefficients and its launcher (a translation unit of its own).
#include "msdr_biquad_df1_pc.hiph"
#include "msdr_block.h"

namespace msdr {

template <int S>
static void sbqpc_launch(hipStream_t stream, bool seg, unsigned grid, const float *x, float *y, long long n, int channels, const float *tab,
                         const float *state_in, float *state_out, int nseg, long long seg_len, int warm, const float *scratch)
{
    if (seg) hipLaunchKernelGGL((biquad_df1_seq_pc_kernel<S, true>), dim3(grid), dim3(64), 0, stream, x, y, n, channels, tab, state_in, state_out, nseg, seg_len, warm, scratch);
    else hipLaunchKernelGGL((biquad_df1_seq_pc_kernel<S, false>), dim3(grid), dim3(64), 0, stream, x, y, n, channels, tab, state_in, state_out, 1, n, 0, (const float *)nullptr);
}

hipError_t launch_biquad_df1_seq_pc(hipStream_t stream, int stages, const float *x, float *y, long long n, int channels, const float *tab,
                                    const float *state_in, float *state_out, int nseg, long long seg_len, int warm, const float *scratch)
{
    if (stages < 1 || stages > kMaxStages || channels <= 0 || n <= 0 || nseg < 1 || !tab) return hipErrorInvalidValue;
    const bool seg = nseg > 1;
    // a segmented launch: segment starts on 4-sample boundaries, every segment non-empty, the warm-up copies in place
    if (seg && (seg_len <= 0 || (seg_len & 3) || (warm & 3) || warm < 0 || !scratch || (long long)(nseg - 1) * seg_len >= n || (long long)nseg * seg_len < n || state_in == state_out))
        return hipErrorInvalidValue;
    const long long units = (long long)channels * nseg;
    const unsigned grid = (unsigned)((units + 63) / 64);
    switch (stages) {
    case 1: sbqpc_launch<1>(stream, seg, grid, x, y, n, channels, tab, state_in, state_out, nseg, seg_len, warm, scratch); break;
    case 2: sbqpc_launch<2>(stream, seg, grid, x, y, n, channels, tab, state_in, state_out, nseg, seg_len, warm, scratch); break;
    case 3: sbqpc_launch<3>(stream, seg, grid, x, y, n, channels, tab, state_in, state_out, nseg, seg_len, warm, scratch); break;
    default: sbqpc_launch<4>(stream, seg, grid, x, y, n, channels, tab, state_in, state_out, nseg, seg_len, warm, scratch); break;
    }
    return hipGetLastError();
}

}  // namespace msdr
