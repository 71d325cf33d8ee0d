// msdr_chain_f32pc.hip -- the fp32 chain kernel with per-channel FIR coefficients and its launcher (a translation unit of its own).
#include <algorithm>
#include "msdr_chain_f32pc.hiph"
#include "msdr_block.h"

namespace msdr {

template <int CPW>
static void pf_launch(hipStream_t stream, bool fir_only, bool fs4, unsigned grid, unsigned block, size_t lds, const PcfParams &p)
{
    if (fir_only) hipLaunchKernelGGL((chain_f32pc_kernel<CPW, true, false>), dim3(grid), dim3(block), lds, stream, p);
    else if (fs4) hipLaunchKernelGGL((chain_f32pc_kernel<CPW, false, true>), dim3(grid), dim3(block), lds, stream, p);
    else hipLaunchKernelGGL((chain_f32pc_kernel<CPW, false, false>), dim3(grid), dim3(block), lds, stream, p);
}

hipError_t launch_chain_f32pc(hipStream_t stream, bool fir_only, int num_cus, int time_segments, PcfParams p, PcLaunch *geo)
{
    if (p.np <= 0 || (p.np & 3) || p.channels <= 0 || p.n <= 0) return hipErrorInvalidValue;
    const bool fs4 = !fir_only && p.mixer == kMixerFs4;
    int cpw = p.n <= 128 ? 4 : p.n <= 256 ? 2 : 1;
    int nw = 4;
    while (f32pc_lds_bytes(p.np, cpw, fir_only, fs4, nw) > kPfLdsCap && nw > 1) nw >>= 1;
    while (f32pc_lds_bytes(p.np, cpw, fir_only, fs4, nw) > kPfLdsCap && cpw > 1) cpw >>= 1;
    if (f32pc_lds_bytes(p.np, cpw, fir_only, fs4, nw) > kPfLdsCap) return hipErrorInvalidValue;
    const int tile = (64 / cpw) * kPfR;
    const long long groups = ((long long)p.channels + cpw - 1) / cpw;
    const long long tiles = (p.n + tile - 1) / tile;
    // enough waves for two rounds of 16 per compute unit, no segment shorter than 4 tiles
    long long nseg = std::max<long long>(1, std::min<long long>((32LL * num_cus + groups - 1) / groups, tiles / 4));
    if (time_segments == 1) nseg = 1;
    else if (time_segments > 1) nseg = std::max<long long>(1, std::min<long long>(time_segments, tiles));
    const long long seg_tiles = (tiles + nseg - 1) / nseg;
    nseg = (tiles + seg_tiles - 1) / seg_tiles;
    p.nseg = (int)nseg; p.seg_len = seg_tiles * tile; p.nw = nw;
    const long long units = groups * nseg;
    const unsigned grid = (unsigned)((units + nw - 1) / nw), block = (unsigned)nw * 64;
    const size_t lds = f32pc_lds_bytes(p.np, cpw, fir_only, fs4, nw);
    switch (cpw) {
    case 4: pf_launch<4>(stream, fir_only, fs4, grid, block, lds, p); break;
    case 2: pf_launch<2>(stream, fir_only, fs4, grid, block, lds, p); break;
    default: pf_launch<1>(stream, fir_only, fs4, grid, block, lds, p); break;
    }
    if (geo) { geo->grid = grid; geo->block = block; geo->lds_bytes = lds; geo->cpw = cpw; geo->nseg = (int)nseg; geo->tile = tile; }
    return hipGetLastError();
}

}  // namespace msdr
