// msdr_chain_q15pc.hip -- the Q15 chain kernel with per-channel FIR coefficients and its launcher (a translation unit of its own).
#include <algorithm>
#include "msdr_chain_q15pc.hiph"
#include "msdr_block.h"

namespace msdr {

template <int CPW>
static void pc_launch(hipStream_t stream, bool fir_only, unsigned grid, unsigned block, size_t lds, const PcParams &p)
{
    if (fir_only) hipLaunchKernelGGL((chain_q15pc_kernel<CPW, true>), dim3(grid), dim3(block), lds, stream, p);
    else hipLaunchKernelGGL((chain_q15pc_kernel<CPW, false>), dim3(grid), dim3(block), lds, stream, p);
}

hipError_t launch_chain_q15pc(hipStream_t stream, bool fir_only, int num_cus, PcParams p, PcLaunch *geo)
{
    if (p.np <= 0 || (p.np & 7) || p.channels <= 0 || p.n <= 0) return hipErrorInvalidValue;
    int cpw = p.n <= 128 ? 4 : p.n <= 256 ? 2 : 1;
    int nw = 4;
    const size_t cap = 64 * 1024;
    while (pc_lds_bytes(p.np, cpw, fir_only, nw) > cap && nw > 1) nw >>= 1;
    while (pc_lds_bytes(p.np, cpw, fir_only, nw) > cap && cpw > 1) cpw >>= 1;
    if (pc_lds_bytes(p.np, cpw, fir_only, nw) > cap) return hipErrorInvalidValue;
    const int tile = (64 / cpw) * kPcR;
    const long long groups = ((long long)p.channels + cpw - 1) / cpw;
    const long long tiles = (p.n + tile - 1) / tile;
    // enough waves for two rounds of 16 per compute unit, no segment shorter than 4 tiles
    long long nseg = std::max<long long>(1, std::min<long long>((32LL * num_cus + groups - 1) / groups, tiles / 4));
    const long long seg_tiles = (tiles + nseg - 1) / nseg;
    nseg = (tiles + seg_tiles - 1) / seg_tiles;
    p.nseg = (int)nseg; p.seg_len = seg_tiles * tile; p.nw = nw;
    const long long units = groups * nseg;
    const unsigned grid = (unsigned)((units + nw - 1) / nw), block = (unsigned)nw * 64;
    const size_t lds = pc_lds_bytes(p.np, cpw, fir_only, nw);
    switch (cpw) {
    case 4: pc_launch<4>(stream, fir_only, grid, block, lds, p); break;
    case 2: pc_launch<2>(stream, fir_only, grid, block, lds, p); break;
    default: pc_launch<1>(stream, fir_only, grid, block, lds, p); break;
    }
    if (geo) { geo->grid = grid; geo->block = block; geo->lds_bytes = lds; geo->cpw = cpw; geo->nseg = (int)nseg; geo->tile = tile; }
    return hipGetLastError();
}

}  // namespace msdr
