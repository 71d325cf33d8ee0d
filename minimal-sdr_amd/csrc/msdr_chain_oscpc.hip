// msdr_chain_oscpc.hip -- the chain kernels with per-channel oscillator tables and their launchers (a translation unit of its own).
#include <algorithm>
#include "msdr_chain_oscpc.hiph"
#include "msdr_block.h"

namespace msdr {

// launch geometry as launch_chain_q15pc / launch_chain_f32pc choose it: CPW by block length, fewer waves / channels per wave where LDS asks
hipError_t launch_chain_q15pco(hipStream_t stream, int num_cus, PcParams p, PcLaunch *geo)
{
    if (p.np <= 0 || (p.np & 7) || p.channels <= 0 || p.n <= 0 || p.osc_len <= 0 || p.mixer != kMixerNco || !p.osc) return hipErrorInvalidValue;
    int cpw = p.n <= 128 ? 4 : p.n <= 256 ? 2 : 1;
    int nw = 4;
    const size_t cap = 64 * 1024;
    while (pco_lds_bytes(p.np, p.osc_len, cpw, nw) > cap && nw > 1) nw >>= 1;
    while (pco_lds_bytes(p.np, p.osc_len, cpw, nw) > cap && cpw > 1) cpw >>= 1;
    if (pco_lds_bytes(p.np, p.osc_len, cpw, nw) > cap) return hipErrorInvalidValue;
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
    const size_t lds = pco_lds_bytes(p.np, p.osc_len, cpw, nw);
    switch (cpw) {
    case 4: hipLaunchKernelGGL((chain_q15pco_kernel<4>), dim3(grid), dim3(block), lds, stream, p); break;
    case 2: hipLaunchKernelGGL((chain_q15pco_kernel<2>), dim3(grid), dim3(block), lds, stream, p); break;
    default: hipLaunchKernelGGL((chain_q15pco_kernel<1>), dim3(grid), dim3(block), lds, stream, p); break;
    }
    if (geo) { geo->grid = grid; geo->block = block; geo->lds_bytes = lds; geo->cpw = cpw; geo->nseg = (int)nseg; geo->tile = tile; }
    return hipGetLastError();
}

hipError_t launch_chain_f32pco(hipStream_t stream, int num_cus, int time_segments, PcfParams p, PcLaunch *geo)
{
    if (p.np <= 0 || (p.np & 3) || p.channels <= 0 || p.n <= 0 || p.osc_len <= 0 || p.mixer != kMixerNco || !p.osc) return hipErrorInvalidValue;
    int cpw = p.n <= 128 ? 4 : p.n <= 256 ? 2 : 1;
    int nw = 4;
    while (f32pco_lds_bytes(p.np, p.osc_len, cpw, nw) > kPfLdsCap && nw > 1) nw >>= 1;
    while (f32pco_lds_bytes(p.np, p.osc_len, cpw, nw) > kPfLdsCap && cpw > 1) cpw >>= 1;
    if (f32pco_lds_bytes(p.np, p.osc_len, cpw, nw) > kPfLdsCap) return hipErrorInvalidValue;
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
    const size_t lds = f32pco_lds_bytes(p.np, p.osc_len, cpw, nw);
    switch (cpw) {
    case 4: hipLaunchKernelGGL((chain_f32pco_kernel<4>), dim3(grid), dim3(block), lds, stream, p); break;
    case 2: hipLaunchKernelGGL((chain_f32pco_kernel<2>), dim3(grid), dim3(block), lds, stream, p); break;
    default: hipLaunchKernelGGL((chain_f32pco_kernel<1>), dim3(grid), dim3(block), lds, stream, p); break;
    }
    if (geo) { geo->grid = grid; geo->block = block; geo->lds_bytes = lds; geo->cpw = cpw; geo->nseg = (int)nseg; geo->tile = tile; }
    return hipGetLastError();
}

}  // namespace msdr
