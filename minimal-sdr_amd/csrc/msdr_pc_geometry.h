// msdr_pc_geometry.h -- launch geometry of the per-receiver chain kernels (chain_q15pc / chain_f32pc / chain_q15pco / chain_f32pco /
// chain_q15pcn / chain_f32pcn; its LDS-fitting step also of chain_f32pcb / chain_q15pcb): plain host C++, no HIP, so that the rule is testable on its own (tests/test_pc_geometry.py).
//
//   channels per wave   CPW = 4 for calls of up to 128 samples (the reference's block), 2 up to 256, else 1; a lane owns R consecutive outputs,
//                       so a channel's tile is R * 64 / CPW outputs
//   waves               4 per workgroup; halved, and then CPW halved, until the workgroup's LDS fits the cap (pc_fit_lds)
//   time segments       enough (channel group, segment) units for two rounds of 16 waves per compute unit, no segment shorter than 4 tiles;
//                       time_segments (msdr_chain_config.time_segments) overrides: 1 = never split, > 1 = that many as far as the call has
//                       tiles, 0 = the rule above.  Segments are whole tiles of equal count; empty ones are dropped.
#pragma once
#include <algorithm>
#include <cstddef>
#include <type_traits>

namespace msdr {

constexpr size_t kPcLdsCap = 64 * 1024;          // LDS of one workgroup of these kernels

struct PcLaunch { unsigned grid, block; size_t lds_bytes; int cpw, nseg, tile; };
struct PcGeometry { PcLaunch launch; long long seg_len; int nw; };          // seg_len / nw: what the kernels' parameter blocks carry besides nseg

// lds_bytes(cpw, nw): the LDS of a workgroup of nw waves with cpw channels each.  false: one wave with one channel does not fit.
template <typename LdsBytes>
inline bool pc_fit_lds(long long n, size_t cap, LdsBytes lds_bytes, int *cpw_out, int *nw_out)
{
    int cpw = n <= 128 ? 4 : n <= 256 ? 2 : 1, nw = 4;
    while ((size_t)lds_bytes(cpw, nw) > cap && nw > 1) nw >>= 1;
    while ((size_t)lds_bytes(cpw, nw) > cap && cpw > 1) cpw >>= 1;
    if ((size_t)lds_bytes(cpw, nw) > cap) return false;
    *cpw_out = cpw; *nw_out = nw;
    return true;
}

template <typename LdsBytes>
inline bool pc_geometry(long long n, int channels, int num_cus, int time_segments, int outs_per_lane, size_t cap, LdsBytes lds_bytes, PcGeometry *geo)
{
    int cpw = 0, nw = 0;
    if (n <= 0 || channels <= 0 || !pc_fit_lds(n, cap, lds_bytes, &cpw, &nw)) return false;
    const int tile = (64 / cpw) * outs_per_lane;
    const long long groups = ((long long)channels + cpw - 1) / cpw;
    const long long tiles = (n + tile - 1) / tile;
    long long nseg = std::max<long long>(1, std::min<long long>((32LL * num_cus + groups - 1) / groups, tiles / 4));
    if (time_segments == 1) nseg = 1;
    else if (time_segments > 1) nseg = std::max<long long>(1, std::min<long long>(time_segments, tiles));
    const long long seg_tiles = (tiles + nseg - 1) / nseg;
    nseg = (tiles + seg_tiles - 1) / seg_tiles;
    const long long units = groups * nseg;
    geo->launch = PcLaunch{(unsigned)((units + nw - 1) / nw), (unsigned)nw * 64, (size_t)lds_bytes(cpw, nw), cpw, (int)nseg, tile};
    geo->seg_len = seg_tiles * tile;
    geo->nw = nw;
    return true;
}

// f(std::integral_constant<int, CPW>) for the kernels' three instantiations
template <typename F>
inline void pc_dispatch_cpw(int cpw, F f)
{
    switch (cpw) {
    case 4: f(std::integral_constant<int, 4>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    default: f(std::integral_constant<int, 1>()); break;
    }
}

}  // namespace msdr
