// msdr_chain_ncopc.hip -- the chain kernels with a per-channel phase-accumulator oscillator and their launchers (a translation unit of its own).
#include "msdr_chain_ncopc.hiph"
#include "msdr_block.h"

namespace msdr {

int chain_pcn_max_taps(bool f32) { return f32 ? f32pcn_max_taps() : pcn_max_taps(); }

// launch geometry as launch_chain_q15pc / launch_chain_f32pc choose it (pc_geometry), with the sine table's LDS counted in
hipError_t launch_chain_q15pcn(hipStream_t stream, int num_cus, PcnParams p, PcLaunch *geo)
{
    if (p.np <= 0 || (p.np & 7) || p.channels <= 0 || p.n <= 0 || p.mixer != kMixerNco || !p.osc || !p.sin_tab) return hipErrorInvalidValue;
    PcGeometry g;          // (time_segments = 0: the Q15 chains do not look at the configuration's value)
    if (!pc_geometry(p.n, p.channels, num_cus, 0, kPcR, kPcLdsCap, [&](int cpw, int nw) { return pcn_lds_bytes(p.np, cpw, nw); }, &g)) return hipErrorInvalidValue;
    p.nseg = g.launch.nseg; p.seg_len = g.seg_len; p.nw = g.nw;
    const PcLaunch &l = g.launch;
    pc_dispatch_cpw(l.cpw, [&](auto cpw) { hipLaunchKernelGGL((chain_q15pcn_kernel<decltype(cpw)::value>), dim3(l.grid), dim3(l.block), l.lds_bytes, stream, p); });
    if (geo) *geo = l;
    return hipGetLastError();
}

hipError_t launch_chain_f32pcn(hipStream_t stream, int num_cus, int time_segments, PcfnParams p, PcLaunch *geo)
{
    if (p.np <= 0 || (p.np & 3) || p.channels <= 0 || p.n <= 0 || p.mixer != kMixerNco || !p.osc || !p.sin_tab) return hipErrorInvalidValue;
    PcGeometry g;
    if (!pc_geometry(p.n, p.channels, num_cus, time_segments, kPfR, kPcLdsCap, [&](int cpw, int nw) { return f32pcn_lds_bytes(p.np, cpw, nw); }, &g))
        return hipErrorInvalidValue;
    p.nseg = g.launch.nseg; p.seg_len = g.seg_len; p.nw = g.nw;
    const PcLaunch &l = g.launch;
    pc_dispatch_cpw(l.cpw, [&](auto cpw) { hipLaunchKernelGGL((chain_f32pcn_kernel<decltype(cpw)::value>), dim3(l.grid), dim3(l.block), l.lds_bytes, stream, p); });
    if (geo) *geo = l;
    return hipGetLastError();
}

}  // namespace msdr
