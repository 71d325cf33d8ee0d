// msdr_chain_f32pc.hip -- the fp32 chain kernel with per-channel FIR coefficients and its launcher (a translation unit of its own).
#include "msdr_chain_f32pc.hiph"
#include "msdr_block.h"

namespace msdr {

hipError_t launch_chain_f32pc(hipStream_t stream, bool fir_only, int num_cus, int time_segments, PcfParams p, PcLaunch *geo)
{
    if (p.np <= 0 || (p.np & 3) || p.channels <= 0 || p.n <= 0) return hipErrorInvalidValue;
    const bool fs4 = !fir_only && p.mixer == kMixerFs4;
    PcGeometry g;
    if (!pc_geometry(p.n, p.channels, num_cus, time_segments, kPfR, kPcLdsCap, [&](int cpw, int nw) { return f32pc_lds_bytes(p.np, cpw, fir_only, fs4, nw); }, &g))
        return hipErrorInvalidValue;
    p.nseg = g.launch.nseg; p.seg_len = g.seg_len; p.nw = g.nw;
    const PcLaunch &l = g.launch;
    pc_dispatch_cpw(l.cpw, [&](auto cpw) {
        if (fir_only) hipLaunchKernelGGL((chain_f32pc_kernel<decltype(cpw)::value, true, false>), dim3(l.grid), dim3(l.block), l.lds_bytes, stream, p);
        else if (fs4) hipLaunchKernelGGL((chain_f32pc_kernel<decltype(cpw)::value, false, true>), dim3(l.grid), dim3(l.block), l.lds_bytes, stream, p);
        else hipLaunchKernelGGL((chain_f32pc_kernel<decltype(cpw)::value, false, false>), dim3(l.grid), dim3(l.block), l.lds_bytes, stream, p);
    });
    if (geo) *geo = l;
    return hipGetLastError();
}

}  // namespace msdr
