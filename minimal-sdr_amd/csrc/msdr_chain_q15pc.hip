// msdr_chain_q15pc.hip -- the Q15 chain kernel with per-channel FIR coefficients and its launcher (a translation unit of its own).
#include "msdr_chain_q15pc.hiph"
#include "msdr_block.h"

namespace msdr {

hipError_t launch_chain_q15pc(hipStream_t stream, bool fir_only, int num_cus, PcParams p, PcLaunch *geo)
{
    if (p.np <= 0 || (p.np & 7) || p.channels <= 0 || p.n <= 0) return hipErrorInvalidValue;
    PcGeometry g;          // (time_segments = 0: the Q15 chains do not look at the configuration's value)
    if (!pc_geometry(p.n, p.channels, num_cus, 0, kPcR, kPcLdsCap, [&](int cpw, int nw) { return pc_lds_bytes(p.np, cpw, fir_only, nw); }, &g)) return hipErrorInvalidValue;
    p.nseg = g.launch.nseg; p.seg_len = g.seg_len; p.nw = g.nw;
    const PcLaunch &l = g.launch;
    pc_dispatch_cpw(l.cpw, [&](auto cpw) {
        if (fir_only) hipLaunchKernelGGL((chain_q15pc_kernel<decltype(cpw)::value, true>), dim3(l.grid), dim3(l.block), l.lds_bytes, stream, p);
        else hipLaunchKernelGGL((chain_q15pc_kernel<decltype(cpw)::value, false>), dim3(l.grid), dim3(l.block), l.lds_bytes, stream, p);
    });
    if (geo) *geo = l;
    return hipGetLastError();
}

}  // namespace msdr
