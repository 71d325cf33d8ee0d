// msdr_chain_q15pcb.hip -- the Q15 per-channel chain at block cadence in one launch and its launcher (a translation unit of its own).
#include "msdr_chain_q15pcb.hiph"
#include "msdr_block.h"

namespace msdr {

bool chain_q15pcb_lds(int n, int np, int osc_len, PcLaunch *geo)
{
    int cpw = 0, nw = 0;
    if (!qpcb_geometry(n, np, osc_len, &cpw, &nw)) return false;
    if (geo) { geo->grid = 0; geo->block = (unsigned)nw * 64; geo->lds_bytes = qpcb_lds_bytes(n, np, osc_len, cpw, nw); geo->cpw = cpw; geo->nseg = 1; geo->tile = (64 / cpw) * kPcR; }
    return true;
}

hipError_t launch_chain_q15pcb(hipStream_t stream, bool fs4, QpcbParams p, PcLaunch *geo)
{
    if (p.channels <= 0 || p.n < 8 || (p.n & 7) || p.hist_len < 0 || p.nnodes < 0 || p.nnodes > 2 || !p.x || !p.out || !p.hist_in || !p.hist_out ||
        p.hist_in == p.hist_out || !p.taps || !p.chan_mode || (p.nnodes > 0 && !p.defs0) || (p.nnodes > 1 && !p.defs1) ||
        (!fs4 && (p.osc_len <= 0 || !p.osc || (p.osc_stride != 0 && p.osc_stride != p.osc_len))))
        return hipErrorInvalidValue;
    PcLaunch g;
    if (!chain_q15pcb_lds(p.n, p.np, fs4 ? 0 : p.osc_len, &g)) return hipErrorInvalidValue;
    if (g.tile < p.n) return hipErrorInvalidValue;          // (a call is one tile)
    p.nw = (int)g.block / 64;
    const long long per_wg = (long long)g.cpw * p.nw;
    g.grid = (unsigned)(((long long)p.channels + per_wg - 1) / per_wg);
    pc_dispatch_cpw(g.cpw, [&](auto cpw) {
        if (fs4) hipLaunchKernelGGL((chain_q15pcb_kernel<decltype(cpw)::value, true>), dim3(g.grid), dim3(g.block), g.lds_bytes, stream, p);
        else hipLaunchKernelGGL((chain_q15pcb_kernel<decltype(cpw)::value, false>), dim3(g.grid), dim3(g.block), g.lds_bytes, stream, p);
    });
    if (geo) *geo = g;
    return hipGetLastError();
}

}  // namespace msdr
