// msdr_chain_f32pcb.hip -- the fp32 per-channel chain at block cadence in one launch and its launcher (a translation unit of its own).
#include "msdr_chain_f32pcb.hiph"
#include "msdr_block.h"

namespace msdr {

bool chain_f32pcb_lds(int n, int np, int osc_len, PcLaunch *geo)
{
    int cpw = 0, nw = 0;
    if (!f32pcb_geometry(n, np, osc_len, &cpw, &nw)) return false;
    if (geo) { geo->grid = 0; geo->block = (unsigned)nw * 64; geo->lds_bytes = f32pcb_lds_bytes(np, osc_len, cpw, nw); geo->cpw = cpw; geo->nseg = 1; geo->tile = (64 / cpw) * kPfR; }
    return true;
}

hipError_t launch_chain_f32pcb(hipStream_t stream, bool fs4, PcbParams p, PcLaunch *geo)
{
    if (p.channels <= 0 || p.n < 8 || (p.n & 7) || p.hist_len < 0 || p.stages < 0 || p.stages > kMaxStages || !p.x || !p.out || !p.hist_in || !p.hist_out ||
        p.hist_in == p.hist_out || !p.taps || !p.chan_mode || (p.stages && (!p.bq_tab || !p.bq_state)) || (!fs4 && (p.osc_len <= 0 || !p.osc)))
        return hipErrorInvalidValue;
    PcLaunch g;
    if (!chain_f32pcb_lds(p.n, p.np, fs4 ? 0 : p.osc_len, &g)) return hipErrorInvalidValue;
    if (g.tile < p.n) return hipErrorInvalidValue;          // (a call is one tile)
    p.nw = (int)g.block / 64;
    const long long per_wg = (long long)g.cpw * p.nw;
    g.grid = (unsigned)(((long long)p.channels + per_wg - 1) / per_wg);
    pc_dispatch_cpw(g.cpw, [&](auto cpw) {
        if (fs4) hipLaunchKernelGGL((chain_f32pcb_kernel<decltype(cpw)::value, true>), dim3(g.grid), dim3(g.block), g.lds_bytes, stream, p);
        else hipLaunchKernelGGL((chain_f32pcb_kernel<decltype(cpw)::value, false>), dim3(g.grid), dim3(g.block), g.lds_bytes, stream, p);
    });
    if (geo) *geo = g;
    return hipGetLastError();
}

}  // namespace msdr
