// msdr_chain_cxncopc.hip -- the complex-input twins of the phase-accumulator chain kernels and their launchers (a translation unit of its own).
#include "msdr_chain_cxpc.hiph"
#include "msdr_block.h"
#include "msdr_pc_launch.h"

namespace msdr {

// validation, geometry and LDS as launch_chain_q15pcn / launch_chain_f32pcn have them; rows of pairs are dwords
hipError_t launch_chain_q15pcn_cx(hipStream_t stream, int num_cus, PcnCxParams p, PcLaunch *geo)
{
    return pc_launch(stream, p, p.np > 0 && !(p.np & 7) && p.channels > 0 && p.n > 0 && p.mixer == kMixerNco && p.osc && p.sin_tab && iq_ok(p, p.n) && cx_ok(p.x, p.hist_in, p.cx_dir), num_cus, 0, kPcR,
                     [&](int cpw, int nw) { return pcn_lds_bytes(p.np, cpw, nw); },
                     [&](auto cpw) {
                         constexpr int CPW = decltype(cpw)::value;
                         if (p.iq) return p.meter ? chain_q15pcn_cx_iq_meter_kernel<CPW> : chain_q15pcn_cx_iq_kernel<CPW>;
                         return p.meter ? chain_q15pcn_cx_meter_kernel<CPW> : chain_q15pcn_cx_kernel<CPW>;
                     }, geo);
}

hipError_t launch_chain_f32pcn_cx(hipStream_t stream, int num_cus, int time_segments, PcfnCxParams p, PcLaunch *geo)
{
    return pc_launch(stream, p, p.np > 0 && !(p.np & 3) && p.channels > 0 && p.n > 0 && p.mixer == kMixerNco && p.osc && p.sin_tab && iq_ok(p, p.n) && cx_ok(p.x, p.hist_in, p.cx_dir), num_cus, time_segments, kPfR,
                     [&](int cpw, int nw) { return f32pcn_lds_bytes(p.np, cpw, nw); },
                     [&](auto cpw) {
                         constexpr int CPW = decltype(cpw)::value;
                         if (p.iq) return p.meter ? chain_f32pcn_cx_iq_meter_kernel<CPW> : chain_f32pcn_cx_iq_kernel<CPW>;
                         return p.meter ? chain_f32pcn_cx_meter_kernel<CPW> : chain_f32pcn_cx_kernel<CPW>;
                     }, geo);
}

}  // namespace msdr
