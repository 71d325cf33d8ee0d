// msdr_chain_ncopc.hip -- the chain kernels with a per-channel phase-accumulator oscillator and their launchers (a translation unit of its own).
#include "msdr_chain_ncopc.hiph"
#include "msdr_block.h"
#include "msdr_pc_launch.h"

namespace msdr {

int chain_pcn_max_taps(bool f32) { return f32 ? f32pcn_max_taps() : pcn_max_taps(); }

// launch geometry as launch_chain_q15pc / launch_chain_f32pc choose it (pc_geometry), with the sine table's LDS counted in
hipError_t launch_chain_q15pcn(hipStream_t stream, int num_cus, PcnParams p, PcLaunch *geo)
{
    return pc_launch(stream, p, p.np > 0 && !(p.np & 7) && p.channels > 0 && p.n > 0 && p.mixer == kMixerNco && p.osc && p.sin_tab && iq_ok(p, p.n), num_cus, 0, kPcR,
                     [&](int cpw, int nw) { return pcn_lds_bytes(p.np, cpw, nw); },
                     [&](auto cpw) {
                         constexpr int CPW = decltype(cpw)::value;
                         if (p.iq) return p.meter ? chain_q15pcn_iq_meter_kernel<CPW> : chain_q15pcn_iq_kernel<CPW>;
                         return p.meter ? chain_q15pcn_meter_kernel<CPW> : chain_q15pcn_kernel<CPW>;
                     }, geo);
}

hipError_t launch_chain_f32pcn(hipStream_t stream, int num_cus, int time_segments, PcfnParams p, PcLaunch *geo)
{
    return pc_launch(stream, p, p.np > 0 && !(p.np & 3) && p.channels > 0 && p.n > 0 && p.mixer == kMixerNco && p.osc && p.sin_tab && iq_ok(p, p.n), num_cus, time_segments, kPfR,
                     [&](int cpw, int nw) { return f32pcn_lds_bytes(p.np, cpw, nw); },
                     [&](auto cpw) {
                         constexpr int CPW = decltype(cpw)::value;
                         if (p.iq) return p.meter ? chain_f32pcn_iq_meter_kernel<CPW> : chain_f32pcn_iq_kernel<CPW>;
                         return p.meter ? chain_f32pcn_meter_kernel<CPW> : chain_f32pcn_kernel<CPW>;
                     }, geo);
}

}  // namespace msdr
