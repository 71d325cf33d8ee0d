// msdr_chain_oscpc.hip -- the chain kernels with per-channel oscillator tables and their launchers (a translation unit of its own).
#include "msdr_chain_oscpc.hiph"
#include "msdr_block.h"
#include "msdr_pc_launch.h"

namespace msdr {

// launch geometry as launch_chain_q15pc / launch_chain_f32pc choose it (pc_geometry), with the row's LDS counted in
hipError_t launch_chain_q15pco(hipStream_t stream, int num_cus, PcParams p, PcLaunch *geo)
{
    return pc_launch(stream, p, p.np > 0 && !(p.np & 7) && p.channels > 0 && p.n > 0 && p.osc_len > 0 && p.mixer == kMixerNco && p.osc, num_cus, 0, kPcR,
                     [&](int cpw, int nw) { return pco_lds_bytes(p.np, p.osc_len, cpw, nw); },
                     [&](auto cpw) { return p.meter ? chain_q15pco_meter_kernel<decltype(cpw)::value> : chain_q15pco_kernel<decltype(cpw)::value>; }, geo);
}

hipError_t launch_chain_f32pco(hipStream_t stream, int num_cus, int time_segments, PcfParams p, PcLaunch *geo)
{
    return pc_launch(stream, p, p.np > 0 && !(p.np & 3) && p.channels > 0 && p.n > 0 && p.osc_len > 0 && p.mixer == kMixerNco && p.osc, num_cus, time_segments, kPfR,
                     [&](int cpw, int nw) { return f32pco_lds_bytes(p.np, p.osc_len, cpw, nw); },
                     [&](auto cpw) { return p.meter ? chain_f32pco_meter_kernel<decltype(cpw)::value> : chain_f32pco_kernel<decltype(cpw)::value>; }, geo);
}

}  // namespace msdr
