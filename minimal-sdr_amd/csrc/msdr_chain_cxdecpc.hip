// msdr_chain_cxdecpc.hip -- the complex-input twins of the decimating chain kernels and their launchers (a translation unit of its own).
#include "msdr_chain_cxpc.hiph"
#include "msdr_block.h"
#include "msdr_pc_launch.h"

namespace msdr {

// validation, read widths, geometry and LDS as launch_chain_q15pcnd / launch_chain_f32pcnd have them
hipError_t launch_chain_q15pcnd_cx(hipStream_t stream, int num_cus, PcndCxParams p, PcLaunch *geo)
{
    const int D = p.dec;
    return dec_launch(stream, p, p.np > 0 && !(p.np & 7) && p.channels > 0 && p.n > 0 && p.mixer == kMixerNco && p.osc && p.sin_tab && !p.syncam_q && iq_ok(p, p.n / (D > 0 ? D : 1)) && cx_ok(p.x, p.hist_in, p.cx_dir), false, num_cus, 0,
                      (D & 1) ? 0 : (D % 8 == 0) ? 4 : (D % 4 == 0) ? 2 : 1,
                      [&](auto cpw, auto a) {
                          constexpr int CPW = decltype(cpw)::value, AL = decltype(a)::value;
                          if (p.iq) return p.meter ? chain_q15pcnd_cx_iq_meter_kernel<CPW, AL> : chain_q15pcnd_cx_iq_kernel<CPW, AL>;
                          return p.meter ? chain_q15pcnd_cx_meter_kernel<CPW, AL> : chain_q15pcnd_cx_kernel<CPW, AL>;
                      }, geo);
}

hipError_t launch_chain_f32pcnd_cx(hipStream_t stream, int num_cus, int time_segments, PcfndCxParams p, PcLaunch *geo)
{
    const int D = p.dec;
    return dec_launch(stream, p, p.np > 0 && !(p.np & 3) && p.channels > 0 && p.n > 0 && p.mixer == kMixerNco && p.osc && p.sin_tab && iq_ok(p, p.n / (D > 0 ? D : 1)) && cx_ok(p.x, p.hist_in, p.cx_dir), true, num_cus, time_segments,
                      (D % 4 == 0) ? 4 : (D % 2 == 0) ? 2 : 1,
                      [&](auto cpw, auto a) {
                          constexpr int CPW = decltype(cpw)::value, AL = decltype(a)::value == 0 ? 1 : decltype(a)::value;          // (AL = 0 is Q15's)
                          if (p.iq) return p.meter ? chain_f32pcnd_cx_iq_meter_kernel<CPW, AL> : chain_f32pcnd_cx_iq_kernel<CPW, AL>;
                          return p.meter ? chain_f32pcnd_cx_meter_kernel<CPW, AL> : chain_f32pcnd_cx_kernel<CPW, AL>;
                      }, geo);
}

}  // namespace msdr
