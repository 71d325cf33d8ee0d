// msdr_chain_decpc.hip -- the decimating chain kernels with a per-channel phase-accumulator oscillator and their launchers (a translation unit of its own).
#include "msdr_chain_decpc.hiph"
#include "msdr_block.h"
#include "msdr_pc_launch.h"

namespace msdr {

bool chain_dec_fits(bool f32, int np, int D) { return dec_fits(f32, np, D); }
int chain_dec_max(bool f32) { return dec_max_decimation(f32); }
int chain_dec_max_taps(bool f32, int D) { return dec_max_taps(f32, D); }

hipError_t launch_chain_q15pcnd(hipStream_t stream, int num_cus, PcndParams p, PcLaunch *geo)
{
    const int D = p.dec;          // (time_segments = 0: the Q15 chains do not look at the configuration's value)
    return dec_launch(stream, p, p.np > 0 && !(p.np & 7) && p.channels > 0 && p.n > 0 && p.mixer == kMixerNco && p.osc && p.sin_tab && !p.syncam_q && iq_ok(p, p.n / (D > 0 ? D : 1)), false, num_cus, 0,
                      (D & 1) ? 0 : (D % 8 == 0) ? 4 : (D % 4 == 0) ? 2 : 1,
                      [&](auto cpw, auto a) {
                          constexpr int CPW = decltype(cpw)::value, AL = decltype(a)::value;
                          if (p.iq) return p.meter ? chain_q15pcnd_iq_meter_kernel<CPW, AL> : chain_q15pcnd_iq_kernel<CPW, AL>;
                          return p.meter ? chain_q15pcnd_meter_kernel<CPW, AL> : chain_q15pcnd_kernel<CPW, AL>;
                      }, geo);
}

hipError_t launch_chain_f32pcnd(hipStream_t stream, int num_cus, int time_segments, PcfndParams p, PcLaunch *geo)
{
    const int D = p.dec;
    return dec_launch(stream, p, p.np > 0 && !(p.np & 3) && p.channels > 0 && p.n > 0 && p.mixer == kMixerNco && p.osc && p.sin_tab && iq_ok(p, p.n / (D > 0 ? D : 1)), true, num_cus, time_segments,
                      (D % 4 == 0) ? 4 : (D % 2 == 0) ? 2 : 1,
                      [&](auto cpw, auto a) {
                          constexpr int CPW = decltype(cpw)::value, AL = decltype(a)::value == 0 ? 1 : decltype(a)::value;          // (AL = 0 is Q15's)
                          if (p.iq) return p.meter ? chain_f32pcnd_iq_meter_kernel<CPW, AL> : chain_f32pcnd_iq_kernel<CPW, AL>;
                          return p.meter ? chain_f32pcnd_meter_kernel<CPW, AL> : chain_f32pcnd_kernel<CPW, AL>;
                      }, geo);
}

}  // namespace msdr
