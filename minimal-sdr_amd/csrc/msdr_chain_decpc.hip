// msdr_chain_decpc.hip -- the decimating chain kernels with a per-channel phase-accumulator oscillator and their launchers (a translation unit of its own).
#include "msdr_chain_decpc.hiph"
#include "msdr_block.h"
#include "msdr_pc_launch.h"

namespace msdr {

bool chain_dec_fits(bool f32, int np, int D) { return dec_fits(f32, np, D); }
int chain_dec_max(bool f32) { return dec_max_decimation(f32); }
int chain_dec_max_taps(bool f32, int D) { return dec_max_taps(f32, D); }

// f(std::integral_constant<int, AL>) for the kernels' read widths
template <typename F>
static auto dec_dispatch_al(int al, F f)
{
    switch (al) {
    case 4: return f(std::integral_constant<int, 4>());
    case 2: return f(std::integral_constant<int, 2>());
    case 1: return f(std::integral_constant<int, 1>());
    default: return f(std::integral_constant<int, 0>());
    }
}

// pc_launch for the decimating pair: launch geometry from dec_geometry (msdr_decpc_geometry.h), everything in outputs; p.nout and p.opl
// beside the fields every parameter block carries.  kernel_of(CPW, AL): the instantiation for the read width al.
template <typename P, typename KernelOf>
static hipError_t dec_launch(hipStream_t stream, P &p, bool valid, bool f32, int num_cus, int time_segments, int al, KernelOf kernel_of, PcLaunch *geo)
{
    if (!valid || p.dec < 2 || p.n % p.dec) return hipErrorInvalidValue;
    p.nout = p.n / p.dec;
    DecGeometry g;
    const bool ok = dec_geometry(p.nout, p.channels, num_cus, time_segments, kPcLdsCap, [&](int cpw, int nw, int opl) { return dec_lds_bytes(f32, p.np, p.dec, cpw, nw, opl); }, &g);
    if (ok) p.opl = g.opl;
    return pc_launch_geometry(stream, p, ok, g, [&](auto cpw) { return dec_dispatch_al(al, [&](auto a) { return kernel_of(cpw, a); }); }, geo);
}

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
