// msdr_chain_pre.hip -- the two-stage decimating chain kernels (a chain-wide prefilter in front of the per-receiver channel pair) and their
// launchers (a translation unit of its own; msdr_chain_pre.hiph).
#include "msdr_chain_pre.hiph"
#include "msdr_block.h"
#include "msdr_pc_launch.h"

namespace msdr {

bool chain_pre_fits(bool f32, int np1, int D1, int np2, int D2) { return pre_fits(f32, np1, D1, np2, D2); }
int chain_pre_hist_len(int np1, int D1, int np2) { return pre_hist_len(np1, D1, np2); }

// what follows a launcher's own validation: geometry over final outputs, the fields the kernels read of it, the instantiation for the
// channels per wave and the second stage's read width al
template <typename P, typename KernelOf>
static hipError_t pre_launch(hipStream_t stream, P &p, bool valid, bool f32, int num_cus, int time_segments, int al, KernelOf kernel_of, PcLaunch *geo)
{
    if (!valid || !pre_factor_ok(p.pre_dec) || p.dec < 1 || p.n % ((long long)p.pre_dec * p.dec) || p.hist_len < pre_hist_len(p.pre_np, p.pre_dec, p.np)) return hipErrorInvalidValue;
    p.nout = p.n / ((long long)p.pre_dec * p.dec);
    if (!iq_ok(p, p.nout)) return hipErrorInvalidValue;
    DecGeometry g;
    const bool ok = pre_geometry(f32, p.nout, p.channels, num_cus, time_segments, p.pre_np, p.pre_dec, p.np, p.dec, &g);
    if (ok) { p.opl = g.opl; p.pre_chunk = pre_chunk(p.pre_dec, g.launch.cpw); }
    return pc_launch_geometry(stream, p, ok, g, [&](auto cpw) { return dec_dispatch_al(al, [&](auto a) { return kernel_of(cpw, a); }); }, geo);
}

hipError_t launch_chain_q15pcn2(hipStream_t stream, int num_cus, Pcn2Params p, PcLaunch *geo)
{
    const int D = p.dec;          // (time_segments = 0: the Q15 chains do not look at the configuration's value)
    const bool full = p.meter || p.iq || p.agc;
    return pre_launch(stream, p, p.np > 0 && !(p.np & 7) && p.pre_np > 0 && !(p.pre_np & 7) && p.pre_taps && p.channels > 0 && p.n > 0 && p.mixer == kMixerNco && p.osc && p.sin_tab && !p.syncam_q, false, num_cus, 0,
                      (D & 1) ? 0 : (D % 8 == 0) ? 4 : (D % 4 == 0) ? 2 : 1,
                      [&](auto cpw, auto a) {
                          constexpr int CPW = decltype(cpw)::value, AL = decltype(a)::value;
                          return full ? chain_q15pcn2_full_kernel<CPW, AL> : chain_q15pcn2_kernel<CPW, AL>;
                      }, geo);
}

hipError_t launch_chain_f32pcn2(hipStream_t stream, int num_cus, int time_segments, Pcfn2Params p, PcLaunch *geo)
{
    const int D = p.dec;
    const bool full = p.meter || p.iq || p.agc;
    return pre_launch(stream, p, p.np > 0 && !(p.np & 3) && p.pre_np > 0 && !(p.pre_np & 3) && p.pre_taps && p.channels > 0 && p.n > 0 && p.mixer == kMixerNco && p.osc && p.sin_tab, true, num_cus, time_segments,
                      (D % 4 == 0) ? 4 : (D % 2 == 0) ? 2 : 1,
                      [&](auto cpw, auto a) {
                          constexpr int CPW = decltype(cpw)::value, AL = decltype(a)::value == 0 ? 1 : decltype(a)::value;          // (AL = 0 is Q15's)
                          return full ? chain_f32pcn2_full_kernel<CPW, AL> : chain_f32pcn2_kernel<CPW, AL>;
                      }, geo);
}

}  // namespace msdr
