// msdr_chain_decpc.hip -- the decimating chain kernels with a per-channel phase-accumulator oscillator and their launchers (a translation unit of its own).
#include "msdr_chain_decpc.hiph"
#include "msdr_block.h"

namespace msdr {

bool chain_dec_fits(bool f32, int np, int D) { return dec_fits(f32, np, D); }
int chain_dec_max(bool f32) { return dec_max_decimation(f32); }
int chain_dec_max_taps(bool f32, int D) { return dec_max_taps(f32, D); }

// f(std::integral_constant<int, AL>) for the kernels' read widths
template <typename F>
static void dec_dispatch_al(int al, F f)
{
    switch (al) {
    case 4: f(std::integral_constant<int, 4>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 1: f(std::integral_constant<int, 1>()); break;
    default: f(std::integral_constant<int, 0>()); break;
    }
}

// launch geometry from dec_geometry (msdr_decpc_geometry.h): everything in outputs
hipError_t launch_chain_q15pcnd(hipStream_t stream, int num_cus, PcndParams p, PcLaunch *geo)
{
    if (p.np <= 0 || (p.np & 7) || p.channels <= 0 || p.n <= 0 || p.mixer != kMixerNco || !p.osc || !p.sin_tab || p.syncam_q) return hipErrorInvalidValue;
    if (p.dec < 2 || p.n % p.dec) return hipErrorInvalidValue;
    p.nout = p.n / p.dec;
    const int D = p.dec;
    DecGeometry g;          // (time_segments = 0: the Q15 chains do not look at the configuration's value)
    if (!dec_geometry(p.nout, p.channels, num_cus, 0, kPcLdsCap, [&](int cpw, int nw, int opl) { return dec_q15_lds_bytes(p.np, D, cpw, nw, opl); }, &g))
        return hipErrorInvalidValue;
    p.nseg = g.launch.nseg; p.seg_len = g.seg_len; p.nw = g.nw; p.opl = g.opl;
    const PcLaunch &l = g.launch;
    const int al = (D & 1) ? 0 : (D % 8 == 0) ? 4 : (D % 4 == 0) ? 2 : 1;
    pc_dispatch_cpw(l.cpw, [&](auto cpw) {
        dec_dispatch_al(al, [&](auto a) {
            hipLaunchKernelGGL((chain_q15pcnd_kernel<decltype(cpw)::value, decltype(a)::value>), dim3(l.grid), dim3(l.block), l.lds_bytes, stream, p);
        });
    });
    if (geo) *geo = l;
    return hipGetLastError();
}

hipError_t launch_chain_f32pcnd(hipStream_t stream, int num_cus, int time_segments, PcfndParams p, PcLaunch *geo)
{
    if (p.np <= 0 || (p.np & 3) || p.channels <= 0 || p.n <= 0 || p.mixer != kMixerNco || !p.osc || !p.sin_tab) return hipErrorInvalidValue;
    if (p.dec < 2 || p.n % p.dec) return hipErrorInvalidValue;
    p.nout = p.n / p.dec;
    const int D = p.dec;
    DecGeometry g;
    if (!dec_geometry(p.nout, p.channels, num_cus, time_segments, kPcLdsCap, [&](int cpw, int nw, int opl) { return dec_f32_lds_bytes(p.np, D, cpw, nw, opl); }, &g))
        return hipErrorInvalidValue;
    p.nseg = g.launch.nseg; p.seg_len = g.seg_len; p.nw = g.nw; p.opl = g.opl;
    const PcLaunch &l = g.launch;
    const int al = (D % 4 == 0) ? 4 : (D % 2 == 0) ? 2 : 1;
    pc_dispatch_cpw(l.cpw, [&](auto cpw) {
        dec_dispatch_al(al, [&](auto a) {
            if constexpr (decltype(a)::value != 0)
                hipLaunchKernelGGL((chain_f32pcnd_kernel<decltype(cpw)::value, decltype(a)::value>), dim3(l.grid), dim3(l.block), l.lds_bytes, stream, p);
        });
    });
    if (geo) *geo = l;
    return hipGetLastError();
}

}  // namespace msdr
