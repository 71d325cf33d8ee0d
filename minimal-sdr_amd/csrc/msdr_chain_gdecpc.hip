// msdr_chain_gdecpc.hip -- the gain twins of the decimating chain kernels (real and complex input) and their launchers (a translation unit of
// its own; msdr_chain_gain.hiph).
#include "msdr_chain_cxpc.hiph"
#include "msdr_block.h"
#include "msdr_pc_launch.h"

namespace msdr {

// one per family, input, CPW and read width: the superset of the plain, metered and I/Q bodies, under an occupancy attribute of its own (the
// iq_meter instantiations fill the 128 registers of four waves per SIMD without the gain's multiplier, peak and products)
template <int CPW, int AL>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(kGainWavesPerEu))) void chain_q15pcnd_gain_kernel(const PcndGainParams p) { dec_frame_q15<CPW, AL, true, true, PcOscPhase, true>(p); }
template <int CPW, int AL>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(kGainWavesPerEu))) void chain_q15pcnd_cx_gain_kernel(const PcndGainParams p) { dec_frame_q15<CPW, AL, true, true, PcOscPhaseCx, true>(p); }
template <int CPW, int AL>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(kGainWavesPerEu))) void chain_f32pcnd_gain_kernel(const PcfndGainParams p) { dec_frame_f32<CPW, AL, true, true, PfOscPhase, true>(p); }
template <int CPW, int AL>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(kGainWavesPerEu))) void chain_f32pcnd_cx_gain_kernel(const PcfndGainParams p) { dec_frame_f32<CPW, AL, true, true, PfOscPhaseCx, true>(p); }

// validation, read widths, geometry and LDS as launch_chain_q15pcnd[_cx] / launch_chain_f32pcnd[_cx] have them; cx: rows of pairs
hipError_t launch_chain_q15pcnd_gain(hipStream_t stream, int num_cus, bool cx, PcndGainParams p, PcLaunch *geo)
{
    const int D = p.dec;
    return dec_launch(stream, p, p.np > 0 && !(p.np & 7) && p.channels > 0 && p.n > 0 && p.mixer == kMixerNco && p.osc && p.sin_tab && p.agc && !p.syncam_q && iq_ok(p, p.n / (D > 0 ? D : 1)) && (!cx || cx_ok(p.x, p.hist_in, p.cx_dir)), false, num_cus, 0,
                      (D & 1) ? 0 : (D % 8 == 0) ? 4 : (D % 4 == 0) ? 2 : 1,
                      [&](auto cpw, auto a) {
                          constexpr int CPW = decltype(cpw)::value, AL = decltype(a)::value;
                          return cx ? chain_q15pcnd_cx_gain_kernel<CPW, AL> : chain_q15pcnd_gain_kernel<CPW, AL>;
                      }, geo);
}

hipError_t launch_chain_f32pcnd_gain(hipStream_t stream, int num_cus, int time_segments, bool cx, PcfndGainParams p, PcLaunch *geo)
{
    const int D = p.dec;
    return dec_launch(stream, p, p.np > 0 && !(p.np & 3) && p.channels > 0 && p.n > 0 && p.mixer == kMixerNco && p.osc && p.sin_tab && p.agc && iq_ok(p, p.n / (D > 0 ? D : 1)) && (!cx || cx_ok(p.x, p.hist_in, p.cx_dir)), true, num_cus, time_segments,
                      (D % 4 == 0) ? 4 : (D % 2 == 0) ? 2 : 1,
                      [&](auto cpw, auto a) {
                          constexpr int CPW = decltype(cpw)::value, AL = decltype(a)::value == 0 ? 1 : decltype(a)::value;          // (AL = 0 is Q15's)
                          return cx ? chain_f32pcnd_cx_gain_kernel<CPW, AL> : chain_f32pcnd_gain_kernel<CPW, AL>;
                      }, geo);
}

}  // namespace msdr
