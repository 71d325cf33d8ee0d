// msdr_chain_gncopc.hip -- the gain twins of the phase-accumulator chain kernels (real and complex input) and their launchers (a translation
// unit of its own; msdr_chain_gain.hiph).
#include "msdr_chain_cxpc.hiph"
#include "msdr_block.h"
#include "msdr_pc_launch.h"

namespace msdr {

// ---- the sliding-window twins: one per family and input, the superset of the plain, metered and I/Q bodies ------------------------------------------
// (an occupancy attribute of their own: the superset body must not be squeezed into the 128 registers of four waves per SIMD)
template <int CPW>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(kGainWavesPerEu))) void chain_q15pcn_gain_kernel(const PcnGainParams p) { pc_frame<CPW, false, PcOscPhase, true, true, true>(p); }
template <int CPW>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(kGainWavesPerEu))) void chain_q15pcn_cx_gain_kernel(const PcnGainParams p) { pc_frame<CPW, false, PcOscPhaseCx, true, true, true>(p); }
template <int CPW>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(kGainWavesPerEu))) void chain_f32pcn_gain_kernel(const PcfnGainParams p) { pf_frame<CPW, false, false, PfOscPhase, true, true, true>(p); }
template <int CPW>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(kGainWavesPerEu))) void chain_f32pcn_cx_gain_kernel(const PcfnGainParams p) { pf_frame<CPW, false, false, PfOscPhaseCx, true, true, true>(p); }

// validation, geometry and LDS as launch_chain_q15pcn[_cx] / launch_chain_f32pcn[_cx] have them; cx: rows of pairs
hipError_t launch_chain_q15pcn_gain(hipStream_t stream, int num_cus, bool cx, PcnGainParams p, PcLaunch *geo)
{
    return pc_launch(stream, p, p.np > 0 && !(p.np & 7) && p.channels > 0 && p.n > 0 && p.mixer == kMixerNco && p.osc && p.sin_tab && p.agc && iq_ok(p, p.n) && (!cx || cx_ok(p.x, p.hist_in, p.cx_dir)), num_cus, 0, kPcR,
                     [&](int cpw, int nw) { return pcn_lds_bytes(p.np, cpw, nw); },
                     [&](auto cpw) {
                         constexpr int CPW = decltype(cpw)::value;
                         return cx ? chain_q15pcn_cx_gain_kernel<CPW> : chain_q15pcn_gain_kernel<CPW>;
                     }, geo);
}

hipError_t launch_chain_f32pcn_gain(hipStream_t stream, int num_cus, int time_segments, bool cx, PcfnGainParams p, PcLaunch *geo)
{
    return pc_launch(stream, p, p.np > 0 && !(p.np & 3) && p.channels > 0 && p.n > 0 && p.mixer == kMixerNco && p.osc && p.sin_tab && p.agc && iq_ok(p, p.n) && (!cx || cx_ok(p.x, p.hist_in, p.cx_dir)), num_cus, time_segments, kPfR,
                     [&](int cpw, int nw) { return f32pcn_lds_bytes(p.np, cpw, nw); },
                     [&](auto cpw) {
                         constexpr int CPW = decltype(cpw)::value;
                         return cx ? chain_f32pcn_cx_gain_kernel<CPW> : chain_f32pcn_gain_kernel<CPW>;
                     }, geo);
}

}  // namespace msdr
