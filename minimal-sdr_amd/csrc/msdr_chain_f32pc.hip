// msdr_chain_f32pc.hip -- the fp32 chain kernel with per-channel FIR coefficients and its launcher (a translation unit of its own).
#include "msdr_chain_f32pc.hiph"
#include "msdr_block.h"
#include "msdr_pc_launch.h"

namespace msdr {

hipError_t launch_chain_f32pc(hipStream_t stream, bool fir_only, int num_cus, int time_segments, PcfParams p, PcLaunch *geo)
{
    const bool fs4 = !fir_only && p.mixer == kMixerFs4;
    if (fir_only) p.meter = nullptr;          // (the meter measures a chain's I and Q)
    return pc_launch(stream, p, p.np > 0 && !(p.np & 3) && p.channels > 0 && p.n > 0, num_cus, time_segments, kPfR,
                     [&](int cpw, int nw) { return f32pc_lds_bytes(p.np, cpw, fir_only, fs4, nw); },
                     [&](auto cpw) {
                         constexpr int CPW = decltype(cpw)::value;
                         if (p.meter) return fs4 ? chain_f32pc_meter_kernel<CPW, true> : chain_f32pc_meter_kernel<CPW, false>;
                         return fir_only ? chain_f32pc_kernel<CPW, true, false> : fs4 ? chain_f32pc_kernel<CPW, false, true> : chain_f32pc_kernel<CPW, false, false>;
                     }, geo);
}

}  // namespace msdr
