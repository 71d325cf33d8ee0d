// msdr_chain_q15pc.hip -- the Q15 chain kernel with per-channel FIR coefficients and its launcher (a translation unit of its own).
#include "msdr_chain_q15pc.hiph"
#include "msdr_block.h"
#include "msdr_pc_launch.h"

namespace msdr {

hipError_t launch_chain_q15pc(hipStream_t stream, bool fir_only, int num_cus, PcParams p, PcLaunch *geo)
{
    if (fir_only) p.meter = nullptr;          // (the meter measures a chain's I and Q)
    return pc_launch(stream, p, p.np > 0 && !(p.np & 7) && p.channels > 0 && p.n > 0, num_cus, 0, kPcR,
                     [&](int cpw, int nw) { return pc_lds_bytes(p.np, cpw, fir_only, nw); },
                     [&](auto cpw) {
                         constexpr int CPW = decltype(cpw)::value;
                         return fir_only ? chain_q15pc_kernel<CPW, true> : p.meter ? chain_q15pc_meter_kernel<CPW> : chain_q15pc_kernel<CPW, false>;
                     }, geo);
}

}  // namespace msdr
