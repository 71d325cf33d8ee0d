// msdr_pc_launch.h -- the one body of the per-receiver chain launchers (launch_chain_q15pc ... launch_chain_f32pcnd, msdr_block.h): what follows
// a launcher's own validation.  Host code of the translation units that hold the kernels; the geometry rule itself is msdr_pc_geometry.h.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "msdr_pc_geometry.h"
#include "msdr_decpc_geometry.h"
#include "msdr_block.h"

namespace msdr {

// ok: the launcher's validation and its geometry routine both held (g is read only then).  Copies what the kernels' parameter blocks carry
// of the geometry, launches kernel_of(std::integral_constant<int, CPW>) -- the instantiation for the chosen channels per wave -- and reports.
template <typename P, typename G, typename KernelOf>
inline hipError_t pc_launch_geometry(hipStream_t stream, P &p, bool ok, const G &g, KernelOf kernel_of, PcLaunch *geo)
{
    if (!ok) return hipErrorInvalidValue;
    const PcLaunch &l = g.launch;
    p.nseg = l.nseg; p.seg_len = g.seg_len; p.nw = g.nw;
    // msdr_chain_set_meter (p.meter = d_meter; kernel_of picks the metered instantiation by it): one segment writes d_meter itself, more write
    // the chain's partials [channels][nseg], which meter_reduce_kernel adds in segment order behind the kernel
    auto *const d_meter = p.meter;
    if (d_meter && l.nseg > 1) {
        if (!p.meter_part || (long long)p.channels * l.nseg > p.meter_cap) return hipErrorInvalidValue;
        p.meter = p.meter_part;
    }
    pc_dispatch_cpw(l.cpw, [&](auto cpw) { hipLaunchKernelGGL(kernel_of(cpw), dim3(l.grid), dim3(l.block), l.lds_bytes, stream, p); });
    if (geo) *geo = l;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !d_meter || l.nseg == 1) return e;
    return launch_meter_reduce(stream, p.meter_part, d_meter, p.channels, l.nseg);
}

// The sliding-window kernels: pc_geometry with outs_per_lane outputs per lane and lds_bytes(cpw, nw).  time_segments as
// msdr_chain_config.time_segments; the Q15 launchers pass 0 (they do not look at the configuration's value).
template <typename P, typename LdsBytes, typename KernelOf>
inline hipError_t pc_launch(hipStream_t stream, P &p, bool valid, int num_cus, int time_segments, int outs_per_lane, LdsBytes lds_bytes, KernelOf kernel_of, PcLaunch *geo)
{
    PcGeometry g;
    return pc_launch_geometry(stream, p, valid && pc_geometry(p.n, p.channels, num_cus, time_segments, outs_per_lane, kPcLdsCap, lds_bytes, &g), g, kernel_of, geo);
}

// f(std::integral_constant<int, AL>) for the kernels' read widths
template <typename F>
inline auto dec_dispatch_al(int al, F f)
{
    switch (al) {
    case 4: return f(std::integral_constant<int, 4>());
    case 2: return f(std::integral_constant<int, 2>());
    case 1: return f(std::integral_constant<int, 1>());
    default: return f(std::integral_constant<int, 0>());
    }
}

// pc_launch for the decimating kernels (msdr_chain_decpc.hip and the complex-input twins, msdr_chain_cxdecpc.hip): launch geometry from
// dec_geometry (msdr_decpc_geometry.h), everything in outputs; p.nout and p.opl beside the fields every parameter block carries.
// kernel_of(CPW, AL): the instantiation for the read width al.
template <typename P, typename KernelOf>
inline hipError_t dec_launch(hipStream_t stream, P &p, bool valid, bool f32, int num_cus, int time_segments, int al, KernelOf kernel_of, PcLaunch *geo)
{
    if (!valid || p.dec < 2 || p.n % p.dec) return hipErrorInvalidValue;
    p.nout = p.n / p.dec;
    DecGeometry g;
    const bool ok = dec_geometry(p.nout, p.channels, num_cus, time_segments, kPcLdsCap, [&](int cpw, int nw, int opl) { return dec_lds_bytes(f32, p.np, p.dec, cpw, nw, opl); }, &g);
    if (ok) p.opl = g.opl;
    return pc_launch_geometry(stream, p, ok, g, [&](auto cpw) { return dec_dispatch_al(al, [&](auto a) { return kernel_of(cpw, a); }); }, geo);
}

}  // namespace msdr
