// msdr_decpc_geometry.h -- launch geometry of the DECIMATING per-receiver chain kernels (chain_q15pcnd / chain_f32pcnd): plain host C++, no HIP,
// so that the rule is testable on its own (tests/test_decim_geometry.py).  An extension of msdr_pc_geometry.h: the undecimated kernels keep
// that header's rule unchanged.
//
// With decimation D a tile of `tile` OUTPUTS needs a window of tile * D + np mixed samples per stream, so the window -- not the tap rows --
// decides what fits, and the undecimated rule (8 outputs per lane, channels per wave chosen by n alone) is several times the cap at D = 8.
// Everything here counts OUTPUTS (nout = n / D):
//
//   channels per wave   CPW = 4 for calls of up to 128 outputs, 2 up to 256, else 1 (pc_fit_lds's choice, of n / D)
//   outputs per lane    OPL = 8, so a channel's tile is OPL * 64 / CPW outputs; lane g owns outputs g, g + LPC, g + 2 LPC, ... of the tile
//                       (LPC = 64 / CPW): neighbouring lanes read windows D samples apart
//   waves               4 per workgroup
//   fit                 while the workgroup's LDS is over the cap: OPL is halved down to 2 (a smaller window per wave: more waves per
//                       compute unit), then the waves down to 1, then CPW down to 1.  One wave with one channel and two outputs per lane (a
//                       tile of 128 outputs) that does not fit: refused.
//   time segments       as pc_geometry: enough (channel group, segment) units for two rounds of 16 waves per compute unit, no segment shorter
//                       than 4 tiles; time_segments 1 = never split, > 1 = that many as far as the call has tiles.  A segment of outputs
//                       [s, e) starts its input at s * D and needs no warm-up (the window brings np samples of history along).
//
// LDS of a workgroup: CPW x nw channel areas and ONE packed sine table (kDecSineBytes).
//   Q15   copies x 2 streams x (tile * D + np) shorts + 2 tap rows of np shorts; copies = 2 for odd D (the window as it is and moved by one
//         sample: outputs of both parities meet an aligned packed pair), 1 for even D (every output starts on an even sample)
//   F32   2 streams x (tile * D + np) floats + 2 tap rows of np floats
// The setter's limits follow from the rule: dec_max_decimation() is the largest D such that EVERY factor 1 .. D fits with the shortest filter
// (even factors fit further up, but the interface keeps one range), dec_max_taps(f32, D) the longest filter beside factor D.
#pragma once
#include <algorithm>
#include <cstddef>
#include "msdr_pc_geometry.h"

namespace msdr {

constexpr size_t kDecSineBytes = 4096;          // the packed sine table (1024 dwords), once per workgroup
constexpr int kDecOplMax = 8, kDecOplMin = 2;   // outputs per lane

inline int dec_q15_copies(int D) { return (D & 1) ? 2 : 1; }
inline size_t dec_q15_chan_shorts(int np, int D, int tile) { return (size_t)2 * dec_q15_copies(D) * ((size_t)tile * D + np) + (size_t)2 * np; }
inline size_t dec_q15_lds_bytes(int np, int D, int cpw, int nw, int opl)
{
    return dec_q15_chan_shorts(np, D, (64 / cpw) * opl) * 2 * (size_t)cpw * (size_t)nw + kDecSineBytes;
}
inline size_t dec_f32_chan_floats(int np, int D, int tile) { return (size_t)2 * ((size_t)tile * D + np) + (size_t)2 * np; }
inline size_t dec_f32_lds_bytes(int np, int D, int cpw, int nw, int opl)
{
    return dec_f32_chan_floats(np, D, (64 / cpw) * opl) * 4 * (size_t)cpw * (size_t)nw + kDecSineBytes;
}
inline size_t dec_lds_bytes(bool f32, int np, int D, int cpw, int nw, int opl)
{
    return f32 ? dec_f32_lds_bytes(np, D, cpw, nw, opl) : dec_q15_lds_bytes(np, D, cpw, nw, opl);
}

struct DecGeometry { PcLaunch launch; long long seg_len; int nw, opl; };          // launch.tile, seg_len: in outputs

// lds_bytes(cpw, nw, opl): the LDS of a workgroup.  false: one wave with one channel and kDecOplMin outputs per lane does not fit.
template <typename LdsBytes>
inline bool dec_fit_lds(long long nout, size_t cap, LdsBytes lds_bytes, int *cpw_out, int *nw_out, int *opl_out)
{
    int cpw = nout <= 128 ? 4 : nout <= 256 ? 2 : 1, nw = 4, opl = kDecOplMax;
    while ((size_t)lds_bytes(cpw, nw, opl) > cap && opl > kDecOplMin) opl >>= 1;
    while ((size_t)lds_bytes(cpw, nw, opl) > cap && nw > 1) nw >>= 1;
    while ((size_t)lds_bytes(cpw, nw, opl) > cap && cpw > 1) cpw >>= 1;
    if ((size_t)lds_bytes(cpw, nw, opl) > cap) return false;
    *cpw_out = cpw; *nw_out = nw; *opl_out = opl;
    return true;
}

template <typename LdsBytes>
inline bool dec_geometry(long long nout, int channels, int num_cus, int time_segments, size_t cap, LdsBytes lds_bytes, DecGeometry *geo)
{
    int cpw = 0, nw = 0, opl = 0;
    if (nout <= 0 || channels <= 0 || !dec_fit_lds(nout, cap, lds_bytes, &cpw, &nw, &opl)) return false;
    const int tile = (64 / cpw) * opl;
    const long long groups = ((long long)channels + cpw - 1) / cpw;
    const long long tiles = (nout + tile - 1) / tile;
    long long nseg = std::max<long long>(1, std::min<long long>((32LL * num_cus + groups - 1) / groups, tiles / 4));
    if (time_segments == 1) nseg = 1;
    else if (time_segments > 1) nseg = std::max<long long>(1, std::min<long long>(time_segments, tiles));
    const long long seg_tiles = (tiles + nseg - 1) / nseg;
    nseg = (tiles + seg_tiles - 1) / seg_tiles;
    const long long units = groups * nseg;
    geo->launch = PcLaunch{(unsigned)((units + nw - 1) / nw), (unsigned)nw * 64, (size_t)lds_bytes(cpw, nw, opl), cpw, (int)nseg, tile};
    geo->seg_len = seg_tiles * tile;
    geo->nw = nw; geo->opl = opl;
    return true;
}

// whether factor D fits beside filters of np (padded) taps at all: one wave, one channel, kDecOplMin outputs per lane
inline bool dec_fits(bool f32, int np, int D) { return D >= 1 && np > 0 && dec_lds_bytes(f32, np, D, 1, 1, kDecOplMin) <= kPcLdsCap; }
// the longest (padded) filter beside factor D; 0: not even the shortest
inline int dec_max_taps(bool f32, int D)
{
    const int q = f32 ? 4 : 8;
    int np = 0;
    while (dec_fits(f32, np + q, D)) np += q;
    return np;
}
// the largest D such that every factor 1 .. D fits with the shortest filter
inline int dec_max_decimation(bool f32)
{
    int D = 1;
    while (dec_fits(f32, f32 ? 4 : 8, D + 1)) D++;
    return D;
}

}  // namespace msdr
