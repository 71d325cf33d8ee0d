// msdr_prepc_geometry.h -- launch geometry of the TWO-STAGE decimating per-receiver chain kernels (chain_q15pcn2 / chain_f32pcn2,
// msdr_chain_pre.hiph): plain host C++, no HIP, so that the fit rule, the setter's limits and the history formula are testable on their own
// (tests/test_prepc_geometry.py).  An extension of msdr_decpc_geometry.h: the one-stage kernels keep that header's rule unchanged.
//
// A chain-wide prefilter of np1 (padded) taps decimates the mixed stream by D1; the receiver's own channel pair of np2 (padded) taps runs on
// those intermediates and decimates by D2.  Everything here counts FINAL outputs (nout = n / (D1 D2)), and the choice of channels per wave,
// outputs per lane, waves and time segments is dec_geometry's, with this header's LDS count:
//
//   intermediate window   tile * D2 + np2 intermediates per stream: exactly the window of the one-stage kernel at factor D2 (Q15: packed
//                         pairs, two copies for odd D2), which the second stage reads as that kernel does
//   stage-1 chunk         the window is filled in chunks of C = LPC * max(1, 16 / D1) intermediates (LPC = 64 / CPW lanes per channel, so a
//                         lane makes 8, 4, 2, 1 or 1 of them at D1 = 2 .. 32); a chunk stages (C - 1) D1 + np1 mixed samples per stream
//                         (room for C D1 + np1) beside the window -- about 1024 LPC / 64 samples, twice that at D1 = 32
//   prefilter row         np1 taps, ONCE per workgroup, behind the sine table
//
// LDS of a workgroup: CPW x nw channel areas (window | tap rows I, Q | chunk I, Q) | the packed sine table | the prefilter row.
//
// No state beyond the raw history: the oldest raw sample behind an output lies (np2 - 1) D1 + np1 - 1 samples back (pre_hist_len), and a
// tile recomputes the np2 intermediates it shares with the tile before it.
#pragma once
#include <algorithm>
#include <cstddef>
#include "msdr_decpc_geometry.h"

namespace msdr {

// the factors the setter takes: even ones keep one copy of the chunk per stream in Q15
inline bool pre_factor_ok(int D1) { return D1 == 2 || D1 == 4 || D1 == 8 || D1 == 16 || D1 == 32; }
// taps padded in front to the kernels' step: 8 (Q15) or 4 (F32)
inline int pre_pad_taps(bool f32, int num_taps) { const int q = f32 ? 4 : 8; return (num_taps + q - 1) / q * q; }
// intermediates per stage-1 chunk
inline int pre_chunk(int D1, int cpw) { return (64 / cpw) * std::max(1, 16 / D1); }
// mixed samples per stream that a chunk's LDS area has room for
inline size_t pre_chunk_samples(int np1, int D1, int cpw) { return (size_t)pre_chunk(D1, cpw) * D1 + np1; }
// raw IF samples the chain carries from call to call
inline int pre_hist_len(int np1, int D1, int np2) { return (np2 - 1) * D1 + np1 - 1; }
// the stage-1 chunks of one tile
inline int pre_chunks_per_tile(int np2, int D2, int tile, int D1, int cpw)
{
    const int wlen = tile * D2 + np2, C = pre_chunk(D1, cpw);
    return (wlen + C - 1) / C;
}

inline size_t pre_q15_lds_bytes(int np1, int D1, int np2, int D2, int cpw, int nw, int opl)
{
    const size_t chan = dec_q15_chan_shorts(np2, D2, (64 / cpw) * opl) + 2 * pre_chunk_samples(np1, D1, cpw);
    return chan * 2 * (size_t)cpw * (size_t)nw + kDecSineBytes + (size_t)np1 * 2;
}
inline size_t pre_f32_lds_bytes(int np1, int D1, int np2, int D2, int cpw, int nw, int opl)
{
    const size_t chan = dec_f32_chan_floats(np2, D2, (64 / cpw) * opl) + 2 * pre_chunk_samples(np1, D1, cpw);
    return chan * 4 * (size_t)cpw * (size_t)nw + kDecSineBytes + (size_t)np1 * 4;
}
inline size_t pre_lds_bytes(bool f32, int np1, int D1, int np2, int D2, int cpw, int nw, int opl)
{
    return f32 ? pre_f32_lds_bytes(np1, D1, np2, D2, cpw, nw, opl) : pre_q15_lds_bytes(np1, D1, np2, D2, cpw, nw, opl);
}

// whether (D1, np1, np2, D2) fits at all: one wave, one channel, kDecOplMin outputs per lane (padded tap counts)
inline bool pre_fits(bool f32, int np1, int D1, int np2, int D2)
{
    return pre_factor_ok(D1) && np1 > 0 && np2 > 0 && D2 >= 1 && pre_lds_bytes(f32, np1, D1, np2, D2, 1, 1, kDecOplMin) <= kPcLdsCap;
}
// the longest (padded) prefilter beside (D1, np2, D2); 0: not even the shortest
inline int pre_max_taps(bool f32, int D1, int np2, int D2)
{
    const int q = f32 ? 4 : 8;
    int np1 = 0;
    while (pre_fits(f32, np1 + q, D1, np2, D2)) np1 += q;
    return np1;
}
// the largest second factor beside (np1, D1, np2); 0: none
inline int pre_max_decimation(bool f32, int np1, int D1, int np2)
{
    int D2 = 0;
    while (pre_fits(f32, np1, D1, np2, D2 + 1)) D2++;
    return D2;
}

// dec_geometry over FINAL outputs with the two-stage LDS count
inline bool pre_geometry(bool f32, long long nout, int channels, int num_cus, int time_segments, int np1, int D1, int np2, int D2, DecGeometry *geo)
{
    if (!pre_factor_ok(D1) || np1 <= 0 || np2 <= 0 || D2 < 1) return false;
    return dec_geometry(nout, channels, num_cus, time_segments, kPcLdsCap,
                        [&](int cpw, int nw, int opl) { return pre_lds_bytes(f32, np1, D1, np2, D2, cpw, nw, opl); }, geo);
}

}  // namespace msdr
