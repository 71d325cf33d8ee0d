// msdr_iqshare.h -- may the envelope kernel run Q on accumulator 0's tap fragments? (pure C++, host side; no HIP)
//
// Behind the exact Fs/4 mixer (cos = 1 0 -1 0, sin = 0 1 0 -1) at an even rotation, with one low-pass for both streams (hI == hQ, the
// reference's AM case .ino:917-924), the de-interleaved envelope table has
//     I[m] = sum_k h[m - 2k]     (-1)^k even[k]          Q[m] = sum_k h[m - 1 - 2k] (-1)^k odd[k]
// so accumulator 1's tap block is accumulator 0's block moved one column: B_Q[i][b] = B_I[i][b - 1].  Accumulator 0's fragments applied to
// the ODD array then give Q'(a, b) = Q[32 a + b + 1]: the Q the envelope needs, one sample late (msdr_chain_mfw.hiph realigns it behind
// the burst), and one fragment read feeds both accumulators.  Nothing of this is assumed: iqshare_check confirms it on the numbers of the
// two matrices the table builder made, as the values the fragments hold (hi and lo fp16 piece after scaling), and on the runs and merged
// steps it decided.  Any table that fails keeps its own fragments for accumulator 1 (header field qlag = 0).
#pragma once
#include <cstddef>
#include "msdr_sparse24.h"

namespace msdr {

// M0 / M1: the two accumulators' matrices, entry (window sample s, output column b) at [s * 32 + b], s = 2 i + src (src 0 = the even array,
// 1 = the odd array, i = index inside the array), nsamp window samples (a multiple of 32).  j0 / cnt / sp: the header's runs and merged
// steps, [accumulator][source].
inline bool iqshare_check(const double *M0, const double *M1, int nsamp, double scale, const int j0[2][2], const int cnt[2][2], const int sp[2][2])
{
    const int ni = nsamp / 2;                                     // samples per array
    if (nsamp <= 0 || (nsamp & 31) != 0 || ni < 32) return false;
    // accumulator 0 walks the even array alone, accumulator 1 the odd array alone: the same chunks, from chunk 1 on (the first tile of a
    // unit reads one row below the window's rows), the same merged / dense decision
    if (cnt[0][1] != 0 || cnt[1][0] != 0 || cnt[0][0] <= 0 || cnt[1][1] != cnt[0][0]) return false;
    if (j0[0][0] < 1 || j0[1][1] != j0[0][0]) return false;
    if (sp[0][1] != 0 || sp[1][0] != 0 || (sp[0][0] != 0) != (sp[1][1] != 0)) return false;
    auto same = [&](double a, double b) {
        uint16_t ah, al, bh, bl;
        sparse24_split(a, scale, &ah, &al);
        sparse24_split(b, scale, &bh, &bl);
        // (+0 and -0 are the same factor)
        return ((ah == bh) || ((ah | bh) & 0x7fffu) == 0) && ((al == bl) || ((al | bl) & 0x7fffu) == 0);
    };
    for (int i = 0; i < ni; i++)
        for (int b = 0; b < 32; b++) {
            if (M0[(size_t)(2 * i + 1) * 32 + b] != 0.0 || M1[(size_t)(2 * i) * 32 + b] != 0.0) return false;     // (what the runs say, on the numbers)
            const double q = M1[(size_t)(2 * i + 1) * 32 + b], iv = M0[(size_t)(2 * i) * 32 + b];
            if (b >= 1) { if (!same(q, M0[(size_t)(2 * i) * 32 + b - 1])) return false; }
            else if (i >= ni - 16 && !same(q, 0.0)) return false;                                                   // column 0 of the last chunk: nothing
            // column 31 of accumulator 0 is column 0 of accumulator 1 one row (16 samples of the array) further on
            if (b == 31 && !same(iv, i >= 16 ? M1[(size_t)(2 * (i - 16) + 1) * 32] : 0.0)) return false;
        }
    return true;
}

}  // namespace msdr
