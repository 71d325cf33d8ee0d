// msdr_sparse24.h -- the first and the last k-step of a FIR run as ONE 2:4-sparse matrix product (pure C++, host side; no HIP).
//
// A run of the folded FIR (msdr_chain_mfma.hiph) walks cnt 16-sample chunks of one window array.  On a Toeplitz table the tap block of
// the run's first chunk is empty below the band's start and the block of its last chunk is empty above the band's end: for every
// (sample m inside the chunk, output column b) at most ONE of the two blocks holds a tap.  v_smfmac_f32_32x32x32_f16 multiplies K = 32
// values of which, in its first operand, at most two of every aligned four are non-zero -- so the two half-empty K = 16 steps fit one
// instruction when the 32 K values are ordered as eight QUADS
//     quad(i) = ( first[i], first[i+1], last[i], last[i+1] ),   i = 0, 2, .., 14   (first / last = the chunk's samples m = i, i + 1)
// because a column b meets a quad with exactly the taps of first[i], first[i+1] (band started), of last[i], last[i+1] (band not ended
// yet) or of first[i+1], last[i] (the band's two ends fall between the samples); fewer taps are stored as explicit zeros.
//
// THE INSTRUCTION'S OPERAND MAP (pinned on the hardware by tools/probes/smfmac_probe.hip, which applies this same map):
//   D = A B + C, A sparse 32 x 32 stored as 32 x 16 + indices, B dense 32 x 32.  Lane l = (r = l & 31, h = l >> 5).
//   * A, compressed (8 fp16 per lane): element c belongs to row r and to K group G = 4 h + (c >> 1) (K values 4 G .. 4 G + 3); it sits at
//         K = 4 G + ((idx >> (4 (c >> 1) + 2 (c & 1))) & 3)
//     idx = the low 16 bits of the lane's index word (ABID = 0; ABID = 1 takes the high 16): per group a nibble, low two bits = position
//     of element 2 g, high two bits = position of element 2 g + 1, the first strictly below the second.
//   * B, dense (16 fp16 per lane): element j is B[K = 16 (j >> 3) + 8 h + (j & 7)][column r] -- two 32x32x16 operands stacked along K,
//     NOT 16 consecutive K values.
//   * D: register q of lane l = D[row (q & 3) + 8 (q >> 2) + 4 h][column r], as every 32 x 32 product.
//
// HOW THE MERGED STEP USES IT (operands swapped as in the kernel: A = taps, row = output column b; B = window, column = output row a):
//   dense operand, lane (a, h): registers ( f.r0, l.r0, f.r1, l.r1, f.r2, l.r2, f.r3, l.r3 ), f / l = the 16-byte window fragments of the
//   first / last chunk the lane reads today (samples 8 h .. 8 h + 7, register t = samples 8 h + 2 t, + 1).  Register pair t is then the K
//   group G = 4 (t >> 1) + 2 h + (t & 1) and holds quad(i = 8 h + 2 t) in the order above.
//   compressed operand, lane (b, h'): group g is K group G = 4 h' + g, i.e. quad(i) with
//         i = sparse24_quad_sample(h', g) = 8 (g >> 1) + 4 h' + 2 (g & 1).
//   The hi and the lo piece of the taps share the index word (a tap's pieces are zero together or stored at the same position).
#pragma once
#include <cmath>
#include <cstdint>

namespace msdr {

constexpr int kSp24FragHalfs = 512;        // one compressed piece: 64 lanes x 8 fp16
constexpr int kSp24Bytes = 2304;           // a merged step in a table: hi piece (1 KB) | lo piece (1 KB) | 64 index words (256 B)

// fp16 as bits, round to nearest even from double in one rounding -- what (_Float16)v does where the compiler has the type; written out so
// that this header builds with any C++ compiler
inline uint16_t sparse24_half_bits(double v)
{
    const uint16_t sign = std::signbit(v) ? 0x8000u : 0u;
    const double a = std::fabs(v);
    if (a == 0.0) return sign;
    if (!(a < 65520.0)) return (uint16_t)(sign | 0x7c00u);                             // (never a table entry: they stay below 2^14)
    int e;
    const double f = std::frexp(a, &e);                                                // a = f 2^e, f in [0.5, 1)
    int ex = e - 1;
    if (ex < -14) return (uint16_t)(sign | (uint16_t)std::nearbyint(std::ldexp(a, 24)));   // subnormal: units of 2^-24 (1024 = the smallest normal)
    double q = std::nearbyint(std::ldexp(f, 11));                                      // [1024, 2048]
    if (q == 2048.0) { q = 1024.0; ex++; }
    return (uint16_t)(sign | ((unsigned)(ex + 15) << 10) | ((unsigned)q - 1024u));
}
inline double sparse24_half_value(uint16_t h)
{
    const int ex = (h >> 10) & 31, man = h & 1023;
    const double a = ex ? std::ldexp(1024.0 + man, ex - 25) : std::ldexp((double)man, -24);
    return (h & 0x8000u) ? -a : a;
}

inline int sparse24_quad_sample(int lane_half, int group) { return 8 * (group >> 1) + 4 * lane_half + 2 * (group & 1); }

// a tap as the tables store it: scaled, split into two fp16 pieces (the same arithmetic as the dense fragments of msdr_chain_create,
// the `make mutants` branches included)
inline void sparse24_split(double m, double scale, uint16_t *hi, uint16_t *lo)
{
    double val = m * scale;
#if defined(MSDR_MUTATE) && MSDR_MUTATE == 2       /* `make mutants`, never the product: the taps rounded to 16 significant bits */
    if (val != 0.0) { int e_; const double f_ = std::frexp(val, &e_); val = std::ldexp(std::nearbyint(std::ldexp(f_, 16)), e_ - 16); }
#endif
    const uint16_t vh = sparse24_half_bits(val);
    *hi = vh;
    *lo = sparse24_half_bits(val - sparse24_half_value(vh));
#if defined(MSDR_MUTATE) && MSDR_MUTATE == 1       /* `make mutants`, never the product: the lo pieces dropped */
    *lo = 0;
#endif
}

// first / last: the tap blocks of a run's first and last chunk, entry (sample m < 16, column b < 32) at [m * stride + b].
// Writes hi[64 * 8], lo[64 * 8] (fp16 bit patterns), idx[64] and returns true; returns false, with the outputs undefined, where some (m, b) holds a tap in
// both blocks (tables that carry more than the taps in their columns).
inline bool sparse24_merge(const double *first, const double *last, int stride, double scale, uint16_t *hi, uint16_t *lo, uint32_t *idx)
{
    for (int m = 0; m < 16; m++)
        for (int b = 0; b < 32; b++)
            if (first[m * stride + b] != 0.0 && last[m * stride + b] != 0.0) return false;
    for (int l = 0; l < 64; l++) {
        const int b = l & 31, hl = l >> 5;
        uint32_t word = 0;
        for (int g = 0; g < 4; g++) {
            const int i = sparse24_quad_sample(hl, g);
            const double quad[4] = {first[i * stride + b], first[(i + 1) * stride + b], last[i * stride + b], last[(i + 1) * stride + b]};
            int pos[2], n = 0;
            for (int p = 0; p < 4; p++) if (quad[p] != 0.0) pos[n++] = p;           // (at most two: one per sample, see above)
            // explicit zeros fill up to two, at free positions, keeping the pair increasing
            if (n == 0) { pos[0] = 0; pos[1] = 1; }
            else if (n == 1) { if (pos[0] < 3) pos[1] = pos[0] + 1; else { pos[1] = 3; pos[0] = 2; } }
            for (int e = 0; e < 2; e++) sparse24_split(quad[pos[e]], scale, &hi[l * 8 + 2 * g + e], &lo[l * 8 + 2 * g + e]);
            word |= (uint32_t)(pos[0] | (pos[1] << 2)) << (4 * g);
        }
        idx[l] = word;
    }
    return true;
}

// The inverse, by the map above alone: one compressed piece and its index words -> the K-stacked pair, stacked[m * 32 + b] = the first
// chunk's entry (m, b) for m < 16, the last chunk's entry (m - 16, b) for m >= 16 (tests).
inline void sparse24_expand(const uint16_t *piece, const uint32_t *idx, double *stacked)
{
    for (int k = 0; k < 32 * 32; k++) stacked[k] = 0.0;
    for (int l = 0; l < 64; l++) {
        const int b = l & 31, hl = l >> 5;
        for (int c = 0; c < 8; c++) {
            const int g = c >> 1, p = (int)((idx[l] >> (4 * g + 2 * (c & 1))) & 3u), i = sparse24_quad_sample(hl, g);
            const int m = (p < 2) ? i + p : 16 + i + (p - 2);
            stacked[m * 32 + b] += sparse24_half_value(piece[l * 8 + c]);
        }
    }
}

}  // namespace msdr
