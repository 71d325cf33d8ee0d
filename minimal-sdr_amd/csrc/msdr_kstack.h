// msdr_kstack.h -- the A operands of the folded cascade's two sparse matrix products, R sigma and Rd delta (MwIirConsts: Rfrag, Dfrag).
// Host-only arithmetic, no kernel header: tests/cpp/kstack_check.hip includes this file alone.
//
// X (32 rows x 4 components: the response of a row's 32 outputs to 4 values it starts from) meets a 4-vector v, both split into fp16
// pieces hi + lo, and the product kept is  X_hi v_hi + X_hi v_lo + X_lo v_hi.  A v_mfma_f32_32x32x16_f16 sums 16 K rows, the product has
// 4: the three terms are STACKED along K and the instruction's own reduction adds them,
//        [ X_hi | X_hi | X_lo ] . [ v_hi ; v_lo ; v_hi ]
// A operand: lane l = (m = l & 31, h = l >> 5) holds row m's K entries 8 h .. 8 h + 7.
//   stack:  upper lanes (K 8..15) = X_hi[m][0..3], X_hi[m][0..3];  lower lanes (K 0..7) = X_lo[m][0..3], 0 0 0 0
//   lo   :  upper lanes = X_lo[m][0..3], 0 0 0 0;  lower lanes = 0
// B operand, column's upper lanes = v_hi[0..3], v_lo[0..3] in both forms:
//   one instruction : lower lanes = v_hi[0..3], 0 0 0 0 (the hi pieces copied down), against `stack`
//   two instructions: lower lanes = 0, against `stack` and then against `lo`
#pragma once

namespace msdr {

constexpr int kKstackHalves = 512;          // one A operand: 64 lanes x 8 fp16 = 1 KB

// X[m][j] in true units (components not in use: zeros), `scale` = the power of two that takes it into fp16 range.
// MSDR_MUTATE == 5 (`make mutants`, never the product): the lo pieces dropped -- exactly the entries that hold X_lo, in both operands.
inline void kstack_fill(const double (*X)[4], double scale, _Float16 *stack, _Float16 *lo)
{
    for (int i = 0; i < kKstackHalves; i++) { stack[i] = (_Float16)0.0f; lo[i] = (_Float16)0.0f; }
    for (int m = 0; m < 32; m++)
        for (int j = 0; j < 4; j++) {
            const double val = X[m][j] * scale;
            const _Float16 vh = (_Float16)val;
            _Float16 vl = (_Float16)(val - (double)vh);
#if defined(MSDR_MUTATE) && MSDR_MUTATE == 5
            vl = (_Float16)0.0f;
#endif
            stack[(32 + m) * 8 + j] = vh; stack[(32 + m) * 8 + 4 + j] = vh;
            stack[m * 8 + j] = vl;
            lo[(32 + m) * 8 + j] = vl;
        }
}

}  // namespace msdr
