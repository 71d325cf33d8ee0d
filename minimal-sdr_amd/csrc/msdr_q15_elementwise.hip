// msdr_q15_elementwise.hip -- arm_mult_q15 / arm_add_q15 / arm_sub_q15 / arm_copy_q15 over a block batch and their launcher
// (a translation unit of its own).
//
//   arm_mult_q15   freq_conv.cpp:70-96    dst = ssat16((a * b) >> 15)     (only -32768 x -32768 saturates)
//   arm_add_q15    freq_conv.cpp:76, :92   dst = ssat16(a + b)            (__QADD16)
//   arm_sub_q15    freq_conv.cpp:80, :96   dst = ssat16(a - b)            (__QSUB16)
//   arm_copy_q15   Minimal-SDR.ino:577-578 dst = a
//
// The batch is dst[rows][cols], dense; source row r starts at a + r * a_stride (a_stride = 0: one row shared by every channel, the
// oscillator tables of freq_conv.cpp).  Sample i of dst depends only on sample i of each source row and is read and written by the
// same lane, so dst may be either source (the commented-out forms of freq_conv.cpp:75, :91).  Three shapes of the loop:
//   kFlat   both sources dense and every base 16-byte aligned: the batch is one array; 16-byte accesses (8 samples per lane),
//           two of them in flight per source and lane, and a scalar tail of < 8 samples
//   kRows   every row 16-byte aligned (bases aligned, cols and the source strides multiples of 8): 16-byte accesses, row and
//           column of each 8-sample piece from one 32-bit division
//   kAny    any other shape (cols = 7, 129, ..., sources one sample off): one sample per lane
// No LDS, no barrier.  Packed add / sub are v_pk_add_i16 / v_pk_sub_i16 with clamp; mult is two 16 x 16 -> 32 products per word.
#include <algorithm>
#include <hip/hip_runtime.h>
#include "msdr_block.h"

namespace msdr {
namespace {

typedef short ew_s16x2 __attribute__((ext_vector_type(2)));

// two packed samples {lo, hi}
template <int OP>
__device__ __forceinline__ int ew_op2(int a, int b)
{
    if constexpr (OP == kQ15Add) {
        return __builtin_bit_cast(int, __builtin_elementwise_add_sat(__builtin_bit_cast(ew_s16x2, a), __builtin_bit_cast(ew_s16x2, b)));
    } else if constexpr (OP == kQ15Sub) {
        return __builtin_bit_cast(int, __builtin_elementwise_sub_sat(__builtin_bit_cast(ew_s16x2, a), __builtin_bit_cast(ew_s16x2, b)));
    } else if constexpr (OP == kQ15Mult) {
        const int lo = min(((a << 16) >> 16) * ((b << 16) >> 16) >> 15, 32767);     // >= -32767: no lower clamp needed
        const int hi = min((a >> 16) * (b >> 16) >> 15, 32767);
        return (lo & 0xffff) | (hi << 16);
    } else {
        return a;
    }
}
template <int OP>
__device__ __forceinline__ short ew_op1(int a, int b)
{
    if constexpr (OP == kQ15Add) return (short)max(-32768, min(a + b, 32767));
    else if constexpr (OP == kQ15Sub) return (short)max(-32768, min(a - b, 32767));
    else if constexpr (OP == kQ15Mult) return (short)min((a * b) >> 15, 32767);
    else return (short)a;
}
template <int OP>
__device__ __forceinline__ int4 ew_op8(int4 a, int4 b)
{
    return make_int4(ew_op2<OP>(a.x, b.x), ew_op2<OP>(a.y, b.y), ew_op2<OP>(a.z, b.z), ew_op2<OP>(a.w, b.w));
}

constexpr int kShapeFlat = 0, kShapeRows = 1, kShapeAny = 2;

// (no __restrict__: dst may be a or b)
template <int OP, int SHAPE>
__global__ __launch_bounds__(256) void q15_elementwise_kernel(const short *a, long long a_stride, const short *b, long long b_stride, short *dst,
                                                              long long rows, int cols)
{
    constexpr bool kTwo = OP != kQ15Copy;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (long long)gridDim.x * blockDim.x;
    if constexpr (SHAPE == kShapeFlat) {
        const long long n = rows * cols, nv = n >> 3;
        const int4 *va = reinterpret_cast<const int4 *>(a), *vb = reinterpret_cast<const int4 *>(b);
        int4 *vd = reinterpret_cast<int4 *>(dst);
        long long v = gid;
        for (; v + nthreads < nv; v += 2 * nthreads) {
            const int4 a0 = va[v], a1 = va[v + nthreads];
            int4 b0 = a0, b1 = a1;
            if constexpr (kTwo) { b0 = vb[v]; b1 = vb[v + nthreads]; }
            vd[v] = ew_op8<OP>(a0, b0);
            vd[v + nthreads] = ew_op8<OP>(a1, b1);
        }
        if (v < nv) {
            const int4 a0 = va[v];
            int4 b0 = a0;
            if constexpr (kTwo) b0 = vb[v];
            vd[v] = ew_op8<OP>(a0, b0);
        }
        if (gid < n - (nv << 3)) {           // the last n % 8 samples
            const long long i = (nv << 3) + gid;
            dst[i] = ew_op1<OP>(a[i], kTwo ? (int)b[i] : 0);
        }
    } else if constexpr (SHAPE == kShapeRows) {
        const unsigned vpr = (unsigned)cols >> 3;
        const long long nv = rows * vpr;     // < 2^31 (the host refuses larger batches)
        for (long long v = gid; v < nv; v += nthreads) {
            const unsigned r = (unsigned)v / vpr, c = (unsigned)v - r * vpr;
            const int4 av = *reinterpret_cast<const int4 *>(a + r * a_stride + 8 * c);
            int4 bv = av;
            if constexpr (kTwo) bv = *reinterpret_cast<const int4 *>(b + r * b_stride + 8 * c);
            reinterpret_cast<int4 *>(dst)[v] = ew_op8<OP>(av, bv);
        }
    } else {
        const long long n = rows * cols;     // < 2^31
        for (long long i = gid; i < n; i += nthreads) {
            const unsigned r = (unsigned)i / (unsigned)cols, c = (unsigned)i - r * (unsigned)cols;
            const int av = a[r * a_stride + c];
            const int bv = kTwo ? (int)b[r * b_stride + c] : 0;
            dst[i] = ew_op1<OP>(av, bv);
        }
    }
}

template <int OP>
hipError_t launch_shape(hipStream_t stream, int shape, unsigned grid, const short *a, long long a_stride, const short *b, long long b_stride,
                        short *dst, long long rows, int cols)
{
    switch (shape) {
    case kShapeFlat: hipLaunchKernelGGL((q15_elementwise_kernel<OP, kShapeFlat>), dim3(grid), dim3(256), 0, stream, a, a_stride, b, b_stride, dst, rows, cols); break;
    case kShapeRows: hipLaunchKernelGGL((q15_elementwise_kernel<OP, kShapeRows>), dim3(grid), dim3(256), 0, stream, a, a_stride, b, b_stride, dst, rows, cols); break;
    default:         hipLaunchKernelGGL((q15_elementwise_kernel<OP, kShapeAny>), dim3(grid), dim3(256), 0, stream, a, a_stride, b, b_stride, dst, rows, cols); break;
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_q15_elementwise(hipStream_t stream, int op, int max_grid, const short *a, long long a_stride, const short *b, long long b_stride,
                                  short *dst, long long rows, int cols, const char **kernel)
{
    const bool two = op != kQ15Copy;
    auto al16 = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool bases = al16(a) && al16(dst) && (!two || al16(b));
    int shape = kShapeAny;
    if (bases && (rows == 1 || (a_stride == cols && (!two || b_stride == cols)))) shape = kShapeFlat;
    else if (bases && cols % 8 == 0 && a_stride % 8 == 0 && (!two || b_stride % 8 == 0)) shape = kShapeRows;
    const long long n = rows * cols, work = shape == kShapeAny ? n : (n + 7) / 8;
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>((work + 255) / 256, max_grid));
    static const char *names[3] = { "q15_elementwise_kernel<flat>", "q15_elementwise_kernel<rows>", "q15_elementwise_kernel<any>" };
    if (kernel) *kernel = names[shape];
    switch (op) {
    case kQ15Mult: return launch_shape<kQ15Mult>(stream, shape, grid, a, a_stride, b, b_stride, dst, rows, cols);
    case kQ15Add:  return launch_shape<kQ15Add>(stream, shape, grid, a, a_stride, b, b_stride, dst, rows, cols);
    case kQ15Sub:  return launch_shape<kQ15Sub>(stream, shape, grid, a, a_stride, b, b_stride, dst, rows, cols);
    case kQ15Copy: return launch_shape<kQ15Copy>(stream, shape, grid, a, a_stride, b, b_stride, dst, rows, cols);
    default:       return hipErrorInvalidValue;
    }
}

}  // namespace msdr
