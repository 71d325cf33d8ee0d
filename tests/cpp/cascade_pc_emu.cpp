// cascade_pc_emu.cpp -- biquad_df1_seq_pc_kernel (csrc/msdr_biquad_df1_pc.hiph) run on the CPU: a stand-alone program, built with the address
// and undefined-behaviour sanitizers by tests/test_cascade_pc_emulation.py.  The kernel's own text (cut out of the header by the test into
// cascade_pc_kernel_body.inc) is compiled as plain C++ over the small shim below: one std::thread per lane, 64 per workgroup, __syncthreads()
// a barrier, block-shared arrays plain statics (one workgroup at a time).  Exact-size heap blocks, so any access past a row's end is seen.
// Checked against the plain sequential cascade: bit for bit without time segments (partial workgroups, n % 4 != 0, unaligned rows, in place,
// the 16-byte path and the bounds-checked one), and to 1e-6 with segments warmed up long enough.
#include <barrier>
#include <thread>
#include <vector>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <cmath>
#include <cstdlib>
#include <algorithm>
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kMaxStages = 4, kBqStateFloats = 16, kSbqSlab = 128, kSbqPitch = 132, kSbqTabFloats = 20;
struct Idx { int x; };
static thread_local Idx threadIdx, blockIdx;
static std::barrier<> *g_bar;
#define __syncthreads() g_bar->arrive_and_wait()
#define __global__
#define __launch_bounds__(x)
#define __restrict__
#define __forceinline__ inline
#define __device__
// one block at a time: block-shared storage is a plain static
#define __shared__ static
static inline float sbq_mul(float a, float b) { volatile float r = a * b; return r; }
static inline float sbq_add(float a, float b) { volatile float r = a + b; return r; }
static inline float sbq_section(const float (&cf)[5], float (&st)[4], float xn)
{
    float acc = sbq_mul(cf[0], xn);
    acc = sbq_add(acc, sbq_mul(cf[1], st[0]));
    acc = sbq_add(acc, sbq_mul(cf[2], st[1]));
    acc = sbq_add(acc, sbq_mul(cf[3], st[2]));
    acc = sbq_add(acc, sbq_mul(cf[4], st[3]));
    st[1] = st[0]; st[0] = xn; st[3] = st[2]; st[2] = acc;
    return acc;
}
#include "cascade_pc_kernel_body.inc"

template <int S, bool SEG>
static void launch(unsigned grid, const float *x, float *y, long long n, int channels, const float *tab, const float *si, float *so, int nseg, long long seg_len, int warm, const float *scr)
{
    for (unsigned b = 0; b < grid; b++) {
        std::barrier<> bar(64); g_bar = &bar;
        std::vector<std::thread> th;
        for (int l = 0; l < 64; l++) th.emplace_back([=] { threadIdx.x = l; blockIdx.x = (int)b; biquad_df1_seq_pc_kernel<S, SEG>(x, y, n, channels, tab, si, so, nseg, seg_len, warm, scr); });
        for (auto &t : th) t.join();
    }
}
static void gather(const float *x, float *scratch, long long n, int channels, int nseg, long long seg_len, int warm)
{
    const long long total = (long long)channels * nseg * warm;
    for (long long i = 0; i < total; i++) { const long long v = i / warm; const int k = (int)(i - v * warm), seg = (int)(v % nseg); const long long ch = v / nseg;
        if (seg > 0) scratch[i] = x[ch * n + (long long)seg * seg_len - warm + k]; }
}
template <int S>
static int run_case(int channels, long long n, int nseg_req, int warm, int misalign, bool inplace)
{
    // exact-size heap blocks (the sanitizer sees any access past a row's end); misalign: the data starts that many floats into a block
    std::vector<float> tab((size_t)channels * 20, 0.f);
    srand(channels * 131 + (int)n + S);
    for (int c = 0; c < channels; c++) for (int s = 0; s < S; s++) { float *r = &tab[c * 20 + 5 * s]; float rad = 0.5f + 0.45f * (rand() % 100) / 100.f, th = 0.1f + 3.f * (rand() % 100) / 100.f;
        r[0] = 0.3f; r[1] = 0.1f * (c % 7); r[2] = 0.2f; r[3] = 2 * rad * std::cos(th); r[4] = -rad * rad; }
    float *xb = (float *)malloc(((size_t)channels * n + misalign) * 4), *yb = inplace ? xb : (float *)malloc(((size_t)channels * n + misalign) * 4);
    float *x = xb + misalign, *y = yb + misalign;
    std::vector<float> xin((size_t)channels * n);
    for (auto &v : xin) v = (rand() % 2001 - 1000) / 1000.f;
    memcpy(x, xin.data(), xin.size() * 4);
    std::vector<float> st0((size_t)channels * 16, 0.f), st1((size_t)channels * 16, -77.f);
    for (int c = 0; c < channels; c++) for (int k = 0; k < 4 * S; k++) st0[c * 16 + k] = 0.01f * ((c + k) % 13);
    std::vector<float> stref = st0;
    long long nseg = 1, seg_len = n;
    if (nseg_req > 1) { seg_len = ((n + nseg_req - 1) / nseg_req + 3) & ~3LL; nseg = (n + seg_len - 1) / seg_len; }
    std::vector<float> scr;
    unsigned grid = (unsigned)(((long long)channels * nseg + 63) / 64);
    if (nseg > 1) { scr.assign((size_t)channels * nseg * warm, 0.f); gather(x, scr.data(), n, channels, (int)nseg, seg_len, warm);
        launch<S, true>(grid, x, y, n, channels, tab.data(), st0.data(), st1.data(), (int)nseg, seg_len, warm, scr.data()); }
    else launch<S, false>(grid, x, y, n, channels, tab.data(), st0.data(), st0.data(), 1, n, 0, nullptr);
    // reference: the plain sequential cascade from the true state
    double worst = 0; int bad = 0;
    for (int c = 0; c < channels; c++) {
        float cf[S][5], st[S][4];
        for (int s = 0; s < S; s++) { for (int k = 0; k < 5; k++) cf[s][k] = tab[c * 20 + 5 * s + k]; for (int k = 0; k < 4; k++) st[s][k] = stref[c * 16 + 4 * s + k]; }
        double num = 0, den = 0;
        for (long long t = 0; t < n; t++) { float d = xin[c * n + t]; for (int s = 0; s < S; s++) d = sbq_section(cf[s], st[s], d);
            const float g = y[c * n + t]; if (nseg == 1 && memcmp(&g, &d, 4)) bad++; num += (double)(g - d) * (g - d); den += (double)d * d; }
        worst = std::max(worst, std::sqrt(num / std::max(den, 1e-300)));
        const float *so = nseg > 1 ? &st1[c * 16] : &st0[c * 16];
        for (int s = 0; s < S; s++) for (int k = 0; k < 4; k++) { if (nseg == 1 && memcmp(&so[4 * s + k], &st[s][k], 4)) bad++; if (std::fabs(so[4 * s + k] - st[s][k]) > 1e-5f) bad++; }
    }
    printf("S %d ch %d n %lld nseg %lld mis %d inplace %d: worst rel %.2e bad %d\n", S, channels, n, nseg, misalign, (int)inplace, worst, bad);
    free(xb); if (!inplace) free(yb);
    return bad || worst > 1e-6;
}
int main()
{
    int f = 0;
    f |= run_case<1>(1, 128, 1, 0, 0, false); f |= run_case<2>(63, 131, 1, 0, 0, false); f |= run_case<3>(64, 128, 1, 0, 0, true); f |= run_case<4>(130, 131, 1, 0, 0, true);
    f |= run_case<2>(65, 3 * 128 + 5, 1, 0, 0, false); f |= run_case<2>(64, 256, 1, 0, 1, true); f |= run_case<1>(130, 260, 1, 0, 1, false); f |= run_case<4>(64, 384, 1, 0, 0, false);
    f |= run_case<2>(3, 4096, 4, 512, 0, true); f |= run_case<2>(3, 4101, 4, 512, 0, false); f |= run_case<3>(40, 2048, 4, 256, 0, true); f |= run_case<1>(32, 2048, 4, 256, 1, true);
    f |= run_case<2>(128, 1024, 2, 512, 0, true); f |= run_case<4>(5, 1000, 3, 200, 0, false);
    printf(f ? "FAILED\n" : "ALL OK\n");
    return f;
}
