// tools/probes/smfmac_probe.hip -- v_smfmac_f32_32x32x32_f16 (K = 32, 2:4 structured sparsity in the first operand) against
// v_mfma_f32_32x32x16_f16 on gfx950, for the merged first + last k-step of a FIR run (csrc/msdr_sparse24.h).
//   (a) layout: the lane -> (row, K) map of the compressed operand, of its index word and of the dense operand, pinned with one-hot
//       inputs and then with random integer data against a CPU reference that applies the map written down in msdr_sparse24.h.
//       Any mismatch prints the observed map and the program exits non-zero.
//   (b) time: a long stream of 3 sparse products per step against 3 dense products per step, operands in registers with the statistics
//       of the real fragments (scaled windowed-sinc taps and samples, each split hi + lo), on one accumulation chain (as the product
//       kernel issues them) and on two, at one and at four waves per SIMD: cycles per instruction, in-kernel clock, and the shader clock
//       and socket power rocm-smi shows while the stream loops (bench.py's sampling method).
// It is a measurement aid, not product code.   hipcc --offload-arch=gfx950 -O3 -o smfmac_probe smfmac_probe.hip
//   smfmac_probe            both parts          smfmac_probe layout      part (a) alone          smfmac_probe time [seconds per arm]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x16 __attribute__((ext_vector_type(16)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(1); } } while (0)

// ---- (a) layout --------------------------------------------------------------------------------------------------------------
// one case per workgroup of one wave: a[case][lane][8], b[case][lane][16], idx[case][lane], d[case][lane][16]
template <int ABID>
__global__ __launch_bounds__(64) void layout_kernel(const _Float16 *__restrict__ a, const _Float16 *__restrict__ b, const int *__restrict__ idx,
                                                    float *__restrict__ d)
{
    const size_t l = (size_t)blockIdx.x * 64 + threadIdx.x;
    const f16x8 av = *reinterpret_cast<const f16x8 *>(a + l * 8);
    const f16x16 bv = *reinterpret_cast<const f16x16 *>(b + l * 16);
    f32x16 acc = (f32x16)(0.0f);
    acc = __builtin_amdgcn_smfmac_f32_32x32x32_f16(av, bv, acc, idx[l], 0, ABID);
#pragma unroll
    for (int r = 0; r < 16; r++) d[l * 16 + r] = acc[r];
}

// The map under test (the one msdr_sparse24.h documents).  Lane l = (r = l & 31, h = l >> 5).
//   dense operand:      element j (0..15) of lane l is B[k = 16 (j >> 3) + 8 h + (j & 7)][column r]: two 32x32x16 operands, K-stacked
//   compressed operand: element c (0..7) of lane l belongs to row r, group g = c >> 1 (K values 16 h + 4 g .. + 3), and sits at
//                       K = 16 h + 4 g + ((idx16 >> (4 g + 2 (c & 1))) & 3), idx16 = half ABID of the lane's index word
//   result:             register q of lane l is D[row (q & 3) + 8 (q >> 2) + 4 h][column r]
static void reference(const _Float16 *a, const _Float16 *b, const int *idx, int abid, double *D /* [32][32] */)
{
    std::vector<double> A(32 * 32, 0.0), B(32 * 32, 0.0);
    for (int l = 0; l < 64; l++) {
        const int r = l & 31, h = l >> 5;
        const unsigned i16 = ((unsigned)idx[l] >> (16 * abid)) & 0xffffu;
        for (int c = 0; c < 8; c++) A[r * 32 + 16 * h + 4 * (c >> 1) + ((i16 >> (4 * (c >> 1) + 2 * (c & 1))) & 3)] += (double)a[l * 8 + c];
        for (int j = 0; j < 16; j++) B[(16 * (j >> 3) + 8 * h + (j & 7)) * 32 + r] = (double)b[l * 16 + j];
    }
    for (int m = 0; m < 32; m++)
        for (int n = 0; n < 32; n++) {
            double s = 0.0;
            for (int k = 0; k < 32; k++) s += A[m * 32 + k] * B[k * 32 + n];
            D[m * 32 + n] = s;
        }
}

static int run_layout()
{
    // one-hot cases: dense slot (hb, j) x six index patterns, both index halves; then random integer cases
    static const unsigned pats[6] = {0x4, 0xE, 0x9, 0xC, 0x8, 0xD};       // positions (0,1) (2,3) (1,2) (0,3) (0,2) (1,3): low pair first
    const int n_hot = 32 * 6, n_rand = 32, n_cases = n_hot + n_rand;
    int bad_total = 0;
    for (int abid = 0; abid < 2; abid++) {
        std::vector<_Float16> a((size_t)n_cases * 64 * 8), b((size_t)n_cases * 64 * 16, (_Float16)0.0f);
        std::vector<int> idx((size_t)n_cases * 64);
        unsigned s = 777u + abid;
        auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
        auto rand_idx16 = [&]() {
            unsigned v = 0;
            for (int g = 0; g < 4; g++) { const unsigned p = pats[rnd() % 6]; v |= p << (4 * g); }
            return v;
        };
        for (int c = 0; c < n_cases; c++)
            for (int l = 0; l < 64; l++) {
                const size_t L = (size_t)c * 64 + l;
                if (c < n_hot) {
                    const int slot = c / 6, hb = slot >> 4, j = slot & 15;
                    const unsigned p = pats[c % 6], want = p * 0x1111u, other = pats[(c + 3) % 6] * 0x1111u;
                    idx[L] = (int)(abid ? (want << 16) | other : (other << 16) | want);
                    for (int e = 0; e < 8; e++) a[L * 8 + e] = (_Float16)(float)(1 + e + 8 * (l >> 5));      // code of (lane half, element)
                    if ((l >> 5) == hb) b[L * 16 + j] = (_Float16)1.0f;
                } else {
                    const unsigned w0 = rand_idx16(), w1 = rand_idx16();
                    idx[L] = (int)((w1 << 16) | w0);
                    for (int e = 0; e < 8; e++) a[L * 8 + e] = (_Float16)(float)((int)(rnd() % 17) - 8);
                    for (int e = 0; e < 16; e++) b[L * 16 + e] = (_Float16)(float)((int)(rnd() % 17) - 8);
                }
            }
        _Float16 *da, *db; int *di; float *dd;
        CHECK(hipMalloc(&da, a.size() * 2)); CHECK(hipMalloc(&db, b.size() * 2)); CHECK(hipMalloc(&di, idx.size() * 4));
        CHECK(hipMalloc(&dd, (size_t)n_cases * 64 * 16 * 4));
        CHECK(hipMemcpy(da, a.data(), a.size() * 2, hipMemcpyHostToDevice)); CHECK(hipMemcpy(db, b.data(), b.size() * 2, hipMemcpyHostToDevice));
        CHECK(hipMemcpy(di, idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
        if (abid == 0) hipLaunchKernelGGL(layout_kernel<0>, dim3(n_cases), dim3(64), 0, 0, da, db, di, dd);
        else hipLaunchKernelGGL(layout_kernel<1>, dim3(n_cases), dim3(64), 0, 0, da, db, di, dd);
        CHECK(hipDeviceSynchronize());
        std::vector<float> d((size_t)n_cases * 64 * 16);
        CHECK(hipMemcpy(d.data(), dd, d.size() * 4, hipMemcpyDeviceToHost));
        CHECK(hipFree(da)); CHECK(hipFree(db)); CHECK(hipFree(di)); CHECK(hipFree(dd));
        int bad_hot = 0, bad_rand = 0;
        std::vector<double> D(32 * 32);
        for (int c = 0; c < n_cases; c++) {
            reference(&a[(size_t)c * 64 * 8], &b[(size_t)c * 64 * 16], &idx[(size_t)c * 64], abid, D.data());
            int bad = 0;
            for (int l = 0; l < 64; l++)
                for (int q = 0; q < 16; q++) {
                    const int m = (q & 3) + 8 * (q >> 2) + 4 * (l >> 5), n = l & 31;
                    if ((double)d[((size_t)c * 64 + l) * 16 + q] != D[m * 32 + n]) bad++;
                }
            if (bad && c < n_hot) {
                // what the hardware did: with every compressed element carrying the code 1 + c + 8 h, the result names the element (or 0)
                const int slot = c / 6;
                printf("layout MISMATCH abid %d: dense slot (half %d, element %d), index pattern 0x%X: expected code %g, observed row 0 / row 5 codes %g / %g\n",
                       abid, slot >> 4, slot & 15, pats[c % 6], D[0], (double)d[((size_t)c * 64) * 16], (double)d[((size_t)c * 64 + 32) * 16 + 1]);
            }
            if (bad) (c < n_hot ? bad_hot : bad_rand)++;
        }
        printf("{\"probe\": \"smfmac_f32_32x32x32_f16 layout\", \"abid\": %d, \"one_hot_cases\": %d, \"one_hot_bad\": %d, \"random_cases\": %d, \"random_bad\": %d}\n",
               abid, n_hot, bad_hot, n_rand, bad_rand);
        bad_total += bad_hot + bad_rand;
    }
    fflush(stdout);
    return bad_total;
}

// ---- (b) time ----------------------------------------------------------------------------------------------------------------
constexpr int kSets = 3;             // operand sets cycled through (registers)
constexpr int kStepsPerIter = 18;    // as one c3 tile: 18 steps of 3 products

// SPARSE: 3 x smfmac per step, else 3 x mfma 32x32x16; CHAINS accumulators taken in turn
template <bool SPARSE, int CHAINS>
__global__ __launch_bounds__(256) void stream_kernel(const _Float16 *__restrict__ ops, const int *__restrict__ idxs, float *__restrict__ sink, int iters,
                                                     long long *__restrict__ clk)
{
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    // ops: [set][piece: taps hi, taps lo, x hi, x lo][lane][16]
    f16x8 th[kSets], tl[kSets], xh8[kSets], xl8[kSets];
    f16x16 xh16[kSets], xl16[kSets];
    int ix[kSets];
#pragma unroll
    for (int s = 0; s < kSets; s++) {
        const _Float16 *o = ops + ((size_t)s * 4 * 64 + lane) * 16;
        th[s] = *reinterpret_cast<const f16x8 *>(o); tl[s] = *reinterpret_cast<const f16x8 *>(o + 64 * 16);
        xh16[s] = *reinterpret_cast<const f16x16 *>(o + 2 * 64 * 16); xl16[s] = *reinterpret_cast<const f16x16 *>(o + 3 * 64 * 16);
        xh8[s] = *reinterpret_cast<const f16x8 *>(o + 2 * 64 * 16); xl8[s] = *reinterpret_cast<const f16x8 *>(o + 3 * 64 * 16);
        ix[s] = idxs[s * 64 + lane];
    }
    f32x16 acc[CHAINS];
#pragma unroll
    for (int c = 0; c < CHAINS; c++) acc[c] = (f32x16)(0.0f);
    const long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int st = 0; st < kStepsPerIter; st++) {
            const int s = st % kSets, c = st % CHAINS;
            if constexpr (SPARSE) {
                acc[c] = __builtin_amdgcn_smfmac_f32_32x32x32_f16(th[s], xl16[s], acc[c], ix[s], 0, 0);
                acc[c] = __builtin_amdgcn_smfmac_f32_32x32x32_f16(tl[s], xh16[s], acc[c], ix[s], 0, 0);
                acc[c] = __builtin_amdgcn_smfmac_f32_32x32x32_f16(th[s], xh16[s], acc[c], ix[s], 0, 0);
            } else {
                acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(th[s], xl8[s], acc[c], 0, 0, 0);
                acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(tl[s], xh8[s], acc[c], 0, 0, 0);
                acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(th[s], xh8[s], acc[c], 0, 0, 0);
            }
        }
    }       // (|acc| stays below 1e16 over a launch: no reset needed)
    const long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (lane == 0) { clk[2 * wave] = c1 - c0; clk[2 * wave + 1] = r1 - r0; }
    float sum = 0.0f;
#pragma unroll
    for (int c = 0; c < CHAINS; c++)
        for (int i = 0; i < 16; i++) sum += acc[c][i];
    if (sum == 123.456f) sink[lane] = sum;
}

static std::string smi_sample()
{
    std::string out;
    FILE *f = popen("rocm-smi --showclocks --showpower 2>/dev/null", "r");
    if (!f) return out;
    char line[512];
    while (fgets(line, sizeof line, f)) out += line;
    pclose(f);
    return out;
}

static double first_number_after(const std::string &txt, const char *key, const char *open)
{
    size_t p = txt.find(key);
    if (p == std::string::npos) return 0.0;
    p = txt.find(open, p);
    if (p == std::string::npos) return 0.0;
    return atof(txt.c_str() + p + strlen(open));
}

template <typename K>
static void run_stream(K kern, const char *name, int chains, int wps, double seconds, const _Float16 *ops, const int *idxs, float *sink, long long *clk)
{
    const int waves = 256 * 4 * wps, blocks = waves / 4;
    const int iters = 20000 / wps;               // about 15 - 30 ms a launch
    for (int w = 0; w < 5; w++) hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, 0, ops, idxs, sink, iters, clk);
    CHECK(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    std::vector<float> t;
    std::vector<double> sclk, watts;
    const auto start = std::chrono::steady_clock::now();
    int launches = 0, samples = 0;
    while (true) {
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        if (el >= seconds && samples >= 3) break;
        if (el > seconds + 20.0) break;
        // keep a few launches queued, then sample while they run
        CHECK(hipEventRecord(e0));
        for (int q = 0; q < 40; q++) hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, 0, ops, idxs, sink, iters, clk);
        CHECK(hipEventRecord(e1));
        launches += 40;
        if (el >= 0.4 * seconds && samples < 3) {
            const std::string txt = smi_sample();
            const double mhz = first_number_after(txt, "sclk clock level", "("), w = first_number_after(txt, "Power (W)", ":");
            if (mhz > 0) sclk.push_back(mhz);
            if (w > 0) watts.push_back(w);
            samples++;
        }
        CHECK(hipEventSynchronize(e1));
        float ms; CHECK(hipEventElapsedTime(&ms, e0, e1)); t.push_back(ms / 40.0f);
    }
    std::sort(t.begin(), t.end());
    std::vector<long long> h(2 * (size_t)waves);
    CHECK(hipMemcpy(h.data(), clk, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
    std::vector<double> cyc, ghz;
    const double n_inst = (double)iters * kStepsPerIter * 3;
    for (int w = 0; w < waves; w++) if (h[2 * w + 1] > 0) { cyc.push_back((double)h[2 * w] / n_inst); ghz.push_back((double)h[2 * w] / (double)h[2 * w + 1] * 0.1); }
    std::sort(cyc.begin(), cyc.end()); std::sort(ghz.begin(), ghz.end());
    std::sort(sclk.begin(), sclk.end()); std::sort(watts.begin(), watts.end());
    const double ms = t[t.size() / 2];
    printf("{\"probe\": \"%s\", \"chains\": %d, \"waves_per_simd\": %d, \"launches\": %d, \"ms_median\": %.4f, \"ns_per_instruction_per_simd\": %.3f, "
           "\"cycles_per_instruction_wave_median\": %.2f, \"in_kernel_clock_GHz\": %.3f, \"smi_sclk_mhz\": %.0f, \"smi_power_w\": %.0f, \"smi_samples\": %zu}\n",
           name, chains, wps, launches, ms, ms * 1e6 / (n_inst * wps), cyc.empty() ? 0.0 : cyc[cyc.size() / 2], ghz.empty() ? 0.0 : ghz[ghz.size() / 2],
           sclk.empty() ? 0.0 : sclk[sclk.size() / 2], watts.empty() ? 0.0 : watts[watts.size() / 2], watts.size());
    fflush(stdout);
    CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
}

static void run_time(double seconds)
{
    // operands with the statistics of the real fragments: taps = Hamming-windowed sinc scaled so that max |tap| lies in [2^13, 2^14),
    // samples = uniform in +-8000 times a quarter-rate oscillator; each split as hi = fp16(v), lo = fp16(v - hi)
    std::vector<_Float16> ops((size_t)kSets * 4 * 64 * 16);
    std::vector<int> idxs(kSets * 64);
    unsigned s = 4242u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
    static const unsigned pats[3] = {0x4, 0xE, 0x9};
    for (int set = 0; set < kSets; set++)
        for (int l = 0; l < 64; l++) {
            unsigned w = 0;
            for (int g = 0; g < 4; g++) w |= pats[rnd() % 3] << (4 * g);
            idxs[set * 64 + l] = (int)(w | (w << 16));
            for (int e = 0; e < 16; e++) {
                const double tpos = (double)(set * 16 + e) - 127.5 + (l & 31);
                const double arg = 3.14159265358979 * 0.1 * tpos;
                const double tap = (std::fabs(arg) < 1e-9 ? 1.0 : std::sin(arg) / arg) * (0.54 + 0.46 * std::cos(3.14159265358979 * tpos / 160.0)) * 12000.0;
                const double x = ((double)(int)(rnd() & 0xffff) - 32768.0) * (8000.0 / 32768.0) * ((e & 1) ? 0.7071 : 1.0);
                const _Float16 th = (_Float16)tap, xh = (_Float16)x;
                _Float16 *o = &ops[((size_t)set * 4 * 64 + l) * 16 + e];
                o[0] = th; o[64 * 16] = (_Float16)(tap - (double)th); o[2 * 64 * 16] = xh; o[3 * 64 * 16] = (_Float16)(x - (double)xh);
            }
        }
    _Float16 *dops; int *didx; float *sink; long long *clk;
    CHECK(hipMalloc(&dops, ops.size() * 2)); CHECK(hipMalloc(&didx, idxs.size() * 4)); CHECK(hipMalloc(&sink, 64 * 4));
    CHECK(hipMalloc(&clk, 2 * 4096 * sizeof(long long)));
    CHECK(hipMemcpy(dops, ops.data(), ops.size() * 2, hipMemcpyHostToDevice)); CHECK(hipMemcpy(didx, idxs.data(), idxs.size() * 4, hipMemcpyHostToDevice));
    for (int wps : {1, 4}) {
        run_stream(stream_kernel<false, 1>, "3 x v_mfma_f32_32x32x16_f16 per step", 1, wps, seconds, dops, didx, sink, clk);
        run_stream(stream_kernel<true, 1>, "3 x v_smfmac_f32_32x32x32_f16 per step", 1, wps, seconds, dops, didx, sink, clk);
        run_stream(stream_kernel<false, 2>, "3 x v_mfma_f32_32x32x16_f16 per step", 2, wps, seconds, dops, didx, sink, clk);
        run_stream(stream_kernel<true, 2>, "3 x v_smfmac_f32_32x32x32_f16 per step", 2, wps, seconds, dops, didx, sink, clk);
    }
    CHECK(hipFree(dops)); CHECK(hipFree(didx)); CHECK(hipFree(sink)); CHECK(hipFree(clk));
}

int main(int argc, char **argv)
{
    const bool layout = argc < 2 || !strcmp(argv[1], "layout"), time = argc < 2 || !strcmp(argv[1], "time");
    int bad = 0;
    if (layout) bad = run_layout();
    if (bad) { printf("layout: %d cases differ from the documented map\n", bad); return 1; }
    if (time) run_time(argc > 2 ? atof(argv[2]) : 3.0);
    return 0;
}
