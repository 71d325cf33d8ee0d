// msdr_cmsis.cpp -- include/msdr_cmsis.h: the reference's CMSIS-DSP argument lists over the batched C ABI (no device code here).
#include "../../include/msdr_cmsis.h"

#include <cstdio>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <vector>

// msdr_api.hip (not part of the C ABI): a pinned host buffer mapped into the device's address space; what a pointer points into (1 device
// memory of ctx's device with its allocation's range, 0 host-readable, -1 another device); a counter msdr_free advances; msdr_last_error()'s text
int msdr_mapped_alloc(msdr_ctx *ctx, size_t bytes, void **host, void **dev);
void msdr_mapped_free(msdr_ctx *ctx, void *host);
int msdr_ptr_query(msdr_ctx *ctx, const void *p, uintptr_t *base, size_t *size);
unsigned msdr_free_generation(void);
int msdr_cmsis_fail(int code, const char *text);

namespace {

// kind: 0 fir q15, 1 fir f32, 2 biquad df1 f32.  coef: the bytes of pCoeffs the device tables were last built from -- CMSIS reads
// the caller's array on every call (the instance holds a pointer, arm_fir_init_q15.c:100-109), and the reference rewrites it in place
// under the running filter (UI.cpp:337-345, Minimal-SDR.ino:221-223), so every process call compares and, on a change, rebuilds the
// tables with the filter state kept (msdr_fir_*_set_coeffs, msdr_biquad_df1_f32_set_coeffs).
struct Entry { int kind; void *handle; std::vector<char> coef; };
struct Binding {
    std::mutex mu;
    msdr_ctx *ctx = nullptr;
    uint32_t channels = 0;
    std::unordered_map<const void *, Entry> inst;  // keyed by the caller's instance struct, as CMSIS identifies a filter
    // msdr_cmsis_bind_host: pSrc / pDst are HOST arrays (the sketch's stack buffers, Minimal-SDR.ino:525-526, 574-575), staged through two
    // PINNED host buffers the device reads and writes in place (they grow with the largest block seen): a call is memcpy in, the kernel,
    // one stream synchronisation, memcpy out -- no copy command on the stream (two of them, each with a synchronisation of its own, were
    // 37 of the 41 us of a 128-sample call)
    bool host = false;
    void *h_in = nullptr, *h_out = nullptr;      // host addresses
    void *d_in = nullptr, *d_out = nullptr;      // the same buffers as the device sees them
    size_t cap = 0;
    void *h_in2 = nullptr, *d_in2 = nullptr;     // the second source of arm_mult_q15 / arm_add_q15 / arm_sub_q15
    size_t cap2 = 0;
    // msdr_cmsis_bind: device allocations seen lately (most recent first), valid while msdr_free's counter stays at `gen`
    struct Range { uintptr_t base; size_t size; };
    std::vector<Range> ranges;
    unsigned gen = 0;
    // msdr_cmsis_bind: host rows shared by every channel (freq_conv.cpp's oscillator tables), keyed by their address: the bytes last
    // uploaded and the device copy
    struct Row { std::vector<char> snap; void *dev = nullptr; size_t cap = 0; uint64_t used = 0; };
    std::unordered_map<const void *, Row> rows;
    uint64_t row_clock = 0;
};
Binding &binding() { static Binding b; return b; }

void destroy(const Entry &e)
{
    if (e.kind == 0) msdr_fir_q15_destroy((msdr_fir_q15 *)e.handle);
    else if (e.kind == 1) msdr_fir_f32_destroy((msdr_fir_f32 *)e.handle);
    else msdr_biquad_df1_f32_destroy((msdr_biquad_df1_f32 *)e.handle);
}
// registers (or replaces: a re-init of the same instance) the device object behind S
void remember(const void *S, int kind, void *handle, const void *coef, size_t coef_bytes)
{
    Binding &b = binding();
    std::vector<char> snap((const char *)coef, (const char *)coef + (coef ? coef_bytes : 0));
    auto it = b.inst.find(S);
    if (it != b.inst.end()) { destroy(it->second); it->second = Entry{kind, handle, std::move(snap)}; }
    else b.inst.emplace(S, Entry{kind, handle, std::move(snap)});
}
// a failed (re-)init: the instance struct already shows the new filter, so the OLD device object must not answer for it any more --
// later process calls on S do nothing and msdr_last_error() holds the create's text
void forget(const void *S)
{
    Binding &b = binding();
    auto it = b.inst.find(S);
    if (it != b.inst.end()) { destroy(it->second); b.inst.erase(it); }
}
// (caller holds the lock, and keeps it across the process call: a concurrent re-init or msdr_cmsis_bind cannot destroy the object
//  under a running enqueue -- process calls only queue work on the context's stream, so the lock is held for microseconds)
Entry *lookup_locked(const void *S, int kind)
{
    Binding &b = binding();
    auto it = b.inst.find(S);
    return (it != b.inst.end() && it->second.kind == kind) ? &it->second : nullptr;
}
// The caller's coefficient array against the snapshot.  On a change the tables are rebuilt through `set` (state kept); the snapshot takes
// the new bytes only once that has SUCCEEDED -- after a failed rebuild (a cascade whose state cannot cross to the new coefficients, an
// allocation that failed) the old snapshot stays, so the next call compares unequal again and retries, and this call runs the filter with
// the tables it still has (pDst is written either way; msdr_last_error() has the text of the failure).
template <typename Set>
void follow_coeffs(Entry *e, const void *pCoeffs, Set &&set)
{
    if (!pCoeffs || e->coef.empty() || memcmp(e->coef.data(), pCoeffs, e->coef.size()) == 0) return;
    if (set() == 0) memcpy(e->coef.data(), pCoeffs, e->coef.size());
}
void drop_staging(Binding &b)
{
    if (b.ctx) { msdr_mapped_free(b.ctx, b.h_in); msdr_mapped_free(b.ctx, b.h_out); msdr_mapped_free(b.ctx, b.h_in2); }
    b.h_in = b.h_out = b.d_in = b.d_out = b.h_in2 = b.d_in2 = nullptr; b.cap = b.cap2 = 0;
}
void drop_rows(Binding &b)
{
    if (b.ctx) for (auto &kv : b.rows) if (kv.second.dev) msdr_free(b.ctx, kv.second.dev);
    b.rows.clear();
    b.ranges.clear();
}
// the pinned staging buffers of the host-array binding: h_in / h_out of >= bytes each, and h_in2 as well when `two`
bool ensure_staging(Binding &b, size_t bytes, bool two)
{
    if (bytes > b.cap) {
        msdr_mapped_free(b.ctx, b.h_in); msdr_mapped_free(b.ctx, b.h_out);
        b.h_in = b.h_out = b.d_in = b.d_out = nullptr; b.cap = 0;
        if (msdr_mapped_alloc(b.ctx, bytes, &b.h_in, &b.d_in) != 0 || msdr_mapped_alloc(b.ctx, bytes, &b.h_out, &b.d_out) != 0) {
            msdr_mapped_free(b.ctx, b.h_in); msdr_mapped_free(b.ctx, b.h_out);
            b.h_in = b.h_out = b.d_in = b.d_out = nullptr;
            return false;
        }
        b.cap = bytes;
    }
    if (two && bytes > b.cap2) {
        msdr_mapped_free(b.ctx, b.h_in2);
        b.h_in2 = b.d_in2 = nullptr; b.cap2 = 0;
        if (msdr_mapped_alloc(b.ctx, bytes, &b.h_in2, &b.d_in2) != 0) { b.h_in2 = b.d_in2 = nullptr; return false; }
        b.cap2 = bytes;
    }
    return true;
}
void refuse(const char *fmt, const char *what)
{
    char text[256];
    snprintf(text, sizeof text, fmt, what);
    msdr_cmsis_fail(MSDR_STATUS_ARGUMENT_ERROR, text);
}
// 1 = device memory of the bound device, 0 = host-readable memory, -1 = device memory of another device (caller holds the lock)
int classify(Binding &b, const void *p)
{
    const unsigned gen = msdr_free_generation();
    if (gen != b.gen) { b.ranges.clear(); b.gen = gen; }
    const uintptr_t u = (uintptr_t)p;
    for (size_t i = 0; i < b.ranges.size(); i++) {
        if (u - b.ranges[i].base < b.ranges[i].size) {
            if (i) std::swap(b.ranges[i], b.ranges[0]);
            return 1;
        }
    }
    uintptr_t base = 0;
    size_t size = 0;
    const int k = msdr_ptr_query(b.ctx, p, &base, &size);
    if (k == 1) {
        b.ranges.insert(b.ranges.begin(), Binding::Range{base, size});
        if (b.ranges.size() > 16) b.ranges.pop_back();
    }
    return k;
}
// msdr_cmsis_bind: a source operand as the kernels take it -- the caller's device batch (stride blockSize), or the device copy of a shared
// host row (stride 0), uploaded again when its bytes changed.  nullptr = refused (msdr_last_error() has the text).
const q15_t *device_source(Binding &b, const q15_t *p, uint32_t blockSize, uint64_t *stride, const char *what)
{
    const int k = classify(b, p);
    if (k == 1) { *stride = blockSize; return p; }
    if (k < 0) { refuse("%s: a source in device memory of another device", what); return nullptr; }
    const size_t bytes = (size_t)blockSize * sizeof(q15_t);
    auto it = b.rows.find(p);
    if (it == b.rows.end()) {
        if (b.rows.size() >= 64) {          // the least recently used row goes
            auto old = b.rows.begin();
            for (auto j = b.rows.begin(); j != b.rows.end(); ++j) if (j->second.used < old->second.used) old = j;
            if (old->second.dev) msdr_free(b.ctx, old->second.dev);
            b.rows.erase(old);
        }
        it = b.rows.emplace(p, Binding::Row()).first;
    }
    Binding::Row &r = it->second;
    r.used = ++b.row_clock;
    if (r.cap < bytes) {
        if (r.dev) msdr_free(b.ctx, r.dev);
        r.dev = nullptr; r.cap = 0; r.snap.clear();
        if (msdr_malloc(b.ctx, bytes, &r.dev) != 0) { r.dev = nullptr; return nullptr; }
        r.cap = bytes;
    }
    if (r.snap.size() != bytes || memcmp(r.snap.data(), p, bytes) != 0) {
        r.snap.assign((const char *)p, (const char *)p + bytes);
        if (msdr_memcpy_h2d(b.ctx, r.dev, r.snap.data(), bytes) != 0) { r.snap.clear(); return nullptr; }
    }
    *stride = 0;
    return (const q15_t *)r.dev;
}
// arm_mult_q15 / arm_add_q15 / arm_sub_q15 (two sources) and arm_copy_q15 (pSrcB null) under either binding
template <typename Run>
void elementwise(const q15_t *pSrcA, const q15_t *pSrcB, q15_t *pDst, uint32_t blockSize, bool two, const char *what, Run &&run)
{
    Binding &b = binding();
    std::lock_guard<std::mutex> g(b.mu);
    if (!b.ctx) { refuse("%s: no context bound (msdr_cmsis_bind / msdr_cmsis_bind_host first); nothing written", what); return; }
    if (blockSize == 0) return;
    if (!pSrcA || !pDst || (two && !pSrcB)) { refuse("%s: null buffer", what); return; }
    if (!b.host) {
        if (classify(b, pDst) != 1) { refuse("%s: pDst is not device memory of the bound device (msdr_cmsis_bind); nothing written", what); return; }
        uint64_t sa = 0, sb = 0;
        const q15_t *a = device_source(b, pSrcA, blockSize, &sa, what);
        const q15_t *s2 = two ? device_source(b, pSrcB, blockSize, &sb, what) : nullptr;
        if (!a || (two && !s2)) return;
        (void)run(b.ctx, a, sa, s2, sb, pDst, b.channels, blockSize);
        return;
    }
    if (classify(b, pSrcA) != 0 || classify(b, pDst) != 0 || (two && classify(b, pSrcB) != 0)) {
        refuse("%s: a device pointer under msdr_cmsis_bind_host (operands are host arrays); nothing written", what);
        return;
    }
    const size_t bytes = (size_t)b.channels * blockSize * sizeof(q15_t);
    if (!two) { memmove(pDst, pSrcA, bytes); return; }          // arm_copy_q15 between host arrays: no device involved
    if (!ensure_staging(b, bytes, true)) return;
    memcpy(b.h_in, pSrcA, bytes);
    memcpy(b.h_in2, pSrcB, bytes);
    if (run(b.ctx, (const q15_t *)b.d_in, blockSize, (const q15_t *)b.d_in2, blockSize, (q15_t *)b.d_out, b.channels, blockSize) != 0) return;
    if (msdr_ctx_synchronize(b.ctx) != 0) return;
    memcpy(pDst, b.h_out, bytes);
}
// the library-owned complex-FFT instance msdr_arm_rfft_init_q15 points pCfft at: {64, twiddleCoef_64_q15, no bit-reversal table}
const msdr_arm_cfft_instance_q15 *cfft64()
{
    static q15_t twiddle[96];
    static const msdr_arm_cfft_instance_q15 inst = [] {
        int16_t t[352];
        msdr_rfft128_tables(t);
        memcpy(twiddle, t, sizeof twiddle);
        return msdr_arm_cfft_instance_q15{64, twiddle, nullptr, 0};
    }();
    return &inst;
}
// host-array binding: the block batch [channels][blockSize] of `esz`-byte samples goes into the pinned input buffer, `run` reads it and writes
// the pinned output buffer over PCIe, and the call returns when pDst holds the result, as the CMSIS function does.  Device-pointer binding:
// `run` on the caller's pointers.
template <typename Run>
void with_buffers(Binding &b, const void *pSrc, void *pDst, uint32_t blockSize, size_t esz, Run &&run)
{
    if (!b.host) { (void)run(pSrc, pDst); return; }
    const size_t bytes = (size_t)b.channels * blockSize * esz;
    if (bytes == 0 || !pSrc || !pDst) return;
    if (bytes > b.cap) {
        drop_staging(b);
        if (msdr_mapped_alloc(b.ctx, bytes, &b.h_in, &b.d_in) != 0 || msdr_mapped_alloc(b.ctx, bytes, &b.h_out, &b.d_out) != 0) { drop_staging(b); return; }
        b.cap = bytes;
    }
    memcpy(b.h_in, pSrc, bytes);
    if (run(b.d_in, b.d_out) != 0) return;
    if (msdr_ctx_synchronize(b.ctx) != 0) return;
    memcpy(pDst, b.h_out, bytes);
}

}  // namespace

// msdr_ctx_destroy calls this (msdr_api.hip): a context that goes away takes its binding and the objects made through it along,
// so that no msdr_arm_* call can reach a dangling handle.  Not part of the C ABI.
__attribute__((visibility("hidden"))) void msdr_cmsis_ctx_gone(msdr_ctx *ctx)
{
    Binding &b = binding();
    std::lock_guard<std::mutex> g(b.mu);
    if (b.ctx != ctx) return;
    for (auto &kv : b.inst) destroy(kv.second);
    b.inst.clear();
    drop_staging(b);
    drop_rows(b);
    b.ctx = nullptr; b.channels = 0; b.host = false;
}

static int bind_common(msdr_ctx *ctx, uint32_t channels, bool host)
{
    Binding &b = binding();
    std::lock_guard<std::mutex> g(b.mu);
    for (auto &kv : b.inst) destroy(kv.second);    // objects of the previous binding go with it
    b.inst.clear();
    drop_staging(b);
    drop_rows(b);
    b.ctx = ctx; b.channels = ctx ? channels : 0; b.host = ctx ? host : false;
    return (ctx && channels == 0) ? MSDR_STATUS_ARGUMENT_ERROR : MSDR_STATUS_SUCCESS;
}
extern "C" int msdr_cmsis_bind(msdr_ctx *ctx, uint32_t channels) { return bind_common(ctx, channels, false); }
extern "C" int msdr_cmsis_bind_host(msdr_ctx *ctx, uint32_t channels) { return bind_common(ctx, channels, true); }

extern "C" msdr_arm_status msdr_arm_fir_init_q15(msdr_arm_fir_instance_q15 *S, uint16_t numTaps, q15_t *pCoeffs, q15_t *pState, uint32_t blockSize)
{
    if (numTaps & 1u) return MSDR_ARM_MATH_ARGUMENT_ERROR;                       // arm_fir_init_q15.c:93-96: status only, S untouched
    S->numTaps = numTaps; S->pCoeffs = pCoeffs; S->pState = pState;              // :100-109
    if (pState) memset(pState, 0, ((size_t)numTaps + blockSize) * sizeof(q15_t));   // :106
    Binding &b = binding();
    std::lock_guard<std::mutex> g(b.mu);
    msdr_fir_q15 *h = nullptr;
    if (!b.ctx || msdr_fir_q15_create(b.ctx, numTaps, pCoeffs, b.channels, &h) != 0) { forget(S); return MSDR_ARM_MATH_ARGUMENT_ERROR; }
    remember(S, 0, h, pCoeffs, (size_t)numTaps * sizeof(q15_t));
    return MSDR_ARM_MATH_SUCCESS;
}
extern "C" void msdr_arm_fir_fast_q15(const msdr_arm_fir_instance_q15 *S, q15_t *pSrc, q15_t *pDst, uint32_t blockSize)
{
    std::lock_guard<std::mutex> g(binding().mu);
    Entry *e = lookup_locked(S, 0);
    if (!e) return;
    follow_coeffs(e, S->pCoeffs, [&] { return msdr_fir_q15_set_coeffs((msdr_fir_q15 *)e->handle, S->pCoeffs); });
    with_buffers(binding(), pSrc, pDst, blockSize, sizeof(q15_t), [&](const void *src, void *dst) { return msdr_fir_q15_process((msdr_fir_q15 *)e->handle, (const q15_t *)src, (q15_t *)dst, blockSize); });
}

extern "C" void msdr_arm_fir_init_f32(msdr_arm_fir_instance_f32 *S, uint16_t numTaps, float32_t *pCoeffs, float32_t *pState, uint32_t blockSize)
{
    S->numTaps = numTaps; S->pCoeffs = pCoeffs; S->pState = pState;
    if (pState && numTaps) memset(pState, 0, ((size_t)numTaps + blockSize - 1u) * sizeof(float32_t));     // state length arm_math.h:1050
    Binding &b = binding();
    std::lock_guard<std::mutex> g(b.mu);
    msdr_fir_f32 *h = nullptr;
    if (b.ctx && msdr_fir_f32_create(b.ctx, numTaps, pCoeffs, b.channels, &h) == 0) remember(S, 1, h, pCoeffs, (size_t)numTaps * sizeof(float32_t));
    else forget(S);
}
extern "C" void msdr_arm_fir_f32(const msdr_arm_fir_instance_f32 *S, float32_t *pSrc, float32_t *pDst, uint32_t blockSize)
{
    std::lock_guard<std::mutex> g(binding().mu);
    Entry *e = lookup_locked(S, 1);
    if (!e) return;
    follow_coeffs(e, S->pCoeffs, [&] { return msdr_fir_f32_set_coeffs((msdr_fir_f32 *)e->handle, S->pCoeffs); });
    with_buffers(binding(), pSrc, pDst, blockSize, sizeof(float32_t), [&](const void *src, void *dst) { return msdr_fir_f32_process((msdr_fir_f32 *)e->handle, (const float32_t *)src, (float32_t *)dst, blockSize); });
}

extern "C" void msdr_arm_biquad_cascade_df1_init_f32(msdr_arm_biquad_casd_df1_inst_f32 *S, uint8_t numStages, float32_t *pCoeffs, float32_t *pState)
{
    S->numStages = numStages; S->pCoeffs = pCoeffs; S->pState = pState;
    if (pState) memset(pState, 0, (size_t)4 * numStages * sizeof(float32_t));    // 4 state values per stage, arm_math.h:1233
    Binding &b = binding();
    std::lock_guard<std::mutex> g(b.mu);
    msdr_biquad_df1_f32 *h = nullptr;
    if (b.ctx && msdr_biquad_df1_f32_create(b.ctx, numStages, pCoeffs, b.channels, &h) == 0) remember(S, 2, h, pCoeffs, (size_t)5 * numStages * sizeof(float32_t));
    else forget(S);
}
extern "C" void msdr_arm_biquad_cascade_df1_f32(const msdr_arm_biquad_casd_df1_inst_f32 *S, float32_t *pSrc, float32_t *pDst, uint32_t blockSize)
{
    std::lock_guard<std::mutex> g(binding().mu);
    Entry *e = lookup_locked(S, 2);
    if (!e) return;
    follow_coeffs(e, S->pCoeffs, [&] { return msdr_biquad_df1_f32_set_coeffs((msdr_biquad_df1_f32 *)e->handle, S->pCoeffs); });
    with_buffers(binding(), pSrc, pDst, blockSize, sizeof(float32_t), [&](const void *src, void *dst) { return msdr_biquad_df1_f32_process((msdr_biquad_df1_f32 *)e->handle, (const float32_t *)src, (float32_t *)dst, blockSize); });
}

extern "C" void msdr_arm_mult_q15(q15_t *pSrcA, q15_t *pSrcB, q15_t *pDst, uint32_t blockSize)
{
    elementwise(pSrcA, pSrcB, pDst, blockSize, true, "arm_mult_q15", msdr_mult_q15);
}
extern "C" void msdr_arm_add_q15(q15_t *pSrcA, q15_t *pSrcB, q15_t *pDst, uint32_t blockSize)
{
    elementwise(pSrcA, pSrcB, pDst, blockSize, true, "arm_add_q15", msdr_add_q15);
}
extern "C" void msdr_arm_sub_q15(q15_t *pSrcA, q15_t *pSrcB, q15_t *pDst, uint32_t blockSize)
{
    elementwise(pSrcA, pSrcB, pDst, blockSize, true, "arm_sub_q15", msdr_sub_q15);
}
extern "C" void msdr_arm_copy_q15(q15_t *pSrc, q15_t *pDst, uint32_t blockSize)
{
    elementwise(pSrc, nullptr, pDst, blockSize, false, "arm_copy_q15",
                [](msdr_ctx *ctx, const q15_t *a, uint64_t sa, const q15_t *, uint64_t, q15_t *dst, uint32_t channels, uint32_t n) {
                    return msdr_copy_q15(ctx, a, sa, dst, channels, n);
                });
}

extern "C" msdr_arm_status msdr_arm_rfft_init_q15(msdr_arm_rfft_instance_q15 *S, uint32_t fftLenReal, uint32_t ifftFlagR, uint32_t bitReverseFlag)
{
    // arm_rfft_init_q15.c:2166-2183: the fields first (the length as uint16_t), then the switch on that length
    S->fftLenReal = (uint16_t)fftLenReal;
    S->pTwiddleAReal = nullptr;                  // (CMSIS: realCoefAQ15 / realCoefBQ15, 8192 entries; not held here, not needed)
    S->pTwiddleBReal = nullptr;
    S->ifftFlagR = (uint8_t)ifftFlagR;
    S->bitReverseFlagR = (uint8_t)bitReverseFlag;
    const int rc = msdr_rfft_q15_init_check(S->fftLenReal, S->ifftFlagR, S->bitReverseFlagR);
    if (rc == MSDR_STATUS_ARGUMENT_ERROR) return MSDR_ARM_MATH_ARGUMENT_ERROR;      // :2217-2220: modifier and pCfft untouched
    S->twidCoefRModifier = 8192u / S->fftLenReal;                                // :2185-2216
    if (rc != 0) { S->pCfft = nullptr; return MSDR_ARM_MATH_LENGTH_ERROR; }      // valid for CMSIS, not built here
    S->pCfft = cfft64();
    return MSDR_ARM_MATH_SUCCESS;
}
extern "C" void msdr_arm_rfft_q15(const msdr_arm_rfft_instance_q15 *S, q15_t *pSrc, q15_t *pDst)
{
    Binding &b = binding();
    std::lock_guard<std::mutex> g(b.mu);
    const char *what = "arm_rfft_q15";
    if (!b.ctx) { refuse("%s: no context bound (msdr_cmsis_bind / msdr_cmsis_bind_host first); nothing written", what); return; }
    if (!S || S->pCfft != cfft64() || S->fftLenReal != 128 || S->ifftFlagR != 0 || S->bitReverseFlagR != 1) {
        refuse("%s: the instance was not set up by a successful arm_rfft_init_q15(S, 128, 0, 1); nothing written", what);
        return;
    }
    if (!pSrc || !pDst) { refuse("%s: null buffer", what); return; }
    if (!b.host) {
        if (classify(b, pSrc) != 1 || classify(b, pDst) != 1) {
            refuse("%s: pSrc and pDst must be device memory of the bound device (msdr_cmsis_bind); nothing written", what);
            return;
        }
        (void)msdr_rfft128_q15_inplace(b.ctx, pSrc, 128, pDst, nullptr, b.channels);     // refuses an unaligned pSrc / pDst
        return;
    }
    if (classify(b, pSrc) != 0 || classify(b, pDst) != 0) {
        refuse("%s: a device pointer under msdr_cmsis_bind_host (operands are host arrays); nothing written", what);
        return;
    }
    const size_t in_bytes = (size_t)b.channels * 128 * sizeof(q15_t), out_bytes = 2 * in_bytes;
    if (!ensure_staging(b, out_bytes, false)) return;
    memcpy(b.h_in, pSrc, in_bytes);
    if (msdr_rfft128_q15_inplace(b.ctx, (q15_t *)b.d_in, 128, (q15_t *)b.d_out, nullptr, b.channels) != 0) return;
    if (msdr_ctx_synchronize(b.ctx) != 0) return;
    memcpy(pSrc, b.h_in, in_bytes);                 // the CMSIS work buffer
    memcpy(pDst, b.h_out, out_bytes);
}
