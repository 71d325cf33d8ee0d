// tests/cpp/test_cmsis_relink.cpp -- a C++ program written against the CMSIS-DSP names (MSDR_CMSIS_NAMES): every DSP call below is an
// arm_* call with CMSIS's own argument list, relinked onto libmsdr.so through include/msdr_cmsis.h.
//
//   (a) the FIR section of demodulation() (Minimal-SDR.ino:568-578) with init_FIR()'s globals (:111-114, :901-930) under
//       msdr_cmsis_bind_host(ctx, 1): two arm_fir_fast_q15 and two arm_copy_q15 per block on host stack arrays, and one in-place
//       rewrite of a coefficient array mid-stream (the bandwidth menu, UI.cpp:337-345)
//   (b) a node over AudioStream whose update() is freq_conv.cpp's mult / add / sub sequence on block->data with the host-global
//       oscillator tables, under msdr_cmsis_bind(ctx, 64), wired beside the native AudioEffectFreqConv on the same inputs: both
//       directions, pass = false and a table rewrite mid-stream, outputs bit-exact equal
//   (c) showSpectrum()'s call (UI.cpp:520-551): arm_rfft_init_q15(&FFT, 128, 0, 1), arm_rfft_q15(&FFT, data, FFT_out), FFT_out and the
//       clobbered data against the golden answers, on device block batches and on a host array
//
// usage: test_cmsis_relink DATADIR   (the expected answers, raw little-endian int16 files written by tests/test_gpu_cmsis_relink.py)
//        test_cmsis_relink --no-gpu  (the program refuses to run without a device, and the unbound shims write nothing)
// Exit code 0 = every check passed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define MSDR_CMSIS_NAMES
#include "../../include/msdr_cmsis.h"
#include "../../minimal-sdr_amd/host/msdr_nodes.h"

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static const int B = AUDIO_BLOCK_SAMPLES;
static std::string g_dir;

static std::vector<int16_t> load(const char *name)
{
    std::vector<int16_t> v;
    FILE *f = fopen((g_dir + "/" + name).c_str(), "rb");
    if (!f) { CHECK(false, "cannot open %s", name); return v; }
    int16_t buf[4096];
    size_t n;
    while ((n = fread(buf, sizeof(int16_t), 4096, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

// ---- (a) the sketch's FIR globals (Minimal-SDR.ino:111-114) --------------------------------------------------------------------
#define MAX_NUM_TAPS 120
arm_fir_instance_q15 FIR_I, FIR_Q;
q15_t FIR_I_state[MAX_NUM_TAPS + AUDIO_BLOCK_SAMPLES], FIR_Q_state[MAX_NUM_TAPS + AUDIO_BLOCK_SAMPLES];
q15_t FIR_I_coeffs[MAX_NUM_TAPS], FIR_Q_coeffs[MAX_NUM_TAPS];
static int num_taps_i = 0, num_taps_q = 0;

static void init_FIR(void)
{
    memset(FIR_I_state, 0, sizeof FIR_I_state);
    memset(FIR_Q_state, 0, sizeof FIR_Q_state);
    CHECK(arm_fir_init_q15(&FIR_I, num_taps_i, FIR_I_coeffs, FIR_I_state, AUDIO_BLOCK_SAMPLES) == ARM_MATH_SUCCESS, "init FIR_I: %s", msdr_last_error());
    CHECK(arm_fir_init_q15(&FIR_Q, num_taps_q, FIR_Q_coeffs, FIR_Q_state, AUDIO_BLOCK_SAMPLES) == ARM_MATH_SUCCESS, "init FIR_Q: %s", msdr_last_error());
}

// one block of the FIR section: the I / Q buffers in, the filtered blocks back in the same buffers
static void fir_section(int16_t *I_buffer, int16_t *Q_buffer)
{
    q15_t I_FIR_out[AUDIO_BLOCK_SAMPLES];
    q15_t Q_FIR_out[AUDIO_BLOCK_SAMPLES];
    arm_fir_fast_q15(&FIR_I, I_buffer, I_FIR_out, AUDIO_BLOCK_SAMPLES);
    arm_fir_fast_q15(&FIR_Q, Q_buffer, Q_FIR_out, AUDIO_BLOCK_SAMPLES);
    arm_copy_q15(I_FIR_out, I_buffer, AUDIO_BLOCK_SAMPLES);
    arm_copy_q15(Q_FIR_out, Q_buffer, AUDIO_BLOCK_SAMPLES);
}

static void part_a(msdr_ctx *ctx)
{
    const std::vector<int16_t> ti = load("fir_taps_i.bin"), ti2 = load("fir_taps_i2.bin"), tq = load("fir_taps_q.bin");
    const std::vector<int16_t> xi = load("fir_x_i.bin"), xq = load("fir_x_q.bin"), wi = load("fir_want_i.bin"), wq = load("fir_want_q.bin");
    const std::vector<int16_t> when = load("fir_rewrite_block.bin");
    if (ti.empty() || ti.size() != ti2.size() || ti.size() > MAX_NUM_TAPS || tq.size() > MAX_NUM_TAPS || xi.size() != wi.size() ||
        xq.size() != wq.size() || xi.size() != xq.size() || when.size() != 1) { CHECK(false, "(a) inputs"); return; }
    CHECK(msdr_cmsis_bind_host(ctx, 1) == 0, "bind_host: %s", msdr_last_error());
    num_taps_i = (int)ti.size(); num_taps_q = (int)tq.size();
    memcpy(FIR_I_coeffs, ti.data(), ti.size() * sizeof(q15_t));
    memcpy(FIR_Q_coeffs, tq.data(), tq.size() * sizeof(q15_t));
    init_FIR();
    const size_t blocks = xi.size() / B;
    for (size_t k = 0; k < blocks; k++) {
        if ((int)k == when[0]) memcpy(FIR_I_coeffs, ti2.data(), ti2.size() * sizeof(q15_t));     // rewritten in place, no init_FIR()
        int16_t I_buffer[AUDIO_BLOCK_SAMPLES], Q_buffer[AUDIO_BLOCK_SAMPLES];
        memcpy(I_buffer, &xi[k * B], sizeof I_buffer);
        memcpy(Q_buffer, &xq[k * B], sizeof Q_buffer);
        fir_section(I_buffer, Q_buffer);
        CHECK(!memcmp(I_buffer, &wi[k * B], sizeof I_buffer), "(a) I block %zu differs", k);
        CHECK(!memcmp(Q_buffer, &wq[k * B], sizeof Q_buffer), "(a) Q block %zu differs", k);
    }
}

// ---- (b) freq_conv.cpp's update() over the CMSIS names, beside the native node ---------------------------------------------------
q15_t Osc_Q_buffer_i[AUDIO_BLOCK_SAMPLES];
q15_t Osc_I_buffer_i[AUDIO_BLOCK_SAMPLES];

class FreqConvCmsis : public AudioStream {
public:
    FreqConvCmsis() : AudioStream(2, inputQueueArray), dir(0), pass(1) {}
    void direction(bool d) { dir = d; }
    void passthrough(bool p) { pass = p; }
    virtual void update(void)
    {
        audio_block_t *blockI = receiveWritable(0), *blockQ = receiveWritable(1);
        if (!blockI) { if (blockQ) release(blockQ); return; }
        if (!blockQ) { release(blockI); return; }
        if (!pass) {
            transmit(blockI, 0); transmit(blockQ, 1);
            release(blockI); release(blockQ);
            return;
        }
        audio_block_t *blockA = allocate(), *blockB = allocate(), *blockC = allocate(), *blockD = allocate();
        if (blockA && blockB && blockC && blockD) {
            if (!dir) {
                arm_mult_q15((q15_t *)blockI->data, (q15_t *)Osc_Q_buffer_i, (q15_t *)blockA->data, AUDIO_BLOCK_SAMPLES);     // A = I * sinQ
                arm_mult_q15((q15_t *)blockQ->data, (q15_t *)Osc_I_buffer_i, (q15_t *)blockB->data, AUDIO_BLOCK_SAMPLES);     // B = Q * sinI
                arm_mult_q15((q15_t *)blockQ->data, (q15_t *)Osc_Q_buffer_i, (q15_t *)blockC->data, AUDIO_BLOCK_SAMPLES);     // C = Q * sinQ
                arm_mult_q15((q15_t *)blockI->data, (q15_t *)Osc_I_buffer_i, (q15_t *)blockD->data, AUDIO_BLOCK_SAMPLES);     // D = I * sinI
                arm_add_q15((q15_t *)blockA->data, (q15_t *)blockB->data, (q15_t *)blockI->data, AUDIO_BLOCK_SAMPLES);        // I = A + B
                arm_sub_q15((q15_t *)blockC->data, (q15_t *)blockD->data, (q15_t *)blockQ->data, AUDIO_BLOCK_SAMPLES);        // Q = C - D
            } else {
                arm_mult_q15((q15_t *)blockQ->data, (q15_t *)Osc_Q_buffer_i, (q15_t *)blockA->data, AUDIO_BLOCK_SAMPLES);     // A = Q * sinQ
                arm_mult_q15((q15_t *)blockI->data, (q15_t *)Osc_I_buffer_i, (q15_t *)blockB->data, AUDIO_BLOCK_SAMPLES);     // B = I * sinI
                arm_mult_q15((q15_t *)blockI->data, (q15_t *)Osc_Q_buffer_i, (q15_t *)blockC->data, AUDIO_BLOCK_SAMPLES);     // C = I * sinQ
                arm_mult_q15((q15_t *)blockQ->data, (q15_t *)Osc_I_buffer_i, (q15_t *)blockD->data, AUDIO_BLOCK_SAMPLES);     // D = Q * sinI
                arm_add_q15((q15_t *)blockA->data, (q15_t *)blockB->data, (q15_t *)blockQ->data, AUDIO_BLOCK_SAMPLES);        // Q = A + B
                arm_sub_q15((q15_t *)blockC->data, (q15_t *)blockD->data, (q15_t *)blockI->data, AUDIO_BLOCK_SAMPLES);        // I = C - D
            }
            transmit(blockI, 0);
            transmit(blockQ, 1);
        }
        if (blockA) release(blockA);
        if (blockB) release(blockB);
        if (blockC) release(blockC);
        if (blockD) release(blockD);
        release(blockI);
        release(blockQ);
    }

private:
    audio_block_t *inputQueueArray[2];
    bool dir, pass;
};

// a source node fed with host data [channels][128]
class HostSource : public AudioStream {
public:
    HostSource() : AudioStream(0, nullptr), next(nullptr) {}
    const int16_t *next;
    virtual void update(void)
    {
        if (!next) return;
        audio_block_t *b = allocate();
        if (!b) return;
        msdr_memcpy_h2d(AudioGPU.context(), b->data, next, AudioGPU.block_bytes());
        transmit(b);
        release(b);
        next = nullptr;
    }
};

static HostSource src_i, src_q;
static FreqConvCmsis conv_cmsis;
static AudioEffectFreqConv conv_native;
static AudioRecordQueue cap_ci, cap_cq, cap_ni, cap_nq;
static AudioConnection c1(src_i, 0, conv_cmsis, 0), c2(src_q, 0, conv_cmsis, 1), c3(src_i, 0, conv_native, 0), c4(src_q, 0, conv_native, 1);
static AudioConnection c5(conv_cmsis, 0, cap_ci, 0), c6(conv_cmsis, 1, cap_cq, 0), c7(conv_native, 0, cap_ni, 0), c8(conv_native, 1, cap_nq, 0);

static bool fetch(AudioRecordQueue &q, std::vector<int16_t> &out)
{
    int16_t *d = q.readBuffer();
    out.assign(AudioGPU.block_bytes() / sizeof(int16_t), 0);
    const bool ok = d && msdr_memcpy_d2h(AudioGPU.context(), out.data(), d, AudioGPU.block_bytes()) == 0;
    q.freeBuffer();
    return ok;
}

static void osc_tables(double cycles, double phase)
{
    for (int i = 0; i < B; i++) {
        Osc_I_buffer_i[i] = (q15_t)(32767.0 * __builtin_sin(2 * 3.14159265358979 * cycles * i / B + phase));
        Osc_Q_buffer_i[i] = (q15_t)(32767.0 * __builtin_cos(2 * 3.14159265358979 * cycles * i / B + phase));
    }
    Osc_I_buffer_i[3] = -32768;          // the one product that saturates
}

static void part_b(uint32_t channels)
{
    CHECK(msdr_cmsis_bind(AudioGPU.context(), channels) == 0, "bind: %s", msdr_last_error());
    cap_ci.begin(); cap_cq.begin(); cap_ni.begin(); cap_nq.begin();
    std::vector<int16_t> xi((size_t)channels * B), xq((size_t)channels * B), a, b, c, d;
    osc_tables(32, 0.0);
    // tick: dir, pass, a table rewrite before it
    const struct { bool dir, pass; double retune; } ticks[] = {
        {false, true, 0}, {false, true, 0}, {true, true, 0}, {true, true, 5.0}, {false, true, 0}, {false, false, 0}, {true, false, 0},
        {false, true, 11.5}, {true, true, 0},
    };
    int t = 0;
    for (const auto &tk : ticks) {
        if (tk.retune != 0) osc_tables(tk.retune, 0.3);            // the global tables rewritten in place between two updates
        conv_cmsis.direction(tk.dir); conv_cmsis.passthrough(tk.pass);
        conv_native.direction(tk.dir); conv_native.passthrough(tk.pass);
        for (size_t i = 0; i < xi.size(); i++) {
            xi[i] = (int16_t)((rand() % 65536) - 32768);
            xq[i] = (int16_t)((rand() % 65536) - 32768);
        }
        xi[0] = xq[0] = -32768;
        src_i.next = xi.data(); src_q.next = xq.data();
        AudioStream::update_all();
        const bool got = fetch(cap_ci, a) && fetch(cap_cq, b) && fetch(cap_ni, c) && fetch(cap_nq, d);
        CHECK(got, "(b) tick %d: a capture queue is empty (%s)", t, msdr_last_error());
        CHECK(got && a == c && b == d, "(b) tick %d (dir %d, pass %d): the CMSIS-form node differs from AudioEffectFreqConv", t, (int)tk.dir, (int)tk.pass);
        if (!tk.pass) CHECK(a == xi && b == xq, "(b) tick %d: pass = false must forward untouched", t);
        else CHECK(a != xi, "(b) tick %d: nothing was mixed", t);
        t++;
    }
    CHECK(AudioMemoryUsage() == 0, "(b) blocks leaked: %d", (int)AudioMemoryUsage());
}

// ---- (c) initSpectrum() / showSpectrum()'s transform --------------------------------------------------------------------------
static arm_rfft_instance_q15 FFT;

static void part_c(msdr_ctx *ctx)
{
    const std::vector<int16_t> x = load("fft_x.bin"), want_out = load("fft_out.bin"), want_work = load("fft_work.bin");
    const size_t nfft = x.size() / 128;
    if (nfft == 0 || want_out.size() != nfft * 256 || want_work.size() != x.size()) { CHECK(false, "(c) inputs"); return; }
    CHECK(arm_rfft_init_q15(&FFT, 128, 0, 1) == ARM_MATH_SUCCESS, "arm_rfft_init_q15");
    arm_rfft_instance_q15 other;
    CHECK(arm_rfft_init_q15(&other, 256, 0, 1) == ARM_MATH_LENGTH_ERROR, "only the 128-point transform is built");
    CHECK(arm_rfft_init_q15(&other, 100, 0, 1) == ARM_MATH_ARGUMENT_ERROR, "100 is no RFFT length");
    // device block batch: `data` is the block the sketch hands on to AGC(p_adc)
    CHECK(msdr_cmsis_bind(ctx, (uint32_t)nfft) == 0, "bind: %s", msdr_last_error());
    void *d_data = nullptr, *d_out = nullptr;
    CHECK(msdr_malloc(ctx, x.size() * 2, &d_data) == 0 && msdr_malloc(ctx, nfft * 512, &d_out) == 0, "malloc");
    msdr_memcpy_h2d(ctx, d_data, x.data(), x.size() * 2);
    arm_rfft_q15(&FFT, (q15_t *)d_data, (q15_t *)d_out);
    std::vector<int16_t> got_work(x.size()), got_out(nfft * 256);
    msdr_memcpy_d2h(ctx, got_work.data(), d_data, x.size() * 2);
    msdr_memcpy_d2h(ctx, got_out.data(), d_out, nfft * 512);
    CHECK(got_out == want_out, "(c) device FFT_out differs: %s", msdr_last_error());
    CHECK(got_work == want_work, "(c) device data after arm_rfft_q15 is not the CMSIS work buffer");
    msdr_free(ctx, d_data);
    msdr_free(ctx, d_out);
    // a host array of one block, as on the Teensy (FFT_out[264], UI.cpp:547)
    CHECK(msdr_cmsis_bind_host(ctx, 1) == 0, "bind_host: %s", msdr_last_error());
    for (size_t f = 0; f < nfft; f++) {
        int16_t data[128], FFT_out[264];
        memcpy(data, &x[f * 128], sizeof data);
        arm_rfft_q15(&FFT, data, FFT_out);
        CHECK(!memcmp(FFT_out, &want_out[f * 256], 512) && !memcmp(data, &want_work[f * 128], 256), "(c) host transform %zu differs", f);
    }
}

int main(int argc, char **argv)
{
    if (argc < 2) { printf("usage: %s DATADIR | --no-gpu\n", argv[0]); return 2; }
    if (!strcmp(argv[1], "--no-gpu")) {
        // unbound: the shims write nothing and say why
        msdr_cmsis_bind(nullptr, 0);
        int16_t a[8] = {1, 2, 3, 4, 5, 6, 7, 8}, b[8] = {1, 1, 1, 1, 1, 1, 1, 1}, y[8] = {9, 9, 9, 9, 9, 9, 9, 9};
        arm_add_q15(a, b, y, 8);
        arm_copy_q15(a, y, 8);
        bool untouched = true;
        for (int i = 0; i < 8; i++) untouched &= y[i] == 9;
        CHECK(untouched && strstr(msdr_last_error(), "no context bound"), "unbound shims must write nothing (%s)", msdr_last_error());
        CHECK(arm_rfft_init_q15(&FFT, 128, 0, 1) == ARM_MATH_SUCCESS && FFT.twidCoefRModifier == 64, "arm_rfft_init_q15 needs no device");
        int16_t out[264] = {0};
        int16_t data[128] = {0};
        data[0] = 1000;
        arm_rfft_q15(&FFT, data, out);
        CHECK(data[0] == 1000 && out[0] == 0, "unbound arm_rfft_q15 must write nothing");
        if (msdr_device_count() == 0) {
            const int rc = AudioGPU.begin(0, 64);
            CHECK(rc == MSDR_STATUS_NO_DEVICE, "begin() without a GPU returned %d", rc);
        }
        printf("no-gpu path: %s\n", fails ? "FAILED" : "OK");
        return fails ? 1 : 0;
    }
    g_dir = argv[1];
    const uint32_t channels = 64;
    if (AudioGPU.begin(0, channels) != 0) { printf("AudioGPU.begin failed: %s\n", msdr_last_error()); return 2; }
    if (AudioMemory(40) != 0) { printf("AudioMemory failed: %s\n", msdr_last_error()); return 2; }
    part_a(AudioGPU.context());
    part_b(channels);
    part_c(AudioGPU.context());
    msdr_cmsis_bind(nullptr, 0);
    AudioGPU.end();
    printf("%s (a) FIR section under bind_host, (b) freq_conv node vs AudioEffectFreqConv, (c) arm_rfft_q15\n", fails ? "FAILED" : "OK");
    return fails ? 1 : 0;
}
