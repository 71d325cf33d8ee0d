// tests/cpp/test_complex_input.cpp -- a complex antenna stream through the AudioStream runtime: two play queues (I, Q) -> AudioSDRDemodulator with
// setNco + setComplexInput(true, 0) -> record queue, for a bank of receivers:
//     demod.setNco(steps, phases);  demod.setComplexInput(true, 0);  ... AudioStream::update_all() ...
//
// usage: test_complex_input DATADIR   raw little-endian files written by tests/test_gpu_complex_input_nodes.py:
//            nco.bin                uint32 [2][channels]    steps, start phases
//            taps.bin               int16 [102]             the AM tap set the chain is created with
//            xi.bin, xq.bin         int16 [blocks][channels][128]   the I and the Q blocks
//            want.bin               int16 [blocks][channels][128]   the composed oracle's audio of the complex stream, dir 0
//            real.bin               int16 [blocks][channels][128]   the oracle's audio of the real stream xi
//        test_complex_input --no-gpu  (argument errors on a machine without a device)
// Exit code 0 = every check passed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../minimal-sdr_amd/host/msdr_nodes.h"

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static const int B = AUDIO_BLOCK_SAMPLES;
static std::string g_dir;

template <typename T>
static std::vector<T> load(const char *name)
{
    std::vector<T> v;
    FILE *f = fopen((g_dir + "/" + name).c_str(), "rb");
    if (!f) { CHECK(false, "cannot open %s", name); return v; }
    T buf[4096];
    size_t n;
    while ((n = fread(buf, sizeof(T), 4096, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

AudioPlayQueue queue_i, queue_q;
AudioSDRDemodulator demod;
AudioRecordQueue capture;
AudioConnection patchCord1(queue_i, 0, demod, 0);
AudioConnection patchCord2(queue_q, 0, demod, 1);
AudioConnection patchCord3(demod, 0, capture, 0);

// one tick: the I block, the Q block (nullptr: that queue plays nothing), the audio the graph hands out
static void tick(size_t k, const int16_t *bi, const int16_t *bq, std::vector<int16_t> &audio)
{
    const int16_t *src[2] = {bi, bq};
    AudioPlayQueue *q[2] = {&queue_i, &queue_q};
    for (int j = 0; j < 2; j++) {
        if (!src[j]) continue;
        int16_t *p = q[j]->getBuffer();
        CHECK(p != nullptr, "block %zu: no buffer", k);
        if (!p) return;
        msdr_memcpy_h2d(AudioGPU.context(), p, src[j], AudioGPU.block_bytes());
        CHECK(q[j]->playBuffer(), "block %zu: playBuffer", k);
    }
    AudioStream::update_all();
    int16_t *d = capture.readBuffer();
    CHECK(d != nullptr, "block %zu: nothing captured", k);
    if (d) CHECK(msdr_memcpy_d2h(AudioGPU.context(), audio.data(), d, AudioGPU.block_bytes()) == 0, "d2h: %s", msdr_last_error());
    capture.freeBuffer();
}

int main(int argc, char **argv)
{
    if (argc < 2) { printf("usage: %s DATADIR | --no-gpu\n", argv[0]); return 2; }
    if (!strcmp(argv[1], "--no-gpu")) {
        // a demodulator without a chain refuses; the library refuses a null chain before it looks at anything else
        int on = 7, dir = 7;
        CHECK(demod.setComplexInput(true, 0) == MSDR_STATUS_ARGUMENT_ERROR && demod.setComplexInput(false, 0) == MSDR_STATUS_ARGUMENT_ERROR, "a demodulator without a chain must refuse");
        CHECK(msdr_chain_set_complex_input(nullptr, 1, 0) == MSDR_STATUS_ARGUMENT_ERROR, "null chain");
        CHECK(msdr_chain_get_complex_input(nullptr, &on, &dir) == MSDR_STATUS_ARGUMENT_ERROR && on == 7 && dir == 7, "null chain");
        CHECK((unsigned)MSDR_FLAVOUR_COMPLEX_IN == 0x800000u, "the flavour bit");
        if (msdr_device_count() == 0) {
            const int rc = AudioGPU.begin(0, 8);
            CHECK(rc == MSDR_STATUS_NO_DEVICE, "begin() without a GPU returned %d", rc);
        }
        printf("no-gpu path: %s\n", fails ? "FAILED" : "OK");
        return fails ? 1 : 0;
    }
    g_dir = argv[1];
    const std::vector<uint32_t> nco = load<uint32_t>("nco.bin");
    const std::vector<int16_t> taps = load<int16_t>("taps.bin"), xi = load<int16_t>("xi.bin"), xq = load<int16_t>("xq.bin"), want = load<int16_t>("want.bin"),
                               real = load<int16_t>("real.bin");
    const uint32_t channels = (uint32_t)(nco.size() / 2);
    if (!channels || nco.size() != 2 * (size_t)channels || taps.empty() || (taps.size() & 1) || xi.empty() || xi.size() % ((size_t)channels * B) ||
        xq.size() != xi.size() || want.size() != xi.size() || real.size() != xi.size()) { printf("FAILED: inputs\n"); return 2; }
    const size_t per_block = (size_t)channels * B, blocks = xi.size() / per_block;

    if (AudioGPU.begin(0, channels) != 0) { printf("AudioGPU.begin failed: %s\n", msdr_last_error()); return 2; }
    if (AudioMemory(16) != 0) { printf("AudioMemory failed: %s\n", msdr_last_error()); return 2; }
    std::vector<int16_t> osc(B, 0);          // the table mixer's tables at creation; nothing reads them once the oscillators are phase accumulators
    msdr_chain_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg; cfg.arith = MSDR_ARITH_Q15; cfg.channels = channels; cfg.mixer = MSDR_MIXER_NCO;
    cfg.num_taps = (uint32_t)taps.size(); cfg.num_tapsets = 1; cfg.coeffs_i[0] = taps.data(); cfg.coeffs_q[0] = taps.data();
    cfg.osc_len = B; cfg.osc_i = osc.data(); cfg.osc_q = osc.data();
    cfg.default_mode = MSDR_MODE_AM;
    if (demod.begin(cfg) != 0) { printf("demod.begin failed: %s\n", msdr_last_error()); return 2; }
    CHECK(demod.setComplexInput(true, 0) == MSDR_STATUS_ARGUMENT_ERROR, "setComplexInput before setNco must be refused (no phase-accumulator oscillator yet)");
    CHECK(demod.setNco(nco.data(), nco.data() + channels) == 0, "setNco: %s", msdr_last_error());
    CHECK(demod.setComplexInput(true, 2) == MSDR_STATUS_ARGUMENT_ERROR, "dir 2 must be refused");
    CHECK(demod.setComplexInput(true, 0) == 0 && demod.setComplexInput(true, 0) == 0, "setComplexInput: %s", msdr_last_error());

    std::vector<int16_t> audio(per_block, 0);
    capture.begin();
    for (size_t k = 0; k < blocks; k++) {
        tick(k, &xi[k * per_block], &xq[k * per_block], audio);
        CHECK(!memcmp(audio.data(), &want[k * per_block], per_block * sizeof(int16_t)), "block %zu: the audio is not the composed oracle's", k);
    }
    msdr_chain_info info;
    CHECK(demod.info(&info) == 0 && !strncmp(info.kernel, "chain_q15pcn_kernel", 19), "kernel: %s", info.kernel);
    CHECK(demod.setComplexInput(false, 0) == MSDR_STATUS_ARGUMENT_ERROR, "a switch over a history that holds samples must be refused");

    // back to the real input: init_FIR() clears the history, the oscillators start where the first run started, port 1 is released unread
    CHECK(demod.init_FIR() == 0, "init_FIR: %s", msdr_last_error());
    CHECK(demod.setComplexInput(false, 0) == 0, "setComplexInput(false) over a clear history: %s", msdr_last_error());
    CHECK(demod.setNco(nco.data(), nco.data() + channels) == 0, "setNco: %s", msdr_last_error());
    for (size_t k = 0; k < blocks; k++) {
        tick(k, &xi[k * per_block], k == 0 ? &xq[0] : nullptr, audio);
        CHECK(!memcmp(audio.data(), &real[k * per_block], per_block * sizeof(int16_t)), "block %zu: the real-input audio is not the oracle's", k);
    }
    capture.end();
    capture.clear();
    CHECK(AudioMemoryUsage() == 0, "blocks leaked: %d", (int)AudioMemoryUsage());
    printf("%s queue_i, queue_q -> demodulator -> capture, %u receivers x %zu blocks complex, then real\n", fails ? "FAILED" : "OK", channels, blocks);
    return fails ? 1 : 0;
}
