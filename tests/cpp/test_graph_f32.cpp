// tests/cpp/test_graph_f32.cpp -- the sketch's receive path  queue_adc -> demodulation() -> queue_dac  over the AudioStream runtime with an
// fp32 chain behind the int16 audio blocks (MSDR_ARITH_F32 | MSDR_CHAIN_OUT_I16): every receiver its own FIR pair and its own notch, and the
// whole tick in one launch (demod.setBlockKernel(true): chain_f32pcb_kernel).
//
// usage: test_graph_f32 DATADIR   raw little-endian files written by tests/test_host_graph_f32.py:
//            taps.bin   float [channels][102]      every receiver's AM taps (both filters)
//            bq.bin     float [channels][5]        every receiver's notch {b0, b1, b2, -a1, -a2}
//            x.bin      int16 [blocks][channels][128]   IF blocks
//            want.bin   int16 [blocks][channels][128]   the oracle's fp32 chain, converted as arm_float_to_q15
//        test_graph_f32 --no-gpu  (argument errors on a machine without a device)
// The audio must be within 1 LSB of want.bin (the tolerance MSDR_CHAIN_OUT_I16 documents).  Exit code 0 = every check passed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../minimal-sdr_amd/host/msdr_nodes.h"

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static const int B = AUDIO_BLOCK_SAMPLES, NT = 102;
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

AudioPlayQueue queue_adc;
AudioSDRDemodulator demod;
AudioRecordQueue capture;
AudioConnection patchCord1(queue_adc, 0, demod, 0);
AudioConnection patchCord2(demod, 0, capture, 0);

int main(int argc, char **argv)
{
    if (argc < 2) { printf("usage: %s DATADIR | --no-gpu\n", argv[0]); return 2; }
    if (!strcmp(argv[1], "--no-gpu")) {
        float row[NT];
        memset(row, 0, sizeof row);
        msdr_chain_info info;
        CHECK(demod.setBlockKernel(true) == MSDR_STATUS_ARGUMENT_ERROR, "a demodulator without a chain must refuse");
        CHECK(demod.setTapsChannelF32(0, row) == MSDR_STATUS_ARGUMENT_ERROR, "a demodulator without a chain must refuse");
        CHECK(demod.setBiquadCoeffsChannel(0, row) == MSDR_STATUS_ARGUMENT_ERROR, "a demodulator without a chain must refuse");
        CHECK(demod.info(&info) == MSDR_STATUS_ARGUMENT_ERROR, "a demodulator without a chain must refuse");
        CHECK(msdr_chain_set_block_kernel(nullptr, 1) == MSDR_STATUS_ARGUMENT_ERROR, "null chain");
        if (msdr_device_count() == 0) {
            const int rc = AudioGPU.begin(0, 3);
            CHECK(rc == MSDR_STATUS_NO_DEVICE, "begin() without a GPU returned %d", rc);
        }
        printf("no-gpu path: %s\n", fails ? "FAILED" : "OK");
        return fails ? 1 : 0;
    }
    g_dir = argv[1];
    const std::vector<float> taps = load<float>("taps.bin"), bq = load<float>("bq.bin");
    const std::vector<int16_t> x = load<int16_t>("x.bin"), want = load<int16_t>("want.bin");
    const uint32_t channels = (uint32_t)(taps.size() / NT);
    if (!channels || taps.size() != (size_t)channels * NT || bq.size() != (size_t)channels * 5 || x.empty() || x.size() != want.size() ||
        x.size() % ((size_t)channels * B)) { printf("FAILED: inputs\n"); return 2; }
    const size_t per_block = (size_t)channels * B, blocks = x.size() / per_block;

    if (AudioGPU.begin(0, channels) != 0) { printf("AudioGPU.begin failed: %s\n", msdr_last_error()); return 2; }
    if (AudioMemory(16) != 0) { printf("AudioMemory failed: %s\n", msdr_last_error()); return 2; }
    msdr_chain_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg; cfg.arith = MSDR_ARITH_F32; cfg.channels = channels; cfg.mixer = MSDR_MIXER_FS4;
    cfg.num_taps = NT; cfg.num_tapsets = 1; cfg.coeffs_i[0] = taps.data(); cfg.coeffs_q[0] = taps.data();          // receiver 0's taps for everybody, until each gets its own
    cfg.default_mode = MSDR_MODE_AM; cfg.num_biquad_stages = 1; cfg.biquad_coeffs = bq.data();
    CHECK(demod.begin(cfg) == MSDR_STATUS_ARGUMENT_ERROR, "an fp32 chain with float audio has no place behind int16 blocks");
    cfg.flags = MSDR_CHAIN_OUT_I16;
    if (demod.begin(cfg) != 0) { printf("demod.begin failed: %s\n", msdr_last_error()); return 2; }
    CHECK(demod.setBlockKernel(true) == 0, "setBlockKernel: %s", msdr_last_error());
    for (uint32_t rx = 0; rx < channels; rx++) {
        CHECK(demod.setTapsChannelF32(rx, &taps[(size_t)rx * NT]) == 0, "setTapsChannelF32(%u): %s", rx, msdr_last_error());
        CHECK(demod.setBiquadCoeffsChannel(rx, &bq[(size_t)rx * 5]) == 0, "setBiquadCoeffsChannel(%u): %s", rx, msdr_last_error());
    }
    CHECK(demod.setTapsChannelF32(channels, taps.data()) == MSDR_STATUS_ARGUMENT_ERROR, "a receiver past the bank must be refused");

    capture.begin();
    std::vector<int16_t> got(per_block);
    int worst = 0;
    for (size_t k = 0; k < blocks; k++) {
        int16_t *p = queue_adc.getBuffer();
        CHECK(p != nullptr, "block %zu: no buffer", k);
        if (!p) break;
        msdr_memcpy_h2d(AudioGPU.context(), p, &x[k * per_block], AudioGPU.block_bytes());
        CHECK(queue_adc.playBuffer(), "block %zu: playBuffer", k);
        AudioStream::update_all();
        int16_t *d = capture.readBuffer();
        const bool ok = d && msdr_memcpy_d2h(AudioGPU.context(), got.data(), d, AudioGPU.block_bytes()) == 0;
        capture.freeBuffer();
        CHECK(ok, "block %zu: nothing captured (%s)", k, msdr_last_error());
        if (!ok) break;
        msdr_chain_info info;
        CHECK(demod.info(&info) == 0 && !strncmp(info.kernel, "chain_f32pcb_kernel", 19), "block %zu ran %s", k, info.kernel);
        for (size_t i = 0; i < per_block; i++) {
            const int e = abs((int)got[i] - (int)want[k * per_block + i]);
            if (e > worst) worst = e;
        }
        long long energy = 0;
        for (size_t i = 0; i < per_block; i++) energy += abs((int)got[i]);
        CHECK(energy > (long long)per_block * 16, "block %zu is silent", k);
    }
    CHECK(worst <= 1, "worst difference %d LSB", worst);
    capture.end();
    capture.clear();
    CHECK(AudioMemoryUsage() == 0, "blocks leaked: %d", (int)AudioMemoryUsage());
    printf("%s queue_adc -> fp32 demodulator (one launch per tick) -> capture, %u receivers x %zu blocks, worst %d LSB\n", fails ? "FAILED" : "OK", channels, blocks, worst);
    return fails ? 1 : 0;
}
