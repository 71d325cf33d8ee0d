// tests/cpp/test_biquad_channels.cpp -- the sketch's output path  queue_dac -> biquad1_dac -> biquad2_dac  (Minimal-SDR.ino:77-81) for a bank of
// receivers, every receiver with the notch of its own frequency as a per-receiver tune() sets it:
//     biquad2_dac.channel(rx).setNotch(0, pdb_freq_actual / 8.0 * CORR_FACT, 15.0);          (Minimal-SDR.ino:356)
// The first half of the receivers is tuned BEFORE AudioGPU.begin (the calls queue in the node, in order with the all-channel calls), the
// second half after it, and a range of receivers is retuned while the graph runs.
//
// usage: test_biquad_channels DATADIR   raw little-endian files written by tests/test_gpu_biquad_channels_nodes.py:
//            notch_hz.bin   float32 [channels]      notch frequency of every receiver
//            retune.bin     float32 [3 + count]     {block, first receiver, count, count new frequencies}: retuned before that block
//            lowpass.bin    float32 [2]             biquad1_dac.setLowpass(0, f, q)
//            x.bin, want.bin int16 [blocks][channels][128]   input blocks and the oracle's output blocks
//        test_biquad_channels --no-gpu  (setters queue without a device; begin() without a GPU says so)
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

// the sketch's graph (Minimal-SDR.ino:73-81), without the I2S output behind it
AudioPlayQueue queue_dac;
AudioFilterBiquad biquad1_dac;
AudioFilterBiquad biquad2_dac;
AudioRecordQueue capture;
AudioConnection patchCord7(queue_dac, 0, biquad1_dac, 0);
AudioConnection patchCord8(biquad1_dac, 0, biquad2_dac, 0);
AudioConnection patchCord9(biquad2_dac, 0, capture, 0);

// tune() of one receiver, its last line
static void tune(uint32_t rx, float notch_hz) { biquad2_dac.channel(rx).setNotch(0, notch_hz, 15.0); }

int main(int argc, char **argv)
{
    if (argc < 2) { printf("usage: %s DATADIR | --no-gpu\n", argv[0]); return 2; }
    if (!strcmp(argv[1], "--no-gpu")) {
        // without a context the setters only queue: nothing is dereferenced, nothing is lost
        biquad1_dac.setLowpass(0, 5400.0f, 0.54f);
        for (uint32_t rx = 0; rx < 8; rx++) tune(rx, 3000.0f + rx);
        const int coef[5] = {1 << 30, 0, 0, 0, 0};
        const double dcoef[5] = {1.0, 0, 0, 0, 0};
        biquad2_dac.channel(3).setCoefficients(1, coef);
        biquad2_dac.channel(3).setCoefficients(2, dcoef);
        biquad2_dac.channel(3).setCoefficients(7, coef);          // filter_biquad.cpp:86: ignored
        biquad2_dac.channel(1).setLowShelf(0, 300.0f, -3.0f);
        biquad2_dac.channel(1).setHighShelf(0, 3000.0f, 3.0f, 0.5f);
        biquad2_dac.channel(2).setBandpass(0, 1000.0f);
        biquad2_dac.channel(2).setHighpass(0, 300.0f);
        biquad2_dac.channel(2).setLowpass(0, 2500.0f, 0.9f);
        int32_t def[32];
        CHECK(biquad2_dac.getDefinition(0, def) == MSDR_STATUS_NO_DEVICE, "getDefinition without a context");
        AudioSDRDemodulator demod;
        CHECK(demod.setNodeNotchChannel(1, 0, 0, 3000.0f, 15.0f) == MSDR_STATUS_ARGUMENT_ERROR, "a demodulator without a chain must refuse");
        CHECK(demod.setNodeCoefficientsChannel(1, 0, 0, coef) == MSDR_STATUS_ARGUMENT_ERROR, "a demodulator without a chain must refuse");
        if (msdr_device_count() == 0) {
            const int rc = AudioGPU.begin(0, 8);
            CHECK(rc == MSDR_STATUS_NO_DEVICE, "begin() without a GPU returned %d", rc);
        }
        printf("no-gpu path: %s\n", fails ? "FAILED" : "OK");
        return fails ? 1 : 0;
    }
    g_dir = argv[1];
    const std::vector<float> hz = load<float>("notch_hz.bin"), retune = load<float>("retune.bin"), lp = load<float>("lowpass.bin");
    const std::vector<int16_t> x = load<int16_t>("x.bin"), want = load<int16_t>("want.bin");
    const uint32_t channels = (uint32_t)hz.size();
    if (!channels || lp.size() != 2 || retune.size() < 3 || retune.size() != 3 + (size_t)retune[2] || x.empty() || x.size() != want.size() ||
        x.size() % ((size_t)channels * B)) { printf("FAILED: inputs\n"); return 2; }
    const size_t per_block = (size_t)channels * B, blocks = x.size() / per_block;
    const size_t retune_block = (size_t)retune[0];
    const uint32_t retune_first = (uint32_t)retune[1], retune_count = (uint32_t)retune[2];

    // setup(): queued, no device yet (Minimal-SDR.ino:391-393 for biquad1_dac; biquad2_dac first gets the bank-wide default notch)
    biquad1_dac.setLowpass(0, lp[0], lp[1]);
    biquad2_dac.setNotch(0, hz[0], 15.0);
    for (uint32_t rx = 0; rx < channels / 2; rx++) tune(rx, hz[rx]);

    if (AudioGPU.begin(0, channels) != 0) { printf("AudioGPU.begin failed: %s\n", msdr_last_error()); return 2; }
    if (AudioMemory(16) != 0) { printf("AudioMemory failed: %s\n", msdr_last_error()); return 2; }
    for (uint32_t rx = channels / 2; rx < channels; rx++) tune(rx, hz[rx]);
    biquad2_dac.channel(channels).setNotch(0, 1000.0f, 15.0);     // no such receiver: refused by the library, no record touched
    CHECK(strstr(msdr_last_error(), "channels"), "a receiver past the bank must be refused (%s)", msdr_last_error());

    capture.begin();
    std::vector<int16_t> got(per_block);
    for (size_t k = 0; k < blocks; k++) {
        if (k == retune_block)
            for (uint32_t i = 0; i < retune_count; i++) tune(retune_first + i, retune[3 + i]);
        int16_t *p = queue_dac.getBuffer();
        CHECK(p != nullptr, "block %zu: no buffer", k);
        if (!p) break;
        msdr_memcpy_h2d(AudioGPU.context(), p, &x[k * per_block], AudioGPU.block_bytes());
        CHECK(queue_dac.playBuffer(), "block %zu: playBuffer", k);
        AudioStream::update_all();
        int16_t *d = capture.readBuffer();
        const bool ok = d && msdr_memcpy_d2h(AudioGPU.context(), got.data(), d, AudioGPU.block_bytes()) == 0;
        capture.freeBuffer();
        CHECK(ok, "block %zu: nothing captured (%s)", k, msdr_last_error());
        if (!ok) break;
        for (uint32_t rx = 0; rx < channels; rx++)
            CHECK(!memcmp(&got[(size_t)rx * B], &want[k * per_block + (size_t)rx * B], B * sizeof(int16_t)), "block %zu receiver %u differs", k, rx);
    }
    // the records themselves: every receiver holds its own b1 (a notch's b1 = -2 cos(w0) / (1 + alpha) moves with the frequency)
    int32_t d0[32], d1[32];
    CHECK(biquad2_dac.getDefinition(0, d0) == 0 && biquad2_dac.getDefinition(channels - 1, d1) == 0, "getDefinition: %s", msdr_last_error());
    CHECK(channels < 2 || d0[1] != d1[1], "receivers 0 and %u hold the same notch", channels - 1);
    capture.end();
    capture.clear();
    CHECK(AudioMemoryUsage() == 0, "blocks leaked: %d", (int)AudioMemoryUsage());
    printf("%s queue_dac -> biquad1_dac -> biquad2_dac, %u receivers x %zu blocks, every receiver its own notch\n", fails ? "FAILED" : "OK", channels, blocks);
    return fails ? 1 : 0;
}
