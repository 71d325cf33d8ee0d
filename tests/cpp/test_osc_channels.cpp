// tests/cpp/test_osc_channels.cpp -- the sketch's receive path  queue_adc -> demodulation() -> queue_dac  (Minimal-SDR.ino:518-775) for a bank of
// receivers over the AudioStream runtime, every receiver mixing with the oscillator tables of its own tuning as tune() sets them:
//     demod.setOscChannel(rx, Osc_I_buffer_i of rx, Osc_Q_buffer_i of rx);     (Minimal-SDR.ino:328-368, freq_conv.h:33-34)
//
// usage: test_osc_channels DATADIR   raw little-endian files written by tests/test_gpu_osc_channels_nodes.py:
//            osc_i.bin, osc_q.bin   int16 [channels][128]   the tables of every receiver
//            retune.bin             int16 [3 + 2 * count * 128]   {block, first receiver, count, count new osc_i rows, count new osc_q rows}:
//                                   changed before that block
//            taps.bin               int16 [102]             the AM tap set the chain is created with
//            x.bin, want.bin        int16 [blocks][channels][128]   IF blocks and the oracle's audio blocks
//        test_osc_channels --no-gpu  (argument errors on a machine without a device)
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

AudioPlayQueue queue_adc;
AudioSDRDemodulator demod;
AudioRecordQueue capture;
AudioConnection patchCord1(queue_adc, 0, demod, 0);
AudioConnection patchCord2(demod, 0, capture, 0);

int main(int argc, char **argv)
{
    if (argc < 2) { printf("usage: %s DATADIR | --no-gpu\n", argv[0]); return 2; }
    if (!strcmp(argv[1], "--no-gpu")) {
        // a demodulator without a chain refuses; the library refuses null handles before it looks at anything else
        int16_t tab[B];
        memset(tab, 0, sizeof tab);
        CHECK(demod.setOscChannel(0, tab, tab) == MSDR_STATUS_ARGUMENT_ERROR, "a demodulator without a chain must refuse");
        CHECK(demod.setOsc(tab, tab) == MSDR_STATUS_ARGUMENT_ERROR, "a demodulator without a chain must refuse");
        CHECK(msdr_chain_set_osc_channels(nullptr, 0, 1, tab, tab) == MSDR_STATUS_ARGUMENT_ERROR, "null chain");
        CHECK(msdr_chain_set_osc_channels(nullptr, 0, 0, nullptr, nullptr) == MSDR_STATUS_ARGUMENT_ERROR, "null chain, count 0");
        if (msdr_device_count() == 0) {
            const int rc = AudioGPU.begin(0, 8);
            CHECK(rc == MSDR_STATUS_NO_DEVICE, "begin() without a GPU returned %d", rc);
        }
        printf("no-gpu path: %s\n", fails ? "FAILED" : "OK");
        return fails ? 1 : 0;
    }
    g_dir = argv[1];
    const std::vector<int16_t> osc_i = load<int16_t>("osc_i.bin"), osc_q = load<int16_t>("osc_q.bin"), retune = load<int16_t>("retune.bin");
    const std::vector<int16_t> taps = load<int16_t>("taps.bin"), x = load<int16_t>("x.bin"), want = load<int16_t>("want.bin");
    const uint32_t channels = (uint32_t)(osc_i.size() / B);
    if (!channels || osc_i.size() != (size_t)channels * B || osc_q.size() != osc_i.size() || taps.empty() || (taps.size() & 1) || retune.size() < 3 ||
        retune[2] < 0 || retune.size() != 3 + 2 * (size_t)retune[2] * B || x.empty() || x.size() != want.size() || x.size() % ((size_t)channels * B)) { printf("FAILED: inputs\n"); return 2; }
    const size_t per_block = (size_t)channels * B, blocks = x.size() / per_block;
    const size_t retune_block = (size_t)retune[0];
    const uint32_t retune_first = (uint32_t)retune[1], retune_count = (uint32_t)retune[2];
    const int16_t *new_i = retune.data() + 3, *new_q = new_i + (size_t)retune_count * B;

    if (AudioGPU.begin(0, channels) != 0) { printf("AudioGPU.begin failed: %s\n", msdr_last_error()); return 2; }
    if (AudioMemory(16) != 0) { printf("AudioMemory failed: %s\n", msdr_last_error()); return 2; }
    msdr_chain_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg; cfg.arith = MSDR_ARITH_Q15; cfg.channels = channels; cfg.mixer = MSDR_MIXER_NCO;
    cfg.num_taps = (uint32_t)taps.size(); cfg.num_tapsets = 1; cfg.coeffs_i[0] = taps.data(); cfg.coeffs_q[0] = taps.data();
    cfg.osc_len = B; cfg.osc_i = osc_i.data(); cfg.osc_q = osc_q.data();          // receiver 0's tables for everybody, until each gets its own
    cfg.default_mode = MSDR_MODE_AM;
    if (demod.begin(cfg) != 0) { printf("demod.begin failed: %s\n", msdr_last_error()); return 2; }
    for (uint32_t rx = 0; rx < channels; rx++)
        CHECK(demod.setOscChannel(rx, &osc_i[(size_t)rx * B], &osc_q[(size_t)rx * B]) == 0, "setOscChannel(%u): %s", rx, msdr_last_error());
    CHECK(demod.setOscChannel(channels, osc_i.data(), osc_q.data()) == MSDR_STATUS_ARGUMENT_ERROR, "a receiver past the bank must be refused");
    CHECK(demod.setOscChannel(0, nullptr, osc_q.data()) == MSDR_STATUS_ARGUMENT_ERROR, "a null table must be refused");

    capture.begin();
    std::vector<int16_t> got(per_block);
    for (size_t k = 0; k < blocks; k++) {
        if (k == retune_block)
            for (uint32_t i = 0; i < retune_count; i++)
                CHECK(demod.setOscChannel(retune_first + i, new_i + (size_t)i * B, new_q + (size_t)i * B) == 0, "retune %u: %s", retune_first + i, msdr_last_error());
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
        for (uint32_t rx = 0; rx < channels; rx++)
            CHECK(!memcmp(&got[(size_t)rx * B], &want[k * per_block + (size_t)rx * B], B * sizeof(int16_t)), "block %zu receiver %u differs", k, rx);
    }
    capture.end();
    capture.clear();
    CHECK(AudioMemoryUsage() == 0, "blocks leaked: %d", (int)AudioMemoryUsage());
    printf("%s queue_adc -> demodulator -> capture, %u receivers x %zu blocks, every receiver its own oscillator tables\n", fails ? "FAILED" : "OK", channels, blocks);
    return fails ? 1 : 0;
}
