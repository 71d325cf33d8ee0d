// tests/cpp/test_nco_channels.cpp -- the sketch's receive path  queue_adc -> demodulation() -> queue_dac  (Minimal-SDR.ino:518-775) for a bank of
// receivers over the AudioStream runtime, every receiver's local oscillator a phase accumulator that tune() sets to any frequency:
//     demod.setNco(steps, phases);  demod.tuneChannel(rx, f_hz);     (Minimal-SDR.ino:328-368)
//
// usage: test_nco_channels DATADIR   raw little-endian files written by tests/test_gpu_nco_channels_nodes.py:
//            nco.bin                uint32 [2][channels]    steps, start phases
//            tune.bin               float64 [3 * count]     {before which block, receiver, frequency in Hz} per retune (fs = 24000)
//            taps.bin               int16 [102]             the AM tap set the chain is created with
//            x.bin, want.bin        int16 [blocks][channels][128]   IF blocks and the oracle's audio blocks
//        test_nco_channels --no-gpu  (argument errors on a machine without a device)
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
        // a demodulator without a chain refuses; the library refuses null handles before it looks at anything else; the host functions need no device
        const uint32_t step = 1u << 30;
        uint32_t s = 0, p = 0;
        CHECK(demod.setNco(&step) == MSDR_STATUS_ARGUMENT_ERROR, "a demodulator without a chain must refuse");
        CHECK(demod.tuneChannel(0, 6000.0) == MSDR_STATUS_ARGUMENT_ERROR, "a demodulator without a chain must refuse");
        CHECK(msdr_chain_set_nco_channels(nullptr, 0, 1, &step, nullptr) == MSDR_STATUS_ARGUMENT_ERROR, "null chain");
        CHECK(msdr_chain_set_nco_channels(nullptr, 0, 0, nullptr, nullptr) == MSDR_STATUS_ARGUMENT_ERROR, "null chain, count 0");
        CHECK(msdr_chain_get_nco(nullptr, 0, &s, &p) == MSDR_STATUS_ARGUMENT_ERROR, "null chain");
        CHECK(msdr_nco_step(6000.0, 24000.0) == 0x40000000u && msdr_nco_step(-6000.0, 24000.0) == 0xC0000000u, "msdr_nco_step");
        int16_t tab[1025], sn = 1, cs = 1;
        const uint32_t quarter = 0x40000000u;
        msdr_nco_table(tab);
        msdr_nco_q15(&quarter, 1, &sn, &cs);
        CHECK(tab[0] == 0 && tab[256] == 32767 && tab[1024] == 0 && sn == 32767 && cs == 0, "msdr_nco_table / msdr_nco_q15");
        if (msdr_device_count() == 0) {
            const int rc = AudioGPU.begin(0, 8);
            CHECK(rc == MSDR_STATUS_NO_DEVICE, "begin() without a GPU returned %d", rc);
        }
        printf("no-gpu path: %s\n", fails ? "FAILED" : "OK");
        return fails ? 1 : 0;
    }
    g_dir = argv[1];
    const std::vector<uint32_t> nco = load<uint32_t>("nco.bin");
    const std::vector<double> tune = load<double>("tune.bin");
    const std::vector<int16_t> taps = load<int16_t>("taps.bin"), x = load<int16_t>("x.bin"), want = load<int16_t>("want.bin");
    const uint32_t channels = (uint32_t)(nco.size() / 2);
    if (!channels || nco.size() != 2 * (size_t)channels || tune.size() % 3 || taps.empty() || (taps.size() & 1) || x.empty() || x.size() != want.size() ||
        x.size() % ((size_t)channels * B)) { printf("FAILED: inputs\n"); return 2; }
    const size_t per_block = (size_t)channels * B, blocks = x.size() / per_block;

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
    if (channels > 1) CHECK(demod.tuneChannel(0, 1000.0) == MSDR_STATUS_ARGUMENT_ERROR, "one receiver's tune() before setNco must be refused (the first call names the bank)");
    CHECK(demod.setNco(nullptr) == MSDR_STATUS_ARGUMENT_ERROR, "a null step array must be refused");
    CHECK(demod.setNco(nco.data(), nco.data() + channels) == 0, "setNco: %s", msdr_last_error());
    CHECK(demod.tuneChannel(channels, 1000.0) == MSDR_STATUS_ARGUMENT_ERROR, "a receiver past the bank must be refused");
    CHECK(demod.setOsc(osc.data(), osc.data()) == MSDR_STATUS_ARGUMENT_ERROR, "oscillator tables on a bank of phase accumulators must be refused");

    capture.begin();
    std::vector<int16_t> got(per_block);
    for (size_t k = 0; k < blocks; k++) {
        for (size_t r = 0; r < tune.size(); r += 3)
            if ((size_t)tune[r] == k)
                CHECK(demod.tuneChannel((uint32_t)tune[r + 1], tune[r + 2]) == 0, "tuneChannel(%u): %s", (uint32_t)tune[r + 1], msdr_last_error());
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
    msdr_chain_info info;
    CHECK(demod.info(&info) == 0 && !strncmp(info.kernel, "chain_q15pcn_kernel", 19), "kernel: %s", info.kernel);
    capture.end();
    capture.clear();
    CHECK(AudioMemoryUsage() == 0, "blocks leaked: %d", (int)AudioMemoryUsage());
    printf("%s queue_adc -> demodulator -> capture, %u receivers x %zu blocks, every receiver its own phase-accumulator oscillator\n", fails ? "FAILED" : "OK", channels, blocks);
    return fails ? 1 : 0;
}
