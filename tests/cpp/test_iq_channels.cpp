// tests/cpp/test_iq_channels.cpp -- the sketch's receive path  queue_adc -> demodulation() -> queue_dac  (Minimal-SDR.ino:518-775) for a bank of
// receivers over the AudioStream runtime with the baseband output its feature list ends with ("Decoding of time signals or other digital
// modes [tbd]", Minimal-SDR.ino:40):
//     demod.setIqOut(true);  ... AudioStream::update_all() ...  demod.readIq(pairs, &n_out);
//
// usage: test_iq_channels DATADIR   raw little-endian files written by tests/test_gpu_iq_channels_nodes.py:
//            nco.bin                uint32 [2][channels]    steps, start phases
//            taps.bin               int16 [102]             the AM tap set the chain is created with
//            x.bin                  int16 [blocks][channels][128]   IF blocks
//            want.bin               int16 [blocks][channels][128][2]   the oracle's pairs {i, q}, per tick and receiver
//        test_iq_channels --no-gpu  (argument errors on a machine without a device)
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
        // a demodulator without a chain refuses; the library refuses a null chain before it looks at anything else
        int16_t pair[2] = {0, 0};
        uint32_t n_out = 0;
        void *p = nullptr;
        uint64_t pitch = 0;
        CHECK(demod.setIqOut(true) == MSDR_STATUS_ARGUMENT_ERROR && demod.setIqOut(false) == MSDR_STATUS_ARGUMENT_ERROR, "a demodulator without a chain must refuse");
        CHECK(demod.readIq(pair, &n_out) == MSDR_STATUS_ARGUMENT_ERROR, "a demodulator without a chain must refuse");
        CHECK(msdr_chain_set_iq_out(nullptr, nullptr, 0) == MSDR_STATUS_ARGUMENT_ERROR, "null chain");
        CHECK(msdr_chain_get_iq_out(nullptr, &p, &pitch) == MSDR_STATUS_ARGUMENT_ERROR, "null chain");
        CHECK((unsigned)MSDR_FLAVOUR_IQ_OUT == 0x400000u, "the flavour bit");
        if (msdr_device_count() == 0) {
            const int rc = AudioGPU.begin(0, 8);
            CHECK(rc == MSDR_STATUS_NO_DEVICE, "begin() without a GPU returned %d", rc);
        }
        printf("no-gpu path: %s\n", fails ? "FAILED" : "OK");
        return fails ? 1 : 0;
    }
    g_dir = argv[1];
    const std::vector<uint32_t> nco = load<uint32_t>("nco.bin");
    const std::vector<int16_t> taps = load<int16_t>("taps.bin"), x = load<int16_t>("x.bin"), want = load<int16_t>("want.bin");
    const uint32_t channels = (uint32_t)(nco.size() / 2);
    if (!channels || nco.size() != 2 * (size_t)channels || taps.empty() || (taps.size() & 1) || x.empty() || x.size() % ((size_t)channels * B) ||
        want.size() != 2 * x.size()) { printf("FAILED: inputs\n"); return 2; }
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
    std::vector<int16_t> pairs(2 * per_block, 0), abi(2 * per_block, 0);
    uint32_t n_out = 0;
    CHECK(demod.readIq(pairs.data(), &n_out) == MSDR_STATUS_ARGUMENT_ERROR, "readIq before setIqOut(true) must be refused");
    CHECK(demod.setIqOut(true) == MSDR_STATUS_ARGUMENT_ERROR, "setIqOut before setNco must be refused (no phase-accumulator oscillator yet)");
    CHECK(demod.setNco(nco.data(), nco.data() + channels) == 0, "setNco: %s", msdr_last_error());
    CHECK(demod.setIqOut(true) == 0 && demod.setIqOut(true) == 0, "setIqOut: %s", msdr_last_error());
    CHECK(demod.readIq(nullptr, &n_out) == MSDR_STATUS_ARGUMENT_ERROR, "a null array must be refused");

    capture.begin();
    for (size_t k = 0; k < blocks; k++) {
        int16_t *p = queue_adc.getBuffer();
        CHECK(p != nullptr, "block %zu: no buffer", k);
        if (!p) break;
        msdr_memcpy_h2d(AudioGPU.context(), p, &x[k * per_block], AudioGPU.block_bytes());
        CHECK(queue_adc.playBuffer(), "block %zu: playBuffer", k);
        AudioStream::update_all();
        CHECK(capture.readBuffer() != nullptr, "block %zu: nothing captured", k);
        capture.freeBuffer();
        n_out = 0;
        CHECK(demod.readIq(pairs.data(), &n_out) == 0 && n_out == (uint32_t)B, "readIq: %s (n_out %u)", msdr_last_error(), n_out);
        CHECK(!memcmp(pairs.data(), &want[k * 2 * per_block], 2 * per_block * sizeof(int16_t)), "block %zu: the pairs are not the oracle's", k);
        // ... and they are the C ABI's buffer: the pointer the chain reports, read back with the library's own copy
        void *d_iq = nullptr;
        uint64_t pitch = 0;
        CHECK(demod.iqOut(&d_iq, &pitch) == 0 && d_iq != nullptr && pitch == (uint64_t)B, "get_iq_out: pitch %llu", (unsigned long long)pitch);
        if (d_iq) {
            CHECK(msdr_memcpy_d2h(AudioGPU.context(), abi.data(), d_iq, abi.size() * sizeof(int16_t)) == 0, "d2h: %s", msdr_last_error());
            CHECK(abi == pairs, "block %zu: readIq and the C ABI's buffer differ", k);
        }
    }
    msdr_chain_info info;
    CHECK(demod.info(&info) == 0 && !strncmp(info.kernel, "chain_q15pcn_kernel", 19), "kernel: %s", info.kernel);
    CHECK(demod.setIqOut(false) == 0, "setIqOut(false): %s", msdr_last_error());
    {
        void *d_iq = &info;
        uint64_t pitch = 1;
        CHECK(demod.iqOut(&d_iq, &pitch) == 0 && d_iq == nullptr && pitch == 0, "setIqOut(false) must clear the chain's buffer");
    }
    CHECK(demod.readIq(pairs.data(), &n_out) == MSDR_STATUS_ARGUMENT_ERROR, "readIq after setIqOut(false) must be refused");
    capture.end();
    capture.clear();
    CHECK(AudioMemoryUsage() == 0, "blocks leaked: %d", (int)AudioMemoryUsage());
    printf("%s queue_adc -> demodulator -> capture, %u receivers x %zu blocks, readIq after every tick\n", fails ? "FAILED" : "OK", channels, blocks);
    return fails ? 1 : 0;
}
