// tests/cpp/test_spectrum_channels.cpp -- the sketch's receive path  queue_adc -> demodulation() -> queue_dac  (Minimal-SDR.ino:518-775) for a bank
// of receivers over the AudioStream runtime with the second display item of its to-do list ("Spectrum display optional", Minimal-SDR.ino:48-51),
// once per receiver:
//     demod.setNco(...); demod.setDecimation(8); demod.setSpectrum(true, 1);  ... AudioStream::update_all() ...  demod.readSpectrum(power, &drawn);
//
// usage: test_spectrum_channels DATADIR   raw little-endian files written by tests/test_gpu_spectrum_channels_nodes.py:
//            nco.bin                uint32 [2][channels]    steps, start phases
//            taps.bin               int16 [102]             the AM tap set the chain is created with
//            x.bin                  int16 [blocks][channels][128]   IF blocks
//            want.bin               uint32 [blocks][channels][64]   the golden power rows, per tick and receiver (oracle pairs, model tail, oracle transform)
//        test_spectrum_channels --no-gpu  (argument errors on a machine without a device)
// Exit code 0 = every check passed.
#include <cmath>
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
        uint32_t row[MSDR_SPECTRUM_BINS];
        uint64_t drawn = 7;
        CHECK(demod.setSpectrum(true, 1) == MSDR_STATUS_ARGUMENT_ERROR && demod.setSpectrum(false) == MSDR_STATUS_ARGUMENT_ERROR, "a demodulator without a chain must refuse");
        CHECK(demod.readSpectrum(row, &drawn) == MSDR_STATUS_ARGUMENT_ERROR && drawn == 7, "a demodulator without a chain must refuse");
        CHECK(msdr_chain_set_spectrum(nullptr, nullptr, nullptr, 0) == MSDR_STATUS_ARGUMENT_ERROR, "null chain");
        CHECK(msdr_chain_get_spectrum(nullptr, nullptr, nullptr, nullptr, &drawn) == MSDR_STATUS_ARGUMENT_ERROR, "null chain");
        CHECK((unsigned)MSDR_FLAVOUR_SPECTRUM == 0x4000000u && MSDR_SPECTRUM_BINS == 64, "the flavour bit and the row length");
        CHECK(msdr_spectrum_dbfs(268435456.0, 32768.0) == 0.0 && msdr_spectrum_dbfs(0.0, 32768.0) == -HUGE_VAL, "the dBFS convention");
        if (msdr_device_count() == 0) {
            const int rc = AudioGPU.begin(0, 8);
            CHECK(rc == MSDR_STATUS_NO_DEVICE, "begin() without a GPU returned %d", rc);
        }
        printf("no-gpu path: %s\n", fails ? "FAILED" : "OK");
        return fails ? 1 : 0;
    }
    g_dir = argv[1];
    const std::vector<uint32_t> nco = load<uint32_t>("nco.bin"), want = load<uint32_t>("want.bin");
    const std::vector<int16_t> taps = load<int16_t>("taps.bin"), x = load<int16_t>("x.bin");
    const uint32_t channels = (uint32_t)(nco.size() / 2);
    if (!channels || nco.size() != 2 * (size_t)channels || taps.empty() || (taps.size() & 1) || x.empty() || x.size() % ((size_t)channels * B)) { printf("FAILED: inputs\n"); return 2; }
    const size_t per_block = (size_t)channels * B, blocks = x.size() / per_block, per_row = (size_t)channels * MSDR_SPECTRUM_BINS;
    if (want.size() != blocks * per_row) { printf("FAILED: inputs\n"); return 2; }

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
    std::vector<uint32_t> power(per_row, 0);
    uint64_t drawn = 0;
    CHECK(demod.readSpectrum(power.data(), &drawn) == MSDR_STATUS_ARGUMENT_ERROR, "readSpectrum before setSpectrum(true) must be refused");
    CHECK(demod.setSpectrum(true, 1) == MSDR_STATUS_ARGUMENT_ERROR, "setSpectrum before setNco must be refused (no phase-accumulator oscillator yet)");
    CHECK(demod.setNco(nco.data(), nco.data() + channels) == 0, "setNco: %s", msdr_last_error());
    CHECK(demod.setDecimation(8) == 0, "setDecimation: %s", msdr_last_error());
    CHECK(demod.setSpectrum(true, 1) == 0 && demod.setSpectrum(true, 1) == 0, "setSpectrum: %s", msdr_last_error());
    CHECK(demod.readSpectrum(nullptr, &drawn) == MSDR_STATUS_ARGUMENT_ERROR, "a null array must be refused");

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
        drawn = 0;
        CHECK(demod.readSpectrum(power.data(), &drawn) == 0 && drawn == k + 1, "readSpectrum: %s (drawn %llu)", msdr_last_error(), (unsigned long long)drawn);
        CHECK(!memcmp(power.data(), &want[k * per_row], per_row * sizeof(uint32_t)), "block %zu: the spectrum is not the golden row", k);
    }
    // the peak of the last spectrum of receiver 0 -- tuned to the carrier -- is column 32, in dBFS what a carrier of that amplitude reads
    {
        size_t peak = 0;
        for (size_t c = 1; c < MSDR_SPECTRUM_BINS; c++) if (power[c] > power[peak]) peak = c;
        const double db = msdr_spectrum_dbfs((double)power[peak], 32768.0);
        CHECK(peak == 32 && db > -6.0 && db < 0.0, "receiver 0: peak in column %zu at %.2f dBFS", peak, db);
    }
    msdr_chain_info info;
    CHECK(demod.info(&info) == 0 && !strncmp(info.kernel, "chain_q15pcnd_kernel", 20), "kernel: %s", info.kernel);
    CHECK(demod.setSpectrum(false) == 0, "setSpectrum(false): %s", msdr_last_error());
    CHECK(demod.readSpectrum(power.data(), &drawn) == MSDR_STATUS_ARGUMENT_ERROR, "readSpectrum after setSpectrum(false) must be refused");
    capture.end();
    capture.clear();
    CHECK(AudioMemoryUsage() == 0, "blocks leaked: %d", (int)AudioMemoryUsage());
    printf("%s queue_adc -> demodulator -> capture, %u receivers x %zu blocks at D = 8, readSpectrum after every tick\n", fails ? "FAILED" : "OK", channels, blocks);
    return fails ? 1 : 0;
}
