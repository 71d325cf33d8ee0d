// tests/cpp/test_input_rows.cpp -- one queue_adc feeds a bank of receivers: the sketch's receive path  queue_adc -> demodulation() -> queue_dac
// (Minimal-SDR.ino:518-775) over the AudioStream runtime with
//     demod.setInputRows(n_inputs, rows);     receiver rx hears row rows[rx] of the incoming block (msdr_chain_set_input_rows)
// and every receiver mixing with the oscillator tables of its own tuning (demod.setOscChannel).  The incoming block stays
// [channels][128]; only its first n_inputs rows are filled with samples, the rest holds a sentinel.
//
// usage: test_input_rows DATADIR   raw little-endian files written by tests/test_gpu_input_rows_nodes.py:
//            osc_i.bin, osc_q.bin   int16 [channels][128]   the tables of every receiver
//            maps.bin               uint32 [2 + 2 * channels]   {n_inputs, block, the map from the start, the map from `block` on}
//            taps.bin               int16 [102]             the AM tap set the chain is created with
//            x.bin                  int16 [blocks][n_inputs][128]   IF blocks
//            want.bin               int16 [blocks][channels][128]   the oracle's audio blocks
//        test_input_rows --no-gpu  (argument errors on a machine without a device)
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
        const uint32_t rows[4] = {0, 1, 1, 0};
        CHECK(demod.setInputRows(2, rows) == MSDR_STATUS_ARGUMENT_ERROR, "a demodulator without a chain must refuse");
        CHECK(demod.setInputRows(0, nullptr) == MSDR_STATUS_ARGUMENT_ERROR, "a demodulator without a chain must refuse the identity too");
        CHECK(msdr_chain_set_input_rows(nullptr, 2, rows) == MSDR_STATUS_ARGUMENT_ERROR, "null chain");
        CHECK(msdr_chain_set_input_rows(nullptr, 2, nullptr) == MSDR_STATUS_ARGUMENT_ERROR, "null chain, null array");
        CHECK(msdr_chain_set_input_rows(nullptr, 0, nullptr) == MSDR_STATUS_ARGUMENT_ERROR, "null chain, n_inputs 0");
        CHECK(MSDR_FLAVOUR_SHARED_IF == 0x40000u, "MSDR_FLAVOUR_SHARED_IF");
        if (msdr_device_count() == 0) {
            const int rc = AudioGPU.begin(0, 8);
            CHECK(rc == MSDR_STATUS_NO_DEVICE, "begin() without a GPU returned %d", rc);
        }
        printf("no-gpu path: %s\n", fails ? "FAILED" : "OK");
        return fails ? 1 : 0;
    }
    g_dir = argv[1];
    const std::vector<int16_t> osc_i = load<int16_t>("osc_i.bin"), osc_q = load<int16_t>("osc_q.bin");
    const std::vector<uint32_t> maps = load<uint32_t>("maps.bin");
    const std::vector<int16_t> taps = load<int16_t>("taps.bin"), x = load<int16_t>("x.bin"), want = load<int16_t>("want.bin");
    const uint32_t channels = (uint32_t)(osc_i.size() / B);
    if (!channels || osc_i.size() != (size_t)channels * B || osc_q.size() != osc_i.size() || taps.empty() || maps.size() != 2 + 2 * (size_t)channels ||
        maps[0] == 0 || maps[0] > channels || x.empty() || x.size() % ((size_t)maps[0] * B) || want.size() != x.size() / maps[0] * channels) { printf("FAILED: inputs\n"); return 2; }
    const uint32_t n_inputs = maps[0];
    const size_t in_block = (size_t)n_inputs * B, per_block = (size_t)channels * B, blocks = x.size() / in_block, change_block = maps[1];
    const uint32_t *map0 = maps.data() + 2, *map1 = map0 + channels;

    if (AudioGPU.begin(0, channels) != 0) { printf("AudioGPU.begin failed: %s\n", msdr_last_error()); return 2; }
    if (AudioMemory(16) != 0) { printf("AudioMemory failed: %s\n", msdr_last_error()); return 2; }
    msdr_chain_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg; cfg.arith = MSDR_ARITH_Q15; cfg.channels = channels; cfg.mixer = MSDR_MIXER_NCO;
    cfg.num_taps = (uint32_t)taps.size(); cfg.num_tapsets = 1; cfg.coeffs_i[0] = taps.data(); cfg.coeffs_q[0] = taps.data();
    cfg.osc_len = B; cfg.osc_i = osc_i.data(); cfg.osc_q = osc_q.data();          // receiver 0's tables for everybody, until each gets its own
    cfg.default_mode = MSDR_MODE_AM;
    if (demod.begin(cfg) != 0) { printf("demod.begin failed: %s\n", msdr_last_error()); return 2; }
    // the refusals change nothing: an entry past the rows, a null array, more rows than the block has
    std::vector<uint32_t> bad(map0, map0 + channels);
    bad[channels - 1] = n_inputs;
    CHECK(demod.setInputRows(n_inputs, bad.data()) == MSDR_STATUS_ARGUMENT_ERROR, "an entry >= n_inputs must be refused");
    CHECK(demod.setInputRows(n_inputs, nullptr) == MSDR_STATUS_ARGUMENT_ERROR, "a null array must be refused");
    CHECK(demod.setInputRows(channels + 1, map0) == MSDR_STATUS_ARGUMENT_ERROR, "more rows than the block holds must be refused");
    CHECK(demod.setInputRows(n_inputs, map0) == 0, "setInputRows: %s", msdr_last_error());
    for (uint32_t rx = 0; rx < channels; rx++)
        CHECK(demod.setOscChannel(rx, &osc_i[(size_t)rx * B], &osc_q[(size_t)rx * B]) == 0, "setOscChannel(%u): %s", rx, msdr_last_error());

    capture.begin();
    std::vector<int16_t> got(per_block);
    for (size_t k = 0; k < blocks; k++) {
        if (k == change_block) CHECK(demod.setInputRows(n_inputs, map1) == 0, "setInputRows at block %zu: %s", k, msdr_last_error());
        int16_t *p = queue_adc.getBuffer();
        CHECK(p != nullptr, "block %zu: no buffer", k);
        if (!p) break;
        msdr_memset(AudioGPU.context(), p, 0x5A, AudioGPU.block_bytes());          // the rows nobody hears
        msdr_memcpy_h2d(AudioGPU.context(), p, &x[k * in_block], in_block * sizeof(int16_t));
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
    printf("%s queue_adc -> demodulator -> capture, %u receivers on %u rows x %zu blocks\n", fails ? "FAILED" : "OK", channels, n_inputs, blocks);
    return fails ? 1 : 0;
}
