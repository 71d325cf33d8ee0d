// tests/cpp/test_graph_q15_block.cpp -- the sketch's receive path  queue_adc -> demodulation() -> biquad2_dac -> queue_dac  over the AudioStream
// runtime with a bank of individually tuned Q15 receivers: every receiver its own bandwidth (demod.setBandwidthChannel) and its own oscillator
// tables (demod.setOscChannel), the chain's two AudioFilterBiquad nodes behind the demodulator, and a biquad2_dac node of the graph behind the
// chain.  Half way through, tune() of ONE receiver: a new bandwidth, new tables, a new notch in the chain's second node
// (demod.setNodeNotchChannel) and in biquad2_dac (biquad2_dac.channel(rx).setNotch).  With demod.setBlockKernelQ15(true) a tick of the chain is
// one launch (chain_q15pcb_kernel), without it three; the audio must not know the difference.
//
// usage: test_graph_q15_block DATADIR on|off   raw little-endian files written by tests/test_host_graph_q15_block.py:
//            taps.bin               int16 [102]             the AM tap set the chain is created with
//            osc_i.bin, osc_q.bin   int16 [channels + 1][128]   the tables of every receiver; the last row pair: the retuned receiver's new tables
//            x.bin                  int16 [blocks][channels][128]   IF blocks
//        writes DATADIR/got_on.bin or got_off.bin, int16 [blocks][channels][128]: the captured audio (the Python test holds both against the
//        oracle and against each other) and checks which kernel every tick ran.
//        test_graph_q15_block --no-gpu  (argument errors on a machine without a device)
// The constants below are restated in the Python test.  Exit code 0 = every check passed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../minimal-sdr_amd/host/msdr_nodes.h"

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static const int B = AUDIO_BLOCK_SAMPLES;
static const float CORR = (float)(AUDIO_SAMPLE_RATE_EXACT / 24000.0);
static const uint32_t kRetuneRx = 1;
static const size_t kRetuneBlock = 4;
static float bandwidth_of(uint32_t rx) { return 2000.0f + 400.0f * (float)rx; }
static const float kNewBandwidth = 1500.0f, kLowpass = 5400.0f, kNotch = 3000.0f, kNewChainNotch = 2900.0f, kDacNotch = 3300.0f, kNewDacNotch = 3100.0f;
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
AudioFilterBiquad biquad2_dac;
AudioRecordQueue capture;
AudioConnection patchCord1(queue_adc, 0, demod, 0);
AudioConnection patchCord2(demod, 0, biquad2_dac, 0);
AudioConnection patchCord3(biquad2_dac, 0, capture, 0);

int main(int argc, char **argv)
{
    if (argc < 2) { printf("usage: %s DATADIR on|off | --no-gpu\n", argv[0]); return 2; }
    if (!strcmp(argv[1], "--no-gpu")) {
        msdr_chain_info info;
        CHECK(demod.setBlockKernelQ15(true) == MSDR_STATUS_ARGUMENT_ERROR, "a demodulator without a chain must refuse");
        CHECK(demod.setBlockKernelQ15(false) == MSDR_STATUS_ARGUMENT_ERROR, "a demodulator without a chain must refuse");
        CHECK(demod.setBandwidthChannel(0, 2400.0f) == MSDR_STATUS_ARGUMENT_ERROR, "a demodulator without a chain must refuse");
        CHECK(demod.info(&info) == MSDR_STATUS_ARGUMENT_ERROR, "a demodulator without a chain must refuse");
        CHECK(msdr_chain_set_block_kernel_q15(nullptr, 1) == MSDR_STATUS_ARGUMENT_ERROR, "null chain");
        CHECK(msdr_chain_set_block_kernel_q15(nullptr, 0) == MSDR_STATUS_ARGUMENT_ERROR, "null chain");
        if (msdr_device_count() == 0) {
            const int rc = AudioGPU.begin(0, 3);
            CHECK(rc == MSDR_STATUS_NO_DEVICE, "begin() without a GPU returned %d", rc);
        }
        printf("no-gpu path: %s\n", fails ? "FAILED" : "OK");
        return fails ? 1 : 0;
    }
    if (argc < 3 || (strcmp(argv[2], "on") && strcmp(argv[2], "off"))) { printf("usage: %s DATADIR on|off | --no-gpu\n", argv[0]); return 2; }
    const bool on = !strcmp(argv[2], "on");
    g_dir = argv[1];
    const std::vector<int16_t> osc_i = load<int16_t>("osc_i.bin"), osc_q = load<int16_t>("osc_q.bin");
    const std::vector<int16_t> taps = load<int16_t>("taps.bin"), x = load<int16_t>("x.bin");
    if (osc_i.size() < 2 * (size_t)B || osc_i.size() % B || osc_q.size() != osc_i.size() || taps.empty()) { printf("FAILED: inputs\n"); return 2; }
    const uint32_t channels = (uint32_t)(osc_i.size() / B) - 1;
    const size_t per_block = (size_t)channels * B;
    if (channels <= kRetuneRx || x.empty() || x.size() % per_block || x.size() / per_block <= kRetuneBlock + 2) { printf("FAILED: inputs\n"); return 2; }
    const size_t blocks = x.size() / per_block;

    if (AudioGPU.begin(0, channels) != 0) { printf("AudioGPU.begin failed: %s\n", msdr_last_error()); return 2; }
    if (AudioMemory(16) != 0) { printf("AudioMemory failed: %s\n", msdr_last_error()); return 2; }
    int32_t lp[5], nt[5];
    if (msdr_biquad_design(MSDR_BQ_LOWPASS, kLowpass * CORR, 0.54f, 1.0f, AUDIO_SAMPLE_RATE_EXACT, lp) != 0 ||
        msdr_biquad_design(MSDR_BQ_NOTCH, kNotch * CORR, 15.0f, 1.0f, AUDIO_SAMPLE_RATE_EXACT, nt) != 0) { printf("FAILED: biquad design\n"); return 2; }
    msdr_chain_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg; cfg.arith = MSDR_ARITH_Q15; cfg.channels = channels; cfg.mixer = MSDR_MIXER_NCO;
    cfg.num_taps = (uint32_t)taps.size(); cfg.num_tapsets = 1; cfg.coeffs_i[0] = taps.data(); cfg.coeffs_q[0] = taps.data();
    cfg.osc_len = B; cfg.osc_i = osc_i.data(); cfg.osc_q = osc_q.data();          // receiver 0's tables for everybody, until each gets its own
    cfg.default_mode = MSDR_MODE_AM;
    cfg.num_biquad_nodes = 2; cfg.node_stages[0] = 1; cfg.node_coefs[0] = lp; cfg.node_stages[1] = 1; cfg.node_coefs[1] = nt;          // biquad1_dac, biquad2_dac of the chain
    if (demod.begin(cfg) != 0) { printf("demod.begin failed: %s\n", msdr_last_error()); return 2; }
    if (on) CHECK(demod.setBlockKernelQ15(true) == 0, "setBlockKernelQ15: %s", msdr_last_error());          // (before the chain enters per-channel mode: it waits for it)
    CHECK(demod.setBlockKernel(true) == MSDR_STATUS_ARGUMENT_ERROR, "the fp32 switch must keep refusing a Q15 chain");
    for (uint32_t rx = 0; rx < channels; rx++) {
        CHECK(demod.setBandwidthChannel(rx, bandwidth_of(rx)) == 0, "setBandwidthChannel(%u): %s", rx, msdr_last_error());
        CHECK(demod.setOscChannel(rx, &osc_i[(size_t)rx * B], &osc_q[(size_t)rx * B]) == 0, "setOscChannel(%u): %s", rx, msdr_last_error());
    }
    biquad2_dac.setNotch(0, kDacNotch * CORR, 15.0f);

    capture.begin();
    std::vector<int16_t> got(blocks * per_block);
    size_t fused_ticks = 0;
    for (size_t k = 0; k < blocks; k++) {
        if (k == kRetuneBlock) {          // tune() of one receiver
            CHECK(demod.setBandwidthChannel(kRetuneRx, kNewBandwidth) == 0, "setBandwidthChannel: %s", msdr_last_error());
            CHECK(demod.setOscChannel(kRetuneRx, &osc_i[(size_t)channels * B], &osc_q[(size_t)channels * B]) == 0, "setOscChannel: %s", msdr_last_error());
            CHECK(demod.setNodeNotchChannel(1, kRetuneRx, 0, kNewChainNotch * CORR, 15.0f) == 0, "setNodeNotchChannel: %s", msdr_last_error());
            biquad2_dac.channel(kRetuneRx).setNotch(0, kNewDacNotch * CORR, 15.0f);
        }
        int16_t *p = queue_adc.getBuffer();
        CHECK(p != nullptr, "block %zu: no buffer", k);
        if (!p) break;
        msdr_memcpy_h2d(AudioGPU.context(), p, &x[k * per_block], AudioGPU.block_bytes());
        CHECK(queue_adc.playBuffer(), "block %zu: playBuffer", k);
        AudioStream::update_all();
        int16_t *d = capture.readBuffer();
        const bool ok = d && msdr_memcpy_d2h(AudioGPU.context(), &got[k * per_block], d, AudioGPU.block_bytes()) == 0;
        capture.freeBuffer();
        CHECK(ok, "block %zu: nothing captured (%s)", k, msdr_last_error());
        if (!ok) break;
        msdr_chain_info info;
        CHECK(demod.info(&info) == 0, "info: %s", msdr_last_error());
        const bool fused = !strncmp(info.kernel, "chain_q15pcb_kernel", 19);
        fused_ticks += fused ? 1 : 0;
        // a tick behind setOscChannel still holds samples of the earlier tables in its history (102 taps: one tick): unfused either way
        const bool pending = k == 0 || k == kRetuneBlock;
        CHECK(fused == (on && !pending), "block %zu ran %s", k, info.kernel);
        if (!fused) CHECK(!strncmp(info.kernel, "chain_q15pco_kernel", 19), "block %zu ran %s", k, info.kernel);
    }
    CHECK(fused_ticks == (on ? blocks - 2 : 0), "%zu fused ticks of %zu", fused_ticks, blocks);
    capture.end();
    capture.clear();
    CHECK(AudioMemoryUsage() == 0, "blocks leaked: %d", (int)AudioMemoryUsage());
    FILE *f = fopen((g_dir + (on ? "/got_on.bin" : "/got_off.bin")).c_str(), "wb");
    CHECK(f && fwrite(got.data(), sizeof(int16_t), got.size(), f) == got.size(), "cannot write the captured audio");
    if (f) fclose(f);
    printf("%s queue_adc -> Q15 demodulator (%s) -> biquad2_dac -> capture, %u receivers x %zu blocks, %zu fused ticks\n", fails ? "FAILED" : "OK",
           on ? "one launch per tick" : "three launches per tick", channels, blocks, fused_ticks);
    return fails ? 1 : 0;
}
