// msdr_nodes.h -- the graph nodes on the demodulation path, as AudioStream subclasses over the C ABI.
// Class and method names follow the reference so a sketch's wiring reads the same:
//   AudioFilterBiquad    src/Audio/filter_biquad.{h,cpp}
//   AudioEffectFreqConv  freq_conv.{h,cpp}
//   AudioRecordQueue     src/Audio/record_queue.{h,cpp}     (graph -> main loop)
//   AudioPlayQueue       src/Audio/play_queue.{h,cpp}       (main loop -> graph)
// plus AudioSDRDemodulator, the fused node (one kernel for demodulation() + the biquad nodes behind it).
// Every block is a block batch in HBM (AudioStream.h); update() enqueues kernels, never touches samples.
#pragma once
#include <atomic>
#include <cstring>
#include <vector>

#include "AudioStream.h"

// ------------------------------------------------------------------------------------------------
// AudioFilterBiquad -- up to 4 cascaded biquads, Q2.30 coefficients, int16 data (filter_biquad.h:33-155)
// ------------------------------------------------------------------------------------------------
class AudioFilterBiquad : public AudioStream {
public:
    AudioFilterBiquad(void) : AudioStream(1, inputQueueArray), node(nullptr) {}
    ~AudioFilterBiquad() { if (node) msdr_biquad_q15_destroy(node); }
    virtual void update(void)
    {
        audio_block_t *block = receiveWritable();
        if (!block) return;                                    // filter_biquad.cpp:41
        if (ensure()) msdr_biquad_q15_update(node, block->data, AUDIO_BLOCK_SAMPLES);
        transmit(block);
        release(block);
    }
    void setCoefficients(uint32_t stage, const int *coefficients) { set(kAll, stage, coefficients); }
    void setCoefficients(uint32_t stage, const double *coefficients) { set(kAll, stage, coefficients); }      // filter_biquad.h:43-51
    void setLowpass(uint32_t stage, float frequency, float q = 0.7071f) { design(kAll, stage, MSDR_BQ_LOWPASS, frequency, q, 1.0f); }
    void setHighpass(uint32_t stage, float frequency, float q = 0.7071f) { design(kAll, stage, MSDR_BQ_HIGHPASS, frequency, q, 1.0f); }
    void setBandpass(uint32_t stage, float frequency, float q = 1.0f) { design(kAll, stage, MSDR_BQ_BANDPASS, frequency, q, 1.0f); }
    void setNotch(uint32_t stage, float frequency, float q = 1.0f) { design(kAll, stage, MSDR_BQ_NOTCH, frequency, q, 1.0f); }
    void setLowShelf(uint32_t stage, float frequency, float gain, float slope = 1.0f) { design(kAll, stage, MSDR_BQ_LOWSHELF, frequency, gain, slope); }
    void setHighShelf(uint32_t stage, float frequency, float gain, float slope = 1.0f) { design(kAll, stage, MSDR_BQ_HIGHSHELF, frequency, gain, slope); }
    // One receiver of the bank: the node's own setters on channel ch only, so a per-receiver tune() reads
    //     biquad2_dac.channel(rx).setNotch(0, pdb_freq_actual / 8.0 * CORR_FACT, 15.0);          (Minimal-SDR.ino:356)
    // (A proxy, not overloads with a leading channel argument: setNotch(0, 3000, 15) would be ambiguous.)  Calls made before
    // AudioGPU.begin queue with their channel, in order with the all-channel calls.
    class Channel {
    public:
        void setCoefficients(uint32_t stage, const int *coefficients) { node.set(ch, stage, coefficients); }
        void setCoefficients(uint32_t stage, const double *coefficients) { node.set(ch, stage, coefficients); }
        void setLowpass(uint32_t stage, float frequency, float q = 0.7071f) { node.design(ch, stage, MSDR_BQ_LOWPASS, frequency, q, 1.0f); }
        void setHighpass(uint32_t stage, float frequency, float q = 0.7071f) { node.design(ch, stage, MSDR_BQ_HIGHPASS, frequency, q, 1.0f); }
        void setBandpass(uint32_t stage, float frequency, float q = 1.0f) { node.design(ch, stage, MSDR_BQ_BANDPASS, frequency, q, 1.0f); }
        void setNotch(uint32_t stage, float frequency, float q = 1.0f) { node.design(ch, stage, MSDR_BQ_NOTCH, frequency, q, 1.0f); }
        void setLowShelf(uint32_t stage, float frequency, float gain, float slope = 1.0f) { node.design(ch, stage, MSDR_BQ_LOWSHELF, frequency, gain, slope); }
        void setHighShelf(uint32_t stage, float frequency, float gain, float slope = 1.0f) { node.design(ch, stage, MSDR_BQ_HIGHSHELF, frequency, gain, slope); }
    private:
        friend class AudioFilterBiquad;
        Channel(AudioFilterBiquad &n, uint32_t c) : node(n), ch(c) {}
        AudioFilterBiquad &node;
        uint32_t ch;
    };
    Channel channel(uint32_t ch) { return Channel(*this, ch); }
    // definition[32] of one channel, as filter_biquad.h:152 lays it out (test/debug aid)
    int getDefinition(uint32_t channel, int32_t definition[32]) { return ensure() ? msdr_biquad_q15_get_definition(node, channel, definition) : MSDR_STATUS_NO_DEVICE; }

private:
    static const uint32_t kAll = 0xFFFFFFFFu;                  // Pending::channel of a call on the node itself
    struct Pending { uint32_t channel, stage; int32_t coef[5]; };
    void set(uint32_t ch, uint32_t stage, const int *coefficients)
    {
        if (stage >= 4) return;                                // filter_biquad.cpp:86
        pending.push_back({ch, stage, {coefficients[0], coefficients[1], coefficients[2], coefficients[3], coefficients[4]}});
        if (AudioGPU.context()) ensure();
    }
    void set(uint32_t ch, uint32_t stage, const double *coefficients)
    {
        int coef[5];
        for (int i = 0; i < 5; i++) coef[i] = (int)(coefficients[i] * 1073741824.0);
        set(ch, stage, coef);
    }
    void design(uint32_t ch, uint32_t stage, int kind, float f, float q, float slope)
    {
        int32_t coef[5];
        if (msdr_biquad_design(kind, f, q, slope, AUDIO_SAMPLE_RATE_EXACT, coef) == 0) set(ch, stage, (const int *)coef);
    }
    bool ensure(void)
    {
        if (!node) {
            if (!AudioGPU.context() || msdr_biquad_q15_create(AudioGPU.context(), AudioGPU.channels(), &node) != 0) { node = nullptr; return false; }
        }
        for (const Pending &p : pending) {
            if (p.channel == kAll) msdr_biquad_q15_set_coefficients(node, p.stage, p.coef);
            else msdr_biquad_q15_set_coefficients_channels(node, p.channel, 1, p.stage, p.coef);      // (a channel past the bank: refused there)
        }
        pending.clear();
        return true;
    }
    msdr_biquad_q15 *node;
    std::vector<Pending> pending;
    audio_block_t *inputQueueArray[1];
};

// ------------------------------------------------------------------------------------------------
// AudioAmplifier -- gain stage, Q16.16 multiplier, saturating (mixer.h:67-82, mixer.cpp:34-47, :134-159).
// amp_adc / amp_dac of the sketch (Minimal-SDR.ino:67, :73); AGC() drives amp_adc.gain() (:446-515).
// ------------------------------------------------------------------------------------------------
class AudioAmplifier : public AudioStream {
public:
    AudioAmplifier(void) : AudioStream(1, inputQueueArray), multiplier(65536) {}
    virtual void update(void)
    {
        const int32_t mult = multiplier;
        if (mult == 0) {                                       // mixer.cpp:139-142: discard, transmit nothing
            audio_block_t *block = receiveReadOnly(0);
            if (block) release(block);
        } else if (mult == 65536) {                            // :143-149: unity, pass the block on untouched
            audio_block_t *block = receiveReadOnly(0);
            if (block) { transmit(block); release(block); }
        } else {                                               // :150-157
            audio_block_t *block = receiveWritable(0);
            if (block) {
                if (AudioGPU.context()) msdr_amp_q15(AudioGPU.context(), mult, block->data, AudioGPU.channels(), AUDIO_BLOCK_SAMPLES, nullptr);
                transmit(block);
                release(block);
            }
        }
    }
    void gain(float n) { multiplier = msdr_amp_multiplier(n); } // mixer.h:75-79

private:
    int32_t multiplier;
    audio_block_t *inputQueueArray[1];
};

// ------------------------------------------------------------------------------------------------
// AudioEffectFreqConv -- complex (I,Q) x oscillator mix in q15 (freq_conv.h:36-56, freq_conv.cpp:30-116).
// The oscillator tables are globals of the application, exactly as in the reference (freq_conv.h:33-34).
// Unlike the reference the kernel needs no temporary blocks, so the node cannot run out of pool memory.
// ------------------------------------------------------------------------------------------------
extern q15_t Osc_Q_buffer_i[AUDIO_BLOCK_SAMPLES];
extern q15_t Osc_I_buffer_i[AUDIO_BLOCK_SAMPLES];

class AudioEffectFreqConv : public AudioStream {
public:
    AudioEffectFreqConv() : AudioStream(2, inputQueueArray), dir(0), pass(1) {}
    void direction(bool d) { dir = d; }
    void passthrough(bool p) { pass = p; }
    virtual void update(void)
    {
        audio_block_t *blockI = receiveWritable(0);
        audio_block_t *blockQ = receiveWritable(1);
        if (!blockI) { if (blockQ) release(blockQ); return; }                 // freq_conv.cpp:40-47
        if (!blockQ) { release(blockI); return; }
        // `pass` keeps the reference's inverted meaning: pass == false forwards untouched (:49-56)
        msdr_freqconv_q15(AudioGPU.context(), blockI->data, blockQ->data, Osc_I_buffer_i, Osc_Q_buffer_i, AUDIO_BLOCK_SAMPLES,
                          dir ? 1 : 0, pass ? 1 : 0, AudioGPU.channels(), AUDIO_BLOCK_SAMPLES);
        transmit(blockI, 0);
        transmit(blockQ, 1);
        release(blockI);
        release(blockQ);
    }

private:
    audio_block_t *inputQueueArray[2];
    bool dir, pass;
};

// ------------------------------------------------------------------------------------------------
// BlockRing -- a single-producer / single-consumer ring of block pointers.  One side is the graph tick (update(), the software
// interrupt of the reference), the other the main loop; each side owns one free-running counter, so neither ever writes what
// the other one writes and a full ring is told from an empty one without giving up a slot.
// ------------------------------------------------------------------------------------------------
template <unsigned CAPACITY>
class BlockRing {
public:
    unsigned size(void) const { return pushed.load(std::memory_order_acquire) - popped.load(std::memory_order_acquire); }
    bool push(audio_block_t *block)                   // producer side; false = full
    {
        const unsigned w = pushed.load(std::memory_order_relaxed);
        if (w - popped.load(std::memory_order_acquire) >= CAPACITY) return false;
        slot[w % CAPACITY] = block;
        pushed.store(w + 1, std::memory_order_release);
        return true;
    }
    audio_block_t *pop(void)                          // consumer side; NULL = empty
    {
        const unsigned r = popped.load(std::memory_order_relaxed);
        if (r == pushed.load(std::memory_order_acquire)) return nullptr;
        audio_block_t *block = slot[r % CAPACITY];
        popped.store(r + 1, std::memory_order_release);
        return block;
    }

private:
    audio_block_t *slot[CAPACITY];
    std::atomic<unsigned> pushed{0}, popped{0};
};

// ------------------------------------------------------------------------------------------------
// AudioRecordQueue -- hands graph blocks to the main loop (interface of record_queue.h:34-58; the reference keeps 53 slots of which
// 52 can be occupied, and drops the incoming block when they are: record_queue.cpp:91-92).
// readBuffer() returns a DEVICE pointer to [channels][128] int16.
// ------------------------------------------------------------------------------------------------
class AudioRecordQueue : public AudioStream {
public:
    AudioRecordQueue(void) : AudioStream(1, inputQueueArray), lent(nullptr), recording(false) {}
    void begin(void) { clear(); recording.store(true); }
    void end(void) { recording.store(false); }
    int available(void) { return (int)ring.size(); }
    void clear(void)
    {
        freeBuffer();
        while (audio_block_t *b = ring.pop()) release(b);
    }
    int16_t *readBuffer(void)                         // one block at a time is out with the main loop
    {
        if (lent) return nullptr;
        lent = ring.pop();
        return lent ? lent->data : nullptr;
    }
    void freeBuffer(void)
    {
        if (lent) release(lent);
        lent = nullptr;
    }
    virtual void update(void)
    {
        audio_block_t *block = receiveReadOnly();
        if (!block) return;
        if (!recording.load() || !ring.push(block)) release(block);
    }

private:
    audio_block_t *inputQueueArray[1];
    BlockRing<52> ring;
    audio_block_t *lent;
    std::atomic<bool> recording;
};

// ------------------------------------------------------------------------------------------------
// AudioPlayQueue -- main loop feeds blocks into the graph (interface of play_queue.h:34-52; 32 slots of which 31 can be occupied).
// Where the reference busy-waits (allocate() in getBuffer, a full ring in playBuffer: play_queue.cpp:42-46, :56) these return
// NULL / false: there is no interrupt here that could end the wait.
// ------------------------------------------------------------------------------------------------
class AudioPlayQueue : public AudioStream {
public:
    AudioPlayQueue(void) : AudioStream(0, nullptr), filling(nullptr) {}
    bool available(void) { return getBuffer() != nullptr; }
    int16_t *getBuffer(void)
    {
        if (!filling) filling = allocate();
        return filling ? filling->data : nullptr;
    }
    bool playBuffer(void)
    {
        if (!filling || !ring.push(filling)) return false;
        filling = nullptr;
        return true;
    }
    virtual void update(void)
    {
        if (audio_block_t *block = ring.pop()) {
            transmit(block);
            release(block);
        }
    }

private:
    BlockRing<31> ring;
    audio_block_t *filling;
};

// ------------------------------------------------------------------------------------------------
// AudioSDRDemodulator -- the whole demodulation() step (+ optional biquad nodes) as ONE graph node and ONE
// kernel per tick: IF block batch in, audio block batch out.  Configure with a msdr_chain_config whose
// `channels` equals AudioGPU.channels() and whose arith is MSDR_ARITH_Q15, or MSDR_ARITH_F32 with MSDR_CHAIN_OUT_I16 in `flags` (the
// audio blocks are int16 either way: an fp32 chain converts as arm_float_to_q15 does).
// ------------------------------------------------------------------------------------------------
class AudioSDRDemodulator : public AudioStream {
public:
    // (two input ports, as AudioEffectFreqConv has: port 1 is the Q block of a complex stream under setComplexInput, released unread otherwise)
    AudioSDRDemodulator(void) : AudioStream(2, inputQueueArray), chain(nullptr), num_taps(0), d_meter(nullptr), d_iq(nullptr), d_cx(nullptr), d_spec(nullptr), f32(false), in_scale(0.0f) {}
    ~AudioSDRDemodulator() { if (chain) msdr_chain_destroy(chain); freeMeter(); freeIq(); freeCx(); freeSpec(); }
    int begin(const msdr_chain_config &cfg)
    {
        if (chain) { msdr_chain_destroy(chain); chain = nullptr; }
        freeMeter();
        freeIq();
        freeCx();
        freeSpec();
        f32 = cfg.arith == MSDR_ARITH_F32; in_scale = cfg.in_scale != 0.0f ? cfg.in_scale : 1.0f / 32768.0f;
        const bool i16_audio = cfg.arith == MSDR_ARITH_Q15 || (cfg.arith == MSDR_ARITH_F32 && (cfg.flags & MSDR_CHAIN_OUT_I16));
        if (!i16_audio || cfg.channels != AudioGPU.channels()) return MSDR_STATUS_ARGUMENT_ERROR;
        num_taps = cfg.num_taps;
        return msdr_chain_create(AudioGPU.context(), &cfg, &chain);
    }
    int init_FIR(void) { return chain ? msdr_chain_init_fir(chain) : MSDR_STATUS_ARGUMENT_ERROR; }     // Minimal-SDR.ino:901-930
    int setMode(uint32_t channel, int mode, int tapset) { return chain ? msdr_chain_set_mode(chain, channel, mode, tapset) : MSDR_STATUS_ARGUMENT_ERROR; }
    // what the sketch changes while audio plays, filter state kept (include/msdr.h "live updates"):
    // calc_demod_filter() rewriting FIR_AM_coeffs (Minimal-SDR.ino:221-223), tune()'s biquad2_dac.setNotch (:356), new oscillator tables (freq_conv.h:33-34)
    int setTaps(uint32_t tapset, const void *coeffs_i, const void *coeffs_q) { return chain ? msdr_chain_set_taps(chain, tapset, coeffs_i, coeffs_q) : MSDR_STATUS_ARGUMENT_ERROR; }
    int setNodeCoefficients(uint32_t node, uint32_t stage, const int *coef) { return chain ? msdr_chain_set_node_coefficients(chain, node, stage, (const int32_t *)coef) : MSDR_STATUS_ARGUMENT_ERROR; }
    int setNodeNotch(uint32_t node, uint32_t stage, float frequency, float q = 1.0f)
    {
        int32_t coef[5];
        if (int rc = msdr_biquad_design(MSDR_BQ_NOTCH, frequency, q, 1.0f, AUDIO_SAMPLE_RATE_EXACT, coef)) return rc;
        return setNodeCoefficients(node, stage, (const int *)coef);
    }
    // one receiver's node: tune() of receiver `channel` (msdr_chain_set_node_coefficients_channels)
    int setNodeCoefficientsChannel(uint32_t node, uint32_t channel, uint32_t stage, const int *coef)
    {
        return chain ? msdr_chain_set_node_coefficients_channels(chain, node, channel, 1, stage, (const int32_t *)coef) : MSDR_STATUS_ARGUMENT_ERROR;
    }
    int setNodeNotchChannel(uint32_t node, uint32_t channel, uint32_t stage, float frequency, float q = 1.0f)
    {
        int32_t coef[5];
        if (int rc = msdr_biquad_design(MSDR_BQ_NOTCH, frequency, q, 1.0f, AUDIO_SAMPLE_RATE_EXACT, coef)) return rc;
        return setNodeCoefficientsChannel(node, channel, stage, (const int *)coef);
    }
    // one receiver's FIR pair: the station's own filterBandwidth (stations.h:10-16; msdr_chain_set_taps_channels).  coeffs_q == nullptr: the
    // same array behind both filters, as init_FIR() binds FIR_AM_coeffs for AM / SYNCAM (Minimal-SDR.ino:917-924)
    int setTapsChannel(uint32_t channel, const int16_t *coeffs_i, const int16_t *coeffs_q = nullptr)
    {
        return chain ? msdr_chain_set_taps_channels(chain, channel, 1, coeffs_i, coeffs_q) : MSDR_STATUS_ARGUMENT_ERROR;
    }
    // the same on an fp32 chain (msdr_chain_set_taps_channels_f32): float rows in CMSIS order
    int setTapsChannelF32(uint32_t channel, const float *coeffs_i, const float *coeffs_q = nullptr)
    {
        return chain ? msdr_chain_set_taps_channels_f32(chain, channel, 1, coeffs_i, coeffs_q) : MSDR_STATUS_ARGUMENT_ERROR;
    }
    // one receiver's cascade on an fp32 chain: 5 x num_biquad_stages coefficients, tune()'s notch (msdr_chain_set_biquad_coeffs_channels)
    int setBiquadCoeffsChannel(uint32_t channel, const float *coeffs)
    {
        return chain ? msdr_chain_set_biquad_coeffs_channels(chain, channel, 1, coeffs) : MSDR_STATUS_ARGUMENT_ERROR;
    }
    // fp32 chain in per-channel mode: the whole tick in one launch (msdr_chain_set_block_kernel: chain_f32pcb_kernel)
    int setBlockKernel(bool on) { return chain ? msdr_chain_set_block_kernel(chain, on ? 1 : 0) : MSDR_STATUS_ARGUMENT_ERROR; }
    // Q15 chain in per-channel mode: demodulator, both biquad nodes and the next history in one launch (msdr_chain_set_block_kernel_q15: chain_q15pcb_kernel)
    int setBlockKernelQ15(bool on) { return chain ? msdr_chain_set_block_kernel_q15(chain, on ? 1 : 0) : MSDR_STATUS_ARGUMENT_ERROR; }
    // which kernel the last tick ran (msdr_chain_get_info)
    int info(msdr_chain_info *out) { return chain ? msdr_chain_get_info(chain, out) : MSDR_STATUS_ARGUMENT_ERROR; }
    // calc_demod_filter() of receiver `channel` (Minimal-SDR.ino:221-223): calc_FIR_coeffs(FIR_AM_coeffs, numTaps, filter_bandwidth, 70, 0, 0.0, 24000)
    int setBandwidthChannel(uint32_t channel, float bandwidth_hz)
    {
        if (!chain || !num_taps) return MSDR_STATUS_ARGUMENT_ERROR;
        std::vector<int16_t> buf(2 * (size_t)num_taps + 8, 0);      // (room for the designer's other filter types)
        msdr_calc_FIR_coeffs(buf.data(), (int)num_taps, bandwidth_hz, 70, 0, 0.0, 24000);
        return setTapsChannel(channel, buf.data(), nullptr);
    }
    // ANR_on per receiver (host array of channels() values; nullptr: anr_on_all for every receiver), Minimal-SDR.ino:702-770
    int setAnr(const int32_t *anr_on, int32_t anr_on_all = 0) { return chain ? msdr_chain_set_anr(chain, anr_on, anr_on_all) : MSDR_STATUS_ARGUMENT_ERROR; }
    int setOsc(const void *osc_i, const void *osc_q) { return chain ? msdr_chain_set_osc(chain, osc_i, osc_q) : MSDR_STATUS_ARGUMENT_ERROR; }
    // tune() of receiver `channel` (Minimal-SDR.ino:328-368): that receiver's own Osc_I_buffer_i / Osc_Q_buffer_i (osc_len entries each), nobody else's
    int setOscChannel(uint32_t channel, const void *osc_i, const void *osc_q)
    {
        return chain ? msdr_chain_set_osc_channels(chain, channel, 1, osc_i, osc_q) : MSDR_STATUS_ARGUMENT_ERROR;
    }
    // phase-accumulator oscillators for the whole bank (msdr_chain_set_nco_channels): step[c] = msdr_nco_step(f, fs) of receiver c, phase[c] the
    // phase of its next sample (nullptr: the phases carry on).  The first call of the node's life, before the first tick or directly after init_FIR()
    int setNco(const uint32_t *step, const uint32_t *phase = nullptr)
    {
        return chain ? msdr_chain_set_nco_channels(chain, 0, AudioGPU.channels(), step, phase) : MSDR_STATUS_ARGUMENT_ERROR;
    }
    // tune() of receiver `channel` (Minimal-SDR.ino:328-368) to ANY frequency: that receiver's step and nobody else's, phase-continuous (after setNco)
    int tuneChannel(uint32_t channel, double f_hz, double fs_hz = 24000.0)
    {
        if (!chain || !(fs_hz > 0.0) || !(f_hz == f_hz)) return MSDR_STATUS_ARGUMENT_ERROR;
        const uint32_t step = msdr_nco_step(f_hz, fs_hz);
        return msdr_chain_set_nco_channels(chain, channel, 1, &step, nullptr);
    }
    // the bank's output rate (msdr_chain_set_decimation; after setNco): every tick still consumes AUDIO_BLOCK_SAMPLES per receiver.  NOTE for
    // what is wired behind this node: with D > 1 the block it transmits is no longer full -- its first channels() * AUDIO_BLOCK_SAMPLES / D
    // samples are the tick's outputs as [channels()][AUDIO_BLOCK_SAMPLES / D], densely, and the rest of the block is not written.  No node of
    // this runtime knows D; connect only consumers of the caller's that do (readIq, readLevels, readSpectrum follow D by themselves)
    int setDecimation(uint32_t D) { return chain ? msdr_chain_set_decimation(chain, D) : MSDR_STATUS_ARGUMENT_ERROR; }
    // two-stage decimation (msdr_chain_set_prefilter[_f32]; after setNco, before the first tick or directly after init_FIR()): ONE real row of n
    // taps in CMSIS order decimates every receiver's mixed stream by D1 in front of its channel pair, which then runs at fs / D1 and decimates
    // by setDecimation's factor.  The block behind this node holds AUDIO_BLOCK_SAMPLES / (D1 * D) samples per receiver, as setDecimation's
    // note says of D; readLevels, readIq and readSpectrum follow the product by themselves.  D1 == 1 or n == 0: off
    int setPrefilter(uint32_t D1, const int16_t *taps, uint32_t n) { return chain ? msdr_chain_set_prefilter(chain, D1, n, taps) : MSDR_STATUS_ARGUMENT_ERROR; }
    int setPrefilter(uint32_t D1, const float *taps, uint32_t n) { return chain ? msdr_chain_set_prefilter_f32(chain, D1, n, taps) : MSDR_STATUS_ARGUMENT_ERROR; }
    // input samples per output of the bank: setPrefilter's factor times setDecimation's
    int rateDivisor(uint32_t *div)
    {
        uint32_t D = 1, D1 = 1;
        if (int rc = msdr_chain_get_decimation(chain, &D)) return rc;
        if (int rc = msdr_chain_get_prefilter(chain, &D1, nullptr)) return rc;
        *div = D * D1;
        return 0;
    }
    // one queue_adc feeds the bank (msdr_chain_set_input_rows): receiver c hears row rows[c] of the incoming block.  The block stays
    // [AudioGPU.channels()][AUDIO_BLOCK_SAMPLES]; with a map in force the node reads only its first n_inputs rows (so n_inputs <= channels()).
    // n_inputs == 0: every receiver hears its own row again
    int setInputRows(uint32_t n_inputs, const uint32_t *rows)
    {
        if (!chain || n_inputs > AudioGPU.channels()) return MSDR_STATUS_ARGUMENT_ERROR;
        return msdr_chain_set_input_rows(chain, n_inputs, rows);
    }
    // the bank's S-meter (msdr_chain_set_meter; the sketch's to-do list begins with it, Minimal-SDR.ino:48-50): every tick measures each receiver's
    // power behind its channel filter; the node owns the device buffer.  setMeter(false) switches the measurement off and frees it.
    int setMeter(bool on)
    {
        if (!chain) return MSDR_STATUS_ARGUMENT_ERROR;
        if (on && !d_meter) {
            void *p = nullptr;
            if (int rc = msdr_malloc(AudioGPU.context(), (size_t)AudioGPU.channels() * 8, &p)) return rc;
            if (int rc = msdr_chain_set_meter(chain, p)) { msdr_free(AudioGPU.context(), p); return rc; }
            d_meter = p;
        } else if (!on && d_meter) {
            if (int rc = msdr_chain_set_meter(chain, nullptr)) return rc;
            freeMeter();
        }
        return 0;
    }
    // the last tick's level of every receiver in dBFS (msdr_meter_dbfs: 0 = a full-scale carrier at the tuned frequency), channels() doubles.
    // Copies the meter back, so this one waits for the tick's kernels; -HUGE_VAL for a silent receiver.
    int readLevels(double *dbfs)
    {
        if (!chain || !d_meter || !dbfs) return MSDR_STATUS_ARGUMENT_ERROR;
        const uint32_t ch = AudioGPU.channels();
        std::vector<uint64_t> raw(ch);
        uint32_t D = 1;          // (setDecimation, setPrefilter: the tick's sums run over AUDIO_BLOCK_SAMPLES / D outputs)
        if (int rc = rateDivisor(&D)) return rc;
        if (int rc = msdr_memcpy_d2h(AudioGPU.context(), raw.data(), d_meter, (size_t)ch * 8)) return rc;
        for (uint32_t c = 0; c < ch; c++) {
            double s;
            if (f32) memcpy(&s, &raw[c], 8); else s = (double)raw[c];          // (F32 chains write doubles, Q15 chains exact integers)
            dbfs[c] = msdr_meter_dbfs(s, AUDIO_BLOCK_SAMPLES / D, f32 ? 32768.0 * (double)in_scale : 32768.0);
        }
        return 0;
    }
    // the bank's baseband output (msdr_chain_set_iq_out; the sketch's feature list ends with "Decoding of time signals or other digital modes [tbd]",
    // Minimal-SDR.ino:40): every tick stores each receiver's pairs {I, Q} behind its channel filter; the node owns the device buffer,
    // [channels()][AUDIO_BLOCK_SAMPLES] pairs (two int16 on Q15 chains, two floats on F32).  After setNco() only.  setIqOut(false) switches the
    // output off and frees the buffer.
    int setIqOut(bool on)
    {
        if (!chain) return MSDR_STATUS_ARGUMENT_ERROR;
        if (on && !d_iq) {
            void *p = nullptr;
            if (int rc = msdr_malloc(AudioGPU.context(), iqBytes(), &p)) return rc;
            if (int rc = msdr_chain_set_iq_out(chain, p, AUDIO_BLOCK_SAMPLES)) { msdr_free(AudioGPU.context(), p); return rc; }
            d_iq = p;
        } else if (!on && d_iq) {
            if (int rc = msdr_chain_set_iq_out(chain, nullptr, 0)) return rc;
            freeIq();
        }
        return 0;
    }
    // the buffer and pitch the chain writes to (msdr_chain_get_iq_out): for kernels of the caller's that consume the pairs on the device
    int iqOut(void **d_iq_out, uint64_t *pitch) { return chain ? msdr_chain_get_iq_out(chain, d_iq_out, pitch) : MSDR_STATUS_ARGUMENT_ERROR; }
    // the last tick's pairs of every receiver: `pairs` takes the whole buffer, [channels()][AUDIO_BLOCK_SAMPLES] pairs, of which the first
    // *n_out = AUDIO_BLOCK_SAMPLES / decimation of each row are the tick's (the rest is whatever an earlier tick left).  Copies the buffer
    // back, so this one waits for the tick's kernels.  n_out may be nullptr.
    int readIq(void *pairs, uint32_t *n_out)
    {
        if (!chain || !d_iq || !pairs) return MSDR_STATUS_ARGUMENT_ERROR;
        uint32_t D = 1;
        if (int rc = rateDivisor(&D)) return rc;
        if (int rc = msdr_memcpy_d2h(AudioGPU.context(), pairs, d_iq, iqBytes())) return rc;
        if (n_out) *n_out = AUDIO_BLOCK_SAMPLES / D;
        return 0;
    }
    // the bank's panadapter (msdr_chain_set_spectrum; "Spectrum display optional" on the sketch's to-do list, Minimal-SDR.ino:48-51, once per
    // receiver): every tick keeps each receiver's most recent 64 pairs behind its channel filter and, on showSpectrum's cadence (the first tick,
    // then every `every`-th; 0 = 25, UI.cpp:534-535), transforms them; the node owns the device buffer, [channels()][MSDR_SPECTRUM_BINS] powers
    // in display order (column 32 = the tuned frequency; uint32_t on Q15 chains, float on F32).  After setNco() only.  A repeated
    // setSpectrum(true, every) changes the cadence alone; setSpectrum(false) switches the display off and frees the buffer.
    int setSpectrum(bool on, uint32_t every = 0)
    {
        if (!chain) return MSDR_STATUS_ARGUMENT_ERROR;
        if (on) {
            void *p = d_spec;
            if (!p) if (int rc = msdr_malloc(AudioGPU.context(), specBytes(), &p)) return rc;
            if (int rc = msdr_chain_set_spectrum(chain, nullptr, p, every)) { if (!d_spec) msdr_free(AudioGPU.context(), p); return rc; }
            d_spec = p;
        } else if (d_spec) {
            if (int rc = msdr_chain_set_spectrum(chain, nullptr, nullptr, 0)) return rc;
            freeSpec();
        }
        return 0;
    }
    // the last spectrum drawn: `power` takes the whole buffer, [channels()][MSDR_SPECTRUM_BINS] entries of 4 bytes (msdr_spectrum_dbfs turns one
    // into dBFS), *drawn the spectra drawn since setSpectrum(true) -- unchanged since the last look means the buffer is, too.  Copies the
    // buffer back, so this one waits for the tick's kernels.  drawn may be nullptr.
    int readSpectrum(void *power, uint64_t *drawn)
    {
        if (!chain || !d_spec || !power) return MSDR_STATUS_ARGUMENT_ERROR;
        if (int rc = msdr_memcpy_d2h(AudioGPU.context(), power, d_spec, specBytes())) return rc;
        return msdr_chain_get_spectrum(chain, nullptr, nullptr, nullptr, drawn);
    }
    // a complex antenna stream (msdr_chain_set_complex_input; AudioEffectFreqConv's two ports in front of every receiver's filters): while on, port 0
    // carries I and port 1 carries Q of the tick -- a missing Q block counts as zeros -- and the node interleaves them into the block of pairs
    // {I, Q} it uploads for the chain, which applies freq_conv's full mix in direction dir (0: down by the receiver's frequency, 1: up).  After
    // setNco() only, and only over a clear FIR history: before the first tick, or directly after init_FIR().  The two blocks pass through the
    // host, so this tick waits for what produced them.  setComplexInput(false, 0) brings the real input back and frees the buffer.
    int setComplexInput(bool on, int dir)
    {
        if (!chain) return MSDR_STATUS_ARGUMENT_ERROR;
        void *p = nullptr;
        if (on && !d_cx) if (int rc = msdr_malloc(AudioGPU.context(), 2 * AudioGPU.block_bytes(), &p)) return rc;
        if (int rc = msdr_chain_set_complex_input(chain, on ? 1 : 0, dir)) { if (p) msdr_free(AudioGPU.context(), p); return rc; }
        if (p) d_cx = p;
        if (!on) freeCx();
        return 0;
    }
    // the bank's amp_adc / AGC() pair, once per receiver (msdr_chain_set_gain ...; Minimal-SDR.ino:385, 445-515): while on, every receiver's pair
    // behind its channel filter is amplified on the FIR accumulators before the demodulator sees it, and every tick ends with one AGC() step of
    // the receivers whose AGC is on -- the reference's cadence.  After setNco() only.  setGain(true) alone changes nothing (gain 1.0, AGC off).
    int setGain(bool on) { return chain ? msdr_chain_set_gain(chain, on ? 1 : 0) : MSDR_STATUS_ARGUMENT_ERROR; }
    // amp_adc.gain(n) of receiver rx: AGC_val = n and its multiplier from the next tick on
    int gain(uint32_t rx, float n) { return chain ? msdr_chain_set_gain_channels(chain, rx, 1, &n) : MSDR_STATUS_ARGUMENT_ERROR; }
    // AGC_on per receiver (host array of channels() values of 0 / 1; nullptr: agc_on_all for every receiver)
    int setAgc(const int32_t *agc_on, int32_t agc_on_all = 0) { return chain ? msdr_chain_set_agc(chain, agc_on, agc_on_all) : MSDR_STATUS_ARGUMENT_ERROR; }
    // receiver rx's record behind the last tick (msdr_chain_get_agc: multiplier, agc_idx, AGC_val bits, absmax, steps, 0, 0, agc_buffer[25]);
    // waits for the tick's kernels
    int readAgc(uint32_t rx, int32_t state[MSDR_AGC_STATE_WORDS]) { return chain ? msdr_chain_get_agc(chain, rx, state) : MSDR_STATUS_ARGUMENT_ERROR; }
    // Synchronous AM and the LMS filter for the bank (msdr_chain_set_bank_post): BEFORE setNco() and the first tick; from setNco() on the PLL
    // demodulator and the LMS filter run behind the per-receiver kernel on the stored pairs, at the bank's output rate.  For the node's life.
    int setBankPost(bool on = true) { return chain ? msdr_chain_set_bank_post(chain, on ? 1 : 0) : MSDR_STATUS_ARGUMENT_ERROR; }
    // the rate the PLL constants are evaluated for from the next tick on (msdr_chain_set_pll_rate): 0 = the reference's; after setBankPost()
    int setPllRate(double sample_rate) { return chain ? msdr_chain_set_pll_rate(chain, sample_rate) : MSDR_STATUS_ARGUMENT_ERROR; }
    // receiver rx's loop behind the last tick (msdr_chain_get_pll_state: fil_out, omega2, phzerror); waits for the tick's kernels
    int readPllState(uint32_t rx, float state[3]) { return chain ? msdr_chain_get_pll_state(chain, rx, state) : MSDR_STATUS_ARGUMENT_ERROR; }
    virtual void update(void)
    {
        audio_block_t *in = receiveReadOnly(0);
        audio_block_t *inq = receiveReadOnly(1);
        if (!in) { if (inq) release(inq); return; }
        audio_block_t *out = chain ? allocate() : nullptr;
        if (out) {
            // (a tick whose pairs could not be put together is dropped: the chain must never read a real block as pairs)
            const bool ok = !d_cx || interleave(in, inq) == 0;
            if (ok) {
                msdr_chain_process(chain, d_cx ? (const int16_t *)d_cx : in->data, out->data, AUDIO_BLOCK_SAMPLES);
                transmit(out);
            }
            release(out);
        }
        release(in);
        if (inq) release(inq);
    }

private:
    void freeMeter(void)
    {
        if (d_meter) msdr_free(AudioGPU.context(), d_meter);
        d_meter = nullptr;
    }
    size_t iqBytes(void) const { return (size_t)AudioGPU.channels() * AUDIO_BLOCK_SAMPLES * (f32 ? 2 * sizeof(float) : 2 * sizeof(int16_t)); }
    void freeIq(void)
    {
        if (d_iq) msdr_free(AudioGPU.context(), d_iq);
        d_iq = nullptr;
    }
    size_t specBytes(void) const { return (size_t)AudioGPU.channels() * MSDR_SPECTRUM_BINS * 4; }
    void freeSpec(void)
    {
        if (d_spec) msdr_free(AudioGPU.context(), d_spec);
        d_spec = nullptr;
    }
    void freeCx(void)
    {
        if (d_cx) msdr_free(AudioGPU.context(), d_cx);
        d_cx = nullptr;
    }
    // the tick's I block and Q block (nullptr: zeros) as [channels()][AUDIO_BLOCK_SAMPLES] pairs in d_cx
    int interleave(const audio_block_t *bi, const audio_block_t *bq)
    {
        const size_t n = (size_t)AudioGPU.channels() * AUDIO_BLOCK_SAMPLES;
        h_i.resize(n); h_q.assign(n, 0); h_pairs.resize(2 * n);
        if (int rc = msdr_memcpy_d2h(AudioGPU.context(), h_i.data(), bi->data, AudioGPU.block_bytes())) return rc;
        if (bq) if (int rc = msdr_memcpy_d2h(AudioGPU.context(), h_q.data(), bq->data, AudioGPU.block_bytes())) return rc;
        for (size_t k = 0; k < n; k++) { h_pairs[2 * k] = h_i[k]; h_pairs[2 * k + 1] = h_q[k]; }
        return msdr_memcpy_h2d(AudioGPU.context(), d_cx, h_pairs.data(), 2 * AudioGPU.block_bytes());
    }
    audio_block_t *inputQueueArray[2];
    msdr_chain *chain;
    uint32_t num_taps;
    void *d_meter;              // setMeter(true): [channels()] 8-byte sums, the node's own
    void *d_iq;                 // setIqOut(true): [channels()][AUDIO_BLOCK_SAMPLES] pairs {I, Q}, the node's own
    void *d_cx;                 // setComplexInput(true, dir): [channels()][AUDIO_BLOCK_SAMPLES] pairs {I, Q} of the tick, the node's own
    void *d_spec;               // setSpectrum(true): [channels()][MSDR_SPECTRUM_BINS] powers in display order, the node's own
    std::vector<int16_t> h_i, h_q, h_pairs;          // ... and the host side of the interleave
    bool f32;                   // the chain's arithmetic and int16 -> float scale, for readLevels and the size of a pair
    float in_scale;
};
