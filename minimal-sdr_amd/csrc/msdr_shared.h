// msdr_shared.h -- definitions shared by the host C-ABI layer and the gfx950 kernels.
#pragma once
#include <stdint.h>

namespace msdr {

constexpr int kThreads   = 256;                 // one workgroup = 4 wave64, one per SIMD of a CU
constexpr int kWaves     = kThreads / 64;
// Outputs per lane in the fused chain.  The LDS window holds {I,Q} pairs (8 B); a lane's window
// starts R pairs = R/2 16-byte slots after its neighbour's.  R/2 must be ODD so that the 16 lanes
// ds_read_b128 services per LDS cycle hit 16 different 16-byte slots (no bank conflict, no padding).
constexpr int kChainR    = 10;
constexpr int kChainTile = kThreads * kChainR;  // 2560 output samples per workgroup tile
// Single-stream FIR (arm_fir_f32 / arm_fir_fast_q15 mirrors): 4-byte elements, lane stride R/4 slots.
constexpr int kFirR      = 12;                  // 3 slots: odd
constexpr int kFirTile   = kThreads * kFirR;    // 3072
// Folded fp32 chain: one float per sample in LDS, 12 outputs per lane (3 slots: odd), and 12 is a
// multiple of every supported NCO period (1, 2, 4), so a lane's r-th output always has phase r mod P.
constexpr int kFoldR     = 12;
constexpr int kFoldTile  = kThreads * kFoldR;   // 3072
// Biquad-only kernel (arm_biquad_cascade_df1_f32 mirror)
constexpr int kBqR       = 8;
constexpr int kBqTile    = kThreads * kBqR;     // 2048

constexpr int kMaxStages = 4;

// Host-precomputed tables for the in-workgroup parallel evaluation of a df1 biquad CASCADE whose lanes
// each own L consecutive samples (DESIGN.md "IIR along time").  The cascade
//     H(z) = prod_s (b0 + b1 z^-1 + b2 z^-2)_s / (1 - a1 z^-1 - a2 z^-2)_s
// is evaluated as ONE numerator FIR  v = C(z) d,  C = prod_s B_s  (2S+1 taps, in registers), followed by
// S all-pole sections  w_s[n] = w_(s-1)[n] + a1 w_s[n-1] + a2 w_s[n-2].  For an all-pole section:
//   end state of a lane run from zero state   Z = sum_j (g[L-1-j], g[L-2-j]) v_j      (g = impulse response)
//   lane transition                           (y[L-1], y[L-2]) = M (p, q) + Z
template <int L>
struct BiquadCascadeTables {
    int nstages;
    int pad0[3];
    float num[2 * kMaxStages + 1 + 3];   // c_0 .. c_2S, zero padded to 12
    struct Section {
        float a1, a2;
        float pad1[2];
        float g[L][2];        // g[j] = (g_(L-1-j), g_(L-2-j))
        float mcol[4][2][2];  // M^(2^k), k = 0..3, stored by columns: [k][col][row]
        float m64[4];         // M^64 row-major 2x2 (one whole wave)
        float mlane[64][4];   // M^(l+1) stored {M00, M10, M01, M11} (columns), l = lane in wave
    } sec[kMaxStages];
};
// per-channel cascade state in HBM: 16 floats = d[n-1..n-8] (numerator history) | (w1, w2) per section
constexpr int kBqStateFloats = 16;

// Oscillator tables that were in force before a live change, oldest first (device memory, behind ONE pointer of ChainParams: the
// matrix-core kernels are at their register budget, every kernel argument costs them scalar registers).  A carried history sample at
// time t < sw[k] (t relative to the call, so sw <= 0) was mixed with table k when it arrived (freq_conv.cpp:70-103 mixes each block with
// the tables as they are at that update()), and chain_kernel<Arith> mixes it with that table again.
constexpr int kOscHistMax = 16;      // oscillator tables that can still have samples in one FIR history (msdr_chain_set_osc)
// stride (at the END: the kernels above read tab / sw / n where they always were): the per-channel-oscillator kernels (msdr_chain_oscpc.hiph)
// read channel ch's row of generation k at tab[k] + ch * stride[k] pairs -- 0 for a table that all channels shared, osc_len for a copy of
// the whole bank (msdr_chain_set_osc_channels)
struct OscHistory { const void *tab[kOscHistMax]; long long sw[kOscHistMax]; int n; int stride[kOscHistMax]; };

constexpr int kChainOutI16 = 0x40000000;

struct ChainParams {
    const int16_t *x;          // [channels][n] IF samples
    void *out;                 // [channels][n] float (F32) or int16 (Q15)
    const int16_t *hist_in;    // [channels][hist_len] raw IF history, oldest first
    int16_t *hist_out;         // written by the state kernel
    long long n;               // samples per channel in this call
    int channels;
    int nseg;                  // time segments per channel
    long long seg_len;         // multiple of the tile
    int warm;                  // IIR warm-up samples for segments > 0 (multiple of the tile)
    int ntaps_pad;             // taps per filter, front-padded with zeros to a multiple of 4
    int hist_len;              // = ntaps_pad - 1
    const void *taps;          // [tapsets][ntaps_pad] pairs {hI[k], hQ[k]}: float2 (F32) / int2 (Q15)
    const int *chan_mode;      // [channels]
    const int *chan_tapset;    // [channels]
    int mixer;                 // MSDR_MIXER_*
    const void *osc;           // [osc_len] pairs {osc_q ("cos"), osc_i ("sin")}: float2 / int2
    int osc_len;
    int phase0;                // (absolute index of sample 0 of this call) mod osc_len (mod 4 for FS4)
    float in_scale;
    int sqrt_kind;
    int nstages;               // F32 biquad stages
    const BiquadCascadeTables<kChainR> *bq;
    float *bq_state;           // [channels][kBqStateFloats]
    short *syncam_q;           // Q15, MSDR_CHAIN_SYNCAM_PLL: [channels][n] post-FIR Q of SYNCAM channels (their I goes to `out`); else null
    // folded F32 kernel (mixer folded into the taps; see DESIGN.md "Tap folding")
    const float *ftaps;        // [fsets][P rotations][steps][PE rows][2][2] folded tap pairs, in_scale included
    const int *chan_fset;      // [channels] folded-set index
    int fold_period;           // P: NCO period in samples (1, 2 or 4)
    int fold_rot;              // (absolute index of sample 0 of this call) mod P
    const BiquadCascadeTables<kFoldR> *bq_fold;   // lanes own kFoldR samples
    // matrix-core kernel (msdr_chain_mfma.hiph); uses chan_fset, fold_period, fold_rot
    const void *mf_tab;        // [fsets][P rotations] tables: MfmaTableHeader (1 KB) + B fragments, mf_stride bytes apart
    int mf_stride;
    int mf_halo;               // H: window samples before the tile, a multiple of 32 >= ntaps - 1
    int mf_bsteps;             // k-steps the LDS B region holds (max n0 + n1 over the tables)
    int mf_xsteps;             // wave-stream kernel: 2 KB steps of merged first + last k-steps behind them (msdr_sparse24.h), 0 = none
    const void *bq_mf;         // BiquadCascadeTables<16>: 16-sample chunks
    const void *bq_mf32;       // BiquadCascadeTables<32>: 32-sample blocks (msdr_biquad_paired.hiph)
    int mf_waves;              // waves per workgroup: 4 or 8
    // wave-stream matrix-core kernel (msdr_chain_mfw.hiph)
    const int *mf_units;       // [workgroups][mf_nw] pairs (channel, segment); channel < 0 = idle wave
    int mf_nw;                 // waves per workgroup (1..16)
    unsigned long long *dbg_buf;   // diagnostic build (-DMSDR_STAMPS): per-phase cycle sums, 8 per unit
    int dbg;                   // diagnostic bits: read from MSDR_DBG by the -DMSDR_STAMPS build only; the product build looks at ONE bit of it:
                               // kChainOutI16 -- chain_mfw_kernel / chain_amtr_kernel, F32: `out` is int16 [channels][n], written as arm_float_to_q15
                               // converts (MSDR_CHAIN_OUT_I16).  (A bit of an existing field: these kernels are at their register budget and
                               // every kernel argument costs them scalar registers -- a field of its own made the headline flavour spill.)
    const float *mw_iir;       // wave-stream kernel, folded IIR: MwIirConsts block (scan matrices, response fragments), or null
    float *bq_state_out;       // [channels][kBqStateFloats] cascade state after this call (ping-pong partner of bq_state)
    // chain_kernel<Arith> only: oscillator tables that were in force before a live change (msdr_chain_set_osc), or null -- see OscHistory
    const struct OscHistory *osc_hist;
};

// chain_q15pc_kernel (msdr_chain_q15pc.hiph): the Q15 chain / the arm_fir_fast_q15 stage with per-channel coefficients
struct PcParams {
    const int16_t *x;          // [channels][n] IF samples (FIR stage: input)
    short *out;                // [channels][n] audio (FIR stage: output)
    const int16_t *hist_in;    // [channels][hist_len] raw history, oldest first
    long long n;
    int channels;
    int hist_len;
    int np;                    // taps per row of the table: numTaps front-padded with zeros to a multiple of 8
    const int16_t *taps;       // [channels][2][np] (I row, Q row; CMSIS order) -- FIR stage: [channels][np]
    const int *chan_mode;      // [channels] (unused by the FIR stage)
    int mixer;                 // MSDR_MIXER_*
    const void *osc;           // [osc_len] int2 pairs {osc_q ("cos"), osc_i ("sin")}
    int osc_len;
    int phase0;                // (absolute index of sample 0 of this call) mod osc_len (mod 4 for FS4)
    int sqrt_kind;
    short *syncam_q;           // MSDR_CHAIN_SYNCAM_PLL: [channels][n] post-FIR Q of SYNCAM channels (their I goes to `out`); else null
    const struct OscHistory *osc_hist;     // oscillator tables in force before a live change, or null
    int nseg;                  // time segments per channel group
    long long seg_len;         // a multiple of the tile (8 * 64 / channels per wave)
    int nw;                    // waves per workgroup
    const int *in_row;         // [channels]: channel ch hears row in_row[ch] of x (msdr_chain_set_input_rows), x being [n_inputs][n]; null: row ch
    // msdr_chain_set_meter (msdr_chain_meter.hiph; read by the metered instantiations alone): the caller gives meter = d_meter [channels] (null:
    // off) and the chain's partials buffer; the launcher points `meter` at where the main kernel writes entry ch * nseg + segment
    unsigned long long *meter;
    unsigned long long *meter_part;        // [meter_cap] partials for calls in more than one time segment
    long long meter_cap;
};

// chain_f32pc_kernel (msdr_chain_f32pc.hiph): the fp32 chain / the arm_fir_f32 stage with per-channel coefficients
struct PcfParams {
    const void *x;             // [channels][n] IF samples, int16 (FIR stage: float input)
    float *out;                // [channels][n] audio before the cascade (FIR stage: output)
    const void *hist_in;       // [channels][hist_len] raw history, oldest first: int16 (FIR stage: float)
    long long n;
    int channels;
    int hist_len;
    int np;                    // taps per row of the table: numTaps front-padded with zeros to a multiple of 4
    const float *taps;         // [channels][2][np] (I row, Q row; CMSIS order) -- FIR stage: [channels][np]
    const int *chan_mode;      // [channels] (unused by the FIR stage)
    int mixer;                 // MSDR_MIXER_*
    const void *osc;           // [osc_len] float2 pairs {osc_q ("cos"), osc_i ("sin")}
    int osc_len;
    int phase0;                // (absolute index of sample 0 of this call) mod osc_len (mod 4 for FS4)
    float in_scale;
    const struct OscHistory *osc_hist;     // oscillator tables in force before a live change, or null
    int nseg;                  // time segments per channel group
    long long seg_len;         // a multiple of the tile (8 * 64 / channels per wave)
    int nw;                    // waves per workgroup
    const int *in_row;         // [channels]: channel ch hears row in_row[ch] of x (msdr_chain_set_input_rows), x being [n_inputs][n]; null: row ch
                               // (chains only: the FIR stage leaves it null)
    double *meter;             // msdr_chain_set_meter, as in PcParams: sums of squares in in_scale units
    double *meter_part;
    long long meter_cap;
};

// chain_q15pcn_kernel / chain_f32pcn_kernel (msdr_chain_ncopc.hiph): the two blocks above with the phase-accumulator oscillator's operands.
// `osc` is the bank [channels] of pairs {base0, step} (uint2), osc_len and phase0 are not read; a pending generation (osc_hist) is a copy
// of the whole bank, stride 1.
struct PcnParams : PcParams {
    const unsigned *sin_tab;   // [1024] packed sine table (msdr_nco.h: nco_pack), copied to LDS once per workgroup
    unsigned t0;               // chain time of sample 0 of this call: the low 32 bits of the sample count since msdr_chain_reset
    // msdr_chain_set_iq_out (msdr_chain_iq.hiph; read by the IQ instantiations alone, which the launchers pick by it): [channels][iq_pitch]
    // pairs {I, Q} of two int16, 16-byte aligned, iq_pitch a multiple of 8; null: off.  In those instantiations a null `out` skips the audio.
    int *iq;
    long long iq_pitch;
};
struct PcfnParams : PcfParams {
    const unsigned *sin_tab;
    unsigned t0;
    float *iq;                 // msdr_chain_set_iq_out, as in PcnParams: pairs of two floats ([channels][iq_pitch][2])
    long long iq_pitch;
};

// chain_q15pcnd_kernel / chain_f32pcnd_kernel (msdr_chain_decpc.hiph): the two blocks above with a decimator behind the FIR pair.  x, n, t0
// and the history are the INPUT's (full rate); `out` is [channels][nout], nseg / seg_len count outputs (seg_len a multiple of the tile
// opl * 64 / channels per wave).
struct PcndParams : PcnParams {
    int dec;                   // decimation D >= 2: output m is the demodulator's value at input sample m * D + D - 1
    int opl;                   // outputs per lane (msdr_decpc_geometry.h)
    long long nout;            // n / D
};
struct PcfndParams : PcfnParams {
    int dec;
    int opl;
    long long nout;
};

// the complex-input twins of those four (msdr_chain_cxpc.hiph; msdr_chain_set_complex_input): x is [channels or n_inputs][n] and hist_in
// [channels][hist_len] PAIRS {I, Q} of two int16, one 4-byte aligned dword each; n, hist_len and every other count stay in samples.  A block of
// its own, so that the real kernels keep their argument layout.
template <typename P>
struct CxParams : P {
    int cx_dir;                // freq_conv's dir: 0 mixes with exp(-j phase), 1 with exp(+j phase)
};
typedef CxParams<PcnParams> PcnCxParams;
typedef CxParams<PcfnParams> PcfnCxParams;
typedef CxParams<PcndParams> PcndCxParams;
typedef CxParams<PcfndParams> PcfndCxParams;

// the gain twins of those eight (msdr_chain_gain.hiph; msdr_chain_set_gain): the complex-input block of the family -- cx_dir is read by the
// twins on rows of pairs alone -- and the receivers' records.  A block of its own again.
constexpr int kGainWords = 32;          // ints per record (MSDR_AGC_STATE_WORDS)
template <typename P>
struct GainParams : P {
    int *agc;                  // [channels][kGainWords]: word 0 is read by every unit, word 6 takes the call's peak (atomicMax)
};
typedef GainParams<PcnCxParams> PcnGainParams;
typedef GainParams<PcfnCxParams> PcfnGainParams;
typedef GainParams<PcndCxParams> PcndGainParams;
typedef GainParams<PcfndCxParams> PcfndGainParams;

// chain_q15pcn2_kernel / chain_f32pcn2_kernel (msdr_chain_pre.hiph; msdr_chain_set_prefilter): the decimating gain twin's block -- a null
// meter / iq / agc skips that part, cx_dir is not read -- with the chain-wide prefilter in front.  `dec` is the SECOND factor (>= 1), nout
// n / (pre_dec * dec), and the history is pre_hist_len samples of raw IF (msdr_prepc_geometry.h).  A block of its own again.
template <typename P>
struct PreParams : P {
    const void *pre_taps;      // [pre_np] the prefilter row in CMSIS order, front-padded with zeros: int16 (Q15) / float (F32)
    int pre_np;                // a multiple of 8 (Q15) / 4 (F32)
    int pre_dec;               // D1: 2, 4, 8, 16 or 32
    int pre_chunk;             // intermediates per stage-1 chunk (the launcher's: pre_chunk(D1, channels per wave))
};
typedef PreParams<PcndGainParams> Pcn2Params;
typedef PreParams<PcfndGainParams> Pcfn2Params;

// chain_f32pcb_kernel (msdr_chain_f32pcb.hiph): a whole block-cadence call of the fp32 chain with per-channel settings in one launch
struct PcbParams {
    const int16_t *x;          // [channels][n] IF samples
    void *out;                 // [channels][n] audio behind the cascade: float, or int16 (out_i16)
    const int16_t *hist_in;    // [channels][hist_len] raw history, oldest first
    int16_t *hist_out;         // [channels][hist_len] the history this call leaves (another buffer than hist_in)
    int n;                     // 32 .. 512 samples, a multiple of 8
    int channels;
    int hist_len;
    int np;                    // taps per row of the table: numTaps front-padded with zeros to a multiple of 4
    const float *taps;         // [channels][2][np] (I row, Q row; CMSIS order)
    const int *chan_mode;      // [channels]
    const void *osc;           // float2 pairs {osc_q ("cos"), osc_i ("sin")}: channel ch reads osc_len pairs from pair ch * osc_stride on (unused: Fs/4)
    int osc_len;
    int osc_stride;            // 0: one table shared by all channels; osc_len: a bank [channels][osc_len]
    int phase0;                // (absolute index of sample 0 of this call) mod osc_len (mod 4 for Fs/4)
    float in_scale;
    int stages;                // 0 .. kMaxStages cascade sections in CMSIS order
    const float *bq_tab;       // channel ch reads 5 x stages coefficients from float ch * bq_stride on
    int bq_stride;             // 0: one row shared by all channels; kSbqTabFloats: a table [channels][kSbqTabFloats]
    float *bq_state;           // [channels][kBqStateFloats]: pState per stage, read and written in place
    int out_i16;               // `out` is int16, converted as arm_float_to_q15
    int nw;                    // waves per workgroup
    const int *in_row;         // [channels]: channel ch hears row in_row[ch] of x (msdr_chain_set_input_rows), x being [n_inputs][n]; null: row ch.
                               // hist_in / hist_out stay rows of the CHANNEL: what that receiver heard
};

// chain_q15pcb_kernel (msdr_chain_q15pcb.hiph): a whole block-cadence call of the Q15 chain with per-channel settings in one launch
struct QpcbParams {
    const int16_t *x;          // [channels][n] IF samples
    short *out;                // [channels][n] audio behind the nodes
    const int16_t *hist_in;    // [channels][hist_len] raw history, oldest first
    int16_t *hist_out;         // [channels][hist_len] the history this call leaves (another buffer than hist_in)
    int n;                     // 32 .. 512 samples, a multiple of 8
    int channels;
    int hist_len;
    int np;                    // taps per row of the table: numTaps front-padded with zeros to a multiple of 8
    const int16_t *taps;       // [channels][2][np] (I row, Q row; CMSIS order)
    const int *chan_mode;      // [channels]
    const void *osc;           // int2 pairs {osc_q ("cos"), osc_i ("sin")}: channel ch reads osc_len pairs from pair ch * osc_stride on (unused: Fs/4)
    int osc_len;
    int osc_stride;            // 0: one table shared by all channels; osc_len: a bank [channels][osc_len]
    int phase0;                // (absolute index of sample 0 of this call) mod osc_len (mod 4 for Fs/4)
    int sqrt_kind;
    int nnodes;                // 0, 1 or 2 AudioFilterBiquad nodes behind the demodulator
    int *defs0, *defs1;        // their records [channels][32]: coefficient words 0..4, state words 5..7 (read and written in place), word 7 bit 31 =
                               // another stage follows; every channel is read from its own record
    int nw;                    // waves per workgroup
    const int *in_row;         // [channels]: channel ch hears row in_row[ch] of x (msdr_chain_set_input_rows), x being [n_inputs][n]; null: row ch.
                               // hist_in / hist_out stay rows of the CHANNEL: what that receiver heard
};

}  // namespace msdr
