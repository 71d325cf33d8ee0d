/*
 * include/msdr.h -- C ABI of the MI355X-native Minimal-SDR demodulation chain.
 *
 * Drop-in boundary for the hot path of FrankBoesing/Minimal-SDR (citations relative to the
 * reference tree): IF samples -> I/Q mix -> FIR pair -> AM/SSB demod -> cascaded IIR biquad.
 * Plain C: pointers and sizes only; no C++/torch types.  Every function returns an msdr_status
 * (0 = OK; negative values mirror CMSIS `arm_status`, src/CMSIS_5/arm_math.h:404-413) and never
 * throws.  The library never takes ownership of caller buffers.
 *
 * Memory convention: pointers named `d_*` are DEVICE pointers (hipMalloc / msdr_malloc /
 * torch tensor data_ptr) valid on the context's GPU; all other pointers are HOST pointers that
 * are read during the call and not retained (the reference's CMSIS functions retain the caller's
 * coefficient/state pointers, arm_fir_init_q15.c:100-109 -- here the library copies coefficients
 * to the device and owns the state, which lives in HBM between calls).
 *
 * Batch layout in HBM: a "block batch" is [channels][block_len] row-major, one contiguous time
 * series per receiver channel (the reference's unit is one audio_block_t = int16[128] of ONE
 * channel, freq_conv.cpp:70, filter_biquad.cpp:42).  Channels are independent.
 *
 * All work is enqueued on the context's HIP stream and is asynchronous with respect to the
 * host; msdr_ctx_synchronize() (or synchronising the stream you supplied) waits for it.
 * There is NO CPU fallback: if no HIP device is usable every entry point fails with
 * MSDR_STATUS_NO_DEVICE.
 */
#ifndef MSDR_H
#define MSDR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSDR_VERSION_MAJOR 0
#define MSDR_VERSION_MINOR 1

typedef int16_t q15_t;     /* arm_math.h:423 */
typedef float float32_t;   /* arm_math.h:438 */

/* ---- status: arm_status values (arm_math.h:404-413) + device errors ------------------- */
typedef enum {
    MSDR_STATUS_SUCCESS        = 0,   /* ARM_MATH_SUCCESS */
    MSDR_STATUS_ARGUMENT_ERROR = -1,  /* ARM_MATH_ARGUMENT_ERROR (e.g. odd numTaps, arm_fir_init_q15.c:93-96) */
    MSDR_STATUS_LENGTH_ERROR   = -2,  /* ARM_MATH_LENGTH_ERROR */
    MSDR_STATUS_SIZE_MISMATCH  = -3,  /* ARM_MATH_SIZE_MISMATCH */
    MSDR_STATUS_NO_DEVICE      = -100,/* no usable HIP device / wrong architecture */
    MSDR_STATUS_HIP_ERROR      = -101,/* a HIP runtime call failed: see msdr_last_error() */
    MSDR_STATUS_OUT_OF_MEMORY  = -102
} msdr_status;

/* ---- demodulator modes: stations.h:4  enum { SYNCAM, AM, LSB, USB, CW } ---------------- */
enum { MSDR_MODE_SYNCAM = 0, MSDR_MODE_AM = 1, MSDR_MODE_LSB = 2, MSDR_MODE_USB = 3, MSDR_MODE_CW = 4 };
/* AM/CW magnitude: Minimal-SDR.ino:606-616 (Teensy 3.6: sqrtf) or :618-627 (Teensy 3.2: arm_sqrt_q31>>16) */
enum { MSDR_SQRT_F32 = 0, MSDR_SQRT_Q31 = 1 };
/* mixer in front of the FIR pair */
enum {
    MSDR_MIXER_FS4 = 0,   /* multiplication-free Fs/4 mixer, Minimal-SDR.ino:546-558 */
    MSDR_MIXER_NCO = 1    /* AudioEffectFreqConv, freq_conv.cpp:30-116: IF on port 0, zeros on port 1, dir = 1 */
};
/* arithmetic flavour of a chain */
enum {
    MSDR_ARITH_Q15 = 0,   /* the reference as written: arm_fir_fast_q15 + integer demod + Teensy biquad; bit-exact */
    MSDR_ARITH_F32 = 1    /* arm_fir_f32 / arm_biquad_cascade_df1_f32 semantics, int16 in, fp32 out */
};
#define MSDR_AUDIO_BLOCK_SAMPLES 128           /* Teensy core default (Minimal-SDR.ino:525) */
#define MSDR_AUDIO_SAMPLE_RATE_EXACT 44117.64706 /* Teensy core constant used by filter_biquad.h:58 */
#define MSDR_MAX_BIQUAD_STAGES 4               /* filter_biquad.cpp:86 */
#define MSDR_MAX_TAPSETS 8

/* ======================================================================================
 * Context: one GPU + one HIP stream.
 * ====================================================================================== */
typedef struct msdr_ctx msdr_ctx;

/* device: HIP device ordinal.  hip_stream: a hipStream_t to enqueue on (e.g. torch's current
 * stream), or NULL to let the context create and own one. */
int  msdr_ctx_create(int device, void *hip_stream, msdr_ctx **out);
int  msdr_ctx_destroy(msdr_ctx *ctx);
int  msdr_ctx_synchronize(msdr_ctx *ctx);
void *msdr_ctx_stream(msdr_ctx *ctx);                       /* the hipStream_t in use */
const char *msdr_last_error(void);                          /* thread-local text of the last failure */
const char *msdr_version(void);
const char *msdr_build_rev(void);                           /* source revision the library was built from ("<git hash>[+dirty]"), for measurement records */
int  msdr_device_count(void);                               /* usable gfx950 devices; never initialises one */

/* device-memory helpers (callers may equally pass pointers from hipMalloc or a torch tensor) */
int msdr_malloc(msdr_ctx *ctx, size_t bytes, void **d_ptr);
int msdr_free(msdr_ctx *ctx, void *d_ptr);
int msdr_memcpy_h2d(msdr_ctx *ctx, void *d_dst, const void *src, size_t bytes);   /* stream-ordered, returns after the copy */
/* Optional: HIP events on the context's stream around the MAIN kernel of each msdr_fir_q15_process / msdr_fir_f32_process call
 * (not its history kernel), for roofline arithmetic; msdr_ctx_get_kernel_time synchronises the stream and returns the sum of
 * the durations and the number of launches since the last reset.  (The fused chain has its own pair: msdr_chain_enable_timing.) */
int msdr_ctx_enable_kernel_timing(msdr_ctx *ctx, int on);
int msdr_ctx_get_kernel_time(msdr_ctx *ctx, double *total_ms, uint64_t *launches, int reset);
int msdr_memcpy_d2h(msdr_ctx *ctx, void *dst, const void *d_src, size_t bytes);
int msdr_memcpy_d2d(msdr_ctx *ctx, void *d_dst, const void *d_src, size_t bytes);     /* stream-ordered, asynchronous */
int msdr_memset(msdr_ctx *ctx, void *d_dst, int value, size_t bytes);

/* ======================================================================================
 * The path's one exchange step: gathering demodulated audio across the GPUs of a node (one
 * process per GPU; channels are sharded).  RCCL over xGMI, driven from C; RCCL is
 * loaded on first use (dlopen of librccl.so.1), so a single-GPU application does not need it.
 *   rank 0: msdr_comm_get_unique_id(id) -> hand the 128 bytes to the other ranks by any host channel
 *   all   : msdr_comm_create(ctx, id, rank, world, &comm)
 *   per block k (two or more audio buffers, slot = k % MSDR_GATHER_SLOTS):
 *           msdr_chain_process(..., audio[k % 2], ...);                    compute on the context's stream
 *           msdr_gather_audio_begin(comm, slot, audio[k % 2], bytes, d_all, root);   asynchronous, on the communicator's own
 *                                                                          stream, ordered after the compute queued so far
 *           ... block k + 1 is demodulated meanwhile ...
 *           msdr_gather_audio_wait(comm, slot, 0) before anything reuses audio[k % 2] / reads d_all (device-side wait on the
 *                                                 context's stream; host_wait = 1 blocks the calling thread instead)
 * root >= 0: only that rank receives, d_recv = [world][local_bytes] in rank order (peers send over one link each);
 * root < 0 : every rank receives (all-gather).  Every rank passes the same local_bytes (pad the last shard).
 * ====================================================================================== */
#define MSDR_GATHER_SLOTS 4
typedef struct msdr_comm msdr_comm;
int msdr_comm_get_unique_id(void *id128);
int msdr_comm_create(msdr_ctx *ctx, const void *id128, int rank, int world, msdr_comm **out);
int msdr_gather_audio_begin(msdr_comm *comm, int slot, const void *d_local, size_t local_bytes, void *d_recv, int root);
int msdr_gather_audio_wait(msdr_comm *comm, int slot, int host_wait);
int msdr_comm_destroy(msdr_comm *comm);

/* ======================================================================================
 * Host-side designers (setup path; pure CPU arithmetic, no device needed).
 * ====================================================================================== */
/* calc_FIR_coeffs, Minimal-SDR.ino:782-872 (with m_sinc :874-881, Izero :883-899).  Same
 * argument list and same overrun behaviour as the reference: type 0 writes numCoeffs entries,
 * types 2/3 write numCoeffs+1, type 4 (Hilbert) writes up to 2*numCoeffs+2. */
void msdr_calc_FIR_coeffs(int16_t *coeffs, int numCoeffs, float32_t fc, float32_t Astop, int type,
                          float dfc, float Fsamprate);
/* The sketch takes `PI` from outside (PIH = PI / 2, .ino:779).  msdr_calc_FIR_coeffs evaluates it as the vendored CMSIS
 * header's float fallback (src/CMSIS_5/arm_math.h:365-367); on a Teensy, Arduino.h's double literal is defined first and
 * `m * PIH` etc. are then evaluated in double, which moves single taps by 1 LSB after the truncation to int16.
 * msdr_calc_FIR_coeffs_pid is that variant.  Both are bit-exact against the compiled reference built with the matching PI. */
void msdr_calc_FIR_coeffs_pid(int16_t *coeffs, int numCoeffs, float32_t fc, float32_t Astop, int type,
                              float dfc, float Fsamprate);
/* AudioFilterBiquad::setLowpass/.../setHighShelf, src/Audio/filter_biquad.h:56-149.
 * coef[5] = {b0,b1,b2,a1,a2} scaled by 2^30 in textbook sign, exactly what the reference hands
 * to setCoefficients(stage, const int*).  sample_rate: the reference hard-codes
 * AUDIO_SAMPLE_RATE_EXACT (callers multiply cut-offs by CORR_FACT, Minimal-SDR.ino:86,391). */
enum { MSDR_BQ_LOWPASS = 0, MSDR_BQ_HIGHPASS, MSDR_BQ_BANDPASS, MSDR_BQ_NOTCH, MSDR_BQ_LOWSHELF, MSDR_BQ_HIGHSHELF };
int msdr_biquad_design(int kind, float frequency, float q_or_gain, float slope, double sample_rate, int32_t coef[5]);

/* ======================================================================================
 * Kernel-function API: CMSIS-DSP / Teensy-Audio mirrors, batched over channels.
 * Instances are opaque handles (state lives in HBM); `blockSize` may differ between calls.
 * d_src/d_dst: [channels][blockSize].  In-place (d_dst == d_src) is allowed where the
 * reference allows it.
 * ====================================================================================== */

/* arm_fir_init_q15 / arm_fir_fast_q15 (arm_math.h:1106-1128; arm_fir_init_q15.c:78-138,
 * arm_fir_fast_q15.c:60-329).  pCoeffs: host, numTaps entries in CMSIS (time-reversed) order,
 * shared by all channels.  Odd numTaps -> MSDR_STATUS_ARGUMENT_ERROR like the reference.
 * Creation zeroes the state (arm_fir_init_q15.c:106). */
typedef struct msdr_fir_q15 msdr_fir_q15;
int msdr_fir_q15_create(msdr_ctx *ctx, uint16_t numTaps, const q15_t *pCoeffs, uint32_t channels, msdr_fir_q15 **out);
int msdr_fir_q15_process(msdr_fir_q15 *S, const q15_t *d_src, q15_t *d_dst, uint32_t blockSize);
int msdr_fir_q15_reset(msdr_fir_q15 *S);
/* New coefficients for a running filter, state kept: what rewriting the caller-owned array behind S->pCoeffs does in the reference
 * (the instance only holds the pointer, arm_fir_init_q15.c:100-109; the bandwidth menu rewrites FIR_AM_coeffs in place with no
 * init_FIR(), UI.cpp:337-345, Minimal-SDR.ino:221-223).  Same numTaps as at creation.  Stream-ordered behind the calls queued so far. */
int msdr_fir_q15_set_coeffs(msdr_fir_q15 *S, const q15_t *pCoeffs);
/* The same for channels first_channel .. first_channel + count - 1 only, each with an array of its own: pCoeffs is a HOST array
 * [count][numTaps] (CMSIS order) -- a bank of arm_fir_instance_q15 whose pCoeffs point at different arrays.  Any int16 value is a legal
 * tap.  State and history length are kept; count == 0 does nothing; a range past `channels` is MSDR_STATUS_ARGUMENT_ERROR.  From the first
 * such call on msdr_fir_q15_process runs the kernel whose coefficient operand is per channel (chain_q15pc_kernel, FIR-only flavour);
 * msdr_fir_q15_set_coeffs keeps writing all channels.  Instances of more than 10 576 taps are refused (MSDR_STATUS_ARGUMENT_ERROR, nothing
 * changed: the kernel keeps a channel's window in 64 KB of LDS).  Synchronises the stream. */
int msdr_fir_q15_set_coeffs_channels(msdr_fir_q15 *S, uint32_t first_channel, uint32_t count, const q15_t *pCoeffs);
int msdr_fir_q15_destroy(msdr_fir_q15 *S);

/* arm_fir_init_f32 / arm_fir_f32 (prototypes arm_math.h:1182-1202; CMSIS-DSP V1.5.x). Any numTaps >= 1. */
typedef struct msdr_fir_f32 msdr_fir_f32;
int msdr_fir_f32_create(msdr_ctx *ctx, uint16_t numTaps, const float32_t *pCoeffs, uint32_t channels, msdr_fir_f32 **out);
/* (The 16..~290-tap kernel deals its tiles from a queue that the launch itself leaves as it found it -- its last wave out re-zeroes the
 * counters --, so a launch can be replayed; what alternates from call to call is the pair of history buffers, as in the chain: a HIP graph
 * a caller records over this stage should hold an even number of consecutive calls.  msdr_fir_f32_kernel_name reports the kernel for
 * blocks below 2^31 tiles x channels; beyond that the one-stream-per-wave kernel runs.) */
int msdr_fir_f32_process(msdr_fir_f32 *S, const float32_t *d_src, float32_t *d_dst, uint32_t blockSize);
int msdr_fir_f32_reset(msdr_fir_f32 *S);
int msdr_fir_f32_set_coeffs(msdr_fir_f32 *S, const float32_t *pCoeffs);   /* as msdr_fir_q15_set_coeffs: state kept, same numTaps */
/* As msdr_fir_q15_set_coeffs_channels, word for word: pCoeffs is a HOST array [count][numTaps] (CMSIS order) for channels first_channel ..
 * first_channel + count - 1.  State and history length are kept; count == 0 does nothing; a range past `channels` and a NULL array are
 * MSDR_STATUS_ARGUMENT_ERROR.  From the first such call on msdr_fir_f32_process runs chain_f32pc_kernel (FIR-only flavour: plain fp32 FMAs,
 * no input-range scaling: msdr_fir_f32_set_input_range has nothing to say there) over the existing history; msdr_fir_f32_set_coeffs keeps
 * writing all channels.  Instances of more than 7 936 taps are refused (MSDR_STATUS_ARGUMENT_ERROR, nothing changed: the kernel keeps a
 * channel's window and tap row in 64 KB of LDS).  Synchronises the stream. */
int msdr_fir_f32_set_coeffs_channels(msdr_fir_f32 *S, uint32_t first_channel, uint32_t count, const float32_t *pCoeffs);
const char *msdr_fir_f32_kernel_name(msdr_fir_f32 *S);      /* the kernel msdr_fir_f32_process launches for this instance */
/* Filters of 16..513 taps run on the matrix cores with the samples as two fp16 pieces (22 bits) after a power-of-two scale.  By
 * default the scale is chosen per 1024-output tile from the data (block floating point): nothing to declare.  max_abs > 0 pins
 * one scale for samples below that magnitude (saves the per-tile maximum; samples above it would overflow); 0 = automatic again.
 * No counterpart in CMSIS (arm_fir_f32 is plain fp32).
 * Guaranteed precision (arm_fir_f32 has none that depends on the input; this does, and here is the bound).  Let Mw be the largest
 * magnitude in the SCALE WINDOW of a tile (tiles are the 1024-output pieces of one call, counted from its first sample; the numTaps - 1
 * samples before a call are the carried history):
 *   16 .. 289 taps (fir_f32tq_kernel): the tile's 1024 samples and the numTaps - 1 before them, rounded up to a multiple of 32;
 *   290 .. 513 taps (fir_f32mf_kernel): the tile's 1024 samples and the whole tile before it (at most: the first tile of one of the
 *     kernel's time segments looks back as far as the line above says);
 *   a pinned range: max_abs rounded up to a power of two, for every tile.
 * Every sample x of a tile's outputs enters the products with an error of at most max(2^-21 |x|, 2^-39 Mw), every tap h with at most
 * max(2^-21 |h|, 2^-38 hmax), the sums are fp32.  (290 .. 513 taps: a sample of the numTaps - 1 before the tile keeps the pieces it was
 * given under the previous tile's scale while the scale grows finer by at most 2^12 -- then read 2^-27 Mw for it -- or coarser by at
 * most 2^24 -- its two pieces are each rounded once more, to the new scale: read 2^-37 Mw --; past either it is converted again.)
 * So a sample keeps its full 22 bits down to 2^-18 of Mw; below that it keeps 22 - (R - 18) bits at 2^-R of Mw (19 bits one part in a million below the window's peak).  An isolated spike therefore costs the quiet
 * outputs of ITS OWN scale windows a relative 2^-19 ... 2^-15 for spikes 10^6 ... 10^7 times the quiet level, never the stretches before
 * or after those windows; a level step costs the quiet side the windows that hold loud samples and nothing behind them.
 * Magnitude range: the scale exponent is limited to +-100, so the bound holds for windows whose Mw lies between 2^-86 and 2^115 (filters
 * whose largest tap lies between 2^-13 and 2^40; the outputs must fit fp32).  A window with a finite sample of 2^116 or more is lost
 * (fp16 infinities), one whose Mw is below 2^-86 keeps fewer bits: in both cases the damage stays in the scale windows that hold such
 * samples, of that channel.
 * Non-finite samples: a NaN or an infinity costs its own channel the outputs of the scale windows that hold it -- more than the numTaps
 * outputs arm_fir_f32 loses: the matrix products spread 0 x NaN, and the window's scale is spent on it --, no other channel, no other
 * window, and not the next call once the history has passed it.  The numTaps outputs that arm_fir_f32 would make non-finite are
 * non-finite here: a NaN is never turned into a number.
 * (tests/fir_f32_edges.py is this paragraph as code; tests/test_gpu_fir_f32_edges.py holds every kernel of the stage to it,
 * tests/test_gpu_stages.py: test_fir_f32_isolated_spike, test_fir_f32_matrix_core_input_ranges.) */
int msdr_fir_f32_set_input_range(msdr_fir_f32 *S, float max_abs);
int msdr_fir_f32_destroy(msdr_fir_f32 *S);

/* arm_biquad_cascade_df1_init_f32 / arm_biquad_cascade_df1_f32 (prototypes arm_math.h:1333-1351).
 * pCoeffs: host, 5*numStages {b0,b1,b2,a1,a2}, feedback terms ADDED (CMSIS convention). */
typedef struct msdr_biquad_df1_f32 msdr_biquad_df1_f32;
int msdr_biquad_df1_f32_create(msdr_ctx *ctx, uint8_t numStages, const float32_t *pCoeffs, uint32_t channels, msdr_biquad_df1_f32 **out);
int msdr_biquad_df1_f32_process(msdr_biquad_df1_f32 *S, const float32_t *d_src, float32_t *d_dst, uint32_t blockSize);
int msdr_biquad_df1_f32_reset(msdr_biquad_df1_f32 *S);
/* New coefficients (all 5 * numStages of them) for a running cascade with CMSIS semantics: the filter carries on from the state
 * arm_biquad_cascade_df1_f32 would hold in pState -- x[n-1], x[n-2], y[n-1], y[n-2] of every stage (arm_math.h:1233) -- as it does
 * when a caller rewrites pCoeffs between two calls.  The block-parallel kernels keep their state in another basis (numerator history
 * + all-pole section states), which depends on the coefficients: the library converts old basis -> CMSIS state -> new basis on the
 * host (csrc/msdr_cascade_state.h), per channel, and switches between the block-parallel and the CMSIS-order kernel if the new
 * cascade's conditioning asks for it (msdr_biquad_df1_f32_cascade_info).  Synchronises the stream.  ARGUMENT_ERROR if the old
 * cascade's state cannot be expressed as a CMSIS state (a later stage's numerator shares a root with an earlier stage's denominator). */
int msdr_biquad_df1_f32_set_coeffs(msdr_biquad_df1_f32 *S, const float32_t *pCoeffs);
/* The same for channels first_channel .. first_channel + count - 1 only, each with an array of its own: pCoeffs is a HOST array
 * [count][5 * numStages] -- a bank of arm_biquad_casd_df1_inst_f32 whose pCoeffs point at different arrays (every receiver its own notch).
 * Per-channel coefficients run in CMSIS order only (biquad_df1_seq_pc_kernel: one lane per channel, every lane its own coefficients), where
 * the state is pState itself and does not depend on the coefficients: the call writes the named rows and leaves every state alone.  At the
 * FIRST call an instance that runs block-parallel is moved to the CMSIS order with its state (the one refusal of
 * msdr_biquad_df1_f32_set_coeffs applies: ARGUMENT_ERROR, nothing changed), and every channel starts from the shared coefficients; the
 * instance stays per-channel for the rest of its life, and msdr_biquad_df1_f32_set_coeffs then writes ALL rows in place (state kept, no
 * change of kernel).  Long blocks of few channels are still split into time segments: the warm-up follows the LARGEST pole radius over all
 * rows, and a row with a pole on the unit circle (radius >= 0.99999) or with no pole at all keeps the call in one piece.  count == 0 does
 * nothing; a range past `channels`, a NULL array and numStages == 0 are MSDR_STATUS_ARGUMENT_ERROR, nothing changed.  Synchronises the stream. */
int msdr_biquad_df1_f32_set_coeffs_channels(msdr_biquad_df1_f32 *S, uint32_t first_channel, uint32_t count, const float32_t *pCoeffs);
/* The state as CMSIS keeps it: pState[4 * numStages] of one channel (synchronises the stream). */
int msdr_biquad_df1_f32_get_cmsis_state(msdr_biquad_df1_f32 *S, uint32_t channel, float32_t *pState);
int msdr_biquad_df1_f32_destroy(msdr_biquad_df1_f32 *S);
/* Host only (no device needed): how the library will evaluate this cascade.  *kappa = ||c||_1 ||g||_1 / ||h||_1 (conditioning of
 * the parallel "numerators first" form), *fp32_noise = distance of the sequential fp32 evaluation (arm_biquad_cascade_df1_f32 as
 * written) from a double evaluation on a fixed test signal, *cmsis_order = 1 if instances created with these coefficients run the
 * cascade section by section in CMSIS order instead of the block-parallel solver (the study: profiles/r02/DESIGN_r02_log.md 4.4c).  Any output pointer may be NULL. */
int msdr_biquad_df1_f32_cascade_info(uint8_t numStages, const float32_t *pCoeffs, double *kappa, double *fp32_noise, int *cmsis_order);
/* Host only: the two state conventions of one cascade (see msdr_biquad_df1_f32_set_coeffs).  lib_state[16]: [0..7] = the cascade's
 * last inputs d[n-1-k] (2 * numStages used), [8 + 2 s], [9 + 2 s] = w[n-1], w[n-2] of all-pole section s.  pState: CMSIS, 4 per stage.
 * from_cmsis keeps lib_state[0..7] as given on entry (the input history; entries 0, 1 must equal pState[0], pState[1]) and fills
 * [8..15] so that the block-parallel form continues exactly as arm_biquad_cascade_df1_f32 would from pState. */
int msdr_biquad_df1_f32_state_to_cmsis(uint8_t numStages, const float32_t *pCoeffs, const float32_t lib_state[16], float32_t *pState);
int msdr_biquad_df1_f32_state_from_cmsis(uint8_t numStages, const float32_t *pCoeffs, const float32_t *pState, float32_t lib_state[16]);

/* AudioFilterBiquad (src/Audio/filter_biquad.cpp:33-100, filter_biquad.h:33-155): up to 4 stages,
 * Q2.30 coefficients, int16 data, 14-bit error feedback.  A new node passes nothing (all-zero
 * definition, filter_biquad.h:36-39).  set_coefficients keeps the filter history like the
 * reference (filter_biquad.cpp:95-97) and silently ignores stage >= 4 (:86).
 * update(): in place on d_data [channels][blockSize]; blockSize must be even (the reference
 * processes sample pairs, :54-74).
 * set_coefficients_channels: the same setCoefficients(stage, coef) on channels first_channel ..
 * first_channel + count - 1 only, each with its own five words -- a bank of receivers, each with the
 * notch of the frequency it is tuned to (tune(), Minimal-SDR.ino:343-356).  coef is a HOST array
 * [count][5] as given to setCoefficients; the other channels' records are not touched; count == 0 and
 * stage >= 4 do nothing; a range past `channels` is MSDR_STATUS_ARGUMENT_ERROR.  From the first such
 * call on update() runs the kernel that reads every channel's own coefficients and stage count
 * (channels may then run 1 .. 4 stages side by side); set_coefficients keeps writing all channels. */
typedef struct msdr_biquad_q15 msdr_biquad_q15;
int msdr_biquad_q15_create(msdr_ctx *ctx, uint32_t channels, msdr_biquad_q15 **out);
int msdr_biquad_q15_set_coefficients(msdr_biquad_q15 *S, uint32_t stage, const int32_t coef[5]);
int msdr_biquad_q15_set_coefficients_channels(msdr_biquad_q15 *S, uint32_t first_channel, uint32_t count,
                                              uint32_t stage, const int32_t *coef);
int msdr_biquad_q15_update(msdr_biquad_q15 *S, q15_t *d_data, uint32_t blockSize);
int msdr_biquad_q15_get_definition(msdr_biquad_q15 *S, uint32_t channel, int32_t definition[32]); /* filter_biquad.h:152 */
int msdr_biquad_q15_destroy(msdr_biquad_q15 *S);

/* ======================================================================================
 * the front end in front of queue_adc (Minimal-SDR.ino:66-69, :76):
 *   adc1 (DC-block high-pass, src/Audio/input_adc.cpp:198-212) -> amp_adc (AudioAmplifier,
 *   src/Audio/mixer.cpp:34-47, :134-159) and AGC() (Minimal-SDR.ino:446-515), which
 *   demodulation() runs on every block it dequeues (:534) and which re-tunes amp_adc.
 * One instance keeps, per channel, what the reference keeps in statics: hpf_x1/hpf_y1
 * (input_adc.h:44-45), amp_adc's multiplier, AGC_val / AGC_on (.ino:100-104) and AGC()'s
 * 25-entry peak buffer + index.  Integer-exact (bit-for-bit with the oracle).
 * ====================================================================================== */
typedef struct msdr_frontend msdr_frontend;
#define MSDR_FE_DCBLOCK 1u           /* input is raw unsigned 16-bit conversions; run the DC-block filter */
#define MSDR_FE_AMP 2u               /* apply amp_adc's gain */
#define MSDR_FE_AGC 4u               /* run AGC() on every 128-sample block (needs MSDR_FE_AMP to have an effect) */
#define MSDR_FE_ALL 7u
#define MSDR_FE_STATE_WORDS 32u      /* [0] hpf_y1 [1] hpf_x1 [2] multiplier [3] agc_idx [4] AGC_val (float bits) [5] AGC_on [6..18] agc_buffer */
/* AudioInputAnalog() + AudioAmplifier() + the sketch's globals: hpf 0/0, AGC_val = AGC_start = 0.25 (.ino:94,:104,:385), AGC_on = 1 */
int msdr_frontend_create(msdr_ctx *ctx, uint32_t channels, msdr_frontend **out);
/* AudioInputAnalog::init, input_adc.cpp:60-63: hpf_x1 = first conversion << 14, hpf_y1 = 0.
 * first_conversion: host array of `count` values, count = 1 (all channels alike) or = channels. */
int msdr_frontend_prime(msdr_frontend *fe, const uint16_t *first_conversion, uint32_t count);
int msdr_frontend_set_agc(msdr_frontend *fe, int on);                     /* AGC_on, .ino:100 */
int msdr_frontend_gain(msdr_frontend *fe, float n);                       /* AGC_val = n; amp_adc.gain(n), mixer.h:75-79 */
/* d_adc: [channels][blockSize] uint16 (MSDR_FE_DCBLOCK) or int16; d_out: [channels][blockSize] int16 (may alias d_adc).
 * blockSize must be a multiple of 128 (AUDIO_BLOCK_SAMPLES: the AGC's update cadence), else MSDR_STATUS_LENGTH_ERROR.
 * A zero multiplier makes AudioAmplifier transmit nothing (mixer.cpp:139-142): such blocks come out as zeros here
 * and do not reach AGC(). */
int msdr_frontend_update(msdr_frontend *fe, const void *d_adc, q15_t *d_out, uint32_t blockSize, uint32_t stages);
int msdr_frontend_get_state(msdr_frontend *fe, uint32_t channel, int32_t state[MSDR_FE_STATE_WORDS]);
int msdr_frontend_destroy(msdr_frontend *fe);
/* AudioAmplifier as a stateless stage: multiplier as gain() computes it (mixer.h:75-79); in place.
 * *transmitted (may be NULL) = 0 when the node would transmit nothing (multiplier 0), else 1. */
int32_t msdr_amp_multiplier(float n);
int msdr_amp_q15(msdr_ctx *ctx, int32_t multiplier, q15_t *d_data, uint32_t channels, uint32_t blockSize, int *transmitted);

/* ======================================================================================
 * synchronous AM -- the PLL branch of the demod switch on Teensy 3.5/3.6
 * (Minimal-SDR.ino:631-688).  State per channel = the statics fil_out, omega2, phzerror
 * (:643-645).  d_mode: device int32 [channels] or NULL; with a mode array only SYNCAM
 * channels run the PLL, the others pass d_I through.  d_out may alias d_I.
 * sinf/cosf/atan2f are evaluated correctly rounded (see oracle/msdr_oracle.h, row f2).
 * In the fused Q15 chain, MSDR_CHAIN_SYNCAM_PLL selects this branch for SYNCAM channels
 * (default: SYNCAM demodulates like AM, the Teensy 3.2 build, .ino:618-627).
 * ====================================================================================== */
typedef struct msdr_syncam msdr_syncam;
int msdr_syncam_create(msdr_ctx *ctx, uint32_t channels, msdr_syncam **out);
int msdr_syncam_q15(msdr_syncam *S, const int32_t *d_mode, const q15_t *d_I, const q15_t *d_Q, q15_t *d_out, uint32_t blockSize);
int msdr_syncam_reset(msdr_syncam *S);
int msdr_syncam_get_state(msdr_syncam *S, uint32_t channel, float state[3]);    /* fil_out, omega2, phzerror */
void msdr_syncam_constants(float c[4]);                                         /* omega_min, omega_max, g1, g2 (:639-642) */
int msdr_syncam_destroy(msdr_syncam *S);

/* ======================================================================================
 * LMS automatic notch / noise reduction (Minimal-SDR.ino:702-770), the step
 * between the demod switch and queue_dac.playBuffer().  ANR_on: 0 = off, 1 = notch filter
 * (output = error), 2 = noise reduction (output = y).  State per channel = the statics
 * ANR_lidx, ANR_ngamma, ANR_in_idx, ANR_w[64] and the part of ANR_d[512] that is ever read.
 * d_anr_on: device int32 [channels] or NULL (then anr_on_all).  In place.
 * In the fused Q15 chain: msdr_chain_set_anr().
 * ====================================================================================== */
typedef struct msdr_anr msdr_anr;
#define MSDR_ANR_STATE_FLOATS 196u   /* lidx, ngamma, in_idx (int bits), pad | w[64] | d[128] (slot = ANR_in_idx & 127) */
int msdr_anr_create(msdr_ctx *ctx, uint32_t channels, msdr_anr **out);
int msdr_anr_q15(msdr_anr *A, const int32_t *d_anr_on, int32_t anr_on_all, q15_t *d_data, uint32_t blockSize);
int msdr_anr_reset(msdr_anr *A);
int msdr_anr_get_state(msdr_anr *A, uint32_t channel, float state[MSDR_ANR_STATE_FLOATS]);
int msdr_anr_destroy(msdr_anr *A);

/* ======================================================================================
 * SURVEY.md 8(f4), second half: the spectrum display's FFT (UI.cpp:520-592).
 *   msdr_rfft128_q15       <-> arm_rfft_q15(&FFT, data, FFT_out) with FFT = arm_rfft_init_q15(&FFT, 128, 0, 1) (UI.cpp:523,
 *                              :551; arm_rfft_q15.c:74-112, Cortex-M4 branches), batched: transform f reads 128 int16 at
 *                              d_src + f * src_stride (src_stride a multiple of 8 samples, d_src 16-byte aligned) and writes
 *                              d_fft_out[f][256] (interleaved re, im of 128 bins, the upper half the conjugate mirror) and/or
 *                              d_columns[f][128] = the 127 column heights showSpectrum draws,
 *                              y_new[x] = min(abs(FFT_out[127 - x]) / 200, 16) (UI.cpp:557-572), entry 127 = 0.
 *                              Either output may be NULL.  Unlike the reference, d_src is NOT transformed in place.
 *   msdr_rfft128_q15_inplace   the same, and like the reference (arm_rfft_q15.c:103-107) each transform also overwrites its
 *                              128 samples of d_src with the buffer CMSIS leaves there: the complex FFT's output after the
 *                              bit reversal (interleaved re, im of 64 bins).  Both outputs may be NULL; d_src is always written.
 *   msdr_rfft_q15_init_check   the argument check of arm_rfft_init_q15 (arm_rfft_init_q15.c:2154-2225): SUCCESS for
 *                              fftLenReal in {32 .. 8192} powers of two, else ARGUMENT_ERROR; this library runs 128 forward
 *                              with bit reversal only (what initSpectrum asks for) and reports other valid sizes as
 *                              MSDR_STATUS_LENGTH_ERROR.
 *   msdr_spectrum_*        <-> initSpectrum() / showSpectrum(): Spectrum_on, and spectrumCounter's "every 25th call"
 *                              cadence (UI.cpp:122, :534-536; the first call after create draws).  *drawn = 1 when this
 *                              call computed a spectrum (outputs written), 0 when it returned early like the reference.
 *   msdr_rfft128_tables    host side, no device: the constant tables the transform uses, regenerated from their documented
 *                              formulas -- twiddleCoef_64_q15[96] | realCoefAQ15 pairs at stride 64 [128] | realCoefBQ15 ditto [128]
 *                              (arm_common_tables.c:12914, arm_rfft_init_q15.c:44-56, :1086-1098).
 *   msdr_cfft64_q15 / msdr_cfft64_f32   a receiver's panadapter line: nfft batched 64-point complex forward transforms (bank_cfft64_q15_kernel /
 *                              bank_cfft64_f32_kernel, msdr_bank_spectrum.hiph).  Transform f reads 64 pairs {I, Q} at
 *                              d_pairs + 2 * f * stride_pairs (64 <= stride_pairs <= 2^40, else MSDR_STATUS_ARGUMENT_ERROR; d_pairs 4-byte
 *                              aligned for Q15, 8-byte for F32) and
 *                              writes d_bins[f][64] pairs {re, im} in natural bin order (bin k = k fs' / 64, k >= 32 the negative
 *                              frequencies) and / or d_power[f][64] in display order: column x = re^2 + im^2 of bin (x + 32) & 63, so
 *                              column 32 is the tuned frequency.  Either output may be NULL (both, or a misaligned operand -- the
 *                              outputs are written in 16-byte slots: MSDR_STATUS_ARGUMENT_ERROR); nfft == 0 does nothing; stream-ordered,
 *                              never synchronises.  Q15 is arm_cfft_q15 of length 64, forward, with bit reversal (arm_cfft_radix4_q15.c's
 *                              Cortex-M4 branch, then arm_bitreversal_16: what arm_rfft_q15 runs in front of its split stage), bit-exact,
 *                              scale 1 / 64; its power is the exact integer in a uint32_t (at most 2^31).  F32 bins are
 *                              (1 / 64) sum_m z[m] exp(-2 pi i k m / 64) in fp32 (twiddles rounded once from double; no atomics:
 *                              bit-identical from run to run), power re^2 + im^2 in fp32.
 *   msdr_spectrum_dbfs     host only: 10 log10(power / (full_scale^2 / 4)), -HUGE_VAL for power <= 0 -- msdr_meter_dbfs's convention
 *                              (full_scale = 32768 for Q15, 32768 * in_scale for F32): a full-scale real carrier on a bin centre behind a
 *                              unity-gain channel filter reads 0 dBFS in its bin.
 */
void msdr_rfft128_tables(int16_t tables[352]);
int msdr_rfft_q15_init_check(uint32_t fftLenReal, uint32_t ifftFlagR, uint32_t bitReverseFlag);
int msdr_rfft128_q15(msdr_ctx *ctx, const q15_t *d_src, uint64_t src_stride, q15_t *d_fft_out, uint8_t *d_columns, uint32_t nfft);
int msdr_rfft128_q15_inplace(msdr_ctx *ctx, q15_t *d_src, uint64_t src_stride, q15_t *d_fft_out, uint8_t *d_columns, uint32_t nfft);
typedef struct msdr_spectrum msdr_spectrum;
int msdr_spectrum_create(msdr_ctx *ctx, uint32_t channels, msdr_spectrum **out);
int msdr_spectrum_set_on(msdr_spectrum *S, int spectrum_on);
int msdr_spectrum_show(msdr_spectrum *S, const q15_t *d_data, uint64_t channel_stride, q15_t *d_fft_out, uint8_t *d_columns, int *drawn);
int msdr_spectrum_destroy(msdr_spectrum *S);
#define MSDR_SPECTRUM_BINS 64
int msdr_cfft64_q15(msdr_ctx *ctx, const q15_t *d_pairs, uint64_t stride_pairs, q15_t *d_bins, uint32_t *d_power, uint32_t nfft);
int msdr_cfft64_f32(msdr_ctx *ctx, const float *d_pairs, uint64_t stride_pairs, float *d_bins, float *d_power, uint32_t nfft);
double msdr_spectrum_dbfs(double power, double full_scale);

/* Stateless per-block stages. */
/* what AudioOutputAnalog::isr writes to the 12-bit DAC, output_dac.cpp:139-151: (sample + 32768) >> 4;
 * d_src == NULL = no block arrived: 2048 (mid-scale).  d_dest may alias d_src. */
int msdr_dac_format_q15(msdr_ctx *ctx, const q15_t *d_src, q15_t *d_dest, uint32_t channels, uint32_t blockSize);
/* Minimal-SDR.ino:546-558; block must start at a sample index = 0 (mod 4), as every 128-block does */
int msdr_mix_fs4_q15(msdr_ctx *ctx, const q15_t *d_x, q15_t *d_i, q15_t *d_q, uint32_t channels, uint32_t blockSize);
/* AudioEffectFreqConv::update, freq_conv.cpp:30-116, in place on d_i/d_q.  osc_i/osc_q: host tables of
 * osc_len entries (Osc_I_buffer_i / Osc_Q_buffer_i, freq_conv.h:33-34), applied at index (n mod osc_len).
 * `pass` keeps the reference's inverted meaning: pass == 0 forwards untouched (:49-56). */
int msdr_freqconv_q15(msdr_ctx *ctx, q15_t *d_i, q15_t *d_q, const q15_t *osc_i, const q15_t *osc_q, uint32_t osc_len,
                      int dir, int pass, uint32_t channels, uint32_t blockSize);
int msdr_freqconv_f32(msdr_ctx *ctx, float32_t *d_i, float32_t *d_q, const float32_t *osc_i, const float32_t *osc_q,
                      uint32_t osc_len, int dir, int pass, uint32_t channels, uint32_t blockSize);
/* arm_mult_q15 / arm_add_q15 / arm_sub_q15 (freq_conv.cpp:70-96) and arm_copy_q15 (Minimal-SDR.ino:577-578) over a block batch,
 * one kernel per call, asynchronous on the context's stream:
 *   d_dst[c][n] = op(d_a[c * a_stride + n], d_b[c * b_stride + n])    c < channels, n < blockSize; d_dst is dense [channels][blockSize]
 *   mult: ssat16((a * b) >> 15)   add: ssat16(a + b)   sub: ssat16(a - b)   copy: a
 * A source stride of 0 means ONE row of blockSize samples shared by every channel (an oscillator table); blockSize makes a source
 * dense [channels][blockSize].  All pointers are device pointers, 2-byte aligned (16-byte aligned rows take 16-byte accesses).  d_dst
 * may be d_a or d_b exactly (not a partial overlap, and not a shared row when channels > 1).  channels x blockSize < 2^31. */
int msdr_mult_q15(msdr_ctx *ctx, const q15_t *d_a, uint64_t a_stride, const q15_t *d_b, uint64_t b_stride, q15_t *d_dst,
                  uint32_t channels, uint32_t blockSize);
int msdr_add_q15(msdr_ctx *ctx, const q15_t *d_a, uint64_t a_stride, const q15_t *d_b, uint64_t b_stride, q15_t *d_dst,
                 uint32_t channels, uint32_t blockSize);
int msdr_sub_q15(msdr_ctx *ctx, const q15_t *d_a, uint64_t a_stride, const q15_t *d_b, uint64_t b_stride, q15_t *d_dst,
                 uint32_t channels, uint32_t blockSize);
int msdr_copy_q15(msdr_ctx *ctx, const q15_t *d_src, uint64_t src_stride, q15_t *d_dst, uint32_t channels, uint32_t blockSize);
/* demod switch, Minimal-SDR.ino:589-627.  d_mode: device int32 [channels] or NULL (then `mode` for all). */
int msdr_demod_q15(msdr_ctx *ctx, int mode, const int32_t *d_mode, int sqrt_kind, const q15_t *d_i, const q15_t *d_q,
                   q15_t *d_out, uint32_t channels, uint32_t blockSize);
int msdr_demod_f32(msdr_ctx *ctx, int mode, const int32_t *d_mode, const float32_t *d_i, const float32_t *d_q,
                   float32_t *d_out, uint32_t channels, uint32_t blockSize);

/* ======================================================================================
 * Fused chain = demodulation() (Minimal-SDR.ino:518-775: mix :546-558, FIR pair :574-575,
 * demod :589-691) + the biquad nodes wired behind queue_dac (.ino:77-81), ONE kernel pass:
 * one HBM read of the IF block batch, one HBM write of the audio block batch.
 * ====================================================================================== */
typedef struct {
    uint32_t struct_size;            /* = sizeof(msdr_chain_config) */
    int32_t  arith;                  /* MSDR_ARITH_Q15 | MSDR_ARITH_F32 */
    uint32_t channels;
    int32_t  mixer;                  /* MSDR_MIXER_FS4 | MSDR_MIXER_NCO */
    /* tap sets: the reference binds one coefficient pair per mode (init_FIR, .ino:901-930) */
    uint32_t num_taps;               /* taps per filter; q15 needs it even */
    uint32_t num_tapsets;            /* 1..MSDR_MAX_TAPSETS */
    const void *coeffs_i[MSDR_MAX_TAPSETS];   /* host; q15_t[num_taps] or float32_t[num_taps] by arith */
    const void *coeffs_q[MSDR_MAX_TAPSETS];
    /* per-channel selection (host arrays of `channels` entries, or NULL for the defaults) */
    int32_t  default_mode;           /* MSDR_MODE_AM / LSB / USB / CW */
    const int32_t *mode;             /* demod mode per channel */
    const int32_t *tapset;           /* tap-set index per channel (default 0) */
    int32_t  sqrt_kind;              /* MSDR_SQRT_F32 | MSDR_SQRT_Q31 (q15 arithmetic only) */
    /* NCO tables for MSDR_MIXER_NCO: q15_t or float32_t by arith; index (n mod osc_len), n counted from reset */
    uint32_t osc_len;
    const void *osc_i;               /* "sin", Osc_I_buffer_i */
    const void *osc_q;               /* "cos", Osc_Q_buffer_i */
    /* IIR stage */
    float    in_scale;               /* F32: int16 -> float scale; 0 means 1/32768 (arm_q15_to_float) */
    uint32_t num_biquad_stages;      /* F32: 0..4 stages of arm_biquad_cascade_df1_f32 */
    const float32_t *biquad_coeffs;  /* F32: host, 5*num_biquad_stages.  ACCURACY CONTRACT of the fp32 chain (tests/test_gpu_f32_contract.py):
                                      *   every output row is within 1e-5 relative RMS of arm_fir_f32 + arm_biquad_cascade_df1_f32 evaluated in CMSIS order in
                                      *   fp32 -- or, where that sequential fp32 evaluation is itself further than that from the exact (float64) result, within
                                      *   TWICE its distance from the exact result (+ fp32_noise + 1e-6, fp32_noise as below).  The second clause matters for cascades whose sections ring
                                      *   (narrow notches, resonant low / high-passes, three or more sections): their fp32 rounding noise, in any order of
                                      *   evaluation, is msdr_biquad_df1_f32_cascade_info()'s *fp32_noise (4e-7 for the reference's LP + notch; 1e-5 and more for
                                      *   random Q 8 sections below 1 kHz), and the block-parallel solver adds up to *kappa times the per-sample rounding; the
                                      *   library switches to the CMSIS order itself (one lane per channel behind the main kernel, *cmsis_order = 1) when
                                      *   kappa > 30 (20 from three sections on), kappa x fp32_noise > 2e-5 or fp32_noise > 2e-6, when a host-side emulation of
                                      *   the block-parallel evaluation is more than 1.5 x fp32_noise + 2e-7 from float64 on the host's test signal, and for three or four sections behind the
                                      *   general kernel.  Where the cascade removes most of its input (stacked high-passes), 1e-5 and 1e-6 are referred to the
                                      *   level of the cascade's input.  With the reference's filters and all BASELINE configurations: 5-6e-7.
                                      *   Round 5, frozen: the second clause is held on EVERY output row, excused or not -- the library is never further from the
                                      *   exact result than twice the CMSIS order's own distance + fp32_noise + 1e-6 of the cascade's input level (measured: at most
                                      *   0.47 of that bound).  That is what gives the gate teeth below 1e-5: builds with the taps cut to 16 bits (4e-6), the lo
                                      *   tap pieces dropped, or time segments without warm-up fail it (tests/test_gpu_f32_teeth.py).  The error model behind each
                                      *   term is DESIGN.md 5; a further term needs an argument from the reference's arithmetic, not a fuzz finding. */
    uint32_t num_biquad_nodes;       /* Q15: 0..2 AudioFilterBiquad nodes in series (biquad1_dac, biquad2_dac) */
    uint32_t node_stages[2];         /* Q15: stages used in each node (1..4) */
    const int32_t *node_coefs[2];    /* Q15: host, 5*node_stages[k] ints as given to setCoefficients */
    /* time segmentation of one call (F32 only; see DESIGN.md "IIR along time"):
     * 0 = automatic; 1 = never split a channel's block in time (IIR state carried exactly);
     * k > 1 = split every channel's block into k segments, each re-converging the IIR over
     * `biquad_warmup` samples (0 = derive from the pole radii for < 1e-9 residual). */
    uint32_t time_segments;
    uint32_t biquad_warmup;
    uint32_t flags;                  /* MSDR_CHAIN_* */
} msdr_chain_config;
#define MSDR_CHAIN_NO_TAP_FOLDING 1u /* F32: keep mixer and FIR pair as separate arithmetic steps (as written) */
#define MSDR_CHAIN_NO_FFT 4u         /* deprecated, accepted and ignored (round 2's FFT kernel is gone) */
#define MSDR_CHAIN_MFMA_WG 16u       /* deprecated, accepted and ignored (round 2's workgroup-tile matrix-core kernel is gone) */
#define MSDR_CHAIN_OUT_I16 128u      /* F32: d_audio is int16 [channels][n_samples] -- the play queue's sample type (src/Audio/play_queue.h:41) -- written as
                                        arm_float_to_q15 converts (prototype arm_math.h:6592; CMSIS-DSP 1.5.x: (q15_t) __SSAT((q31_t)(x * 32768.0f), 16)): 4 B
                                        per sample through HBM instead of 6, and half the bytes in the audio gather.  The matrix-core kernels convert in
                                        their store phase; chains that run a pass behind the main kernel (CMSIS-order cascade, PLL / LMS channels) or
                                        one of the vector-ALU kernels go through an fp32 scratch block batch owned by the chain: channels x n_samples x 4 bytes,
                                        allocated at the first such call and grown (with a stream synchronisation) when a longer call comes, plus one
                                        conversion pass over it -- 10 B per sample through HBM, not 4; call such chains in blocks, not in 2^18-sample
                                        calls (4 GB on c3's shape).  Ignored by Q15 chains. */
/* any other bit in msdr_chain_config.flags is refused with MSDR_STATUS_ARGUMENT_ERROR */
#define MSDR_CHAIN_NO_MFMA 8u        /* never run the FIR on the matrix cores (F32: split-fp16 MFMA kernel; Q15: byte-split i8 MFMA kernel) */
#define MSDR_CHAIN_FOLD_ANY_PERIOD 64u /* F32, NCO: fold the mixer into the taps (matrix-core kernel) also when the oscillator table's only period is its
                                         own length (8, 16 or 32 samples); a table that repeats within its length with period 1 .. 32 is folded by default */
#define MSDR_CHAIN_SYNCAM_PLL 32u    /* SYNCAM channels run the PLL demodulator (.ino:631-688) instead of the AM branch.  Q15: as the reference, on the int16
                                       FIR outputs.  F32 (an extension): the same loop on the fp32 FIR outputs, audio = corr[0] untruncated */

typedef struct msdr_chain msdr_chain;
int msdr_chain_create(msdr_ctx *ctx, const msdr_chain_config *cfg, msdr_chain **out);
/* d_if: int16 [channels][n_samples]; d_audio: int16 (Q15, or F32 with MSDR_CHAIN_OUT_I16) or float (F32) [channels][n_samples].
 * State (FIR history, IIR state, NCO phase) is carried from call to call, so calling with
 * n_samples = 128 reproduces the reference's block cadence and one call with a long block is the
 * same stream.  Q15 arithmetic needs n_samples even when biquad nodes are present. */
int msdr_chain_process(msdr_chain *chain, const int16_t *d_if, void *d_audio, uint64_t n_samples);
/* init_FIR() (Minimal-SDR.ino:901-930: memset + arm_fir_init_q15 of both instances): zeroes the FIR state and nothing else --
 * biquad / PLL / LMS state and the mixer's table position persist across a retune, as in the reference. */
int msdr_chain_init_fir(msdr_chain *chain);
/* stream restart (no counterpart in the reference): FIR state, fp32 cascade state, PLL and LMS state cleared, mixer phase 0.
 * The Teensy biquad NODES of a Q15 chain keep their history (the reference never clears it, filter_biquad.cpp:95-97). */
int msdr_chain_reset(msdr_chain *chain);
int msdr_chain_set_mode(msdr_chain *chain, uint32_t channel, int32_t mode, int32_t tapset);
/* ---- live updates: what the reference changes while the stream runs, every filter state kept ----------------------------------
 * All four synchronise the context's stream, rebuild the device tables of the chain on the host and take effect with the next
 * msdr_chain_process(); FIR history, cascade / node state, PLL and LMS state and the mixer's table position are untouched.
 *
 * msdr_chain_set_taps: new coefficients for one tap set (q15_t[num_taps] or float32_t[num_taps] by arith, CMSIS order) -- the
 *   bandwidth menu rewriting FIR_AM_coeffs in place under the running arm_fir_fast_q15 (UI.cpp:337-345, Minimal-SDR.ino:221-223:
 *   no init_FIR(), the instance holds a pointer, arm_fir_init_q15.c:100-109).  Every channel on that tap set hears the new filter
 *   from its next sample on, over the old filter's history.  F32 chains whose SSB tables carry the cascade's numerator hand the
 *   true numerator history over as first-sample corrections, as msdr_chain_set_mode does.
 * msdr_chain_set_node_coefficients (Q15): AudioFilterBiquad::setCoefficients(stage, coef) on biquad node `node` (0 = biquad1_dac,
 *   1 = biquad2_dac) of a running chain -- tune() re-programming the notch on every retune, Minimal-SDR.ino:356 ->
 *   filter_biquad.cpp:84-100; history kept (:95-97), stage >= 4 silently ignored (:86).
 * msdr_chain_set_node_coefficients_channels (Q15): the same on channels first_channel .. first_channel + count - 1 only, coef a HOST
 *   array [count][5] (msdr_biquad_q15_set_coefficients_channels): every receiver of the bank its own notch.  From the first such call
 *   on the chain runs its nodes as a kernel of their own behind the demodulator kernel (two launches per 128-sample tick instead of
 *   one); a msdr_chain_graph made before that call is refused afterwards, one made after it replays as usual.  The per-channel
 *   coefficients survive msdr_chain_set_taps / set_mode / set_osc, msdr_chain_reset and msdr_chain_init_fir.
 * msdr_chain_set_taps_channels (Q15): FIR coefficients that belong to the CHANNEL -- a bank of stations, each with its own filterBandwidth
 *   (stations.h:10-16; calc_demod_filter() rewriting FIR_AM_coeffs, Minimal-SDR.ino:221-223).  coeffs_i / coeffs_q: HOST arrays
 *   [count][num_taps] in CMSIS order for channels first_channel .. first_channel + count - 1, read during the call; coeffs_q == NULL means
 *   the same array behind both filters (init_FIR() for AM / SYNCAM, .ino:917-924).  num_taps is the chain's.  Any int16 value is a legal
 *   tap (32767 and -32768 included).  Semantics of msdr_chain_set_taps for the named channels only: every state kept, the channel hears
 *   the new filter from its next sample on over the old filter's history.  count == 0 does nothing; a range past `channels`, a NULL
 *   coeffs_i and an fp32 chain are MSDR_STATUS_ARGUMENT_ERROR.  From the first such call on, for the rest of its life, the chain runs
 *   chain_q15pc_kernel (coefficient operand per channel; msdr_chain_get_info().kernel names it) in place of the uniform demodulator
 *   kernels, with the PLL / LMS / biquad-node kernels behind it as before; a chain that never receives the call runs what it always ran.
 *   Interplay: msdr_chain_set_mode(chain, ch, mode, tapset) puts channel ch back on shared tap set `tapset` (its own taps are dropped);
 *   msdr_chain_set_taps(chain, tapset, ...) changes the channels still on that tap set and leaves channels with taps of their own alone;
 *   the per-channel taps survive msdr_chain_init_fir, msdr_chain_reset, msdr_chain_set_osc, msdr_chain_set_anr and both node-coefficient
 *   setters.  A msdr_chain_graph made before the first such call is refused afterwards; one made after it REPLAYS bit-exactly (block
 *   lengths 32 .. 512, no PLL / LMS channels, no pending oscillator change) and stays valid across later msdr_chain_set_taps_channels
 *   calls, which rewrite the table the captured launches read; like every graph it is refused after a live update that rebuilds the chain's
 *   tables (msdr_chain_set_taps, msdr_chain_set_osc, ...) and after msdr_chain_reset.
 * msdr_chain_set_taps_channels_f32 (F32): the same for an fp32 chain, with float arrays [count][num_taps]; the semantics are those of
 *   msdr_chain_set_taps_channels (arguments, states, interplay with msdr_chain_set_mode / set_taps / init_fir / reset / set_osc / set_anr /
 *   set_biquad_coeffs).  A Q15 chain is MSDR_STATUS_ARGUMENT_ERROR (and msdr_chain_set_taps_channels keeps refusing fp32 chains).  From
 *   the first such call on, for the rest of its life, the chain's demodulator kernel is chain_f32pc_kernel (plain fp32 FMAs on the vector
 *   ALU, coefficient operand per channel; msdr_chain_get_info().kernel names it, flavour carries MSDR_FLAVOUR_TAPS_PC); the cascade runs
 *   behind it in CMSIS order (MSDR_FLAVOUR_SEQ_CASCADE) -- at the first call a cascade that ran inside the kernel is moved there with its
 *   state, the way msdr_chain_set_biquad_coeffs moves one (and with that call's one refusal: a running cascade whose block-parallel state
 *   has no unique CMSIS state) --, PLL and LMS channels filter with their own rows, MSDR_CHAIN_OUT_I16 converts last.  Long calls are split
 *   into time segments (MSDR_FLAVOUR_SEGMENTED; msdr_chain_config.time_segments is honoured: 1 never splits, > 1 asks for that many); the
 *   FIR needs no warm-up.  Chains of more than 3 840 taps are refused
 *   (MSDR_STATUS_ARGUMENT_ERROR, nothing changed: a channel's two windows and two tap rows live in 64 KB of LDS).  Graphs: a
 *   msdr_chain_graph made before the first call is refused afterwards (MSDR_STATUS_ARGUMENT_ERROR at launch), and
 *   msdr_chain_graph_create on a chain already in per-channel mode is refused with MSDR_STATUS_ARGUMENT_ERROR (the launch geometry is
 *   chosen per call) -- unless msdr_chain_set_block_kernel is on: see there.
 * msdr_chain_set_block_kernel (F32; default off): with `on` != 0 a block-cadence call (32 .. 512 samples, a divisor of 1024) of a chain in
 *   per-channel mode (msdr_chain_set_taps_channels_f32 / msdr_chain_set_osc_channels, with or without a cascade, shared or per-channel
 *   cascade rows) runs chain_f32pcb_kernel: mixer, FIR, demodulator, the CMSIS-order cascade, the MSDR_CHAIN_OUT_I16 conversion and the next
 *   FIR history in ONE launch, the same operations in the same order as the unfused launches -- bit-identical audio and states.  The call is
 *   a switch of the host's: stream-ordered, every state kept, before or after the chain enters per-channel mode.  A call runs the unfused
 *   launches exactly as before while any of this holds: another block length; an oscillator generation pending (one history length after
 *   msdr_chain_set_osc / set_osc_channels); a chain created with MSDR_CHAIN_SYNCAM_PLL or with an LMS channel on; one wave's windows, tap
 *   rows, oscillator row and output row past 64 KB of LDS.  Both paths work on the same history, table position and cascade state, so a
 *   chain moves between them from call to call.  msdr_chain_get_info(): kernel begins "chain_f32pcb_kernel" (and ends in the name of the
 *   cascade that ran as its second phase), flavour = MSDR_FLAVOUR_BLOCK | MSDR_FLAVOUR_TAPS_PC, plus MSDR_FLAVOUR_OSC_PC,
 *   MSDR_FLAVOUR_SEQ_CASCADE and MSDR_FLAVOUR_CASCADE_PC where they apply.  A Q15 chain and a NULL chain are MSDR_STATUS_ARGUMENT_ERROR.
 *   Graphs: with the block kernel on, msdr_chain_graph_create accepts such a chain where the conditions above hold (and, as ever, `ticks`
 *   is even and the oscillator period divides n_samples).  The graph stays valid across later msdr_chain_set_taps_channels_f32 and
 *   msdr_chain_set_biquad_coeffs_channels calls, which rewrite rows the captured launches read (a call that allocates or moves a table --
 *   the first per-channel cascade call -- invalidates it).  msdr_chain_graph_launch is refused (MSDR_STATUS_ARGUMENT_ERROR, nothing
 *   enqueued) after msdr_chain_set_osc / set_osc_channels, msdr_chain_set_mode / set_taps / set_anr / set_biquad_coeffs, msdr_chain_reset,
 *   msdr_chain_set_block_kernel(chain, 0), an odd number of direct calls, and any other live update that rebuilds tables.
 * msdr_chain_set_block_kernel_q15 (Q15; default off): the same switch for a Q15 chain.  With `on` != 0 a block-cadence call (32 .. 512
 *   samples, a divisor of 1024) of a chain in per-channel mode (msdr_chain_set_taps_channels / set_osc_channels / set_input_rows) runs
 *   chain_q15pcb_kernel: mixer, FIR pair, demodulator, the 0 .. 2 AudioFilterBiquad nodes (every channel from its own records, so uniform
 *   and per-channel node coefficients alike, 1 .. 4 stages) and the next FIR history in ONE launch instead of three.  All arithmetic is
 *   integer and is the unfused kernels' own: audio, history and node records are theirs bit for bit.  The call is a switch of the host's:
 *   stream-ordered, every state kept, before or after the chain enters per-channel mode; off, or never called, nothing changes anywhere.
 *   A call runs the unfused launches exactly as before while any of this holds: another block length; an oscillator generation pending
 *   (one history length after msdr_chain_set_osc / set_osc_channels); a SYNCAM channel on a chain created with MSDR_CHAIN_SYNCAM_PLL; an
 *   LMS channel on (msdr_chain_set_anr); one wave's windows, tap rows, oscillator row and output row past 64 KB of LDS.  Both paths work on
 *   the same history, table position and node records, so a chain moves between them from call to call.  msdr_chain_get_info(): kernel
 *   begins "chain_q15pcb_kernel"; grid, block, lds_bytes, tile and taps_padded are the launch's; flavour stays 0 as on every Q15 chain.
 *   An F32 chain and a NULL chain are MSDR_STATUS_ARGUMENT_ERROR (and msdr_chain_set_block_kernel keeps refusing Q15 chains).
 *   Graphs: msdr_chain_graph_create accepts a Q15 chain in per-channel mode as before; with the switch on a captured tick is one launch.
 *   The graph stays valid across msdr_chain_set_taps_channels, and across msdr_chain_set_node_coefficients[_channels] on a chain whose
 *   nodes were per-channel already when it was made -- a change of a channel's stage count included: those calls rewrite rows and records
 *   in place, and the kernel reads the stage flags from the records at every launch.  msdr_chain_graph_launch is refused
 *   (MSDR_STATUS_ARGUMENT_ERROR, nothing enqueued) after msdr_chain_set_block_kernel_q15 changed the switch, after msdr_chain_set_anr, and
 *   after everything that refuses a Q15 per-channel graph already: msdr_chain_set_osc / set_osc_channels, set_mode, set_taps,
 *   msdr_chain_reset, an odd number of direct calls, msdr_chain_set_input_rows.  The stage instance msdr_fir_q15 is out of scope.
 *   Measured on one MI355X at 4096 channels x 128 samples with two one-stage per-channel nodes the fused tick is SLOWER than the three
 *   launches (48.5 against 38.0 us: the node phase runs on one lane per channel; README.md, profiles/block_pc_q15/): measure before turning
 *   it on.
 * msdr_chain_set_biquad_coeffs (F32): all 5 * num_biquad_stages coefficients of the arm_biquad_cascade_df1_f32 stage, CMSIS
 *   semantics (the filter carries on from the pState arm_biquad_cascade_df1_f32 would hold; see msdr_biquad_df1_f32_set_coeffs).
 *   The number of stages is fixed at creation, as numStages is in CMSIS.
 * msdr_chain_set_biquad_coeffs_channels (F32): the same on channels first_channel .. first_channel + count - 1 only, biquad_coeffs a HOST
 *   array [count][5 * num_biquad_stages] (msdr_biquad_df1_f32_set_coeffs_channels): every receiver of the bank its own notch, as tune()
 *   re-programs biquad2_dac (Minimal-SDR.ino:356).  Per-channel coefficients run in CMSIS order behind the demodulator kernel
 *   (biquad_df1_seq_pc_kernel; msdr_chain_get_info().kernel ends in its name, flavour carries MSDR_FLAVOUR_SEQ_CASCADE and
 *   MSDR_FLAVOUR_CASCADE_PC): at the first call a cascade that ran inside the kernel is moved there with its state, the way
 *   msdr_chain_set_taps_channels_f32 moves one (and with that call's one refusal), and stays there for the rest of the chain's life; the
 *   demodulator kernel is whatever the chain runs with its cascade behind it -- the uniform matrix-core kernels, or chain_f32pc_kernel on a
 *   chain that also has per-channel taps (the two calls combine in either order).  From then on a call writes rows and nothing else: every
 *   state is kept, the channel hears its new filter from its next sample on.  The rows survive msdr_chain_set_taps / set_taps_channels_f32 /
 *   set_mode / set_osc / init_fir and msdr_chain_reset (which clears the state only); msdr_chain_set_biquad_coeffs afterwards writes EVERY
 *   channel's row and the chain stays in per-channel mode.  count == 0 does nothing; a Q15 chain, a chain without a cascade, a range past
 *   `channels`, a NULL array and a coefficient that is not finite are MSDR_STATUS_ARGUMENT_ERROR, nothing changed.  PLL and LMS channels run
 *   a post cascade of their own with the chain's shared coefficients and are out of this call's scope: it is refused (ARGUMENT_ERROR, nothing
 *   changed) on a chain created with MSDR_CHAIN_SYNCAM_PLL and on a chain with any LMS channel on, and on a chain in per-channel-cascade mode
 *   msdr_chain_set_anr with any channel on is refused.  msdr_chain_graph_create is refused as for every cascade behind the kernel.
 * msdr_chain_set_osc: new contents for the NCO tables (same osc_len) -- AudioEffectFreqConv reads the global Osc_I_buffer_i /
 *   Osc_Q_buffer_i on every update() (freq_conv.h:33-34, freq_conv.cpp:70-103), so a sketch that rewrites them retunes the mixer
 *   without touching anything else; the position in the table carries on.  The samples already in the FIR history were mixed with the
 *   table of their own time, as in the reference (the mixer runs in front of the FIR's state buffer): the library keeps up to 16 earlier
 *   tables for as long as the history holds samples of theirs (a 17th change inside ONE history length drops the oldest).
 * msdr_chain_set_osc_channels: oscillator tables that belong to the CHANNEL -- tune() of receiver rx moves that receiver's local oscillator
 *   and nothing else (Minimal-SDR.ino:328-368); a bank of AudioEffectFreqConv nodes is a bank of Osc_I_buffer_i / Osc_Q_buffer_i pairs
 *   (freq_conv.h:33-34).  osc_i / osc_q: HOST arrays [count][osc_len], q15_t or float32_t by the chain's arithmetic as in
 *   msdr_chain_set_osc, for channels first_channel .. first_channel + count - 1, read during the call; osc_len is the chain's.  Semantics of
 *   msdr_chain_set_osc for the named channels only: the table position carries on (it is common to all channels), every filter state is
 *   kept, the samples already in a channel's FIR history stay mixed with the tables of their own time.  count == 0 does nothing; a NULL
 *   chain, a NULL array (either one), a range past `channels`, a chain with the Fs/4 mixer and, on an fp32 chain, a table entry that is not
 *   finite are MSDR_STATUS_ARGUMENT_ERROR, nothing changed.  From the first such call on, for the rest of its life, the chain's demodulator
 *   kernel is chain_q15pco_kernel (Q15; PLL, LMS and node kernels behind it as before) or chain_f32pco_kernel (F32; the cascade moves behind
 *   the kernel in CMSIS order with its state, exactly as the first msdr_chain_set_taps_channels_f32 call moves it and with that call's one
 *   refusal; MSDR_CHAIN_OUT_I16 converts last); msdr_chain_get_info().kernel names it, and on an fp32 chain flavour carries
 *   MSDR_FLAVOUR_OSC_PC beside MSDR_FLAVOUR_TAPS_PC (and MSDR_FLAVOUR_SEQ_CASCADE where there is a cascade).  Both kernels read per-channel
 *   tap rows: a chain without per-channel taps gets its table filled from the shared tap sets, and msdr_chain_set_taps_channels[_f32],
 *   msdr_chain_set_biquad_coeffs_channels and this call combine in any order.  msdr_chain_set_osc afterwards writes EVERY channel's row and
 *   the chain stays in per-channel mode.  The rows survive msdr_chain_set_taps / set_taps_channels[_f32] / set_mode / set_anr, the node and
 *   cascade setters, msdr_chain_init_fir and msdr_chain_reset (which clears the pending generations: no sample of theirs is left).
 *   Generations: one call is ONE generation for the whole chain, whatever `count` (and so is msdr_chain_set_osc); two calls with no
 *   msdr_chain_process between them count once; up to 16 are kept, a 17th inside one history length drops the oldest.  A pending generation
 *   is a device copy of the whole bank, channels x osc_len x 8 bytes, freed once the history has turned over.
 *   Limits: a channel's windows, tap rows and oscillator row live in 64 KB of LDS.  Q15: 12 x num_taps (rounded up to 8) + 4 x osc_len
 *   <= 61 440 -- 5 072 taps at osc_len = 128, every chain (num_taps <= 4096) up to osc_len = 3 072.  F32: 3 776 taps at osc_len = 128 (3 840
 *   without the row; every 64 entries more cost 32 taps).  Longer chains are refused at the first call (ARGUMENT_ERROR, nothing changed).
 *   fp32 chains whose PLL / LMS channels run through the auxiliary chain are out of scope (it is built from the shared tables): the call
 *   is refused (ARGUMENT_ERROR, nothing changed) on an fp32 chain created with MSDR_CHAIN_SYNCAM_PLL or with any LMS channel on, and on an
 *   fp32 chain in this mode msdr_chain_set_anr with any channel on is refused.  Q15 chains have no such limit.
 *   Graphs, Q15: a msdr_chain_graph made before the first call is refused at launch afterwards; one made in this mode is accepted under the
 *   conditions of per-channel taps (block lengths 32 .. 512, no PLL / LMS channels, no pending generation, the oscillator period dividing
 *   n_samples), replays bit-exactly, and is refused after any later msdr_chain_set_osc_channels / msdr_chain_set_osc.  F32:
 *   msdr_chain_graph_create is refused, as on every chain with the cascade behind the kernel.
 * msdr_chain_set_input_rows: one antenna, one ADC stream (or a handful), and a bank of receivers tuned to different stations inside it --
 *   the case per-channel oscillator tables exist for.  input_row: a HOST array [channels], read during the call; entry c names the row of
 *   d_if that receiver c hears.  From the next msdr_chain_process / msdr_chain_graph_create on, d_if is [n_inputs][n_samples] row-major
 *   (d_audio stays [channels][n_samples]) and receiver c produces, bit for bit, what it would produce if d_if[c] held a copy of row
 *   input_row[c].  Every state is kept: FIR history, node and cascade state, PLL / LMS state, the table position, pending oscillator
 *   generations.  The FIR history stays PER CHANNEL -- it holds what that receiver heard -- so a live change of the map is an antenna switch:
 *   the receiver carries on over its own old history, and msdr_chain_get_fir_history, msdr_chain_init_fir, msdr_chain_reset, the oscillator
 *   generations and the move between chain_f32pcb_kernel and the unfused launches work unchanged.  n_inputs == 0 (with any input_row) returns
 *   the chain to the identity: d_if is [channels][n_samples] again, states kept.  Stream-ordered; like its siblings it may synchronise the
 *   stream.  A NULL chain, n_inputs > 0 with a NULL array and an entry >= n_inputs are MSDR_STATUS_ARGUMENT_ERROR, nothing changed.
 *   From the first call on (whatever its n_inputs), for the rest of its life, the chain runs the per-channel kernel family
 *   (chain_q15pc_kernel / chain_q15pco_kernel; chain_f32pc_kernel / chain_f32pco_kernel / chain_f32pcb_kernel), whose kernels take the map as
 *   an operand: a chain not yet in per-channel mode enters it exactly as the first msdr_chain_set_osc_channels / set_taps_channels[_f32] call
 *   does (the tap table filled from the shared tap sets; F32: the cascade behind the kernel in CMSIS order with its state, with that move's
 *   one refusal and the per-channel kernel's tap limit).  The call combines in any order with msdr_chain_set_taps_channels[_f32],
 *   set_osc_channels, set_biquad_coeffs_channels, set_node_coefficients_channels and set_block_kernel; the map survives all of those and
 *   msdr_chain_set_taps / set_osc / set_mode / set_anr / init_fir / reset.  msdr_chain_get_info().kernel names the same kernels as before; on
 *   fp32 chains flavour carries MSDR_FLAVOUR_SHARED_IF while a map is in force.
 *   fp32 chains whose PLL / LMS channels run through the auxiliary chain are out of scope (it gathers its rows from d_if by channel and is
 *   built from the shared tables): the call is refused (ARGUMENT_ERROR, nothing changed) on an fp32 chain created with
 *   MSDR_CHAIN_SYNCAM_PLL or with any LMS channel on, and while a map is in force msdr_chain_set_anr with any channel on is refused on an
 *   fp32 chain, all three unless msdr_chain_set_bank_post is on.  Q15 chains have no such limit: their PLL / LMS / node kernels work on
 *   the demodulator's output.
 *   Graphs: a msdr_chain_graph made before a msdr_chain_set_input_rows call is refused at launch after it -- after ANY later call, the return
 *   to the identity included.  One made while a map is in force is accepted under the conditions per-channel chains have already (Q15: those
 *   of per-channel taps / oscillator tables; F32: only with msdr_chain_set_block_kernel on), its d_if[k] are [n_inputs][n_samples], and it
 *   replays bit-exactly.
 *   Out of scope: the uniform (matrix-core) kernels, the msdr_fir_* stage instances, fp32 chains with PLL / LMS channels, and sharing one
 *   history per input row (the histories cost channels x hist_len x 2 bytes as before).
 * msdr_chain_set_nco_channels: a PHASE-ACCUMULATOR oscillator per channel -- tune() of receiver rx sets that receiver's local oscillator to
 *   ANY frequency (Minimal-SDR.ino:328-368), where an oscillator table sits on multiples of fs / osc_len.  A receiver keeps one 32-bit
 *   phase and one 32-bit step (resolution fs / 2^32); the oscillator of a sample is {osc_q ("cos"), osc_i ("sin")} = {cosq, sinq} of the
 *   phase at that sample, as msdr_nco_q15 computes them (below), and the mixing is the table chains': Q15 ssat16((x * osc) >> 15), F32
 *   x * in_scale * (osc / 32768).  step / phase: HOST arrays of `count` entries for channels first_channel .. first_channel + count - 1,
 *   read during the call; phase may be NULL.  The named channels get step[k] from their next sample on.  With phase == NULL the phase
 *   carries on (a phase-continuous retune); otherwise the next sample has phase[k].  Every filter state is kept; the samples already in the
 *   FIR history stay mixed with the oscillator of their own time.  For step = k * 2^25 the oscillator equals the 128-entry table
 *   round(32767 sin / cos(2 pi k n / 128)): such a chain is bit-identical to the table chain.
 *   Generations: one call is ONE generation for the whole chain, whatever `count`; two calls with no msdr_chain_process between them count
 *   once; up to 16 are kept, a 17th inside one history length drops the oldest.  A generation is channels x 8 bytes, freed once the history
 *   has turned over.
 *   The first call puts the chain, for the rest of its life, into the per-channel kernel family with this oscillator: chain_q15pcn_kernel
 *   (Q15; PLL, LMS and node kernels behind it as before) or chain_f32pcn_kernel (F32; the cascade moves behind the kernel in CMSIS order
 *   with its state, with that move's one refusal; MSDR_CHAIN_OUT_I16 converts last).  The tap table is filled from the shared tap sets as
 *   the other per-channel setters fill it.  The first call must name every channel (first_channel == 0, count == channels) and is accepted
 *   only while the FIR history is clear -- before the first msdr_chain_process, or directly after msdr_chain_reset / msdr_chain_init_fir
 *   (a cleared history needs no generation of the old tables); otherwise MSDR_STATUS_ARGUMENT_ERROR, nothing changed.
 *   Refused (ARGUMENT_ERROR, nothing changed): a NULL chain, a NULL step, a range past `channels`, a chain created with MSDR_MIXER_FS4, a
 *   chain holding per-channel oscillator tables (msdr_chain_set_osc_channels), an fp32 chain created with MSDR_CHAIN_SYNCAM_PLL or with an
 *   LMS channel on (both unless msdr_chain_set_bank_post is on), and a filter too long for 64 KB of LDS beside the 4 KB sine table (Q15: more than 4 776 taps, no chain; F32: more than
 *   3 584).  count == 0 does nothing.
 *   On a chain in this mode msdr_chain_set_osc and msdr_chain_set_osc_channels are refused; msdr_chain_graph_create is refused (the time
 *   of a call's first sample is a launch operand: a replay would repeat one phase) and a graph made earlier is refused at launch;
 *   msdr_chain_set_anr with any channel on is refused on fp32 chains unless msdr_chain_set_bank_post is on; msdr_chain_set_block_kernel[_q15] is accepted and such calls run
 *   the unfused launches.  The bank survives msdr_chain_set_taps[_channels][_f32], set_mode, the node and cascade setters,
 *   msdr_chain_set_input_rows (in either order) and, on Q15 chains, set_anr.  msdr_chain_init_fir keeps phases and steps;
 *   msdr_chain_reset sets the chain's time and every phase to 0, keeps the steps and drops the pending generations.
 *   msdr_chain_get_info().kernel names the kernel; on fp32 chains flavour carries MSDR_FLAVOUR_NCO_PC beside MSDR_FLAVOUR_TAPS_PC (plus
 *   SEQ_CASCADE, SEGMENTED, SHARED_IF where they apply).
 * msdr_chain_get_nco: the channel's step and the phase of its NEXT sample (either pointer may be NULL); ARGUMENT_ERROR on a chain that is
 *   not in this mode.
 * msdr_chain_set_decimation: the third piece of a digital down-converter behind oscillator and FIR -- arm_fir_decimate_q15 /
 *   arm_fir_decimate_fast_q15 / arm_fir_decimate_f32's convention: D new samples into the state, one output ending at the newest.  With
 *   decimation D, output sample m of a call is exactly what the undecimated chain's demodulator would have produced at input sample
 *   m * D + D - 1 of that call, and the passes behind the demodulator run on that decimated stream as if it were the stream.  Mixer, FIR
 *   history and oscillator generations still see every input sample; the FIR pair, the demodulator, the store and every recurrence behind
 *   the kernel shrink by D.  D = 1 (the default) is off.
 *   msdr_chain_process with D > 1: d_if is unchanged ([channels or n_inputs][n_samples]); d_audio is [channels][n_samples / D].
 *   n_samples % D != 0 is MSDR_STATUS_LENGTH_ERROR, nothing enqueued, no state moved (the decimation phase is therefore 0 at every call
 *   boundary); a Q15 chain with biquad nodes needs n_samples / D even, same error.  The chain's time, the history and the generations
 *   advance by n_samples.  The Q15 nodes (shared or per-channel records), the F32 CMSIS-order cascade (shared or per-channel rows) and
 *   MSDR_CHAIN_OUT_I16 with its scratch get n_samples / D samples per channel.
 *   A switch of the host's: stream-ordered, may be called at any time, keeps every state.  The FIR history is raw IF at the full rate and
 *   does not care; node and cascade states simply CONTINUE AT THE NEW RATE -- the caller designs those filters for fs / D
 *   (msdr_biquad_design takes the sample rate).
 *   Scope: chains in phase-accumulator mode only (msdr_chain_set_nco_channels has been called), Q15 and F32; every other chain is
 *   MSDR_STATUS_ARGUMENT_ERROR, nothing changed.  Also refused: a Q15 chain created with MSDR_CHAIN_SYNCAM_PLL, a Q15 chain with an LMS
 *   channel on (and, while D > 1, msdr_chain_set_anr with any channel on), all three unless msdr_chain_set_bank_post is on; fp32 chains in this mode
 *   refuse both already.
 *   Values: 1 .. MSDR_MAX_DECIMATION_Q15 (60) / MSDR_MAX_DECIMATION_F32 (59).  The kernel's window of one wave with one channel --
 *   128 D + np mixed samples per stream (np = num_taps rounded up to 8 (Q15) / 4 (F32)), twice for odd D on Q15 chains -- must fit 64 KB of
 *   LDS beside the tap rows and the 4 KB sine table:
 *     Q15, even D:  512 D +  8 np <= 61 440      Q15, odd D:  1024 D + 12 np <= 61 440      F32:  1024 D + 16 np <= 61 440
 *   The maxima are the largest D such that every factor up to it holds an 8- (4-) tap filter; a D whose window does not fit beside THIS
 *   chain's filter is ARGUMENT_ERROR, nothing changed.  At 102 taps every factor up to 58 is accepted; at D = 8 filters of up to 7 168
 *   (Q15: every chain) / 3 328 (F32) taps, at D = 32 up to 5 632 / 1 792.
 *   Reporting: msdr_chain_get_info().kernel begins chain_q15pcnd_kernel / chain_f32pcnd_kernel, `tile` is the launch's tile in OUTPUTS,
 *   and on fp32 chains flavour carries MSDR_FLAVOUR_DECIMATED beside NCO_PC and TAPS_PC.  Graphs stay refused, as on every chain in this
 *   mode; msdr_chain_set_block_kernel[_q15] is accepted and such calls run the unfused launches.  The setting survives everything the
 *   oscillator bank survives: msdr_chain_reset and init_fir, the tap, node, cascade and NCO setters, msdr_chain_set_input_rows.
 * msdr_chain_get_decimation: the factor in force (1 on every chain that never set one).
 * msdr_chain_set_prefilter / msdr_chain_set_prefilter_f32: two-stage decimation, the way every down-converter reaches a narrow channel from
 *   a wideband input.  A chain-wide prefilter -- ONE real row taps[0 .. num_taps) in CMSIS order, the same for the I and the Q stream of
 *   every receiver -- decimates the mixed stream by D1, and the receiver's own channel pair runs on those intermediates at fs / D1 and
 *   decimates by D2 = msdr_chain_set_decimation's factor (which may be 1):
 *       u[j] = FIR_p over the mixed stream, taken at input sample j * D1 + D1 - 1 (arm_fir_decimate's convention)
 *              Q15: arm_fir_fast_q15's arithmetic (wrapping 32-bit accumulator, >> 15, saturated to int16); F32: arm_fir_f32's
 *       output m = the channel pair over u, taken at intermediate sample m * D2 + D2 - 1 -> demodulator, as the one-stage chain has it
 *   Everything behind the accumulators (meter, pairs, gain, demodulator, PLL / LMS of msdr_chain_set_bank_post, spectrum tail, nodes,
 *   cascade, int16 conversion) sees n_out = n_samples / (D1 * D2) samples at the rate fs / (D1 * D2); n_samples % (D1 * D2) != 0 is
 *   MSDR_STATUS_LENGTH_ERROR, nothing enqueued, no state moved.  The caller designs the channel taps for fs / D1 and node and cascade
 *   filters for fs / (D1 * D2).
 *   NO NEW STATE: the chain keeps raw IF history only, (np2 - 1) * D1 + np1 - 1 samples of it (np: the tap counts rounded up to 8 (Q15) /
 *   4 (F32)); the intermediates that a tile or a call shares with the one before it are recomputed from raw samples, so a Q15 chain is
 *   bit-exact however the stream is cut into calls.  For that reason the prefilter is set, changed or turned off (D1 == 1 or
 *   num_taps == 0) only over a CLEAR FIR history -- before the first msdr_chain_process, or directly after msdr_chain_reset /
 *   msdr_chain_init_fir: the rule of the first msdr_chain_set_nco_channels; at any other time ARGUMENT_ERROR, nothing changed.  The live
 *   setters (per-channel taps, NCO generations -- now over the longer history --, msdr_chain_set_decimation, mode, nodes, cascade, gain,
 *   meter, I/Q output, spectrum, bank post) keep working as they do at D > 1; a live change of the channel taps is the in-place pCoeffs
 *   rewrite of a stage-2 CMSIS instance, whose state is those same intermediates.
 *   Values: D1 in {2, 4, 8, 16, 32}; Q15 tap counts even (arm_fir_init_q15 refuses odd ones).  ARGUMENT_ERROR, nothing changed: a chain
 *   not in phase-accumulator mode, the other arithmetic's setter, a NULL row, non-finite taps, a history that is not clear, complex input
 *   on (msdr_chain_set_complex_input(on) while a prefilter is set is refused too), and a (D1, num_taps, chain taps, D2) whose smallest
 *   geometry -- one wave, one channel, 128 outputs: the window 128 D2 + np2 intermediates, a stage-1 chunk of 64 max(1, 16 / D1) D1 + np1
 *   mixed samples, both per stream, the tap rows, the 4 KB sine table and the prefilter row -- does not fit 64 KB of LDS;
 *   msdr_chain_set_decimation checks the same rule while a prefilter is set.
 *   Reporting: msdr_chain_get_info().kernel begins chain_q15pcn2_kernel / chain_f32pcn2_kernel, `tile` is the launch's tile in FINAL
 *   outputs, and on fp32 chains flavour carries MSDR_FLAVOUR_PREFILTER beside DECIMATED, NCO_PC and TAPS_PC.  Graphs stay refused;
 *   msdr_chain_set_block_kernel[_q15] is accepted and such calls run the unfused launches.  The setting survives what the decimation survives.
 * msdr_chain_get_prefilter: D1 and num_taps in force (1 and 0 while off); either pointer may be NULL.
 * msdr_chain_set_meter: the S-meter of the bank (the reference's to-do list begins with it, Minimal-SDR.ino:48-50) -- the power of every
 *   channel behind its channel filter and before its demodulator, measured inside the per-receiver kernels at no extra pass over memory.
 *   For a call of msdr_chain_process with n_out = n_samples / D outputs per channel
 *       meter[c] = sum over m < n_out of I_c[m]^2 + Q_c[m]^2
 *   with I_c[m], Q_c[m] the two FIR outputs the demodulator of output m receives, whatever the channel's mode (AM, SYNCAM -- under
 *   MSDR_CHAIN_SYNCAM_PLL too -- LSB, USB, CW); no node, cascade, LMS filter or int16 conversion is in it.
 *     Q15   I, Q = the saturated (acc >> 15) of arm_fir_fast_q15; the entry is a uint64_t, an exact integer whatever the launch geometry
 *           (a pair of squares is at most 2^31, 2^31 outputs of that fit)
 *     F32   the two fp32 sums in in_scale units; a lane's 8 outputs are added in fp32, everything beyond in double, in an order that the
 *           launch geometry fixes (no atomics): the entry is a double, bit-identical from run to run
 *   d_meter: device memory of the caller, [channels] entries of 8 bytes, 8-byte aligned; NULL = off (the default).  From the next
 *   msdr_chain_process on every successful call OVERWRITES all `channels` entries, on the chain's stream, without synchronising; a call
 *   that returns an error (MSDR_STATUS_LENGTH_ERROR included) writes nothing.  Integration over calls is the caller's business.  A
 *   misaligned pointer or a NULL chain is MSDR_STATUS_ARGUMENT_ERROR, nothing changed.
 *   The first non-NULL call enters the per-channel kernel family exactly as msdr_chain_set_input_rows does (tap table filled from the
 *   shared tap sets, fp32 cascade behind the kernel in CMSIS order), with that call's refusals: an fp32 chain created with
 *   MSDR_CHAIN_SYNCAM_PLL or with an LMS channel on (and, while a meter is set, msdr_chain_set_anr with a channel on; all three unless msdr_chain_set_bank_post is on), a filter beyond
 *   the per-channel kernel's tap limit.  NULL leaves the chain in that family with the meter off.  The pointer survives everything the
 *   input map survives: msdr_chain_reset and init_fir, every tap / oscillator / NCO / node / cascade / mode setter,
 *   msdr_chain_set_input_rows, msdr_chain_set_decimation.
 *   While a meter is set msdr_chain_set_block_kernel[_q15] stays accepted and calls run the unfused launches; msdr_chain_graph_create is
 *   refused, and a graph made before a msdr_chain_set_meter call is refused at launch after it.
 *   Reporting: msdr_chain_get_info().kernel keeps its names; on fp32 chains flavour carries MSDR_FLAVOUR_METER while a meter is set.
 *   A call in more than one time segment (info.time_segments) writes per-segment partials of the chain's own and adds them in segment
 *   order in a second small kernel (meter_reduce_kernel).
 * msdr_chain_get_meter: the pointer in force (NULL on a chain that never set one).
 * msdr_meter_dbfs (host only): 10 log10((sum_sq / n_out) / (full_scale^2 / 4)); full_scale = 32768 for Q15, 32768 * in_scale for F32;
 *   -HUGE_VAL for sum_sq <= 0 or n_out == 0.  0 dBFS is a full-scale real carrier at the tuned frequency behind a unity-gain channel
 *   filter (I^2 + Q^2 = A^2 / 4): round(32767 sin(2 pi 40 t / 128 + 0.3)) against bin 40 of 128 behind calc_FIR_coeffs(102, 2500 Hz)
 *   reads -0.005 dBFS from the second block on.
 * msdr_chain_set_iq_out: what a digital down-converter hands out -- the complex baseband I[m], Q[m] behind the channel filter at fs / D, for
 *   decoders of digital modes and every demodulator this library does not have (the reference's feature list ends with "Decoding of time
 *   signals or other digital modes [tbd]", Minimal-SDR.ino:40).  The per-receiver kernels hold the pair in registers where their demodulator
 *   consumes it; with a buffer set they store it too, at no extra pass over the IF stream.
 *   d_iq: device memory of the caller, [channels][pitch] pairs {I, Q}, interleaved; NULL = off (the default).
 *     Q15   two int16_t per pair: ssat16(acc >> 15) of each stream
 *     F32   two floats per pair (also under MSDR_CHAIN_OUT_I16): the two fp32 sums in in_scale units
 *   For a call of msdr_chain_process with n_out = n_samples / D outputs per channel, pair m < n_out of row c is I_c[m], Q_c[m] of the meter's
 *   definition above -- the two FIR outputs the demodulator of output m receives, whatever the channel's mode.  I is the stream filtered
 *   with coeffs_i, the oracle's i_out: LSB audio is I - Q, USB audio I + Q.  Pairs m >= n_out of a row are never written.
 *   From the next msdr_chain_process on every successful call OVERWRITES pairs 0 .. n_out - 1 of all rows, on the chain's stream, without
 *   synchronising; a call that returns an error writes nothing.  n_out > pitch is MSDR_STATUS_LENGTH_ERROR: nothing enqueued, no state moved.
 *   d_iq must be 16-byte aligned and pitch a non-zero multiple of 8 (a lane's 8 outputs are whole 16-byte slots of a row); chains in
 *   phase-accumulator mode only (msdr_chain_set_nco_channels has been called -- msdr_chain_set_decimation's scope rule), Q15 and F32.
 *   Anything else, a NULL chain included, is MSDR_STATUS_ARGUMENT_ERROR, nothing changed.  The setting survives everything the meter pointer
 *   survives: msdr_chain_reset and init_fir, every tap / NCO / node / cascade / mode setter, msdr_chain_set_input_rows,
 *   msdr_chain_set_decimation, msdr_chain_set_meter; it combines with all of them in either order.
 *   I/Q-only calls: while a buffer is set msdr_chain_process(chain, d_if, NULL, n) is accepted (without one NULL stays refused).  Mixer, FIR
 *   pair, history, the chain's time, the oscillator generations, the I/Q store and the meter (if set) run as always; the demodulator and the
 *   audio store, the Q15 nodes, the PLL / LMS passes, the fp32 cascade and the int16 conversion do not run and their states are untouched.
 *   The length rules of an audio call apply unchanged.
 *   Reporting: msdr_chain_get_info().kernel keeps its names; on fp32 chains flavour carries MSDR_FLAVOUR_IQ_OUT exactly while a buffer is
 *   set.  Graphs stay refused, as on every chain in this mode.
 * msdr_chain_get_iq_out: the buffer and pitch in force (NULL, 0 on a chain without one); either output may be NULL.
 * msdr_chain_set_complex_input: what a wideband front end delivers -- interleaved complex int16 pairs {I, Q} instead of the Teensy's one ADC
 *   pin.  The reference's mixer node is a complex mixer already: AudioEffectFreqConv::update (freq_conv.cpp:30-116) takes two input ports and
 *   forms all four products, in two directions; the chain's real input is its degenerate form "real IF on port 0, zeros on port 1, dir = 1".
 *   While on, d_if of msdr_chain_process is [channels or n_inputs][n_samples] PAIRS, two int16_t each, I first, 4-byte aligned (anything else:
 *   MSDR_STATUS_ARGUMENT_ERROR, nothing enqueued).  n_samples still counts samples (pairs) and every length rule stays in samples: the
 *   multiple of D, the even n / D with Q15 nodes, the I/Q pitch.  The input map (msdr_chain_set_input_rows) selects rows of pairs.
 *   With c = cosq and s = sinq of the receiver's phase at that sample (msdr_nco_q15):
 *     Q15   freq_conv.cpp:67-103 exactly: the four products ssat16((a * b) >> 15) of the original pair, then
 *             dir == 0:  I' = ssat16(I c + Q s)   Q' = ssat16(Q c - I s)          (the spectrum moves DOWN by the receiver's frequency)
 *             dir == 1:  I' = ssat16(I c - Q s)   Q' = ssat16(Q c + I s)          (up)
 *           dir is a sign on the second product of each sum, not on the oscillator: (-a) >> 15 is not -(a >> 15).
 *     F32   the same four products and two sums in fp32 on I in_scale, Q in_scale, c / 32768, s / 32768, each rounded on its own.
 *   I' feeds the coeffs_i filter and Q' the coeffs_q filter, as always.  With Q = 0 and dir = 1 this is the real chain, bit for bit on Q15.
 *   The FIR history becomes raw pairs (hist_len samples of 4 bytes per channel; a history sample keeps the oscillator generation of its own
 *   time, as always), and while on msdr_chain_get_fir_history returns 2 * hist_len int16_t, interleaved, oldest first: `capacity` counts
 *   int16_t, *hist_len stays in samples.
 *   Chains in phase-accumulator mode only (msdr_chain_set_decimation's scope rule), Q15 and F32; dir must be 0 or 1 when turning on; and the
 *   switch, on or off or to the other direction, is accepted only while the FIR history is clear -- before the first msdr_chain_process, or
 *   directly after msdr_chain_reset / msdr_chain_init_fir, the rule of the first msdr_chain_set_nco_channels call -- so no history is ever
 *   converted.  A repeat call with the values in force does nothing and is always accepted.  Anything else, a NULL chain included, is
 *   MSDR_STATUS_ARGUMENT_ERROR, nothing changed.  The setting survives everything the decimation factor survives and combines, in either
 *   order, with msdr_chain_set_decimation, set_meter, set_iq_out (I/Q-only calls included), set_input_rows, the tap / NCO / mode / node /
 *   cascade setters, MSDR_CHAIN_OUT_I16, and on Q15 chains MSDR_CHAIN_SYNCAM_PLL at D = 1 and msdr_chain_set_anr.
 *   The meter: msdr_meter_dbfs's 0 dBFS is a full-scale REAL carrier (I^2 + Q^2 = A^2 / 4).  A complex exponential of the same amplitude at
 *   the tuned frequency has no image to lose in the channel filter (I^2 + Q^2 = A^2) and reads +6.02 dB.
 *   Reporting: msdr_chain_get_info().kernel keeps its names (the complex-input twins, chain_q15pcn_cx_kernel ..., run under them); on fp32
 *   chains flavour carries MSDR_FLAVOUR_COMPLEX_IN exactly while the mode is on.  Graphs stay refused, as on every chain in this mode.
 * msdr_chain_get_complex_input: the switch and the direction in force (0, 0 on a chain that never set them); either output may be NULL.
 * msdr_chain_set_gain / msdr_chain_set_gain_channels / msdr_chain_set_agc: gain control per RECEIVER.  The reference levels the signal in front
 *   of the FIR with amp_adc.gain(AGC_val) and AGC() (Minimal-SDR.ino:385, 445-515); msdr_frontend has that pair once per input row, and with
 *   one antenna row feeding a bank that is one gain for stations 60 dB apart.  Behind a Q15 channel filter the 15 dropped bits cannot be
 *   amplified back, so the bank's amplifier works on the FIR accumulators.  Every receiver holds AGC_val (float) and
 *   multiplier = AudioAmplifier::gain's (mixer.h:75-79: clamp to +-32767, (int32)(n * 65536.0f)).  While gain is on, the pair I, Q of every
 *   output -- the two FIR outputs the demodulator receives -- is
 *     Q15   ssat16((int64(acc) * multiplier) >> 31), arithmetic shift, acc the wrapping 32-bit accumulator of arm_fir_fast_q15:
 *           applyGain's (mult * s) >> 16 moved in front of the >> 15.  multiplier 65536 is ssat16(acc >> 15) exactly, 0 gives zeros.
 *     F32   acc * gain, one rounded fp32 multiply, gain = AGC_val after the same clamp.
 *   The demodulator (every mode), the hand-over to the Q15 PLL at D = 1 and msdr_chain_set_iq_out receive the GAINED pair (USB / LSB audio
 *   stays I +- Q of the stored pairs); msdr_chain_set_meter keeps measuring the UNGAINED pair: an S-meter does not move with the AGC.
 *   AGC(): behind every successful msdr_chain_process (I/Q-only calls included; a call that returns an error steps nothing), on the chain's
 *   stream and without a host synchronisation, every receiver whose AGC is on takes ONE step of Minimal-SDR.ino:479-513 with
 *     absmax = min(32767, max over the call's n_out outputs of max(|I|, |Q|)) of the gained pair
 *   (F32: (int32) fminf(peak / in_scale, 32767.0f), the division IEEE-rounded): the ring of 25 with the dropped 26th store, the integer mean,
 *   f = 16000 / mean (mean 0: +inf), the five rules and AGC_Max, the multiplier recomputed when a rule fires.  The new multiplier holds from
 *   the NEXT call: inside a call the gain is constant.  At 128 outputs per call this is the reference's cadence; longer calls step more
 *   slowly (one step per call, whatever its length).  absmax is recorded for every receiver, held or stepped.
 *   msdr_chain_set_gain(on): off (default) runs the kernels of a chain without gain and leaves the state alone; on runs the gain twins.
 *   msdr_chain_set_gain_channels: msdr_frontend_gain per receiver -- AGC_val = gain[k] (host array, read during the call) and its multiplier,
 *   behind every call enqueued so far, in force from the next call; the ring is untouched.  msdr_chain_set_agc: agc_on is a host array of
 *   `channels` values or NULL (agc_on_all for every receiver), 0 = held, 1 = stepped.  The state of a receiver is made by the first of these
 *   three calls -- AGC_val 1.0, multiplier 65536, ring zero, agc_idx 25, AGC off, so that msdr_chain_set_gain(on) alone changes no bit of
 *   any output -- and lives until msdr_chain_destroy.
 *   msdr_chain_get_agc synchronises and returns a receiver's record: [0] multiplier (F32: the bits of the clamped gain), [1] agc_idx,
 *   [2] AGC_val (float bits), [3] absmax of the last call, [4] steps taken, [5..6] zero, [7..31] agc_buffer[0..24].
 *   Chains in phase-accumulator mode only (msdr_chain_set_decimation's scope rule), Q15 and F32, every D, real and complex input.  A NULL
 *   chain, a chain in another mode, a range past `channels`, a NULL gain with count > 0, a gain that is not finite and an agc_on value other
 *   than 0 or 1 are MSDR_STATUS_ARGUMENT_ERROR, nothing changed.  Everything survives what the decimation factor survives and combines, in
 *   either order, with msdr_chain_set_decimation, set_meter, set_iq_out, set_complex_input, set_input_rows and MSDR_CHAIN_OUT_I16, and on
 *   Q15 chains with MSDR_CHAIN_SYNCAM_PLL at D = 1 and msdr_chain_set_anr.
 *   Reporting: msdr_chain_get_info().kernel keeps its names (the gain twins, chain_q15pcn_gain_kernel ..., run under them); on fp32 chains
 *   flavour carries MSDR_FLAVOUR_GAIN exactly while gain is on.  Graphs stay refused, as on every chain in this mode.
 * msdr_chain_set_bank_post: synchronous AM and the LMS filter for the bank.  SYNCAM is one of the reference's four modes and the LMS notch its
 *   only interference filter (Minimal-SDR.ino:631-688, 702-770); on = 1 means: once this chain is in phase-accumulator mode
 *   (msdr_chain_set_nco_channels), its PLL demodulator and LMS filter run behind the per-receiver kernel on the PAIR HAND-OVER, at fs / D,
 *   and never through an auxiliary chain.  The hand-over is the pair I_c[m], Q_c[m] of msdr_chain_set_iq_out's definition: a call that
 *   needs it launches the I/Q twin of the kernel it would have launched, which stores into the caller's d_iq where one is set (no second
 *   store) and else into a buffer of the chain's own, [channels][n_out rounded up to 8] pairs, grown on demand.  bank_pll_q15_kernel /
 *   bank_pll_f32_kernel (one lane = one channel) then write the PLL's audio over the rows of the channels whose mode is SYNCAM -- the
 *   statement sequence of msdr_syncam_q15 / the fp32 chain's PLL, state records shared with them -- and leave every other row alone.
 *   With gain on the PLL receives the GAINED pair, the rule of the D = 1 hand-over.
 *   Accepted on Q15 and F32 chains whose mixer is the NCO (not MSDR_MIXER_FS4), only while the FIR history is clear -- the rule of the first
 *   msdr_chain_set_nco_channels call -- and it holds for the rest of the chain's life: a repeat call with 1 does nothing, 0 after 1 is
 *   MSDR_STATUS_ARGUMENT_ERROR, nothing changed, and so is a NULL chain.  It changes nothing until the chain is in phase-accumulator mode:
 *   until then every call behaves as without it, refusals included.  With the switch on:
 *     F32   msdr_chain_set_nco_channels is accepted on a chain created with MSDR_CHAIN_SYNCAM_PLL and / or with LMS channels on; the
 *           auxiliary chain and its buffers are dropped, the per-channel PLL and LMS state records are kept.  In the mode, msdr_chain_set_anr
 *           with channels on, set_mode to and from SYNCAM, set_input_rows, set_meter, set_iq_out (I/Q-only calls included),
 *           set_complex_input, set_gain* / set_agc, set_decimation, set_biquad_coeffs_channels, set_taps_channels_f32 and
 *           MSDR_CHAIN_OUT_I16 are accepted and combine in either order, as on Q15 chains.  Order per call: kernel (demodulator + pair
 *           store) -> PLL on SYNCAM channels -> LMS on its channels -> CMSIS-order cascade (shared or per-channel rows) -> int16 conversion.
 *     Q15   msdr_chain_set_decimation is accepted on a chain created with MSDR_CHAIN_SYNCAM_PLL and with LMS channels on, and
 *           msdr_chain_set_anr while D > 1.  Order: kernel -> PLL -> LMS (anr_kernel) -> biquad nodes, all on n / D samples; a chain with
 *           nodes still needs n / D even.  At D = 1 the pairs are bit for bit what the I / Q hand-over of a chain without the switch
 *           carries, so no output changes by a bit.
 *   The PLL pass runs in every audio call of such a chain that has a PLL while a channel is on SYNCAM, at every D; I/Q-only calls leave the
 *   PLL and LMS states untouched; msdr_chain_reset clears both, msdr_chain_init_fir keeps them.  Graphs stay refused, as on every chain in
 *   this mode.  Reporting: on fp32 chains flavour carries MSDR_FLAVOUR_BANK_POST exactly when the call ran the bank's PLL or LMS pass.
 * msdr_chain_set_spectrum: a panadapter line per receiver.  While on, every successful msdr_chain_process keeps the most recent 64 pairs of
 *   each receiver -- the pairs of msdr_chain_set_iq_out's definition, gained when gain is on, at fs / D -- in a tail [channels][64] of the
 *   chain's own: the tail becomes the last 64 of (old tail ++ this call's n_out pairs) before anything is drawn, so a call with n_out >= 64
 *   transforms its own last 64 outputs and a bank at block cadence with D = 8 the last four ticks.  On the calls showSpectrum's cadence
 *   picks (UI.cpp:534-535: `if (--counter > 0) return; counter = every;`, the counter starting at 0, so the first call draws; every == 0
 *   means 25, the reference's value, every == 1 every call) the 64-point transform of every tail (msdr_cfft64_q15 / msdr_cfft64_f32,
 *   their arithmetic and layouts) overwrites all `channels` rows of d_bins [channels][64] pairs {re, im} and / or d_power [channels][64]
 *   (uint32_t for Q15, float for F32), device memory of the caller's, 16-byte aligned; a call that does not draw writes neither.  One NULL:
 *   only the other is written; both NULL: off (the default).  The pairs come from the caller's d_iq where one is set and else from the
 *   chain's own per-call pair buffer (msdr_chain_set_bank_post's), for which the main launch picks its I/Q twin; I/Q-only calls feed the
 *   window like any other.  One small launch per call while on (bank_cfft64_q15_kernel / bank_cfft64_f32_kernel: the tail moves in place,
 *   the drawing calls transform), stream-ordered, never synchronising.  A msdr_chain_process that returns an error (MSDR_STATUS_LENGTH_ERROR
 *   included) moves neither tail nor counter nor the count of spectra drawn and writes nothing.  Off -> on clears tail, counter and count; a
 *   call while on with other pointers or another `every` keeps all three (the new `every` loads at the next reload); msdr_chain_reset clears
 *   tail and counter, msdr_chain_init_fir keeps both.  Scope: chains in phase-accumulator mode (msdr_chain_set_decimation's rule), Q15 and
 *   F32; a NULL chain, a chain not in the mode, a misaligned buffer and every > 2^31 - 1 (the counter is showSpectrum's int) are
 *   MSDR_STATUS_ARGUMENT_ERROR, nothing changed.  The setting
 *   survives everything the meter pointer survives and combines, in either order, with set_iq_out, set_meter, set_decimation,
 *   set_input_rows, set_complex_input, set_gain / AGC, set_bank_post and the tap, NCO, node, cascade and mode setters;
 *   msdr_chain_set_block_kernel[_q15] stays accepted and such calls run the unfused launches; graphs stay refused, as on every chain in this
 *   mode.  Reporting: msdr_chain_get_info().kernel keeps its names; on fp32 chains flavour carries MSDR_FLAVOUR_SPECTRUM exactly while on.
 *   Orientation: the transform takes the pair as z = I + jQ, and on a real-input chain that z turns clockwise for a carrier ABOVE the tuned
 *   frequency: such a carrier falls LEFT of column 32 (46.875 Hz per column at fs / D = 3000).
 * msdr_chain_get_spectrum: the pointers and `every` in force (0 reads back as 25) and the spectra drawn since the switch went on -- a host
 *   count, nothing synchronises; every output may be NULL.
 * msdr_chain_get_bank_post: the switch (0 on a chain that never set it).
 * msdr_chain_get_pll_state: synchronises and returns fil_out, omega2, phzerror of one channel's loop, msdr_syncam_get_state's shape, on Q15
 *   and F32 chains created with MSDR_CHAIN_SYNCAM_PLL, with or without the switch; a chain without a PLL is MSDR_STATUS_ARGUMENT_ERROR.
 * msdr_syncam_constants_rate (host only): omega_min, omega_max, g1, g2 as msdr_syncam_constants evaluates them (Minimal-SDR.ino:636-641) with
 *   SAMPLE_RATE replaced by sample_rate, under the same arithmetic conversions: bit-equal to msdr_syncam_constants at 24000.  With the
 *   reference's constants a loop that runs at fs / D has its capture range and bandwidth shrunk by D (at D = 8: +-500 Hz, 50 Hz).
 * msdr_chain_set_pll_rate: the rate the bank's PLL constants are evaluated for; 0 (the default) = the reference's constants, otherwise a
 *   finite value > 0 (anything else: MSDR_STATUS_ARGUMENT_ERROR, nothing changed).  Accepted only with msdr_chain_set_bank_post on.  The
 *   constants are an operand of the PLL kernel: stream-ordered, the state is kept, in force from the next call.  Nothing sets it
 *   automatically: the caller passes fs / D, as the caller designs the biquads for fs / D.  msdr_chain_get_pll_rate: the value in force.
 * msdr_chain_post_kernel: a static string, the PLL kernel of the last audio call -- "bank_pll_q15_kernel" / "bank_pll_f32_kernel",
 *   "syncam_pll_kernel" (Q15 without the switch), "post_pll_f32_kernel" (fp32 through the auxiliary chain) -- or "" when none ran.
 * msdr_nco_step (host only): llround(f_hz / fs_hz * 2^32) mod 2^32; a negative frequency wraps (-6000 at 24000: 0xC0000000).
 * msdr_nco_table (host only): T[i] = (int16) lround(32767 sin(2 pi i / 1024)), i = 0 .. 1024, T[1024] = 0.
 * msdr_nco_q15 (host only; what the kernels compute): for each uint32 phase, i = phase >> 22, f = (phase >> 6) & 0xFFFF,
 *   sin = T[i] + (((T[i + 1] - T[i]) * f + 32768) >> 16) (arithmetic shift), cos = sin of phase + 0x40000000 (wrapping); within 1.154 LSB
 *   of 32767 sin, range -32767 .. 32767.  Either output may be NULL. */
uint32_t msdr_nco_step(double f_hz, double fs_hz);
void msdr_nco_table(int16_t table[1025]);
void msdr_nco_q15(const uint32_t *phase, size_t count, int16_t *sin_out, int16_t *cos_out);
int msdr_chain_set_nco_channels(msdr_chain *chain, uint32_t first_channel, uint32_t count,
                                const uint32_t *step, const uint32_t *phase);
int msdr_chain_get_nco(msdr_chain *chain, uint32_t channel, uint32_t *step, uint32_t *phase);
enum { MSDR_MAX_DECIMATION_Q15 = 60, MSDR_MAX_DECIMATION_F32 = 59 };
int msdr_chain_set_decimation(msdr_chain *chain, uint32_t D);   /* 1 = off (default) */
int msdr_chain_get_decimation(msdr_chain *chain, uint32_t *D);
int msdr_chain_set_prefilter(msdr_chain *chain, uint32_t D1, uint32_t num_taps, const int16_t *taps);     /* Q15; D1 == 1 or num_taps == 0: off (default) */
int msdr_chain_set_prefilter_f32(msdr_chain *chain, uint32_t D1, uint32_t num_taps, const float *taps);   /* F32 */
int msdr_chain_get_prefilter(msdr_chain *chain, uint32_t *D1, uint32_t *num_taps);                         /* either may be NULL */
int msdr_chain_set_meter(msdr_chain *chain, void *d_meter);   /* NULL = off (default) */
int msdr_chain_get_meter(msdr_chain *chain, void **d_meter);
double msdr_meter_dbfs(double sum_sq, uint64_t n_out, double full_scale);
int msdr_chain_set_iq_out(msdr_chain *chain, void *d_iq, uint64_t pitch);   /* NULL = off (default) */
int msdr_chain_get_iq_out(msdr_chain *chain, void **d_iq, uint64_t *pitch); /* either may be NULL */
int msdr_chain_set_complex_input(msdr_chain *chain, int on, int dir);   /* off (default): real IF */
int msdr_chain_get_complex_input(msdr_chain *chain, int *on, int *dir); /* either may be NULL */
int msdr_chain_set_gain(msdr_chain *chain, int on);                       /* off (default): the kernels of a chain without gain */
int msdr_chain_get_gain(msdr_chain *chain, int *on);
int msdr_chain_set_gain_channels(msdr_chain *chain, uint32_t first_channel, uint32_t count, const float *gain);
int msdr_chain_set_agc(msdr_chain *chain, const int32_t *agc_on, int32_t agc_on_all);   /* msdr_chain_set_anr's argument shape */
#define MSDR_AGC_STATE_WORDS 32u
int msdr_chain_get_agc(msdr_chain *chain, uint32_t channel, int32_t state[MSDR_AGC_STATE_WORDS]);
int msdr_chain_set_bank_post(msdr_chain *chain, int on);                  /* off (default): PLL / LMS as on a chain without it */
int msdr_chain_get_bank_post(msdr_chain *chain, int *on);
int msdr_chain_get_pll_state(msdr_chain *chain, uint32_t channel, float state[3]);
int msdr_chain_set_spectrum(msdr_chain *chain, void *d_bins, void *d_power, uint32_t every);   /* both NULL = off (default) */
int msdr_chain_get_spectrum(msdr_chain *chain, void **d_bins, void **d_power, uint32_t *every, uint64_t *drawn);
void msdr_syncam_constants_rate(double sample_rate, float c[4]);
int msdr_chain_set_pll_rate(msdr_chain *chain, double sample_rate);       /* 0 (default): the reference's constants */
int msdr_chain_get_pll_rate(msdr_chain *chain, double *sample_rate);
const char *msdr_chain_post_kernel(msdr_chain *chain);
int msdr_chain_set_taps(msdr_chain *chain, uint32_t tapset, const void *coeffs_i, const void *coeffs_q);
int msdr_chain_set_taps_channels(msdr_chain *chain, uint32_t first_channel, uint32_t count,
                                 const q15_t *coeffs_i, const q15_t *coeffs_q);
int msdr_chain_set_taps_channels_f32(msdr_chain *chain, uint32_t first_channel, uint32_t count,
                                     const float32_t *coeffs_i, const float32_t *coeffs_q);
int msdr_chain_set_node_coefficients(msdr_chain *chain, uint32_t node, uint32_t stage, const int32_t coef[5]);
int msdr_chain_set_node_coefficients_channels(msdr_chain *chain, uint32_t node, uint32_t first_channel,
                                              uint32_t count, uint32_t stage, const int32_t *coef);
int msdr_chain_set_biquad_coeffs(msdr_chain *chain, const float32_t *biquad_coeffs);
int msdr_chain_set_biquad_coeffs_channels(msdr_chain *chain, uint32_t first_channel, uint32_t count,
                                          const float32_t *biquad_coeffs);
int msdr_chain_set_osc(msdr_chain *chain, const void *osc_i, const void *osc_q);
int msdr_chain_set_osc_channels(msdr_chain *chain, uint32_t first_channel, uint32_t count,
                                const void *osc_i, const void *osc_q);
int msdr_chain_set_block_kernel(msdr_chain *chain, int on);   /* F32 chains; default off */
int msdr_chain_set_block_kernel_q15(msdr_chain *chain, int on);   /* Q15 chains; default off */
int msdr_chain_set_input_rows(msdr_chain *chain, uint32_t n_inputs, const uint32_t *input_row);
/* ANR_on per channel (host array of `channels` values, or NULL: anr_on_all for every channel); the LMS filter then runs between
 * the demodulator and the biquad nodes / cascade (Minimal-SDR.ino:702-770).  Its state is created on first use and cleared by
 * msdr_chain_reset() (not by msdr_chain_init_fir()).  Q15 chains: as the reference, on the int16 audio.  F32 chains (an
 * extension): the same statements on the fp32 audio, in the reference's sample units (x 32768 in, / 32768 out), nothing truncated;
 * such channels (and SYNCAM channels under MSDR_CHAIN_SYNCAM_PLL) are demodulated by an auxiliary pass behind the main kernel --
 * one lane per channel, serial in time like the reference -- and their cascade restarts when a retune changes the set. */
int msdr_chain_set_anr(msdr_chain *chain, const int32_t *anr_on, int32_t anr_on_all);
int msdr_chain_destroy(msdr_chain *chain);
/* introspection for benchmarks/tests: name of the main kernel variant and launch geometry of the last call */
typedef struct {
    char     kernel[64];
    uint32_t grid, block, lds_bytes;
    uint32_t time_segments, warmup, tile;
    uint32_t taps_padded;
    uint32_t mfma_ksteps;            /* matrix-core kernel: k-steps (3 MFMAs each) issued per 1024-output wave tile, else 0; a run's first and last
                                        16-sample step merged into one 2:4-sparse step (chain_mfw_kernel) count as one */
    uint32_t env_scan;               /* chain_mfw_kernel, envelope tables with a 1- or 2-section cascade as matrix products: how the row states
                                      * were scanned in the last call.  0 = that flavour did not run; 1 = every section (2 x 2 or 4 x 4 matrices);
                                      * 2 / 3 = section 0 / 1 is row-local (its transition over a 32-sample row is nothing in fp32: it takes no
                                      * part in the scan), the other section scans alone with 2 x 2 matrices */
    uint32_t flavour;                /* F32 chains: MSDR_FLAVOUR_* bits of the host decisions that selected device code for the last call, set where
                                      * each launch is made (0 for Q15 chains).  `kernel` names a kernel family; this says which of its paths ran */
} msdr_chain_info;
#define MSDR_FLAVOUR_SSB_UNITS    0x0001u   /* a launch over LSB / USB / CW units (one accumulator, cascade numerator in the taps) */
#define MSDR_FLAVOUR_ENV_UNITS    0x0002u   /* a launch over envelope units (two accumulators) */
#define MSDR_FLAVOUR_SSB_FOLD     0x0004u   /* the SSB units' cascade ran as matrix products (folded into the tap tables) */
#define MSDR_FLAVOUR_ENV_FOLD     0x0008u   /* the envelope units' cascade ran as matrix products (env_scan says how its row states were scanned) */
#define MSDR_FLAVOUR_FULL_RATE    0x0010u   /* full-rate layout: a 128-periodic oscillator table, the mixer products staged as two streams */
#define MSDR_FLAVOUR_COMPACT      0x0020u   /* full-rate layout with compact (shifted-copy) tap fragments */
#define MSDR_FLAVOUR_SHARED_IQ    0x0040u   /* full-rate envelope units whose two accumulators read one set of fragments (coeffs_i == coeffs_q in ANY tap set of the chain) */
#define MSDR_FLAVOUR_AMTR         0x0080u   /* the envelope units ran on the taps-in-registers kernel (chain_amtr_kernel) */
#define MSDR_FLAVOUR_BLOCK        0x0100u   /* block cadence: chain_mfb_kernel, channel-batched tiles; with MSDR_FLAVOUR_TAPS_PC: chain_f32pcb_kernel */
#define MSDR_FLAVOUR_VALU_FOLD    0x0200u   /* chain_fold_kernel<P>; P in bits 12..14 */
#define MSDR_FLAVOUR_SEQ_CASCADE  0x0400u   /* the cascade ran behind the main kernel in CMSIS order */
#define MSDR_FLAVOUR_SEGMENTED    0x0800u   /* a launch split the call into more than one time segment */
#define MSDR_FLAVOUR_FOLD_PERIOD_SHIFT 12
#define MSDR_FLAVOUR_FOLD_PERIOD(f) (((f) >> MSDR_FLAVOUR_FOLD_PERIOD_SHIFT) & 7u)
/* One more bit of `flavour`, an enumerator beside the macros above (their list is mirrored one for one, and counted, by the Python binding's ABI test):
 * chain_f32pc_kernel ran -- per-channel FIR coefficients, msdr_chain_set_taps_channels_f32. */
enum { MSDR_FLAVOUR_TAPS_PC = 0x8000u };
/* And another: the cascade behind the main kernel ran with per-channel coefficients -- biquad_df1_seq_pc_kernel, msdr_chain_set_biquad_coeffs_channels
 * (always beside MSDR_FLAVOUR_SEQ_CASCADE). */
enum { MSDR_FLAVOUR_CASCADE_PC = 0x10000u };
/* And another: the demodulator kernel mixed every channel with its own oscillator row -- chain_f32pco_kernel, msdr_chain_set_osc_channels
 * (always beside MSDR_FLAVOUR_TAPS_PC). */
enum { MSDR_FLAVOUR_OSC_PC = 0x20000u };
/* And another: the demodulator kernel read its IF samples through an input map -- msdr_chain_set_input_rows with n_inputs > 0, d_if
 * [n_inputs][n_samples] (always beside MSDR_FLAVOUR_TAPS_PC). */
enum { MSDR_FLAVOUR_SHARED_IF = 0x40000u };
/* And another: the demodulator kernel computed every channel's oscillator from its phase accumulator -- chain_f32pcn_kernel,
 * msdr_chain_set_nco_channels (always beside MSDR_FLAVOUR_TAPS_PC). */
enum { MSDR_FLAVOUR_NCO_PC = 0x80000u };
/* And another: the demodulator kernel decimated -- chain_f32pcnd_kernel, msdr_chain_set_decimation with D > 1 (always beside
 * MSDR_FLAVOUR_NCO_PC and MSDR_FLAVOUR_TAPS_PC). */
enum { MSDR_FLAVOUR_DECIMATED = 0x100000u };
/* And another: the demodulator kernel measured the channels' power -- the metered flavour of a per-receiver kernel, msdr_chain_set_meter with
 * a buffer (always beside MSDR_FLAVOUR_TAPS_PC). */
enum { MSDR_FLAVOUR_METER = 0x200000u };
/* And another: the demodulator kernel stored the pair behind the channel filter -- the IQ flavour of a phase-accumulator kernel,
 * msdr_chain_set_iq_out with a buffer (always beside MSDR_FLAVOUR_NCO_PC). */
enum { MSDR_FLAVOUR_IQ_OUT = 0x400000u };
/* And another: the demodulator kernel mixed rows of complex pairs -- the complex-input twin of a phase-accumulator kernel,
 * msdr_chain_set_complex_input on (always beside MSDR_FLAVOUR_NCO_PC). */
enum { MSDR_FLAVOUR_COMPLEX_IN = 0x800000u };
/* And another: the demodulator kernel multiplied the pair by every receiver's gain -- the gain twin of a phase-accumulator kernel,
 * msdr_chain_set_gain on (always beside MSDR_FLAVOUR_NCO_PC). */
enum { MSDR_FLAVOUR_GAIN = 0x1000000u };
/* the call ran the bank's PLL or LMS pass behind the per-receiver kernel (msdr_chain_set_bank_post; always beside MSDR_FLAVOUR_NCO_PC). */
enum { MSDR_FLAVOUR_BANK_POST = 0x2000000u };
/* the per-receiver spectrum display is on (msdr_chain_set_spectrum; always beside MSDR_FLAVOUR_NCO_PC). */
enum { MSDR_FLAVOUR_SPECTRUM = 0x4000000u };
/* the demodulator kernel ran a chain-wide prefilter in front of the channel pair -- chain_f32pcn2_kernel, msdr_chain_set_prefilter_f32
 * (always beside MSDR_FLAVOUR_DECIMATED and MSDR_FLAVOUR_NCO_PC). */
enum { MSDR_FLAVOUR_PREFILTER = 0x8000000u };
int msdr_chain_get_info(msdr_chain *chain, msdr_chain_info *info);
/* The wave-stream kernels read the run geometry of a tap table (which chunks of the window each accumulator walks, which runs merge their first
 * and last step) from the table's header -- or, for the geometries the library instantiates, have it as compile-time constants: the same
 * products in the same order, bit-identical results, fewer instructions.  The host compares every table header it builds (create and every
 * live update) with the instantiated geometries and launches such a kernel only where every table the launch can meet has that geometry.
 * *id = what the last call ran: 0 = every launch read the headers (also before the first call, on every other kernel path, and on a chain
 * created with MSDR_MFW_GEOM=0 in the environment); 1 = envelope tables behind the exact Fs/4 mixer, 256 taps, two-section cascade with a
 * row-local section; 2 = the same with 512 taps.  msdr_chain_info is as it was: `kernel`, `env_scan` and `flavour` do not tell the two apart. */
int msdr_chain_get_geometry(msdr_chain *chain, uint32_t *id);
/* Behind the exact Fs/4 mixer at an even rotation, with one low-pass for I and Q, the envelope table's Q block is its I block moved one
 * column: the wave-stream kernels then run Q on the I accumulator's tap fragments over the odd samples (one fragment read feeds both
 * accumulators) and realign the result, which arrives one sample late, behind the FIR burst.  The table builder confirms the relation on the
 * numbers of every table it builds (create and every live update); any other table -- odd rotation, hI != hQ, ... -- keeps its own fragments.
 * *on = 1 where the last call's envelope launch on the wave-stream kernels met only such tables and so ran that way, else 0 (also before
 * the first call, on every other kernel path, and on a chain created with MSDR_MFW_IQ=0 in the environment).  Same products, some sums in
 * another order: the results differ from the unshared path's in the last bits.  The kernels with a constant run geometry
 * (msdr_chain_get_geometry 1 / 2) exist in this form only: a 256- or 512-tap Fs/4 envelope chain with hI != hQ, or one created under
 * MSDR_MFW_IQ=0, runs the header-reading kernel instead (geometry 0), about 2 % slower per call than the constant-geometry kernel it had
 * before this form existed (profiles/mfw_geom/README.md). */
int msdr_chain_get_iq_shared(msdr_chain *chain, uint32_t *on);
/* Which kernel ran the serial recurrences (introspection for tests: tests/q15_ladder_cases.py is the table of every branch below, and
 * tests/test_gpu_q15_ladders.py holds each of them to the oracle bit for bit).  Each getter returns a static string -- the kernel's name
 * with its template arguments, set in the branch that made the launch and handed to the launch's error check as well -- "" before the
 * first call, NULL for a NULL instance.  All of these kernels are bit-exact, so the name is the only way to tell them apart.  The ladders,
 * first match wins; "aligned" = the data pointer is a multiple of 16 bytes; "one stage" = set_coefficients never named a stage above 0:
 *   msdr_biquad_q15_last_kernel (the last msdr_biquad_q15_update):
 *     per-channel records (set_coefficients_channels was called) ........................... "biquad_teensy_pc_kernel<1>"
 *     one stage, blockSize % 128 == 0, aligned, channels % P == 0 ........................... "biquad_teensy_pipe4_kernel<1,P>"
 *       P = channels per workgroup, fixed at create time: MSDR_BIQUAD_PIPE_CH = 16 / 32 / 64 if set, else 64 from 16 384 channels,
 *       32 from 8192, 16 below
 *     otherwise .......................................................................... "biquad_teensy_kernel<1>"
 *   msdr_chain_node_kernel (the biquad nodes of the last msdr_chain_process; "" for no nodes and for fp32 chains):
 *     msdr_chain_set_block_kernel_q15 on and the block kernel took the call, any nodes ....... "chain_q15pcb_kernel"
 *     one node ........................................................................... what msdr_biquad_q15_update reports
 *     two nodes, uniform records, one stage each, n == 128 on the block path (info().kernel = chain_q15mb_kernel), no PLL / LMS
 *       channel, MSDR_Q15_NO_FUSE unset at create time, one tile per wave on three or more waves (the host's choice wherever the
 *       tiles leave it free: every small batch) ........................................... "chain_q15mb_kernel"
 *     two nodes, per-channel records in either ........................................... "biquad_teensy_pc_kernel<2>"
 *     one stage each, n == 128, aligned, and MSDR_BIQUAD_BLK (create time) = 1, or unset and ceil(channels / 16) <= the device's
 *       CU count; MSDR_BIQUAD_BLK=0: never ................................................. "biquad_teensy_blk_kernel"
 *     one stage each, n % 128 == 0, aligned, channels % P == 0 (P of node 0, as above) ...... "biquad_teensy_pipe4_kernel<2,P>"
 *     n % 128 == 0, aligned, channels % 64 == 0 (so: a node with two or more stages) ........ "biquad_teensy_pipe_kernel"
 *     otherwise .......................................................................... "biquad_teensy_kernel<2>"
 *     Under msdr_chain_graph_create it is what the recording enqueued; replays do not change it.
 *   msdr_frontend_last_kernel (the last msdr_frontend_update):
 *     stages == MSDR_FE_ALL, d_adc and d_out aligned, channels % P == 0 ...................... "frontend_pipe4_kernel<P>"
 *       P fixed at create time: MSDR_FRONTEND_PIPE_CH = 16 / 32 / 64 if set, else by the same channel counts as above
 *     otherwise .......................................................................... "frontend_kernel" */
const char *msdr_chain_node_kernel(msdr_chain *chain);
const char *msdr_biquad_q15_last_kernel(msdr_biquad_q15 *S);
const char *msdr_frontend_last_kernel(msdr_frontend *fe);
/* Introspection for tests: what a chain carries from call to call.  get_fir_history: *hist_len = the raw int16 samples the chain keeps per
 * channel (a property of the kernels it runs), and, where hist != NULL (capacity >= that many), channel's samples, oldest first.
 * get_cmsis_state (F32 chains whose cascade runs behind the kernel: MSDR_FLAVOUR_SEQ_CASCADE): 4 * num_biquad_stages floats, as
 * msdr_biquad_df1_f32_get_cmsis_state.  Both wait for the stream. */
int msdr_chain_get_fir_history(msdr_chain *chain, uint32_t channel, int16_t *hist, uint32_t capacity, uint32_t *hist_len);
int msdr_chain_get_cmsis_state(msdr_chain *chain, uint32_t channel, float32_t *pState);
/* Measurement aid (bench.py): when enabled every msdr_chain_process() brackets its MAIN kernel with
 * HIP events on the context's stream; get_kernel_time synchronises and returns the accumulated
 * device time in ms and the number of launches timed (reset != 0 clears the accumulators). */
int msdr_chain_enable_timing(msdr_chain *chain, int on);
int msdr_chain_get_kernel_time(msdr_chain *chain, double *total_ms, uint64_t *launches, int reset);


/* ---- block cadence: `ticks` consecutive calls as ONE HIP graph ------------------------------------------------------------------
 * The reference runs one AUDIO_BLOCK_SAMPLES = 128 block per call (Minimal-SDR.ino:518-530, FIR calls :574-575); at that size a call
 * is a few microseconds of GPU work and the host's launch cost is of the same order.  msdr_chain_graph_create records the launches
 * of `ticks` consecutive msdr_chain_process(chain, d_if[k], d_audio[k], n_samples) calls, k = 0 .. ticks - 1, into a HIP graph on the
 * context's stream; msdr_chain_graph_launch enqueues all of them at once (the caller refills d_if[] and collects d_audio[] between
 * launches, ordered on the same stream).  The chain's state advances exactly as under the direct calls: direct calls, replays and
 * live updates may follow one another -- a replay is REFUSED (MSDR_STATUS_ARGUMENT_ERROR, nothing enqueued) once a live update, a reset
 * or an odd number of direct calls has moved what the recorded launches point at; make the graph again then.
 *   ticks: even, 2 .. 1024 (history and cascade state alternate between two buffers from call to call).
 *   n_samples: a block-cadence length (32, 64, 128, 256 or 512; 16-byte aligned buffers) on a chain whose call is ONE fixed set of
 *   launches: matrix-core tables in use, no PLL / LMS channels behind the kernel, no cascade in CMSIS order behind it, no pending
 *   oscillator change, oscillator period dividing n_samples; anything else returns MSDR_STATUS_ARGUMENT_ERROR with the reason in
 *   msdr_last_error() and leaves the chain untouched. */
typedef struct msdr_chain_graph msdr_chain_graph;
int msdr_chain_graph_create(msdr_chain *chain, uint32_t ticks, const int16_t *const *d_if, void *const *d_audio, uint64_t n_samples, msdr_chain_graph **out);
int msdr_chain_graph_launch(msdr_chain_graph *graph);
int msdr_chain_graph_destroy(msdr_chain_graph *graph);

#ifdef __cplusplus
}
#endif
#endif /* MSDR_H */
