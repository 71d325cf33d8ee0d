// msdr_block.h -- launchers of the kernels that live in translation units of their own, so that a change to a kernel does not rebuild the
// C-ABI layer (msdr_api.hip: host logic and the small stage kernels) and vice versa:
//   msdr_chain_block.hip   the block-cadence kernels (round 5)
//   msdr_chain_stream.hip  the long-call chain kernels: chain_mfw_kernel (all flavours), chain_amtr_kernel, chain_fold_kernel, chain_kernel<Arith>, chain_q15mf_kernel
//   msdr_fir_stage.hip     the arm_fir_f32 stage: fir_f32tq_kernel, fir_f32mf_kernel
//   msdr_q15_elementwise.hip  arm_mult_q15 / arm_add_q15 / arm_sub_q15 / arm_copy_q15 over a block batch: q15_elementwise_kernel
//   msdr_biquad_pc.hip     AudioFilterBiquad with per-channel coefficients: biquad_teensy_pc_kernel
//   msdr_chain_q15pc.hip   the Q15 chain / the arm_fir_fast_q15 stage with per-channel FIR coefficients: chain_q15pc_kernel
//   msdr_chain_f32pc.hip   the fp32 chain / the arm_fir_f32 stage with per-channel FIR coefficients: chain_f32pc_kernel
//   msdr_biquad_df1_pc.hip arm_biquad_cascade_df1_f32 in CMSIS order with per-channel coefficients: biquad_df1_seq_pc_kernel
//   msdr_chain_oscpc.hip   the frames of the two chains above with the oscillator policy "a row of a bank per channel": chain_q15pco_kernel, chain_f32pco_kernel
//   msdr_chain_ncopc.hip   the same frames with the policy "a phase accumulator per channel": chain_q15pcn_kernel, chain_f32pcn_kernel
//   msdr_chain_decpc.hip   that policy under a decimating tile loop: chain_q15pcnd_kernel, chain_f32pcnd_kernel
//   msdr_chain_gncopc.hip, msdr_chain_gdecpc.hip   the gain twins of the phase-accumulator and decimating kernels, real and complex input: chain_*_gain_kernel
//   msdr_chain_meter.hip   the S-meter's second step behind those kernels' metered flavours: meter_reduce_kernel
//                          (the baseband I/Q output, msdr_chain_iq.hiph, is a flavour of the four phase-accumulator kernels in their own units: chain_*_iq_kernel, chain_*_iq_meter_kernel)
//   msdr_chain_f32pcb.hip  the fp32 chain with per-channel settings at block cadence, one launch per call: chain_f32pcb_kernel
//   msdr_chain_q15pcb.hip  the Q15 chain with per-channel settings at block cadence, one launch per call: chain_q15pcb_kernel
//   msdr_bank_post.hip     the PLL demodulator behind the down-converter bank, over the I/Q twins' pairs: bank_pll_q15_kernel, bank_pll_f32_kernel
// Host-side geometry helpers (LDS sizes, table formats) live with the kernels' headers; the launch geometry of the per-receiver chain kernels
// (PcLaunch, pc_geometry, kPcLdsCap) is msdr_pc_geometry.h, plain C++; the eight launchers of those kernels are calls of one body, pc_launch
// (msdr_pc_launch.h).  Every launcher returns the HIP error of its launch.
#pragma once
#include <hip/hip_runtime.h>
#include "msdr_shared.h"
#include "msdr_pc_geometry.h"

namespace msdr {
// chain_mfb_kernel<S, AM> (msdr_chain_mfb.hiph): stages = 0, 1, 2; am = the workgroups' tables are envelope tables.  Returns the HIP error of the launch.
hipError_t launch_chain_mfb(hipStream_t stream, int stages, bool am, unsigned grid, unsigned block, size_t lds_bytes, const ChainParams &p);
// chain_q15mb_kernel<FLAVOUR> (msdr_chain_q15mb.hiph): 0 = LSB / USB channels, 1 = envelope (sqrtf), 2 = envelope (arm_sqrt_q31), 3 = the arm_fir_fast_q15 stage alone
// nodes: the two AudioFilterBiquad nodes as the kernel's second phase (p.bq_state / p.bq_state_out = their records; one tile per wave, >= 3 waves, n = 128)
hipError_t launch_chain_q15mb(hipStream_t stream, int flavour, bool nodes, unsigned grid, unsigned block, size_t lds_bytes, const ChainParams &p);
// ---- msdr_chain_stream.hip ----
hipError_t launch_chain_mfw(hipStream_t stream, int stages, bool am, bool fold, bool full_rate, int rowlocal, unsigned grid, unsigned block, size_t lds_bytes, const ChainParams &p, int geom = 0);
hipError_t launch_chain_amtr(hipStream_t stream, int ns, int stages, unsigned grid, unsigned block, size_t lds_bytes, const ChainParams &p);
hipError_t launch_chain_fold(hipStream_t stream, int period, unsigned grid, size_t lds_bytes, const ChainParams &p);           // period 1, 2, 4
hipError_t launch_chain_generic(hipStream_t stream, bool q15, unsigned grid, size_t lds_bytes, const ChainParams &p);          // chain_kernel<ArithF32 / ArithQ15>
hipError_t launch_chain_q15mf(hipStream_t stream, int flavour, bool full_rate, unsigned grid, unsigned block, size_t lds_bytes, const ChainParams &p);   // flavour 0..3 (3: arm_fir_fast_q15 stage)
// ---- msdr_fir_stage.hip ----
struct TqParams;
hipError_t launch_fir_f32tq(hipStream_t stream, int ns, bool skip1, unsigned grid, size_t lds_bytes, const TqParams &q);
hipError_t launch_fir_f32mf(hipStream_t stream, unsigned grid, unsigned block, size_t lds_bytes, const float *x, float *y, const float *hist, const char *tab,
                            long long n, int channels, int nseg, long long seg_len, int hist_len, int halo, int nsteps, int nw);
// ---- msdr_q15_elementwise.hip ----
constexpr int kQ15Mult = 0, kQ15Add = 1, kQ15Sub = 2, kQ15Copy = 3;
// dst[rows][cols] = op(a row r, b row r); source row r at a + r * a_stride (0: one shared row); b unused for kQ15Copy.  rows * cols < 2^31.
// At most max_grid workgroups of 256 (grid-stride beyond).  *kernel (optional) = the name of the shape launched.
hipError_t launch_q15_elementwise(hipStream_t stream, int op, int max_grid, const short *a, long long a_stride, const short *b, long long b_stride,
                                  short *dst, long long rows, int cols, const char **kernel);
// ---- msdr_biquad_pc.hip ----
// biquad_teensy_pc_kernel<nodes> (msdr_biquad_pc.hiph): nodes = 1 or 2 AudioFilterBiquad nodes in series, in place on data [channels][n] (n even),
// every channel with the coefficients and stage count of its own record in defs0 / defs1 ([channels][32]; defs1 unused for one node)
hipError_t launch_biquad_teensy_pc(hipStream_t stream, int nodes, short *data, int *defs0, int *defs1, int channels, long long n);
// ---- msdr_chain_q15pc.hip ----
// chain_q15pc_kernel<CPW, FIR_ONLY> (msdr_chain_q15pc.hiph).  The launcher chooses the channels per wave (4 up to 128 samples per call, 2 up to
// 256, else 1), the waves per workgroup (4, fewer for very long filters: 64 KB of LDS) and the time segmentation from p.n, p.np, p.channels and
// the number of compute units (pc_geometry; the Q15 launchers never split by msdr_chain_config.time_segments), fills p.nseg / p.seg_len / p.nw
// itself and reports the geometry (PcLaunch).
hipError_t launch_chain_q15pc(hipStream_t stream, bool fir_only, int num_cus, PcParams p, PcLaunch *geo);
// ---- msdr_chain_f32pc.hip ----
// chain_f32pc_kernel<CPW, FIR_ONLY, FS4> (msdr_chain_f32pc.hiph).  The same choices as above (np a multiple of 4; 64 KB of LDS); FS4 is the
// Fs/4 mixer's flavour (p.mixer), one stream and half the products.  time_segments as msdr_chain_config.time_segments: 0 = the launcher's
// choice, 1 = never split, > 1 = that many (as far as the call has tiles).
hipError_t launch_chain_f32pc(hipStream_t stream, bool fir_only, int num_cus, int time_segments, PcfParams p, PcLaunch *geo);
// ---- msdr_chain_oscpc.hip ----
// chain_q15pco_kernel<CPW> / chain_f32pco_kernel<CPW> (msdr_chain_oscpc.hiph): the frames of the two chain kernels above, the oscillator row of
// each channel in LDS.
// p.osc is the bank [channels][osc_len] of pairs, p.mixer MSDR_MIXER_NCO; geometry chosen as above, with the row's LDS counted in.
hipError_t launch_chain_q15pco(hipStream_t stream, int num_cus, PcParams p, PcLaunch *geo);
hipError_t launch_chain_f32pco(hipStream_t stream, int num_cus, int time_segments, PcfParams p, PcLaunch *geo);
// ---- msdr_chain_ncopc.hip ----
// chain_q15pcn_kernel<CPW> / chain_f32pcn_kernel<CPW> (msdr_chain_ncopc.hiph): the same frames with a phase-accumulator oscillator per channel.
// p.osc is the bank [channels] of pairs {base0, step}, p.sin_tab the packed sine table (msdr_nco.h), p.t0 the chain time of the call's first
// sample, p.mixer MSDR_MIXER_NCO; geometry chosen as above, with the table's LDS (once per workgroup) counted in.  chain_pcn_max_taps: the
// longest filter (taps padded as the kernel pads them) one wave with one channel holds beside the table.
int chain_pcn_max_taps(bool f32);
hipError_t launch_chain_q15pcn(hipStream_t stream, int num_cus, PcnParams p, PcLaunch *geo);
hipError_t launch_chain_f32pcn(hipStream_t stream, int num_cus, int time_segments, PcfnParams p, PcLaunch *geo);
// ---- msdr_chain_decpc.hip ----
// chain_q15pcnd_kernel<CPW, AL> / chain_f32pcnd_kernel<CPW, AL> (msdr_chain_decpc.hiph): the phase-accumulator oscillator with decimation p.dec >= 2
// (p.n a multiple of it).  The launcher fills p.nout, p.opl, p.nseg, p.seg_len and p.nw from dec_geometry (msdr_decpc_geometry.h); geo->tile
// is in outputs.  chain_dec_fits: whether factor D fits beside filters of np padded taps at all; chain_dec_max: the setter's largest factor.
bool chain_dec_fits(bool f32, int np, int D);
int chain_dec_max(bool f32);
int chain_dec_max_taps(bool f32, int D);
hipError_t launch_chain_q15pcnd(hipStream_t stream, int num_cus, PcndParams p, PcLaunch *geo);
hipError_t launch_chain_f32pcnd(hipStream_t stream, int num_cus, int time_segments, PcfndParams p, PcLaunch *geo);
// ---- msdr_chain_cxncopc.hip, msdr_chain_cxdecpc.hip ----
// chain_q15pcn_cx_kernel<CPW> ... chain_f32pcnd_cx_kernel<CPW, AL> (msdr_chain_cxpc.hiph): the four families above on rows of pairs {I, Q}
// (msdr_chain_set_complex_input), p.cx_dir freq_conv's direction; validation, geometry and LDS exactly as their real twins'.
hipError_t launch_chain_q15pcn_cx(hipStream_t stream, int num_cus, PcnCxParams p, PcLaunch *geo);
hipError_t launch_chain_f32pcn_cx(hipStream_t stream, int num_cus, int time_segments, PcfnCxParams p, PcLaunch *geo);
hipError_t launch_chain_q15pcnd_cx(hipStream_t stream, int num_cus, PcndCxParams p, PcLaunch *geo);
hipError_t launch_chain_f32pcnd_cx(hipStream_t stream, int num_cus, int time_segments, PcfndCxParams p, PcLaunch *geo);
// ---- msdr_chain_gncopc.hip, msdr_chain_gdecpc.hip ----
// chain_q15pcn_gain_kernel<CPW> ... chain_f32pcnd_cx_gain_kernel<CPW, AL> (msdr_chain_gain.hiph): the gain twins of the eight families above
// (msdr_chain_set_gain), one per family and geometry -- the metered I/Q body with the receiver's gain on the pair; a null p.meter / p.iq skips
// that part.  cx: rows of pairs, p.cx_dir (else not read).  p.agc: the receivers' records [channels][kGainWords]; word 6 of each takes the
// call's peak, which agc_step_kernel (msdr_api.hip) consumes behind the call.  Validation, geometry and LDS exactly as the plain twins'.
hipError_t launch_chain_q15pcn_gain(hipStream_t stream, int num_cus, bool cx, PcnGainParams p, PcLaunch *geo);
hipError_t launch_chain_f32pcn_gain(hipStream_t stream, int num_cus, int time_segments, bool cx, PcfnGainParams p, PcLaunch *geo);
hipError_t launch_chain_q15pcnd_gain(hipStream_t stream, int num_cus, bool cx, PcndGainParams p, PcLaunch *geo);
hipError_t launch_chain_f32pcnd_gain(hipStream_t stream, int num_cus, int time_segments, bool cx, PcfndGainParams p, PcLaunch *geo);
// ---- msdr_chain_pre.hip ----
// chain_q15pcn2_kernel<CPW, AL> / chain_f32pcn2_kernel<CPW, AL> and their *_full twins (msdr_chain_pre.hiph): the decimating kernels with a
// chain-wide prefilter (p.pre_taps, p.pre_np, p.pre_dec) in front of the channel pair, which decimates by p.dec >= 1; p.n a multiple of
// p.pre_dec * p.dec.  The launcher fills p.nout, p.opl, p.pre_chunk, p.nseg, p.seg_len and p.nw from pre_geometry (msdr_prepc_geometry.h) and
// picks the full twin where p.meter, p.iq or p.agc is set; geo->tile is in final outputs.  chain_pre_fits: whether the smallest geometry of
// (np1, D1, np2, D2) -- padded tap counts -- fits 64 KB of LDS; chain_pre_hist_len: the raw history such a chain carries.
bool chain_pre_fits(bool f32, int np1, int D1, int np2, int D2);
int chain_pre_hist_len(int np1, int D1, int np2);
hipError_t launch_chain_q15pcn2(hipStream_t stream, int num_cus, Pcn2Params p, PcLaunch *geo);
hipError_t launch_chain_f32pcn2(hipStream_t stream, int num_cus, int time_segments, Pcfn2Params p, PcLaunch *geo);
// ---- msdr_chain_meter.hip ----
// meter_reduce_kernel<T> (msdr_chain_meter.hiph): d_meter[ch] = the sum of part[ch][0 .. nseg) in that order -- the S-meter of a call that the
// per-receiver kernels above ran in nseg > 1 time segments (their launchers call it; uint64_t sums for Q15, double for F32)
hipError_t launch_meter_reduce(hipStream_t stream, const unsigned long long *part, unsigned long long *d_meter, int channels, int nseg);
hipError_t launch_meter_reduce(hipStream_t stream, const double *part, double *d_meter, int channels, int nseg);
// ---- msdr_biquad_df1_pc.hip ----
// biquad_df1_seq_pc_kernel<S, SEG> (msdr_biquad_df1_pc.hiph): stages = S = 1 .. 4 sections in CMSIS order on data [channels][n] (y may be x), every
// channel with the 5 S coefficients of its own row of tab ([channels][20] floats).  nseg = 1: state_in may be state_out, seg_len / warm / scratch
// unused.  nseg > 1 (SEG): segments of seg_len samples (a multiple of 4), each warmed up over the `warm` samples biquad_seqseg_gather_kernel
// copied to scratch ([channels][nseg][warm]) beforehand; state_out is another buffer than state_in.
constexpr int kSbqTabFloats = 5 * kMaxStages;      // one channel's row of the coefficient table (80 bytes: rows stay 16-byte aligned)
hipError_t launch_biquad_df1_seq_pc(hipStream_t stream, int stages, const float *x, float *y, long long n, int channels, const float *tab,
                                    const float *state_in, float *state_out, int nseg, long long seg_len, int warm, const float *scratch);
// ---- msdr_chain_f32pcb.hip ----
// chain_f32pcb_kernel<CPW, FS4> (msdr_chain_f32pcb.hiph): mixer, FIR, demod, CMSIS-order cascade, fp32 / int16 store and the next history of one
// block-cadence call (p.n = 32 .. 512, a multiple of 8) in one launch.  fs4: the Fs/4 mixer's flavour (p.osc unused).  The geometry follows
// from (p.n, p.np, p.osc_len) alone (f32pcb_geometry: the LDS-fitting step of pc_geometry, one tile, no segments); the launcher fills p.nw.  chain_f32pcb_lds: that geometry without a launch -- false where
// one wave with one channel does not fit 64 KB of LDS (osc_len = 0: Fs/4).
bool chain_f32pcb_lds(int n, int np, int osc_len, PcLaunch *geo);
hipError_t launch_chain_f32pcb(hipStream_t stream, bool fs4, PcbParams p, PcLaunch *geo);
// ---- msdr_chain_q15pcb.hip ----
// chain_q15pcb_kernel<CPW, FS4> (msdr_chain_q15pcb.hiph): mixer, FIR pair, demod, 0 .. 2 AudioFilterBiquad nodes (every channel from its own records),
// int16 store and the next history of one block-cadence call (p.n = 32 .. 512, a multiple of 8) in one launch.  fs4: the Fs/4 mixer's flavour
// (p.osc unused).  The geometry follows from (p.n, p.np, p.osc_len) alone (qpcb_geometry: the LDS-fitting step of pc_geometry, one tile, no
// segments); the launcher fills p.nw.  chain_q15pcb_lds: that geometry without a launch -- false where one wave with one channel does not fit
// 64 KB of LDS (osc_len = 0: Fs/4).
bool chain_q15pcb_lds(int n, int np, int osc_len, PcLaunch *geo);
hipError_t launch_chain_q15pcb(hipStream_t stream, bool fs4, QpcbParams p, PcLaunch *geo);
// ---- msdr_bank_post.hip ----
// bank_pll_q15_kernel / bank_pll_f32_kernel (msdr_bank_post.hiph): the PLL demodulator of msdr_chain_set_bank_post over the pairs the I/Q twins
// of the per-receiver kernels stored -- pairs [channels][pair_pitch] (one packed dword / one float2 each), audio [channels][n] (int16 / float),
// state [channels][4].  Rows of channels whose mode is SYNCAM are rewritten, the others untouched.  The launcher refuses (hipErrorInvalidValue)
// a null operand, n > pair_pitch and pairs that are not aligned to their size.
struct BankPllParams {
    const void *pairs; long long pair_pitch;
    void *audio; long long n;
    float *state; const int *chan_mode; int channels;
    float omega_min, omega_max, g1, g2;          // msdr_syncam_constants' four, or msdr_syncam_constants_rate's
};
hipError_t launch_bank_pll(hipStream_t stream, bool f32, const BankPllParams &p);
}  // namespace msdr
