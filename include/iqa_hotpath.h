/*
 * iqa_hotpath.h -- C ABI of the MI355X-native channelize -> demodulate hot path.
 *
 * This is the drop-in boundary for the DSP stages of rknightion/iq-to-audio
 * (src/iq_to_audio/processing.py and src/iq_to_audio/decoders/).  Every entry
 * point names the reference interface it replaces ("ref:" lines, paths relative to
 * the reference's src/iq_to_audio/).  The reference is pure Python, so its "FFI" is
 * a ctypes binding; INTEGRATION.md shows the stub a maintainer would add.
 *
 * Conventions
 *   - All `*_dev` pointers are DEVICE (HBM) pointers on the current HIP device;
 *     `stream` is a hipStream_t passed as void* (0 = default stream).  Calls only
 *     enqueue work: they never synchronise, allocate or free, so they can be
 *     captured into a hipGraph.
 *   - Complex samples are interleaved float pairs (re, im) == numpy complex64.
 *   - Raw capture frames are interleaved pairs in the capture's own sample format
 *     (iqa_fmt); one frame = one complex sample.
 *   - Return value: IQA_OK or an iqa_status error; iqa_last_error() gives the text
 *     (thread-local).  The Python shim maps IQA_EINVAL -> ValueError, everything
 *     else -> RuntimeError, as the reference raises them.
 *   - Streaming state (FIR history, discriminator previous sample, IIR states, peak)
 *     lives in small caller-owned device buffers whose layouts are given below, so
 *     the library keeps no per-stream or per-capture state and is re-entrant per stream and
 *     per host thread.  What it does keep, process-wide and thread-safe: one bit per
 *     (kernel, device id) "dynamic-LDS limit raised" (atomics), the spectrum entry point's
 *     LRU of rocFFT plans keyed by (device, nfft, batch) behind a mutex, and 64 KiB of pacing
 *     words per device for iqa_channelize_mfma_pairs (the ONE exception to "never allocate":
 *     hipMalloc + hipMemset at the first pair launch on a device -- make that call outside a
 *     stream capture; entries are tagged per launch, nothing is reset afterwards).
 */
#ifndef IQA_HOTPATH_H
#define IQA_HOTPATH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IQA_ABI_VERSION 1
/* Per-segment sums of squares are spread over this many sub-slots (sumsq_dev holds n_segs*IQA_SUMSQ_SLOTS
 * doubles, the caller adds the slots of a segment): float atomics on one address serialise at memory
 * latency, so 40 blocks adding into one word cost ~65 us; eight words cost ~8 us. */
#define IQA_SUMSQ_SLOTS 8

typedef enum {
    IQA_OK = 0,
    IQA_EINVAL = 1, /* bad argument (ValueError in the reference) */
    IQA_EHIP = 2,   /* HIP runtime / launch failure (RuntimeError) */
    IQA_ESTATE = 3  /* call sequence error, e.g. process before setup (RuntimeError) */
} iqa_status;

/* Sample format of a raw capture frame.  ref: input_formats.py:45-94 (_FORMAT_MAP)
 * and the ffmpeg conversion the reference relies on (processing.py:113-158):
 *   S16: x/32768   U8: (x-128)/128   F32: unchanged (also = complex64 stage data). */
typedef enum { IQA_FMT_S16 = 0, IQA_FMT_U8 = 1, IQA_FMT_F32 = 2 } iqa_fmt;

/* ref: IQReader._extract_iq, processing.py:268-279 */
typedef enum { IQA_ORDER_IQ = 0, IQA_ORDER_QI = 1, IQA_ORDER_IQ_INV = 2, IQA_ORDER_QI_INV = 3 } iqa_iq_order;

/* ref: create_decoder, decoders/__init__.py:9-24 */
typedef enum { IQA_DEMOD_NFM = 0, IQA_DEMOD_AM = 1, IQA_DEMOD_USB = 2, IQA_DEMOD_LSB = 3 } iqa_demod;

int iqa_abi_version(void);
const char *iqa_last_error(void);

/* ------------------------------------------------------------------------- *
 * Channelizer: ingest + NCO mix + channel FIR + decimate in ONE kernel.      *
 *                                                                            *
 * ref: the first half of the per-chunk body of ProcessingPipeline.run,       *
 *      processing.py:1088-1096, i.e.                                         *
 *        IQReader._extract_iq        processing.py:268-279                   *
 *        ComplexOscillator.mix       processing.py:289-297                   *
 *        OverlapSaveFIR.process      processing.py:325-346                   *
 *        Decimator.process           processing.py:354-360                   *
 *                                                                            *
 * Math: z[m] = e^{j*2pi*rot(m)} * sum_k g[k] * x[m*D - k],  m = m_first..    *
 * where g[k] = h[k]*e^{+j*s*w*k} are the channel taps pre-rotated on the     *
 * host (so no per-input-sample trig is needed), and rot() is a 64-bit        *
 * fixed-point phase in turns.  Equal to mix -> filter -> keep every D-th     *
 * sample of the reference, with zero initial state (causal convolution, group *
 * delay not compensated).                                                     *
 * ------------------------------------------------------------------------- */
typedef struct {
    int32_t fmt;          /* iqa_fmt of raw frames */
    int32_t ntaps;        /* L */
    int32_t decimation;   /* D >= 1 */
    int32_t conj_sum;     /* 1: conjugate the tap sum before rotation (host folds iq_order into taps + this flag:
                           *    x = c*conj(r)  =>  sum g*x = c*conj(sum conj(g)*r)) */
    int32_t rotate;       /* 0: no output rotation (plain FIR stage), 1: apply rot(m) */
    int32_t reserved;
    uint64_t rot_step;    /* phase advance per OUTPUT sample, turns * 2^64 (wraps) */
    uint64_t rot_base;    /* phase of output m = 0 (global), turns * 2^64 */
    float out_scale_re;   /* constant complex factor applied last (1, j, -j for iq_order) */
    float out_scale_im;
} iqa_chan_params;

/*
 * taps_dev    : float2[ntaps_padded] complex taps in WINDOW order (taps_dev[i] multiplies
 *               x[n0-(L-1)+i]), zero padded to iqa_taps_padded_len(L); already scaled by the
 *               ingest scale (1/32768 for S16, 1/128 for U8).
 * raw_dev     : frames [0, n_frames) of this block; frame 0 has GLOBAL index `consumed`.
 * hist_dev    : the L-1 frames preceding raw_dev (same fmt), or NULL for "all zeros"
 *               (start of capture).  ref: OverlapSaveFIR.state, processing.py:323,341-345.
 * m_first     : global index of the first output to produce; outputs m_first..m_first+n_out-1
 *               need frames up to (m_first+n_out-1)*D, all of which must be < consumed+n_frames.
 * z_out_dev   : float2[n_out].
 */
int64_t iqa_taps_padded_len(int32_t ntaps);
int iqa_channelize(const iqa_chan_params *p, const void *taps_dev, const void *raw_dev, int64_t n_frames,
                   int64_t consumed, const void *hist_dev, int64_t m_first, int64_t n_out, void *z_out_dev,
                   void *stream);

/*
 * int8-MFMA form of iqa_channelize for int16 captures -- and, ring variant only, uint8 ones -- (same reference lines, same result up to the
 * 16-bit fixed-point tap quantisation, ~1e-6 of full scale): the decimating FIR is evaluated as a
 * dense integer GEMM on the matrix cores with exact int32 accumulation (see channelize_mfma.hip).
 * It covers only outputs whose whole read range lies inside raw_dev[0, n_frames): columns
 * (m_first-64)*D+1 ... ; the caller runs iqa_channelize for the few outputs at the block's head
 * (history) and tail.
 * Here (unlike iqa_channelize) `consumed` may be negative: raw_dev then starts |consumed| frames before global
 * frame 0 and those frames must be zero (the filter's zero initial state, OverlapSaveFIR.state processing.py:323);
 * with such a lead-in and some readable slack behind the capture every output of a capture is an interior one.
 *   afrag_dev : tap fragments of THIS pass, k_count*8192 bytes, layout [kstep][rowtile 4][piece 2][lane 64][16 B]
 *               (host: dsp_plan.plan_mfma); unit/c_re/c_im from the same quantisation.
 * One call is one PASS over (q-group, k-step range).  A filter with ceil(L/D) <= 64 whose fragments fit
 * LDS needs a single pass (q_group 0, all k steps, finalize 1).  Longer filters are split into q-groups of
 * 64 tap rows (each pass reads the capture again, shifted by 64*q_group rows), larger decimations into k-step
 * ranges (each pass reads its own part of every row); passes chain their raw sums through
 * partial_out_dev -> partial_in_dev (double2[n_out]) and the last pass (finalize 1) rotates, scales, stores z.
 * A ring pass (reserved & 64) is a one-lane launch of iqa_channelize_mfma_multi: ranges = ceil(n_out/outputs_per_block),
 * 8*ceil(ranges/8) workgroups (the ones past the last range return at once), the same read bounds.
 */
typedef struct {
    int32_t outputs_per_block; /* multiple of 32; LDS = afrag + 16*(outputs_per_block+160) bytes <= 160 KiB */
    int32_t reserved;          /* data-path variant + diagnostics flags.  0 = per-lane row loads; 64 = block-wide
                                * ring through LDS (byte planes staged by loader waves, or LDS-DMA), 64-bit sums (needs iqa_mfma_ring_mode(fmt, D, k_first, k_count, 0) != 0;
                                * its LDS does not depend on outputs_per_block); 64|128 = the ring with 256*S1 + S2
                                * in one int32, for fragments from a quantisation that bounds that sum
                                * (dsp_plan.plan_mfma(acc32=True); iqa_mfma_ring_mode(fmt, D, k_first, k_count, 1) != 0);
                                * bits 0..5 are timing diagnostics of the per-lane kernel, never
                                * set in production; the ring ignores them; 256 = the low tap byte
                                * of these fragments is zero throughout (a hint: the multi-lane launches act on it, lane bit 1) */
    double unit;               /* value of one tap LSB (ingest scale folded in) */
    double c_re, c_im;         /* 128 * sum of quantised taps per output component (low-byte bias) */
    void *debug_stamps;        /* NULL in production; the per-lane kernel writes per-wave cycle stamps here
                                * (64 B per wave) when bit 1 of `reserved` is set (the ring kernels never do) */
    int32_t q_group;           /* tap rows 64*q_group+1 .. 64*q_group+64 */
    int32_t k_first;           /* first k step (32 int16 values each) of this pass */
    int32_t k_count;           /* k steps in this pass; 0 = all remaining */
    int32_t finalize;          /* 1 = last pass */
    const void *partial_in_dev;  /* double2[n_out] raw sums of the previous passes, or NULL */
    void *partial_out_dev;       /* double2[n_out], written when finalize == 0 */
} iqa_mfma_params;
int64_t iqa_mfma_afrag_bytes(int32_t decimation);
/* LDS bytes the ring variant (reserved = 64) spends on its data ring for this decimation; 0 = variant not
 * applicable (it needs D % 4 == 0 and D <= 256).  Every tile of 32 data rows is fetched as 2048*ceil(2D/32)
 * contiguous bytes, so the last output of a ring pass must satisfy
 * (m_last - 1)*D + 512*ceil(2D/32) < consumed + n_frames. */
int64_t iqa_mfma_ring_bytes(int32_t decimation);
/* LDS bytes of a workgroup of the ring kernel iqa_mfma_ring_mode selects for this pass (0: none): a launch may give a CU
 * as many workgroups as fit into its 160 KiB (two at <= 3 k steps -- short rows, e.g. D = 26 at 2.5 MS/s -- where a
 * second one hides the first one's per-round latency). */
int64_t iqa_mfma_ring_lds_bytes(int32_t fmt, int32_t decimation, int32_t k_first, int32_t k_count, int32_t acc32);
/* Which ring kernel covers a pass over k steps [k_first, k_first + k_count) at this decimation: 0 = none (int16: use
 * the per-lane kernel, reserved = 0; uint8: use iqa_channelize), 1 = contiguous slots (int16, all k steps in one
 * pass, D % 4 == 0, D <= 256), 2 = row-staged slots (int16 or uint8, any D, k_count <= 11, int32 sums only:
 * acc32 != 0).  Mode 2 reads exactly the frames the per-lane kernel reads; mode 1 needs the slack described above.
 * For uint8 captures (fmt = IQA_FMT_U8, reserved = 64|128) the data have a single byte piece: pass
 * unit = tap LSB / 256 and c_re = c_im = 0 (dsp_plan.plan_mfma does). */
int32_t iqa_mfma_ring_mode(int32_t fmt, int32_t decimation, int32_t k_first, int32_t k_count, int32_t acc32);
int iqa_channelize_mfma(const iqa_chan_params *p, const iqa_mfma_params *q, const void *afrag_dev,
                        const void *raw_dev, int64_t n_frames, int64_t consumed, int64_t m_first, int64_t n_out,
                        void *z_out_dev, void *stream);

/*
 * Several channels of ONE capture in one launch of the ring kernel (shared ingest).
 * ref: the reference CLI runs a whole pipeline per --ft target over the same file (cli.py:683-710, at most five
 * targets :514-521); here every (channel, tap-row group) is a LANE of one launch: the lanes share the capture, the
 * decimation, the k-step range and the output range, and differ in their tap fragments, scale, rotation and output.
 * Lanes of the same stretch of the capture run at the same time on the CUs of one XCD, so the stretch crosses the
 * fabric once (channelize_ring.hip).  int32 sums only: fragments from dsp_plan.plan_mfma(acc32=True);
 * iqa_mfma_ring_mode(fmt, D, k_first, k_count, 1) must be non-zero.  At most 16 lanes per call.
 * Two lanes may share a q_group (their data rows): a group's taps and the residue of their quantisation as a second lane
 * (the "fine" precision of the host pipeline, dsp_plan.plan_mfma(residual=True)).
 * A filter with several tap-row groups is several lanes with finalize = 0, each writing its raw sums to its own
 * partial_out_dev; iqa_mfma_combine adds them in group order and finishes z.  A decimation whose k steps need several
 * passes is several calls chained through partial_in_dev / partial_out_dev per lane, as with iqa_channelize_mfma.
 * outputs_per_block: multiple of 32; the launch has 8*ceil(ceil(n_out/outputs_per_block)/8)*n_lanes workgroups -- one
 * workgroup per CU (256) when ceil(n_out/outputs_per_block) = 8*floor(32/n_lanes).
 */
typedef struct {
    const void *afrag_dev;      /* this lane's tap fragments, first k step of the pass (as for iqa_channelize_mfma) */
    void *z_out_dev;            /* finalize != 0: float2[n_out] */
    const void *partial_in_dev; /* double2[n_out] raw sums of this lane's earlier k-step passes, or NULL */
    void *partial_out_dev;      /* finalize == 0: double2[n_out] */
    double unit, c_re, c_im;    /* as in iqa_mfma_params */
    uint64_t rot_step, rot_base;        /* as in iqa_chan_params */
    float out_scale_re, out_scale_im;
    int32_t q_group, finalize, conj_sum, rotate;
    int32_t raw_partials;       /* finalize == 0 and no partial_in: partial_out_dev is int32[2*n_out], the integer sums
                                 * (256*S1 + S2 per component) themselves; iqa_mfma_combine scales them (raw_scale) */
    int32_t reserved;           /* bit 0: 64-bit sums ((S1 << 32) + S2 per component: fragments WITHOUT the int32 bound, 16-bit
                                 * taps -- dsp_plan.plan_mfma(acc32=False)); the same for every lane of a launch; contiguous
                                 * slots only, no raw_partials.  See iqa_mfma_ring_lanes.
                                 * bit 1: this lane's LOW tap byte is zero throughout (piece 1 of every fragment: the first
                                 * lane of a tap-row group under dsp_plan.plan_mfma(residual=True)): the kernel skips the
                                 * q2*hi product of every k step (two matrix instructions per k step instead of three).
                                 * bits 8..13: rot -- afrag_dev holds dsp_plan's afrag_rot: the tap rows of either component
                                 * rotated by rot slots so that slots 0..15 are rows whose HIGH tap byte is zero throughout
                                 * (the edge rows of a Kaiser design), whose q1 products the kernel then does not issue.  A
                                 * multiple of 4, at most 32, in a single-lane launch where iqa_mfma_ring_zero_rows() != 0;
                                 * refused elsewhere.  0: not rotated.  Same sums bit for bit. */
} iqa_mfma_lane;
int iqa_channelize_mfma_multi(int32_t fmt, int32_t decimation, int32_t k_first, int32_t k_count,
                              int32_t outputs_per_block, const iqa_mfma_lane *lanes, int32_t n_lanes,
                              const void *raw_dev, int64_t n_frames, int64_t consumed, int64_t m_first,
                              int64_t n_out, void *stream);

/* The same launch with TWO lanes per workgroup: lanes[2i] and lanes[2i+1] (n_lanes even) share every staged tile of the
 * capture -- the workgroup's first four waves hold the tap rows of one, the other four those of the other, one tile
 * per round: half the L2 -> LDS traffic per lane and a ring twice as deep in rounds.  lanes[2i].q_group >=
 * lanes[2i+1].q_group (the first lane's stream is the one staged; the second works two rounds per group of difference
 * behind); lanes[2i+1].afrag_dev may be NULL: a pair without a second lane (that half of the workgroup idles).  Same
 * arguments otherwise, same results bit for bit as iqa_channelize_mfma_multi on the same lanes;
 * 8*ceil(ranges/8)*n_lanes/2 workgroups.  Available where iqa_mfma_ring_pairs(fmt, D, k_first, k_count) != 0 (int16 captures, contiguous slots,
 * 9..16 k steps: the decimations whose single-lane kernel runs without loader waves).
 * ref: the same CLI loop over --ft targets, cli.py:683-710. */
int iqa_channelize_mfma_pairs(int32_t fmt, int32_t decimation, int32_t k_first, int32_t k_count,
                              int32_t outputs_per_block, const iqa_mfma_lane *lanes, int32_t n_lanes,
                              const void *raw_dev, int64_t n_frames, int64_t consumed, int64_t m_first,
                              int64_t n_out, void *stream);
int32_t iqa_mfma_ring_pairs(int32_t fmt, int32_t decimation, int32_t k_first, int32_t k_count);
/* What the multi-lane launches offer for a pass over k steps [k_first, k_first + k_count) at this decimation and sum
 * width (acc32 != 0: one int32 per component; 0: one int64, iqa_mfma_lane.reserved bit 0): bit 0 = iqa_channelize_mfma_multi,
 * bit 1 = iqa_channelize_mfma_pairs.  0: no shared-ingest launch (64-bit sums need contiguous slots: D % 4 == 0, D <= 240;
 * their pairs 9..14 k steps).  The "full" precision of the host pipeline puts a filter's tap-row groups AND the residue of
 * their quantisation into such a launch as lanes (ref: the per---ft loop of the reference CLI, cli.py:683-710). */
int32_t iqa_mfma_ring_lanes(int32_t fmt, int32_t decimation, int32_t k_first, int32_t k_count, int32_t acc32);
/* != 0: a single-lane iqa_channelize_mfma_multi launch over these k steps takes rotated tap fragments (iqa_mfma_lane.reserved
 * bits 8..13): int16 captures, int32 sums, contiguous slots, at most 8 k steps, 1..16 values in the row's last k step. */
int32_t iqa_mfma_ring_zero_rows(int32_t fmt, int32_t decimation, int32_t k_first, int32_t k_count, int32_t acc32);
/* The kernel family the calling thread's last iqa_channelize_mfma_multi launch took (diagnostics and tests; a static string). */
const char *iqa_mfma_ring_last_kernel(void);
/* z[m_first + i] = finish(sum_k partials_dev[k][i]): the float32 conversion, conjugation, rotation and scaling of the
 * kernels' own emission (p supplies conj_sum, rotate, rot_step, rot_base, out_scale).  1..16 buffers of double2[n_out]
 * (a filter's tap-row groups -- and, with residual quantisation, each group's second lane: dsp_plan.plan_mfma(residual=True)),
 * or -- raw_scale != NULL -- of int32[2*n_out] written by lanes with raw_partials = 1; raw_scale is a HOST array of
 * n_partials triples {unit, c_re, c_im} (the lane's own values), applied as (256*v + c)*unit before the sum. */
int iqa_mfma_combine(const iqa_chan_params *p, const void *const *partials_dev, int32_t n_partials,
                     const double *raw_scale, int64_t m_first, int64_t n_out, void *z_out_dev, void *stream);

/* Copy the last L-1 frames of (hist | raw) into hist (handles n_frames < L-1 by shifting).
 * ref: OverlapSaveFIR.process state update, processing.py:341-345.
 * hist_next_dev must not alias hist_dev. */
int iqa_history_update(int32_t fmt, int32_t ntaps, const void *hist_dev, const void *raw_dev, int64_t n_frames,
                       void *hist_next_dev, void *stream);

/* ------------------------------------------------------------------------- *
 * Stand-alone stages of the pluggable stage API                              *
 * ------------------------------------------------------------------------- */

/* ref: ComplexOscillator.mix, processing.py:289-297 (+ ingest conversion when fmt != F32).
 * out[i] = cvt(in[i]) * exp(j*(phase0 + step*i)), phase ramp evaluated in float64 exactly as
 * the reference does; the caller carries phase0 = (phase0 + step*n) mod 2pi on the host. */
int iqa_oscillator_mix(int32_t fmt, int32_t iq_order, const void *in_dev, int64_t n, double phase0, double step,
                       void *out_dev, void *stream);

/* ref: Decimator.process, processing.py:354-360.  out[i] = in[first + i*D]. */
int iqa_decimate(const void *in_dev, int64_t n, int64_t first, int32_t D, void *out_dev, int64_t n_out,
                 void *stream);

/* mean(|z|^2) over z[skip:n] accumulated in float64 into *power_dev (double[1], overwritten).
 * Up to 65536 samples (the mixer-sign probes) one workgroup WRITES the result -- no memset, no atomics -- so
 * power_dev may then be mapped pinned host memory (the probe's read-back without a copy).
 * ref: choose_mix_sign, processing.py:650-658; baseband_power, processing.py:1105. */
int iqa_mean_power(const void *z_dev, int64_t n, int64_t skip, void *power_dev, void *stream);

/* The same for `parts` stretches of n_each samples that lie back to back in z_dev: power_dev[p] = mean(|z|^2) over
 * z[p*n_each + skip : (p+1)*n_each].  One launch when a stretch has at most 65536 samples (then written, not
 * accumulated: power_dev may be mapped pinned host memory) -- the two mixer-sign probes of choose_mix_sign
 * (processing.py:623-663) side by side. */
int iqa_mean_power_batch(const void *z_dev, int64_t n_each, int32_t parts, int64_t skip, void *power_dev, void *stream);

/* Wideband level of raw capture frames: *mean_square_out (double[1], WRITTEN by one workgroup: device or mapped pinned
 * host memory) = mean of value^2 over up to 65536 values -- eight 16 KiB stretches spread evenly over raw_dev[0 : n_values] (int16 / uint8 - 128 /
 * float32 values, I and Q alike; raw_dev 16-byte aligned).  The caller scales: wideband RMS of the complex samples =
 * sqrt(2 * mean_square) * ingest scale.  It is the reference level of the precision guard of the fixed-point
 * channelizers (a channel far below the wideband level is re-run at a finer precision); the reference needs none -- its
 * filter runs in complex128 whatever the levels, processing.py:300-346 -- and the warm-up block it is measured on is the
 * one choose_mix_sign inspects, processing.py:1027-1043. */
int iqa_raw_level(int32_t fmt, const void *raw_dev, int64_t n_values, void *mean_square_out, void *stream);

/* ------------------------------------------------------------------------- *
 * Demodulators (channel rate)                                                 *
 * ------------------------------------------------------------------------- */

/* ref: QuadratureDemod.process, decoders/nfm.py:17-24.
 * out[i] = atan2 of z[i]*conj(z[i-1]); prev_dev = float2[1] state (init 1+0j), updated. */
int iqa_quadrature(const void *z_dev, int64_t n, void *prev_dev, void *out_dev, void *stream);

/* ref: AMDecoder.process envelope, decoders/am.py:28.  out[i] = |z[i]| (float32). */
int iqa_envelope(const void *z_dev, int64_t n, void *out_dev, void *stream);

/* ref: SSBDecoder.process, decoders/ssb.py:42-43.  out[i] = real(z[i]) for usb AND lsb. */
int iqa_real_part(const void *z_dev, int64_t n, void *out_dev, void *stream);

/*
 * First-order recurrences as parallel affine scans (float64 scan arithmetic).
 *
 * iqa_deemphasis : y[n] = (1-a)*x[n] + a*y[n-1]        ref: DeemphasisFilter.process, decoders/nfm.py:48-62
 *                  state_dev = double[1] holding y[last] (reference keeps a*y[last]); init 0.
 * iqa_dc_block   : y[n] = x[n] - x[n-1] + r*y[n-1]     ref: DCBlocker.process, decoders/common.py:16-30
 *                  state_dev = double[2] {x[last], y[last]}; init 0,0.
 * iqa_agc        : g[n] = g[n-1] + decay*(target/|x[n]| - g[n-1]) if |x[n]| > 1e-6 else g[n-1];
 *                  out[n] = x[n]*g[n]; g restarts at 1.0 at element 0 and at every index in
 *                  reset_starts_dev (optional, sorted int64[n_resets]; the reference restarts it on
 *                  every process() call, i.e. at every chunk boundary).  ref: SSBDecoder._apply_agc,
 *                  decoders/ssb.py:65-80.
 * work_dev: scratch, at least iqa_scan_workspace_bytes(n) bytes.
 * The three run on the scan of iqa_demodulate below, from a float input to the unclipped output.
 * y_dev must not alias x_dev: the one-launch form of iqa_deemphasis (iqa_scan_window) reads inputs in front of a
 * workgroup's own range, and the last `window` inputs once more, while other workgroups write their outputs.
 */
int64_t iqa_scan_workspace_bytes(int64_t n);
/* ref: none (DeemphasisFilter.process is one sequential loop, decoders/nfm.py:48-62; this describes the scan's geometry).
 * The de-emphasis scan runs in ONE launch where the pole forgets inside a workgroup's span: *window = the smallest multiple
 * of 512 with alpha^window <= 2^-64, *span = positions per workgroup (the first `window` of them a warm-up from state 0,
 * the rest its own; the first workgroup starts at index 0 from the carried state).  Returns 0 with both filled when that
 * form is used for this pole (window <= span / 2), 1 when the three launches are kept (either pointer may be NULL). */
int iqa_scan_window(double alpha, int64_t *window, int64_t *span);
int iqa_deemphasis(const void *x_dev, int64_t n, double alpha, void *state_dev, void *y_dev, void *work_dev,
                   void *stream);
int iqa_dc_block(const void *x_dev, int64_t n, double radius, void *state_dev, void *y_dev, void *work_dev,
                 void *stream);
int iqa_agc(const void *x_dev, int64_t n, double target, double decay, const void *reset_starts_dev,
            int64_t n_resets, void *y_dev, void *work_dev, void *stream);

/*
 * Whole demodulator + AudioWriter.write for a block of channel samples: three launches (reduce, carry, apply), or one
 * for nfm where the de-emphasis pole forgets inside a workgroup's span (iqa_scan_window).
 * ref: decoder.process (processing.py:1128) for nfm / am / usb / lsb as listed above, followed by
 *      AudioWriter.write (processing.py:1147 -> :440-456) and the per-chunk rms statistic.
 * The source stage (discriminator / |z| / real) and the sink (pre-clip peak, clip +-0.99, per-segment
 * sum of squares) are fused into the scan passes.  state_dev: 32 bytes {float2 prev (init 1+0j);
 * double y_last; double x_last, y_last}, carried across calls.  seg_starts_dev: sorted int64 chunk
 * starts within this block (seg_starts[0] == 0): AGC restarts + statistics segments.
 * scratch_dev: float[n], only used by SSB with AGC.  work_dev: iqa_scan_workspace_bytes(n).
 */
typedef struct {
    int32_t mode;        /* iqa_demod */
    int32_t agc_enabled; /* honoured for USB/LSB only, as in the reference */
    double deemph_alpha; /* exp(-1/(fs_ch*tau)) */
    double dc_radius;    /* 0.995 */
    double agc_target;   /* 10^(-12/20) */
    double agc_decay;    /* 0.001 */
} iqa_demod_params;
int iqa_demodulate(const iqa_demod_params *p, const void *z_dev, int64_t n, void *state_dev,
                   const void *seg_starts_dev, int64_t n_segs, void *peak_dev, void *sumsq_dev, void *audio_out_dev,
                   void *scratch_dev, void *work_dev, void *stream);
/* The same for the FIRST block of a stream: a decoder that has seen nothing (decoder setup / AudioWriter creation in
 * ProcessingPipeline.run, processing.py:1040-1066).  state_dev is not read (prev = 1+0j, filter states 0; it receives the
 * outgoing state as usual), peak_dev and sumsq_dev[0 .. n_segs*IQA_SUMSQ_SLOTS) are cleared by the call itself: no
 * reset copy in front of it (a node less in a captured step).  n > 0. */
int iqa_demodulate_from_reset(const iqa_demod_params *p, const void *z_dev, int64_t n, void *state_dev,
                              const void *seg_starts_dev, int64_t n_segs, void *peak_dev, void *sumsq_dev,
                              void *audio_out_dev, void *scratch_dev, void *work_dev, void *stream);

/* ref: decoder setup / AudioWriter creation in ProcessingPipeline.run, processing.py:1040-1066, as a launch of its own:
 * state_dev (32 bytes) becomes the block of a decoder that has seen nothing (prev = 1+0j, filter states 0), peak_dev
 * (float[1], may be NULL) and sumsq_dev[0 .. n_sums) become 0.  For callers that can issue it on another stream ahead of
 * time and then call iqa_demodulate; iqa_demodulate_from_reset does the same inside its own stream. */
int iqa_demod_reset(void *state_dev, void *peak_dev, void *sumsq_dev, int64_t n_sums, void *stream);

/* ref: AudioWriter.write, processing.py:440-456: peak = max(peak, max|a|) BEFORE the clip, then
 * clip to +-0.99.  peak_dev = float[1] (running, init 0).  In-place allowed (out_dev == a_dev).
 * Also accumulates sum(a^2) (pre-clip, float64) into sumsq_dev[seg*IQA_SUMSQ_SLOTS + slot] for the rms_dbfs statistic
 * (ref: decoders/nfm.py:88-89), where seg = index into seg_starts_dev (sorted int64[n_segs],
 * seg_starts[0] == 0); pass NULL/0 to skip.  peak_dev and out_dev may each be NULL (statistics only). */
int iqa_writer_clip(const void *a_dev, int64_t n, void *peak_dev, const void *seg_starts_dev, int64_t n_segs,
                    void *sumsq_dev, void *out_dev, void *stream);

/* ------------------------------------------------------------------------- *
 * 48 kHz resampler (replaces the `ffmpeg -ar 48000` leg, processing.py:399-418) *
 * BUILD-DEFINED SPEC (the reference's is libswresample: parity unpinned).      *
 *   y[j] = sum_t table[p][t] * x[q - (t - T)],  c = (j0+j)*down, q = c / up, p = c % up          *
 * table_dev: double[up][2T+1] polyphase rows; x zero outside [0, n_in).       *
 * y_dev: float32[n_out] and/or pcm16_dev: int16[n_out] = iqa_float_to_pcm16 of the float32 value (the writer's    *
 * `-acodec pcm_s16le` leg in the same pass); either may be NULL, not both.                                       *
 * Rows of up to 192 taps run on the staged kernel; longer rows (input rates above ~6x the output rate, up to      *
 * 4097 taps) on a direct one, sixteen lanes per output: the same sums, in another fixed order.                  *
 * ------------------------------------------------------------------------- */
int iqa_resample(const void *x_dev, int64_t n_in, const void *table_dev, int32_t up, int32_t down, int32_t T,
                 int64_t j0, int64_t n_out, void *y_dev, void *pcm16_dev, void *stream);

/* float32 -> PCM16 (round-half-even of y*32768, saturated).  Build-defined, see above. */
int iqa_float_to_pcm16(const void *y_dev, int64_t n, void *pcm_dev, void *stream);

/* ------------------------------------------------------------------------- *
 * Wideband FM stereo (--demod wfm)                      *
 * ------------------------------------------------------------------------- */

/* Longest stereo-matrix filter (N taps): fs_channel up to ~1.4 MHz. */
#define IQA_WFM_MAX_TAPS 2047
/* Partial sums of |p|^2 a stereo-matrix call over n samples writes: ceil(n / 2048), 0 for n <= 0. */
int64_t iqa_wfm_partials(int64_t n);
/* One block of the stereo matrix.  theta_dev: float32[n] discriminator output (radians per sample); m = m_scale * theta is
 * the composite (m_scale = fs / (2 pi 75 000)).  With N = ntaps (odd, 3..IQA_WFM_MAX_TAPS), D = (N-1)/2 and causal filters of
 * zero initial state: p = h_p * m, c = -Im((p/|p|)^2) (0 where |p| < 1e-12), md[n] = m[n-D], a = h_a * md, b = h_a * (2 md c).
 * taps_dev: float32[3(D+1)] = h_a[0..D], Re h_p[0..D], Im h_p[0..D] (h_a symmetric, h_p[N-1-k] = conj(h_p[k])).
 * hist_dev: float32[2(N-1)], the discriminator values in front of theta[0] (NULL: zeros, the start of a stream).
 * a_out_dev, b_out_dev: float32[n]; m_out_dev (optional): float32[n] composite; partials_dev (optional):
 * double[iqa_wfm_partials(n)], the sum of |p|^2 over each 2048 outputs.  Every output is summed in one fixed order: the
 * outputs do not depend on how a stream is cut into calls. */
int iqa_wfm_stereo(int32_t ntaps, const void *taps_dev, float m_scale, const void *theta_dev, int64_t n, const void *hist_dev,
                   void *m_out_dev, void *a_out_dev, void *b_out_dev, void *partials_dev, void *stream);
/* left = a + b, right = a - b (float32[n]; in place allowed). */
int iqa_wfm_matrix(const void *a_dev, const void *b_dev, int64_t n, void *left_dev, void *right_dev, void *stream);

/* ------------------------------------------------------------------------- *
 * RDS beside the stereo matrix (--demod wfm --rds)      *
 * ------------------------------------------------------------------------- */

/* Longest matched filter (2 half_taps + 1 taps) and largest decimation: what a channel rate of IQA_WFM_MAX_TAPS needs. */
#define IQA_RDS_MAX_HALF 2400
#define IQA_RDS_MAX_DECIM 80
/* Discriminator values the caller carries in front of a block: 2 half_taps + 2 (ntaps - 1); 0 for invalid arguments. */
int64_t iqa_rds_hist_len(int32_t ntaps, int32_t half_taps);
/* Decimated outputs of a block of n samples whose first has the absolute index pos: the j with pos <= j decim < pos + n. */
int64_t iqa_rds_outputs(int64_t pos, int64_t n, int32_t decim);
/* Dynamic LDS of iqa_rds_baseband at these sizes; 0 where its windows do not fit 64 KiB (the call is then IQA_EINVAL). */
int64_t iqa_rds_lds_bytes(int32_t ntaps, int32_t half_taps, int32_t decim);
/* One block of the RDS baseband.  theta_dev, m_scale, ntaps (N), D and the carried history are iqa_wfm_stereo's; pos is the
 * absolute index of theta[0] in the stream, all indices below are absolute.  With md[n] = m[n-D], p = h_p * m, u = p / |p|
 * (0 where |p| < 1e-12), R = decim, M = half_taps, f = f_mix (57 000 / fs) and the antisymmetric matched filter h_r
 * (h_r[2M-k] = -h_r[k]), for every j with pos <= jR < pos + n:
 *   y[j] = (sum_k h_r[k] md[jR-k] exp(-j 2 pi frac(f (jR-k)))) exp(+j 2 pi frac(f jR)) conj(u[jR])^3
 *   q[j] = rint(angle(u[jR] conj(u[(j-1)R]) exp(-j 2 pi clock_step)) / (2 pi) * 2^44),  q[0] = 0   (clock_step = 19 000 R / fs)
 * pilot_taps_dev: float32[2(D+1)] = Re h_p[0..D], Im h_p[0..D]; mf_taps_dev: float32[M] = h_r[0..M-1];
 * hist_dev: float32[iqa_rds_hist_len] in front of theta[0] (NULL: zeros); y_out_dev: complex64[iqa_rds_outputs];
 * q_out_dev: int64[iqa_rds_outputs].  Every sum runs in one fixed order: outputs do not depend on how a stream is cut. */
int iqa_rds_baseband(int32_t ntaps, const void *pilot_taps_dev, int32_t half_taps, const void *mf_taps_dev, int32_t decim,
                     float m_scale, double f_mix, double clock_step, const void *theta_dev, int64_t n, int64_t pos,
                     const void *hist_dev, void *y_out_dev, void *q_out_dev, void *stream);
/* phi[i] = *total + q[0] + .. + q[i] (int64, exact), *total = phi[n-1]; psi[i] = ((j_first + i) clock_step + phi[i] 2^-44) / 16
 * (float64, each operation rounded once).  total_dev: int64[1] on the device, carried from call to call; work_dev:
 * int64[iqa_rds_clock_chunks(n)] workspace (reduce / apply / carry over chunks of 4096 values). */
int64_t iqa_rds_clock_chunks(int64_t n);
int iqa_rds_clock(const void *q_dev, int64_t n, int64_t j_first, double clock_step, void *total_dev, void *work_dev,
                  void *phi_out_dev, void *psi_out_dev, void *stream);
/* out[0..2] = Re Z, Im Z, sum |y|^2 over j0 <= j < n with Z = sum |y[j]|^2 exp(-j 2 pi psi[j]) (float64; per tile of 1024
 * indices, then over the tiles, both in a fixed order).  partials_dev: double[3 iqa_rds_timing_partials(n)] workspace. */
int64_t iqa_rds_timing_partials(int64_t n);
int iqa_rds_timing(const void *y_dev, const void *psi_dev, int64_t n, int64_t j0, void *partials_dev, void *out_dev, void *stream);
/* Symbols and bits.  r = psi - tau; for j0 < j < n with k = floor(r[j]) > floor(r[j-1]):
 * sym[k - k_first] = y[j-1] + (y[j] - y[j-1]) (k - r[j-1]) / (r[j] - r[j-1]) (complex64; indices outside 0 .. nsym-1 are
 * dropped; the caller zeroes sym), then bits[i] = Re(sym[i+1] conj(sym[i])) < 0 (uint8[nsym - 1]). */
int iqa_rds_symbols(const void *y_dev, const void *psi_dev, int64_t n, int64_t j0, double tau, int64_t k_first, int64_t nsym,
                    void *sym_out_dev, void *bits_out_dev, void *stream);
/* For every bit offset i <= nbits - 26: words[i] = bits i .. i+25, first bit most significant (uint32), synd[i] =
 * crc10(words[i] >> 10) xor (words[i] & 0x3FF) with g = x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1 (uint16). */
int iqa_rds_syndromes(const void *bits_dev, int64_t nbits, void *words_out_dev, void *synd_out_dev, void *stream);

/* ------------------------------------------------------------------------- *
 * POCSAG beside the NFM demodulator (--demod nfm --pocsag) *
 * ------------------------------------------------------------------------- */

/* Most samples per bit (and so the longest bit integrator): the sync kernel stages tile + rint(31 sps) + 1 integrator
 * values in LDS (1024 + 11 905 int32 = 50.5 KiB at the limit).  A baud rate needs 8 <= fs / baud <= this. */
#define IQA_POCSAG_MAX_SPS 384
#define IQA_POCSAG_BAUDS 3
/* Bit instants of one batch: offsets[i] = rint(i sps), i = 0 .. 544 (32 sync bits, 16 x 32 codeword bits, the next sync). */
#define IQA_POCSAG_OFFSETS 545
/* One block of the quantiser and the bit integrators.  t[n] = rint(theta[n] 2^20) (int32, half-even); for each baud b with
 * window[b] = L > 0: S_b[n] = t[n] + t[n-1] + .. + t[n-L+1] (int32), t in front of the block taken from hist_dev.
 * theta_dev: float32[n] (iqa_quadrature's output); hist_dev: int32[hist_len], the hist_len = max L - 1 values of t in front
 * of theta[0], oldest first (NULL: zeros); t_out_dev: int32[n]; s_out_dev[b]: int32[n], or NULL where window[b] = 0.
 * Integer sums: the outputs do not depend on how a stream is cut into blocks. */
int iqa_pocsag_integrate(const void *theta_dev, int64_t n, const void *hist_dev, int32_t hist_len,
                         const int32_t window[IQA_POCSAG_BAUDS], void *t_out_dev, void *const s_out_dev[IQA_POCSAG_BAUDS],
                         void *stream);
/* Sync search of one baud over a whole run.  s_dev: int32[n] (S_b); offsets: HOST int32[32], offsets[i] = rint(i sps),
 * ascending, offsets[0] = 0, offsets[31] <= 31 IQA_POCSAG_MAX_SPS.  For every m with m + offsets[31] < n:
 *   v_i = S[m + offsets[i]], Sigma = sum v_i, x_i = 32 v_i - Sigma, w_i = (x_i < 0), W = w_0 .. w_31 (w_0 most significant),
 *   d+ = popcount(W xor 0x7CD215D8), d- = 32 - d+, E = sum |x_i|; m is a candidate iff min(d+, d-) <= 2 and
 *   128 min |x_i| >= E; score[m] = 2 E + (d- < d+) for a candidate, 0 otherwise (and 0 where m is not evaluated).
 * A candidate is kept iff no candidate m' with |m' - m| <= half_bit has E' > E, or E' = E and m' < m.  Kept syncs are
 * appended in any order to list_dev: int64[4 capacity] = (m, Sigma, inverted, distance) each; *count_dev (int64, zeroed
 * by the call) counts ALL kept syncs: a count above capacity means the list is incomplete and the call must be repeated
 * with a larger one.  score_dev: int64[n] workspace. */
int iqa_pocsag_sync(const void *s_dev, int64_t n, const int32_t offsets[32], int32_t half_bit, void *score_dev,
                    void *list_dev, int64_t capacity, void *count_dev, void *stream);
/* The 16 codewords behind every kept sync.  list_dev as above (nsync entries); offsets_dev: DEVICE int32[545].  For sync
 * (m, Sigma, inverted), codeword c = 0 .. 15, bit b = 0 .. 31 (first bit most significant): instant m + offsets[32 (1 + c) + b],
 * bit = (32 S[instant] < Sigma) xor inverted.  status 3 (absent: raw = fixed = 0) where the last instant is >= n; else with
 * the syndrome of the upper 31 bits modulo x^10 + x^9 + x^8 + x^6 + x^5 + x^3 + 1 and the parity P of all 32 bits:
 * 0 = syndrome 0, P even; 1 = P odd and the syndrome is 0 (parity bit flipped) or that of one of the 31 positions (that bit
 * flipped); 2 = anything else (fixed = raw).  raw_out_dev, fixed_out_dev: uint32[16 nsync]; status_out_dev: uint8[16 nsync]. */
int iqa_pocsag_codewords(const void *s_dev, int64_t n, const void *list_dev, int64_t nsync, const void *offsets_dev,
                         void *fixed_out_dev, void *raw_out_dev, void *status_out_dev, void *stream);

/* ------------------------------------------------------------------------- *
 * Bell-202 AFSK / AX.25 beside the NFM demodulator (--demod nfm --ax25) *
 * ------------------------------------------------------------------------- */

/* Most samples per bit (and so the longest tone correlator): 12 868 . 256 . L stays inside int32 up to L = 512, and the
 * correlator kernel stages 2048 + L quantised values and 4 L taps in LDS.  A channel needs 8 <= fs / 1200 <= this. */
#define IQA_AFSK_MAX_SPS 400
#define IQA_AFSK_PHASES 8   /* sampling phases per bit */
#define IQA_AFSK_GAINS 3    /* slicer gain pairs (a, b) = (1,1), (1,4), (4,1); variant v = IQA_AFSK_PHASES g + p */
#define IQA_AFSK_SLOT_BYTES 332  /* one kept frame's bytes in the list (a frame has 17 .. 330) */
/* One block of the quantiser, the tone correlators and the slicers.  With L = window:
 *   t[n] = rint(theta[n] 4096) (int32, half-even);
 *   I_f[n] = sum_{k<L} c_f[k] t[n-k], Q_f[n] = sum_{k<L} s_f[k] t[n-k] (int32), f = 1200, 2200;
 *   E_f[n] = (I_f[n]^2 + Q_f[n]^2) >> 4 (int64);
 *   sign[n] = bit g set iff a_g E_1200[n] - b_g E_2200[n] > 0 (int64), g = 0 .. 2.
 * theta_dev: float32[n] (iqa_quadrature's output); hist_dev: int32[L - 1], the values of t in front of theta[0], oldest
 * first (NULL: zeros); taps_dev: int16[4][L] = c_1200, s_1200, c_2200, s_2200 with c_f[k] = rint(256 cos(2 pi f k / fs)),
 * s_f[k] = rint(256 sin(2 pi f k / fs)), |tap| <= 256; t_out_dev: int32[n]; sign_out_dev: uint8[n]; e1200_out_dev,
 * e2200_out_dev: int64[n] each, or NULL (not stored).  8 <= window <= IQA_AFSK_MAX_SPS.  Integer sums: the outputs do
 * not depend on how a stream is cut into blocks.
 * Precondition: |t| < 2^23 everywhere, that is |theta[n]| < 2048 rad (a discriminator output has |theta| <= pi, |t| <= 12 868)
 * and |hist_dev[i]| < 2^23 (values of t_out_dev of the block before are).  The products are formed by the 24-bit multiply,
 * which sign-extends its operands from bit 23: outside the precondition I_f and Q_f differ from the formula above. */
int iqa_afsk_correlate(const void *theta_dev, int64_t n, const void *hist_dev, int32_t window, const void *taps_dev,
                       void *t_out_dev, void *sign_out_dev, void *e1200_out_dev, void *e2200_out_dev, void *stream);
/* The 24 NRZI-decoded bit streams of a whole run.  sign_dev: uint8[n]; step = sps / 8 (float64, made once by the caller).
 * Variant v = 8 g + p, bit i = 0 .. nbits - 1: instant n_i = window - 1 + rint((8 i + p) step) (one float64 product, one
 * rint, half-even); m_i = bit g of sign[n_i]; bits[v][i] = (m_i == m_{i-1}), bits[v][0] = 1; 0 where n_i >= n (the bit
 * does not exist).  bits_out_dev: uint8[24][nbits]. */
int iqa_afsk_bits(const void *sign_dev, int64_t n, int32_t window, double step, int64_t nbits, void *bits_out_dev, void *stream);
/* HDLC frames of the 24 bit streams.  bits_dev: uint8[24][nbits]; count_of: HOST int64[8], the number of bits of phase p
 * that exist (<= nbits).  In variant v (b = bits[v], nb = count_of[v mod 8]) position s, 8 <= s, opens a candidate iff
 * b[s-8 .. s-1] = 0,1,1,1,1,1,1,0 and b[s .. s+7] is not that flag (bits at nb and beyond match nothing).  From s bits
 * are collected least significant first into bytes; a 0 after five consecutive 1s is dropped; the sixth consecutive 1 ends
 * the walk: a closing flag iff the next bit exists and is 0 and exactly 6 bits of the current byte are collected, an abort
 * otherwise; a 331st byte aborts; so does the end of the stream.  A closed candidate of >= 17 bytes is counted in
 * counts[1]; it is kept iff the CRC-16/X.25 (reflected 0x8408, init 0xFFFF, final xor 0xFFFF) of all but its last two
 * bytes equals them, low byte first.  Kept frames are appended in any order: list_dev: int64[4 capacity] = (v, s, start
 * instant n_s, byte count) each, slots_dev: uint8[capacity][IQA_AFSK_SLOT_BYTES] = the bytes, zero-filled.
 * counts_dev: int64[2], zeroed by the call; counts[0] counts ALL kept frames: a count above capacity means the list is
 * incomplete and the call must be repeated with a larger one. */
int iqa_afsk_frames(const void *bits_dev, int64_t nbits, const int64_t count_of[IQA_AFSK_PHASES], int32_t window, double step,
                    void *list_dev, void *slots_dev, int64_t capacity, void *counts_dev, void *stream);

/* ------------------------------------------------------------------------- *
 * CTCSS tones and DTMF digits beside the NFM demodulator (--demod nfm --tones) *
 * ------------------------------------------------------------------------- */

/* The tone banks run behind a decimator by R = floor(fs / 8000), 1 <= R <= this (8000 <= fs < 520 000). */
#define IQA_TONES_MAX_R 64
#define IQA_TONES_MAX_FRAME 6400  /* the longest bank frame (CTCSS at fd just below 16 kHz); it is staged in LDS */
#define IQA_TONES_MAX_TONES 64    /* most tones of one bank call */
#define IQA_TONES_CTCSS 50        /* tones of the CTCSS bank, as iqa_tones_decide reads it */
#define IQA_TONES_DTMF 8          /* tones of the DTMF bank: rows 0 .. 3, columns 4 .. 7 */
#define IQA_TONES_NONE 255        /* the code of a frame without a hit */
/* One block of the quantiser and the triangular decimator.  With w[j] = min(j + 1, 2R - 1 - j), j = 0 .. 2R - 2:
 *   t[n] = rint(theta[n] 4096) (int32, half-even);
 *   u[m] = floor((sum_j w[j] t[(m + 1) R - 1 - j]) / R) (int32; floor division), t zero in front of the stream.
 * theta_dev: float32[n] (iqa_quadrature's output), the samples at absolute indices pos .. pos + n - 1; hist_dev:
 * int32[2R - 2], the values of t at pos - (2R - 2) .. pos - 1, oldest first, zero where the index is negative (NULL: all
 * zeros; not read when R = 1); t_out_dev: int32[n]; u_out_dev: int32[(pos + n) / R - pos / R], the outputs m = pos / R ..
 * (pos + n) / R - 1 that this block completes and no other (NULL is allowed where there is none).  n >= 0, pos >= 0,
 * 1 <= R <= IQA_TONES_MAX_R.  Integer sums: u does not depend on how a stream is cut into blocks, down to one sample.
 * Precondition: |t| <= 2^31 / R^2 everywhere (a discriminator output has |theta| <= pi, |t| <= 12 868): the weighted
 * sum is formed in int32. */
int iqa_tones_decimate(const void *theta_dev, int64_t n, int64_t pos, const void *hist_dev, int32_t R, void *t_out_dev,
                       void *u_out_dev, void *stream);
/* One tone bank over a whole stored run.  Frame i = u[i hop .. i hop + frame - 1], i = 0 .. F - 1 with F = 0 where
 * m < frame, else (m - frame) / hop + 1 (nothing is written where F = 0).  For tone f = 0 .. ntones - 1:
 *   I_f = sum_{k < frame} c_f[k] u[i hop + k], Q_f with s_f (exact in int64);  E_f = (I_f >> 12)^2 + (Q_f >> 12)^2;
 *   P = sum_{k < frame} u[i hop + k]^2 (int64).
 * u_dev: int32[m]; taps_dev: int16[ntones][2][frame] = c_f, s_f with |tap| <= 256; e_out_dev: int64[F][ntones];
 * p_out_dev: int64[F] or NULL (not computed).  1 <= hop <= frame <= IQA_TONES_MAX_FRAME, 1 <= ntones <=
 * IQA_TONES_MAX_TONES.  Precondition: |u| < 2^20 (iqa_tones_decimate's output is): then |I| < 2^41, E < 2^59. */
int iqa_tones_bank(const void *u_dev, int64_t m, int32_t frame, int32_t hop, int32_t ntones, const void *taps_dev,
                   void *e_out_dev, void *p_out_dev, void *stream);
/* One byte per frame of each bank; IQA_TONES_NONE where the frame carries nothing.  e_ctcss_dev:
 * int64[frames_ctcss][IQA_TONES_CTCSS]; e_dtmf_dev: int64[frames_dtmf][IQA_TONES_DTMF]; p_dev: int64[frames_dtmf];
 * frame_dtmf: the DTMF bank's frame length; ctcss_out_dev: uint8[frames_ctcss]; dtmf_out_dev: uint8[frames_dtmf].
 * CTCSS: k = the lowest index of the maximum, med = the 25th smallest of the 50 energies; the code is k iff
 * (E[k] >> 6) >= med and E[k] >= 2^16.  DTMF: r, c = the lowest indices of the maxima of E[0 .. 3] and E[4 .. 7], r2, c2 the
 * largest of the other three of each group; the code is 4 r + c iff E_r >= 8 r2, E_c >= 8 c2, E_c <= 16 E_r,
 * E_r <= 16 E_c, E_r >= 2^16, E_c >= 2^16 and 1024 (E_r + E_c) >= frame_dtmf P.  All in int64.
 * Precondition: 0 <= E < 2^59 for CTCSS; 0 <= E < 2^52 and 0 <= frame_dtmf P < 2^63 for DTMF (iqa_tones_bank's outputs
 * with frame_dtmf <= 320 are).  A plane with no frames may be NULL. */
int iqa_tones_decide(const void *e_ctcss_dev, int64_t frames_ctcss, const void *e_dtmf_dev, const void *p_dev,
                     int64_t frames_dtmf, int32_t frame_dtmf, void *ctcss_out_dev, void *dtmf_out_dev, void *stream);

/* ------------------------------------------------------------------------- *
 * ACARS beside the AM demodulator (--demod am --acars) *
 * ------------------------------------------------------------------------- */

/* A channel needs 8 <= fs / 2400 <= IQA_ACARS_MAX_SPS; the correlator window W = rint(fs / 1800) is then at most 533. */
#define IQA_ACARS_MAX_SPS 400
#define IQA_ACARS_MAX_WINDOW 536
#define IQA_ACARS_PHASES 8        /* sampling phases per bit */
#define IQA_ACARS_SLOT_BYTES 244  /* one kept block's bytes in the list: 13 .. 240 up to ETX / ETB, and the two check bytes */
/* The largest value of a run's stored envelope.  e_dev: float32[n]; max_out_dev: float32[1], cleared by the call and then
 * raised to max e (0 for n = 0) by an unsigned atomic maximum of the bit patterns: exact, whatever the order.
 * Precondition: every e[i] is finite and >= 0 (iqa_envelope's output on finite input is); -0 counts as the largest value. */
int iqa_acars_max(const void *e_dev, int64_t n, void *max_out_dev, void *stream);
/* The quantiser, the 1800 Hz correlator and the one-bit differential detector over a whole run.  With W = window,
 * L = delay, everything zero in front of the stream:
 *   q[n] = rint(e[n] 2^shift) (int32, half-even; the scaling is exact);
 *   I[n] = (sum_{k<W} c[k] q[n-k]) >> 8, Q[n] = (sum_{k<W} s[k] q[n-k]) >> 8 (int32 sums, arithmetic shift);
 *   y[n] = cr (Q[n] I[n-L] - I[n] Q[n-L]) - sr (I[n] I[n-L] + Q[n] Q[n-L]) (int64);  same[n] = (y[n] > 0).
 * e_dev: float32[n]; taps_dev: int16[2][W] = c, s with c[k] = rint(256 cos(2 pi 1800 k / fs)), s[k] likewise with sin;
 * q_out_dev, i_out_dev, qq_out_dev (Q): int32[n] each or NULL; y_out_dev: int64[n] or NULL; same_out_dev: uint8[n].
 * 1 <= window <= IQA_ACARS_MAX_WINDOW, 8 <= delay <= IQA_ACARS_MAX_SPS, |cr|, |sr| <= 256.
 * Precondition: 0 <= q <= 2^15 everywhere, that is shift = 14 - floor(log2 max e) with iqa_acars_max's result (max e 2^shift
 * lies in [2^14, 2^15); rounding takes its last 2^-9 up to 2^15), and
 * |tap| <= 256: then a sum is at most 2^15 times a table's positive taps, below 2^31 for every window allowed here, and
 * |I|, |Q| < 2^23, |y| < 2^57.  The products are formed by the 24-bit multiply, which sign-extends its operands from bit
 * 23: outside the precondition I and Q differ from the formula above (nothing is read or written out of bounds). */
int iqa_acars_detect(const void *e_dev, int64_t n, int32_t shift, int32_t window, int32_t delay, const void *taps_dev,
                     int32_t cr, int32_t sr, void *q_out_dev, void *i_out_dev, void *qq_out_dev, void *y_out_dev,
                     void *same_out_dev, void *stream);
/* The 8 transition-symbol streams of a whole run.  same_dev: uint8[n]; step = sps / 8 (float64, made once by the caller).
 * Phase p, symbol i = 0 .. nbits - 1: instant n_i = window - 1 + rint((8 i + p) step) (one float64 product, one rint,
 * half-even); bits[p][i] = same[n_i]; 0 where n_i >= n (the symbol does not exist).  bits_out_dev: uint8[8][nbits]. */
int iqa_acars_bits(const void *same_dev, int64_t n, int32_t window, double step, int64_t nbits, void *bits_out_dev, void *stream);
/* ACARS blocks of the 8 symbol streams.  bits_dev: uint8[8][nbits]; count_of: HOST int64[8], the number of symbols of phase
 * p that exist (<= nbits).  In phase p (g = bits[p], nb = count_of[p]) position s, 31 <= s <= nb, opens a candidate iff
 * g[s-31 .. s-1] are the 31 transitions (1: a bit equals the one before it) inside the 32 bits of 2A 16 16 01, each byte
 * least significant bit first.  With the bit in front of s a zero, bit i = bit i-1 xor !g[i]; bits are collected least
 * significant first into bytes up to the first byte whose low 7 bits are 03 or 17 (ETX, ETB); a 240th byte that is neither
 * aborts, so does the end of the stream.  A candidate that reached ETX / ETB is counted in counts[1].  It is kept iff the two
 * bytes behind it exist, equal the CRC-16/KERMIT (reflected 0x8408, init 0, no final xor) of the bytes up to and including
 * ETX / ETB, low byte first, and those are at least 13.  Kept blocks are appended in any order: list_dev: int64[4 capacity]
 * = (p, s, start instant n_s, byte count with the two check bytes) each, slots_dev: uint8[capacity][IQA_ACARS_SLOT_BYTES] =
 * the bytes, zero-filled.  counts_dev: int64[2], zeroed by the call; counts[0] counts ALL kept blocks: a count above
 * capacity means the list is incomplete and the call must be repeated with a larger one. */
int iqa_acars_frames(const void *bits_dev, int64_t nbits, const int64_t count_of[IQA_ACARS_PHASES], int32_t window, double step,
                     void *list_dev, void *slots_dev, int64_t capacity, void *counts_dev, void *stream);

/* ------------------------------------------------------------------------- *
 * AIS beside the NFM demodulator (--demod nfm --ais) *
 * ------------------------------------------------------------------------- */

/* A channel needs 5 <= fs / 9600 <= IQA_AIS_MAX_SPS; with L = rint(fs / 9600) the pulse filter has W = 3 L - 1 <= 299 taps,
 * and 12 868 . 256 . 299 stays inside int32. */
#define IQA_AIS_MAX_SPS 100
#define IQA_AIS_PHASES 8        /* sampling phases per bit */
#define IQA_AIS_SLOT_BYTES 128  /* one kept frame's bytes in the list (a frame has 11 .. 128, FCS included: five slots) */
/* One block of the quantiser and the pulse filter.  With W = window:
 *   t[n] = rint(theta[n] 4096) (int32, half-even);
 *   S[n] = sum_{k<W} taps[k] t[n-k] (int32).
 * theta_dev: float32[n] (iqa_quadrature's output); hist_dev: int32[W - 1], the values of t in front of theta[0], oldest
 * first (NULL: zeros); taps_dev: int16[W], |tap| <= 256 (dsp_plan.plan_ais: a Gaussian of BT 0.4 over 2 L taps convolved
 * with L ones, scaled to a peak of 256); t_out_dev: int32[n], or NULL (not stored); s_out_dev: int32[n].
 * 1 <= window <= 3 IQA_AIS_MAX_SPS - 1.  Integer sums: the outputs do not depend on how a stream is cut into blocks.
 * Precondition: |t| < 2^23 everywhere, that is |theta[n]| < 2048 rad (a discriminator output has |theta| <= pi, |t| <= 12 868)
 * and |hist_dev[i]| < 2^23, and 12 868 . sum |taps| < 2^31.  The products are formed by the 24-bit multiply, which
 * sign-extends its operands from bit 23: outside the precondition S differs from the formula above. */
int iqa_ais_filter(const void *theta_dev, int64_t n, const void *hist_dev, int32_t window, const void *taps_dev, void *t_out_dev,
                   void *s_out_dev, void *stream);
/* The 8 symbol planes of a whole run.  s_dev: int32[n] (the run's S); step = sps / 8 (float64, made once by the caller).
 * Phase p, symbol i = 0 .. nsym - 1: instant n_i = window - 1 + rint((8 i + p) step) (one float64 product, one rint,
 * half-even); v[p][i] = S[n_i]; 0 where n_i >= n (the symbol does not exist).  v_out_dev: int32[8][nsym]. */
int iqa_ais_symbols(const void *s_dev, int64_t n, int32_t window, double step, int64_t nsym, void *v_out_dev, void *stream);
/* HDLC frames of the 8 symbol planes.  v_dev: int32[8][nsym]; count_of: HOST int64[8], the number of symbols of phase p that
 * exist (<= nsym).  In phase p (v = v[p], nb = count_of[p]) position s, 24 <= s <= nb, has the level sum
 * v[s-24] + .. + v[s-9] (int64, sixteen training symbols); under it m_i = (16 v_i > sum) and b_i = (m_i == m_{i-1}).  s opens a
 * candidate iff b[s-8 .. s-1] = 0,1,1,1,1,1,1,0 and the fourteen bits b[s-22 .. s-9] alternate (either way round).  From s,
 * under the same sum, bits are collected least significant first into bytes; a 0 after five consecutive 1s is dropped; the
 * sixth consecutive 1 ends the walk: a closing flag iff the next bit exists and is 0 and exactly 6 bits of the current byte
 * are collected, an abort otherwise; a 129th byte aborts; so does the end of the stream.  A closed candidate of >= 11 bytes
 * is counted in counts[1]; it is kept iff the CRC-16/X.25 (reflected 0x8408, init 0xFFFF, final xor 0xFFFF) of all but its
 * last two bytes equals them, low byte first.  Kept frames are appended in any order: list_dev: int64[4 capacity] = (p, s,
 * start instant n_s, byte count) each, slots_dev: uint8[capacity][IQA_AIS_SLOT_BYTES] = the bytes, zero-filled.
 * counts_dev: int64[2], zeroed by the call; counts[0] counts ALL kept frames: a count above capacity means the list is
 * incomplete and the call must be repeated with a larger one. */
int iqa_ais_frames(const void *v_dev, int64_t nsym, const int64_t count_of[IQA_AIS_PHASES], int32_t window, double step,
                   void *list_dev, void *slots_dev, int64_t capacity, void *counts_dev, void *stream);

/* ------------------------------------------------------------------------------------- *
 * ADS-B / Mode S squitters beside the AM demodulator (--demod am --adsb) *
 * ------------------------------------------------------------------------------------- */

/* A channel needs 2 <= fs / 1e6 <= IQA_ADSB_MAX_SPS samples per microsecond. */
#define IQA_ADSB_MAX_SPS 20
#define IQA_ADSB_CHIPS 240       /* half-microsecond chips of a long squitter: 16 of the preamble, 224 of 112 bits */
#define IQA_ADSB_MAX_SPAN 2400   /* samples a candidate position reads: o[239] + h <= 240 * 10 */
#define IQA_ADSB_TILE 2048       /* candidate positions of one workgroup of iqa_adsb_search */
#define IQA_ADSB_SLOT_BYTES 14   /* one kept frame's bytes in the list; a 56-bit frame is zero-padded */
/* The quantiser of one block.  e_dev: float32[n] (an envelope: >= 0, or NaN / +inf); q_out_dev: uint16[n].
 * x = e 65536 (float32, exact); q = 65535 unless x < 65535, else rint(x) half-even; NaN and +inf give 65535.  A negative e
 * is outside the precondition and gives 0. */
int iqa_adsb_quantise(const void *e_dev, int64_t n, void *q_out_dev, void *stream);
/* The squitter search over a whole run's q plane.  q_dev: uint16[n]; offsets_dev: int32[IQA_ADSB_CHIPS], o[0] = 0,
 * ascending, o[k] + h <= span; 1 <= h <= IQA_ADSB_MAX_SPS / 2; span <= IQA_ADSB_MAX_SPAN (checked on the HOST copy
 * offsets_host, which must hold the same 240 values).  Chip k at position p: C_k(p) = sum_{j<h} q[p + o[k] + j] (int32).
 * Every p with p + span <= n is a candidate position.  It passes the preamble rule iff, with P = C0 + C2 + C7 + C9,
 * C0 > C1, C2 > C1, C2 > C3, C7 > C6, C7 > C8, C9 > C8, C9 > C10 and 6 C_j < P for j = 4, 5, 11, 12, 13, 14 (all strict).
 * Bit i = (C_{16+2i} > C_{17+2i}), i < 112; DF = bits 0 .. 4 MSB first; nbits = 112 for DF >= 16, else 56; the syndrome is
 * the remainder of the first nbits bits under the generator 0x1FFF409.  A passing position with DF 11, 17 or 18 and
 * syndrome 0 is kept, in any order: list_dev: int64[3 capacity] = (p, nbits, P) each; slots_dev:
 * uint8[capacity][IQA_ADSB_SLOT_BYTES] = the bits MSB first, zero behind nbits.  flags_out_dev: uint8[n - span + 1] or NULL:
 * 1 where the position passes the preamble rule.  counts_dev: int64[2], zeroed by the call: counts[0] counts ALL kept
 * frames (a count above capacity means the list is incomplete and the call must be repeated with a larger one), counts[1]
 * the positions that pass the preamble rule.  n < span: nothing is launched. */
int iqa_adsb_search(const void *q_dev, int64_t n, const void *offsets_dev, const int32_t *offsets_host, int32_t h, int32_t span,
                    void *flags_out_dev, void *list_dev, void *slots_dev, int64_t capacity, void *counts_dev, void *stream);

/* Audio egress (the drain of AudioWriter, processing.py:433-438, without a host thread): copy nbytes from device
 * memory into MAPPED pinned host memory (hipHostMalloc / torch pin_memory) with `workgroups` small workgroups
 * (<= 0: 8), so that the copy can run beside a kernel that occupies every CU.  Both pointers 16-byte aligned. */
int iqa_trickle_copy(const void *src_dev, void *dst_mapped, int64_t nbytes, int32_t workgroups, void *stream);

/* float32 capture -> int16 copy when, and only when, every value is k / 32768 with k an integer in [-32768, 32767]
 * (what SDR software writes for int16 / 12-bit / int8 ADC samples): s16_out[i] = x[i] * 32768, and *flag_dev (int32,
 * zeroed by the caller) is OR-ed with 1 if any value is NOT of that form -- the copy is then not the capture.  Lets
 * cf32 captures that are integer captures in disguise take the matrix-core channelizers (ingest: IQReader._extract_iq,
 * processing.py:268-279, with ffmpeg's f32le -> float being the identity).  n_values == 0 does nothing.  f32_dev 16-byte
 * aligned, s16_out_dev 8-byte aligned. */
int iqa_f32_to_s16_exact(const void *f32_dev, int64_t n_values, void *s16_out_dev, void *flag_dev, void *stream);

/* A float32 capture as TWO int16 planes, x = 2^shift (hi + lo / 32768) / 32768 (hi = rint(2^(15-shift) x), |lo| <= 16384),
 * exact to 2^(shift-31) of full scale: the linear channel filter then gives z = 2^shift (z(hi) + 2^-15 z(lo)) from two
 * passes of the int16 matrix-core channelizers -- a float capture that is NOT on the 2^-15 grid (RTL-SDR's
 * (u - 127.5) / 127.5, k / 32767, resampled recordings) leaves the float32 VALU kernel too.  shift: headroom in bits,
 * 0..15 (the caller picks it from the warm-up block's largest value).  A value fits when rint(2^(15-shift) x), rounded
 * half to even in float32, lies in [-32768, 32767]: at shift 0 that accepts [-32768.5, 32767.5) / 32768 -- 1 - 2^-16
 * itself rounds to 32768 and does NOT fit, -32768.5 / 32768 rounds to -32768 and does.
 * *flag_dev (int32, caller-zeroed) |= 1 when a value does not fit or is a NaN (the planes are then not the capture; hi
 * and lo of such a value are clamped and meaningless), |= 2 when some lo != 0 (otherwise hi alone IS the capture:
 * iqa_f32_to_s16_exact's case at shift 0).  n_values == 0 does nothing.  f32_dev 16-byte aligned, outputs 8-byte
 * aligned, n_values each.
 * ref: the float32 ingest of IQReader (ffmpeg hands the reference everything as f32le, processing.py:113-158, 268-279;
 * input_formats.py:62-64, 86-91). */
int iqa_f32_split_s16(const void *f32_dev, int64_t n_values, int32_t shift, void *hi_out_dev, void *lo_out_dev, void *flag_dev,
                      void *stream);

/* ------------------------------------------------------------------------- *
 * Spectrum / waterfall                                   *
 * ------------------------------------------------------------------------- */

/* ref: spectrum.py _SlidingFFT.psd :143-171, compute_psd :15-45, the frame loop of streaming_waterfall :58-93.
 * For f in [0, n_frames): frame = samples[first + f*hop : ... + use] (fmt / iq_order as in iqa_oscillator_mix),
 *   X = FFT_nfft(complex128(frame) * window[0:use], zero-padded to nfft)          (rocFFT, double complex)
 *   psd_db[f][k] = 10*log10(|X[(k - nfft/2) mod nfft]|^2 / scale + 1e-18)           (fftshift-ed, dB)
 * window_dev = double[use] (np.hanning(use)); scale = use*sample_rate*win_power + 1e-18 (spectrum.py:39,167).
 * work_dev = double2[n_frames*nfft] scratch.  Outputs, each optional (NULL): psd_db_dev double[n_frames][nfft],
 * psd_db_f32_dev float[n_frames][nfft] (the waterfall's slices, spectrum.py:181), sum_db_dev double[nfft]
 * += sum over the batch's frames (the averaged PSD accumulates dB values, spectrum.py:79-82).
 * FFT plans are cached inside the library per (nfft, n_frames). */
int iqa_psd_frames(int32_t fmt, int32_t iq_order, const void *samples_dev, int64_t n_samples, int64_t first,
                   int64_t hop, int32_t n_frames, int32_t nfft, int32_t use, const void *window_dev, double scale,
                   void *work_dev, void *psd_db_dev, void *psd_db_f32_dev, void *sum_db_dev, void *stream);

/* ref: _WaterfallAggregator._maybe_reduce, spectrum.py:190-208.  out[r] = float32((double(in[2r]) + double(in[2r+1]))/2),
 * an odd last row is copied; out_dev (ceil(n_rows/2) rows) must not alias rows_dev. */
int iqa_pair_average_rows(const void *rows_dev, int32_t n_rows, int32_t n_cols, void *out_dev, void *stream);

/* ------------------------------------------------------------------------- *
 * The occupied channels of a capture (--find-channels)  *
 * ------------------------------------------------------------------------- */

/* The finder works on the float32 dB rows of iqa_psd_frames (psd_db_f32_dev), frame f of the run at sample f hop, F frames
 * in all, cut into n_slices = ceil(F / slice_frames) slices of slice_frames frames (the last one may be shorter).  Behind
 * the quantiser every value is an integer in centi-dB, so the results do not depend on how the frames are cut into calls.
 * All planes are int32[nbins] with values inside +-2^28 (the finder's own lie within +-30000). */
#define IQA_FIND_MAX_HALF 8191            /* bins on either side in the window of the local floor */
#define IQA_FIND_MAX_GAP 255              /* cold bins between two hot ones that can be closed */
#define IQA_FIND_MAX_SLICE_FRAMES 65536   /* frames of one slice: its int32 sums cannot overflow */
#define IQA_FIND_C_MIN (-30000)           /* the quantiser's range is IQA_FIND_C_MIN .. -IQA_FIND_C_MIN centi-dB */
/* One batch of rows.  rows_dev: float32[n_frames][nbins], rows_dev[0] being frame first_frame of the run;
 * c = clamp(rint(100.0f row), -30000, 30000) (one float32 product, half-even; NaN reads as -30000, +-inf as the ends).
 * sum_dev: int64[nbins] += c; max_dev: int32[nbins] = max(itself, c) (the caller fills it with IQA_FIND_C_MIN before the
 * first batch and zeroes the other two); slice_dev: int32[n_slices][nbins], row (first_frame + f) / slice_frames += c.
 * first_frame + n_frames <= n_slices slice_frames.  c_out_dev: int16[n_frames][nbins] or NULL: c itself. */
int iqa_find_accumulate(const void *rows_dev, int32_t n_frames, int32_t nbins, int64_t first_frame, int32_t slice_frames,
                        int32_t n_slices, void *sum_dev, void *max_dev, void *slice_dev, void *c_out_dev, void *stream);
/* mean_out_dev: int32[nbins] = floor(sum_dev[k] / frames) (floor division of int64; frames >= 1). */
int iqa_find_mean(const void *sum_dev, int32_t nbins, int64_t frames, void *mean_out_dev, void *stream);
/* The local floor of a plane: floor_out_dev[k] = the value of rank ((hi - lo) num) / den (0-based, ascending) among
 * plane_dev[lo .. hi], lo = max(0, k - half), hi = min(nbins - 1, k + half).  0 <= half <= IQA_FIND_MAX_HALF,
 * 0 <= num <= den <= 65536.  The plane's values must lie inside int16 (they are read as halfwords; anything outside is
 * clamped to -32768 / 32767 first). */
int iqa_find_floor(const void *plane_dev, int32_t nbins, int32_t half, int32_t num, int32_t den, void *floor_out_dev, void *stream);
/* x_out_dev: int32[nbins] = max(mean - fmean - thr, max - fmax - thr_peak).  A bin is hot iff x >= 0 and
 * |k - dc_bin| > dc_guard (a negative dc_guard: no guard), and closed iff it is hot or lies between two hot bins a < k < b
 * with b - a - 1 <= gap (0 <= gap <= IQA_FIND_MAX_GAP).  mask_out_dev: uint8[nbins], bit 0 = hot, bit 1 = closed.  The
 * thresholds lie inside +-2^20. */
int iqa_find_mask(const void *mean_dev, const void *fmean_dev, const void *max_dev, const void *fmax_dev, int32_t nbins, int32_t thr,
                  int32_t thr_peak, int32_t gap, int32_t dc_bin, int32_t dc_guard, void *x_out_dev, void *mask_out_dev, void *stream);
/* A run is a maximal stretch [lo, hi] of closed bins of mask_dev.  Its record is int64[8]: lo, hi, its hot bins, the lowest
 * index of the maximum of e = mean - fmean, e there, sum w and sum w (k - lo) with w = max(e, 0), max_k (max - fmax).  Runs
 * with at least min_hot (>= 1) hot bins are kept, appended in any order to list_dev: int64[capacity][8].  counts_dev:
 * int64[2], zeroed by the call: counts[0] counts ALL kept runs (a count above capacity means the list is incomplete and the
 * call must be repeated with a larger one; nothing is written behind entry capacity - 1), counts[1] every run. */
int iqa_find_runs(const void *mean_dev, const void *fmean_dev, const void *max_dev, const void *fmax_dev, const void *mask_dev,
                  int32_t nbins, int32_t min_hot, void *list_dev, int64_t capacity, void *counts_dev, void *stream);
/* on_out_dev: uint8[n_runs][n_slices]: run j (record j of list_dev, of which lo and hi are read) is on in slice s iff
 * sum_{k = lo .. hi} (slice[s][k] - T_s fmean[k]) >= T_s (hi - lo + 1) thr_act in int64, T_s = min(slice_frames,
 * frames - s slice_frames).  n_slices = ceil(frames / slice_frames); a record with lo < 0, hi >= nbins or lo > hi reads
 * nothing and is off. */
int iqa_find_activity(const void *slice_dev, const void *fmean_dev, const void *list_dev, int64_t n_runs, int32_t nbins,
                      int64_t frames, int32_t slice_frames, int32_t n_slices, int32_t thr_act, void *on_out_dev, void *stream);

/* ------------------------------------------------------------------------- *
 * What a found channel is (--find-describe)            *
 * ------------------------------------------------------------------------- */

#define IQA_DESCRIBE_MAX_SHIFT 30   /* |sh| of the quantiser */
/* Rows of iqa_describe_accumulate for n samples: ceil(n / 2048), 0 for n <= 0. */
int64_t iqa_describe_tiles(int64_t n);
/* Eight integer sums of a channel's baseband.  z_dev: complex64[n], z_dev[0] being sample pos of the channel stream (decimation
 * D, filter delay `delay` raw frames).  q = clamp(rintf(ldexpf(x, sh)), -32767, 32767) per component (float32, half-even; NaN
 * reads as 0, +-inf as +-32767).  Sample m counts iff gate_dev[s] != 0 (uint8[S]) with s = min(max(m D - delay, 0) / hop,
 * F - 1) / T in int64; hop, T, F and S = ceil(F / T) are the find plan's.  With p = qi^2 + qq^2 and, against the sample in
 * front, cr = qi qi' + qq qq', ci = qq qi' - qi qq', a = floor(sqrt(p p')), every tile of 2048 consecutive samples of the
 * call writes one row of partials_dev (int64[iqa_describe_tiles(n)][8]): the gated samples, the pairs whose two samples are
 * both gated, sum p, sum (p >> 8)^2, sum floor(sqrt(p)) over the gated samples, sum cr, sum ci, sum a over those pairs.
 * prev_dev: complex64[1], the sample in front of z_dev[0], or NULL (sample 0 of the call then forms no pair; required at
 * pos 0).  Exact integers: the rows' sums do not depend on how the stream is cut into calls.  (pos + n) D < 2^62.
 * n = 0 returns IQA_OK and touches no pointer. */
int iqa_describe_accumulate(const void *z_dev, int64_t n, int64_t pos, const void *prev_dev, int32_t sh, int32_t D, int32_t delay,
                            int32_t hop, int32_t T, int64_t F, int32_t S, const void *gate_dev, void *partials_dev, void *stream);

/* ------------------------------------------------------------------------- *
 * Whether a found channel is keyed (--find-decode)     *
 * ------------------------------------------------------------------------- */

#define IQA_KEYING_BAUDS 7     /* candidate symbol rates: 512, 1200, 1600, 2400, 3200, 4800, 9600 */
#define IQA_KEYING_SUMS 16     /* int32 values of a row: P, K, then (C_k, Q_k) per candidate */
/* Rows of iqa_keying_accumulate for the samples pos .. pos + n - 1: (pos + n - 1) / 2048 - pos / 2048 + 1, one per window
 * w = m / 2048 of the absolute position that the call touches; 0 for n <= 0. */
int64_t iqa_keying_windows(int64_t pos, int64_t n);
/* The coherence of a discriminator's level crossings with a symbol clock, as exact integer sums.  theta_dev: float32[n]
 * (iqa_quadrature's output of the channel stream, decimation D, filter delay `delay` raw frames), theta_dev[0] being sample
 * pos.  t = clamp(rintf(theta 4096), -32767, 32767) (float32, half-even; NaN reads as 0, +-inf as +-32767); s = (t >= c), c
 * the centre, |c| <= 32767.  gate(m) is iqa_describe_accumulate's: gate_dev[s] != 0 (uint8[S]) with s = min(max(m D - delay,
 * 0) / hop, F - 1) / T in int64; hop, T, F and S = ceil(F / T) are the find plan's.  Sample m >= 1 is a pair iff gate(m) and
 * gate(m - 1), and a crossing iff it is a pair and s[m] != s[m - 1].  front_dev: float32[1], the theta in front of
 * theta_dev[0], or NULL (sample 0 of the call then forms no pair; required at pos 0).  inc: IQA_KEYING_BAUDS clock steps on
 * the host, inc_k = rint(B_k 2^32 / fs_ch), 0 <= inc_k < 2^30 (0: a skipped candidate).  A crossing at m adds
 * cs[((uint64(m) inc_k) mod 2^32) >> 22] to candidate k, cs_dev: int16[1024][2] = (rint(1024 cos(2 pi i / 1024)),
 * rint(1024 sin(2 pi i / 1024))), 4-byte aligned.  Every window the call touches writes one row of rows_dev
 * (int32[iqa_keying_windows(pos, n)][16]): P (pairs), K (crossings), then (C_k, Q_k) = the sums of cs over the crossings;
 * |C_k| <= 2048 * 1024.  A window cut by two calls gets a partial row from each: the host adds the rows of one window number
 * before it squares anything, so nothing depends on how the stream is cut into calls.  (pos + n) D < 2^62.  n = 0 returns
 * IQA_OK and touches no pointer. */
int iqa_keying_accumulate(const void *theta_dev, int64_t n, int64_t pos, const void *front_dev, int32_t c, const int32_t *inc,
                          const void *cs_dev, int32_t D, int32_t delay, int32_t hop, int32_t T, int64_t F, int32_t S,
                          const void *gate_dev, void *rows_dev, void *stream);

/* ------------------------------------------------------------------------- *
 * The protocol of a keyed channel (--find-identify)    *
 * ------------------------------------------------------------------------- */

#define IQA_IDENT_MIN_SPS 4        /* samples to a symbol, and the integrator's window L = rint(sps) */
#define IQA_IDENT_MAX_SPS 224
#define IQA_IDENT_OFFSETS 64       /* o[i] = rint(i sps), i = -16 .. 47, o[i] at index 16 + i */
#define IQA_IDENT_MAX_SYMBOLS 32   /* symbols of a sync pattern */
#define IQA_IDENT_MAX_PATTERNS 8   /* patterns of one search */
#define IQA_IDENT_RECORD 6         /* int64 values of a kept hit: pattern, m, C, E, pre, post */
/* The symbol-long integrator of a stored discriminator stream.  theta_dev: float32[n], index 0 the first stored sample; in
 * front of it t - c reads as 0.  t = clamp(rintf(theta 4096), -32767, 32767) (float32, half-even; NaN reads as 0, +-inf as
 * +-32767); S[m] = sum over j < L, j <= m of (t[m - j] - c) in int32, c the centre, |c| <= 32767; v_dev[m] = S[m] >> sh
 * (int32[n], an arithmetic shift).  IQA_IDENT_MIN_SPS <= L <= IQA_IDENT_MAX_SPS, 0 <= sh <= 8 with (L 65534) >> sh <=
 * 64 * 65534, so |v| <= 64 * 65534.  n <= 2^30.  n = 0 returns IQA_OK and touches no pointer. */
int iqa_ident_integrate(const void *theta_dev, int64_t n, int32_t L, int32_t sh, int32_t c, void *v_dev, void *stream);
/* The frame synchronisation words of one family in v_dev (int32[n], |v| <= 64 * 65534: iqa_ident_integrate's output).
 * offsets (host): IQA_IDENT_OFFSETS sample offsets o[-16] .. o[47], ascending in steps of at most IQA_IDENT_MAX_SPS + 1, o[0]
 * (index 16) = 0.  symbols (host): int8[npat][IQA_IDENT_MAX_SYMBOLS], pattern p's first nsym[p] entries each -3, -1, +1 or
 * +3; 1 <= npat <= IQA_IDENT_MAX_PATTERNS, 1 <= nsym[p] <= IQA_IDENT_MAX_SYMBOLS, o[nsym[p] - 1] <= 31 IQA_IDENT_MAX_SPS.
 * At every m with m + o[N - 1] < n: C = sum p_i v[m + o[i]], E = sum v[m + o[i]]^2 (int64), Pn = sum p_i^2; m is a candidate
 * of p iff E > 0 and 16 C^2 >= 13 Pn E.  score_dev (int32[npat][n]) receives 2 |C| + (C < 0) for a candidate and 0 for every
 * other m.  A candidate is kept iff no candidate of the same pattern within +-half has a larger |C|, or the same |C| at a
 * smaller index (0 <= half <= IQA_IDENT_MAX_SPS).  A kept hit appends IQA_IDENT_RECORD int64 to list_dev
 * (int64[capacity][6]) in no particular order: p, m, C, E, pre, post; bit k of pre = (v[m + o[-16 + k]] > 0) and of post =
 * (v[m + o[N + k]] > 0), k = 0 .. 15, 0 where the position lies outside 0 .. n - 1.  count_dev (int64[1]) is cleared and
 * then counts every kept hit, also those past the capacity: a caller that reads count > capacity repeats the call with
 * room for all.  n <= 2^30.  n = 0 returns IQA_OK and touches no pointer (the count stays as it is). */
int iqa_ident_search(const void *v_dev, int64_t n, const int32_t offsets[IQA_IDENT_OFFSETS], int32_t npat, const int8_t *symbols,
                     const int32_t *nsym, int32_t half, void *score_dev, void *list_dev, int64_t capacity, void *count_dev,
                     void *stream);

/* ------------------------------------------------------------------------- *
 * The pages of a FLEX channel (--find-flex)            *
 * ------------------------------------------------------------------------- */

#define IQA_FLEX_HEADER_OFFSETS 112 /* o16[i] = rint(i sps), i = -16 .. 95, o16[i] at index 16 + i */
#define IQA_FLEX_BLOCKS 11          /* data blocks of a frame */
#define IQA_FLEX_SHIFTS 5           /* timing shifts of a block: (e - 2) step, e = 0 .. 4 */
#define IQA_FLEX_PHASES 4           /* A, B, C, D */
#define IQA_FLEX_WORDS 88           /* words of a phase in a frame */
#define IQA_FLEX_SYMBOLS 2816       /* data symbols of a frame at 1600 symbols/s; twice as many at 3200 */
#define IQA_FLEX_MAX_STEP 28        /* floor(IQA_IDENT_MAX_SPS / 8) */
/* The levels and the frame information word of K sync-1 hits.  plane_dev: int32[n], iqa_ident_integrate's output (|v| <=
 * 64 * 65534).  hits_dev: int64[K][2], (m, s): m where bit 0 of the marker 0xA6C6AAAA ends, s the sign of the hit (negative:
 * -1, else +1).  offsets16 (host): the IQA_FLEX_HEADER_OFFSETS sample offsets of the 1600 bit/s grid, ascending in steps of at
 * most IQA_IDENT_MAX_SPS + 1, o16[0] (index 16) = 0.  out_dev: int64[K][6] per hit: Sigma = sum of x_i = s plane[m + o16[i]]
 * over i = 0 .. 31; A = sum of p_i x_i, p_i the marker's bit i (MSB first) as +-1; the frame information word W as sliced, bit j
 * of it (32 s plane[m + o16[64 + j]] - Sigma > 0); W after the codeword rule; the status; the valid flag.  The codeword rule:
 * W with its bits reversed is a BCH(31,21) codeword of g = 0x769 with even parity over 32 bits; status 0 clean, 1 one bit
 * restored, 2 refused (the raw word kept), 3 an instant of bits 64 .. 95 outside 0 .. n - 1 (both words 0).  valid is 0, with
 * Sigma = A = 0 and status 3, where an instant of bits 0 .. 31 lies outside the stream.  n <= 2^30, K <= 2^20.  n = 0 or K = 0
 * returns IQA_OK and touches no pointer. */
int iqa_flex_frames(const void *plane_dev, int64_t n, const void *hits_dev, int64_t K,
                    const int32_t offsets16[IQA_FLEX_HEADER_OFFSETS], void *out_dev, void *stream);
/* The words of F frames of one mode at five timing shifts.  frames_dev: int64[F][4], (m, s, Sigma, A) of the plane read here.
 * levels 2 or 4; u = 1 (1600 symbols/s) or 2 (3200); offsets_dev: int32[IQA_FLEX_SYMBOLS u] on the device, data symbol q ending
 * at m + offsets[q]; 1 <= step <= IQA_FLEX_MAX_STEP.  At shift e = 0 .. 4 every instant moves by (e - 2) step.  y = s
 * plane[instant], d = 32 y - Sigma: bit_a = (d > 0), bit_b = (3 |d| < 2 A) (4 levels only).  With per = 256 u: block b = q / per,
 * r = q % per, k = r / u, pair = r % u; pair 0 feeds phase A with bit_a and phase B with bit_b, pair 1 phases C and D; bit k of
 * a block and phase is bit k / 8 of word 8 b + k % 8.  fixed_dev, raw_dev (uint32) and status_dev (uint8), each
 * [F][IQA_FLEX_SHIFTS][IQA_FLEX_PHASES][IQA_FLEX_WORDS]: the word after the codeword rule of iqa_flex_frames, as sliced, and
 * its status 0 .. 3 (3: an instant of the word outside 0 .. n - 1, both words 0); a phase that the mode does not send (B and D
 * at 2 levels, C and D at u = 1) reads 0, 0 and status 4.  Every instant is checked against 0 .. n - 1 before it is read.
 * n <= 2^30, F <= 2^20.  n = 0 or F = 0 returns IQA_OK and touches no pointer. */
int iqa_flex_words(const void *plane_dev, int64_t n, const void *frames_dev, int64_t F, int32_t levels, int32_t u, int32_t step,
                   const void *offsets_dev, void *fixed_dev, void *raw_dev, void *status_dev, void *stream);

/* ------------------------------------------------------------------------- *
 * The link control and calls of a DMR channel (--find-dmr) *
 * ------------------------------------------------------------------------- */

#define IQA_DMR_OFFSETS 144 /* o[i] = rint(i sps), i = -66 .. 77, o[i] at index 66 + i */
#define IQA_DMR_WORDS 9     /* uint32 words of a sliced burst: 24 CACH bits, then 264 burst bits */
#define IQA_DMR_RECORD 8    /* int32 values of a decoded burst */
/* The levels and the bits of K sync hits.  plane_dev: int32[n], iqa_ident_integrate's output at 4800 symbols/s (|v| <=
 * 64 * 65534).  hits_dev: int64[K][3], (m, s, kind): m where sync symbol 0 ends, s the sign of the hit (negative: -1, else +1),
 * kind 0 bs voice, 1 bs data, 2 ms voice, 3 ms data (its two low bits are read).  offsets (host): the IQA_DMR_OFFSETS sample
 * offsets of the symbols -66 .. 77, ascending in steps of at most IQA_IDENT_MAX_SPS + 1, o[0] (index 66) = 0.  The burst is
 * symbols -54 .. 77 and is valid iff all their instants lie in 0 .. n - 1; the CACH is symbols -66 .. -55 and is valid iff
 * the kind is a bs one and all its instants do.  Sigma = sum of x_i = plane[m + o[i]] over the sync symbols i = 0 .. 23; A = s
 * sum of sgn_i x_i, sgn_i the sign of symbol i of the bs (kinds 0, 1) or ms (kinds 2, 3) voice sync word.  A symbol at the
 * instant t reads as d = 24 plane[t] - Sigma: its first bit (d < 0), its second (3 |d| >= 2 A).  bits_dev: uint32[K][9], the 24
 * CACH bits then the 264 burst bits, the first sent bit the MSB of word 0; every bit of a burst that is not valid is 0, and so
 * are the CACH bits of a CACH that is not.  levels_dev: int64[K][3]: Sigma, A (both 0 for a burst that is not valid), flags (bit
 * 0 burst valid, bit 1 CACH valid).  Every instant is checked against 0 .. n - 1 before it is read.  n <= 2^30, K <= 2^20.
 * n = 0 or K = 0 returns IQA_OK and touches no pointer. */
int iqa_dmr_slice(const void *plane_dev, int64_t n, const void *hits_dev, int64_t K, const int32_t offsets[IQA_DMR_OFFSETS],
                  void *bits_dev, void *levels_dev, void *stream);
/* The TACT, the slot type and the BPTC(196,96) payload of K sliced bursts.  bits_dev: uint32[K][9] as iqa_dmr_slice writes
 * them; kinds_dev: uint8[K] (the two low bits are read).  info_dev: uint32[K][3], the 96 information bits, the first the MSB of
 * word 0 (0 where the payload is not read).  rec_dev: int32[K][8]: the TACT status (0 clean, 1 one bit restored, 4 an ms kind)
 * and nibble (AT, TC, LCSS1, LCSS0); the slot type's status (0 clean, 1 corrected at a distance of 1 .. 3, 2 refused with the
 * raw top byte kept, 4 a voice kind), distance and byte (colour code, data type); the payload's status (0 clean, 1 corrected,
 * 2 failed, 4 not read: a voice kind or a refused slot type), flips and rounds.  The codes are DESIGN.md section 29's.
 * K <= 2^20.  K = 0 returns IQA_OK and touches no pointer. */
int iqa_dmr_decode(const void *bits_dev, const void *kinds_dev, int64_t K, void *info_dev, void *rec_dev, void *stream);

/* ------------------------------------------------------------------------- *
 * NIDs, link control and TSBKs of a P25 phase 1 channel (--find-p25) *
 * ------------------------------------------------------------------------- */

#define IQA_P25_OFFSETS 864 /* o[i] = rint(i sps), i = 0 .. 863: the symbols of one LDU behind the end of sync symbol 0 */
#define IQA_P25_WORDS 54    /* uint32 words of a sliced frame: symbol i the frame bits 2 i, 2 i + 1 */
#define IQA_P25_INFO 9      /* uint32 words of a decoded frame's information */
#define IQA_P25_RECORD 8    /* int32 values of a decoded frame */
/* The levels and the bits of K frame sync hits.  plane_dev: int32[n], iqa_ident_integrate's output at 4800 symbols/s (|v| <=
 * 64 * 65534).  hits_dev: int64[K][2], (m, s): m where sync symbol 0 ends, s the sign of the hit (negative: -1, the same word
 * with the spectrum inverted; else +1).  offsets (host): the IQA_P25_OFFSETS sample offsets of the symbols 0 .. 863, ascending
 * in steps of at most IQA_IDENT_MAX_SPS + 1, o[0] = 0.  valid = 0 if m + o[0] < 0, else the number of i with m + o[i] < n.
 * With x_i = plane[m + o[i]], i = 0 .. 23, P = sum x_i and Q = sum sgn_i x_i (sgn_i the sign of sync symbol i): A = s (12 Q + P)
 * and Dc = 12 P + Q, 286 times the outer level and the DC; both 0 where valid < 24.  Symbol i < valid reads as d = s (286
 * plane[m + o[i]] - Dc): its first bit (d < 0), its second (3 |d| >= 2 A); every other bit is 0.  bits_dev: uint32[K][54], the
 * first sent bit the MSB of word 0.  levels_dev: int64[K][3]: A, Dc, valid.  Every instant is checked against 0 .. n - 1
 * before it is read.  n <= 2^30, K <= 2^20.  n = 0 or K = 0 returns IQA_OK and touches no pointer. */
int iqa_p25_slice(const void *plane_dev, int64_t n, const void *hits_dev, int64_t K, const int32_t offsets[IQA_P25_OFFSETS],
                  void *bits_dev, void *levels_dev, void *stream);
/* The network identifier of K sliced frames: the data bits 48 .. 111 (data dibit q is frame symbol q + q / 35), the first 63
 * against the 65 536 codewords of BCH(63,16,23).  nid_dev: int32[K][4]: status (0 clean, 1 corrected at a distance of 1 .. 11,
 * 2 refused with the raw top 16 bits kept), distance, value (NAC << 4 | DUID; on equal distance the smaller), parity_ok (the 64
 * bits have even weight).  K <= 2^20.  K = 0 returns IQA_OK and touches no pointer. */
int iqa_p25_nid(const void *bits_dev, int64_t K, void *nid_dev, void *stream);
/* What lies behind the NID of K sliced frames, by DUID (duids_dev: uint8[K], the four low bits are read): 0x5 the 24
 * Hamming(10,6,3) words of an LDU1's link control (class 1), 0xF the twelve Golay(24,12,8) words of a TDULC (class 2), 0x7 the
 * three rate 1/2 trellis blocks of a TSBK frame (class 3); any other DUID gives zeros (class 0).  info_dev: uint32[K][9]:
 * classes 1 and 2 the 144 link control bits in words 0 .. 4, class 3 the 96 bits of block b in words 3 b .. 3 b + 2, the first
 * bit the MSB.  rec_dev: int32[K][8]: the class, then for classes 1 and 2 the corrected words, the unmatched (Hamming) or
 * refused (Golay, distance over 3: the raw top 12 bits kept) words and the bits changed, for class 3 the three blocks' metrics
 * (channel bits changed); the rest 0.  The codes are DESIGN.md section 31's.  K <= 2^20.  K = 0 returns IQA_OK and touches no
 * pointer. */
int iqa_p25_decode(const void *bits_dev, const void *duids_dev, int64_t K, void *info_dev, void *rec_dev, void *stream);

/* ------------------------------------------------------------------------- *
 * FICH and data channels of a YSF (System Fusion) channel (--find-ysf) *
 * ------------------------------------------------------------------------- */

#define IQA_YSF_OFFSETS 480     /* o[i] = rint(i sps), i = 0 .. 479: the symbols of one frame behind the end of sync symbol 0 */
#define IQA_YSF_WORDS 30        /* uint32 words of a sliced frame: symbol i the frame bits 2 i, 2 i + 1 */
#define IQA_YSF_FICH_RECORD 5   /* int32 values of a decoded FICH */
#define IQA_YSF_INFO 12         /* uint32 words of a frame's decoded data channels: six to a block */
#define IQA_YSF_RECORD 4        /* int32 values of a frame's decoded data channels */
/* The levels and the bits of K frame sync hits.  plane_dev: int32[n], iqa_ident_integrate's output at 4800 symbols/s (|v| <=
 * 64 * 65534).  hits_dev: int64[K][2], (m, s): m where sync symbol 0 ends, s the sign of the hit (negative: -1, the same word
 * with the spectrum inverted; else +1).  offsets (host): the IQA_YSF_OFFSETS sample offsets of the symbols 0 .. 479, ascending
 * in steps of at most IQA_IDENT_MAX_SPS + 1, o[0] = 0.  valid = 0 if m + o[0] < 0, else the number of i with m + o[i] < n.
 * The sync word 0xD471C9634D holds inner levels (s_i in -3, -1, 1, 3; sum s_i = 12, sum s_i^2 = 124), so the levels are the
 * least squares fit of x_i = plane[m + o[i]], i = 0 .. 19, to Dc + L s s_i: with P = sum x_i and Q = sum s_i x_i,
 * Dc = 31 P - 3 Q and A = s (15 Q - 9 P), 584 times the DC and the outer level (3 L); both 0 where valid < 20.  Symbol
 * i < valid reads as d = s (584 plane[m + o[i]] - Dc): its first bit (d < 0), its second (3 |d| >= 2 A); every other bit is
 * 0.  bits_dev: uint32[K][30], the first sent bit the MSB of word 0.  levels_dev: int64[K][3]: A, Dc, valid.  Every instant
 * is checked against 0 .. n - 1 before it is read.  n <= 2^30, K <= 2^20.  n = 0 or K = 0 returns IQA_OK and touches no
 * pointer. */
int iqa_ysf_slice(const void *plane_dev, int64_t n, const void *hits_dev, int64_t K, const int32_t offsets[IQA_YSF_OFFSETS],
                  void *bits_dev, void *levels_dev, void *stream);
/* The frame information channel of K sliced frames: the 100 dibits of the frame bits 40 .. 239, coded dibit i the channel dibit
 * 20 (i mod 5) + i / 5, through the 16-state Viterbi decoder of the rate 1/2, K = 5 code (g1 = d + d3 + d4, g2 = d + d1 + d2 +
 * d4, g1 sent first; the trellis starts and ends in state 0; Hamming metric; on equal metrics the predecessor with the smaller
 * state index d1 d2 d3 d4 survives), then the four Golay(24,12,8) words of the 96 decoded bits against the 4096 codewords: a
 * word at a distance of 3 or less is corrected (on equal distance the smaller data value), else refused with its raw top 12
 * bits kept.  fich_dev: uint32[K][2]: the 48 data bits, word 0 the four FICH bytes, the top 16 bits of word 1 their CRC.
 * rec_dev: int32[K][5]: status (0 clean, 1 corrected, 2 a Golay word refused), the Viterbi metric (channel bits changed), the
 * Golay words corrected, refused, and the bits changed in the corrected ones.  K <= 2^20.  K = 0 returns IQA_OK and touches
 * no pointer. */
int iqa_ysf_fich(const void *bits_dev, int64_t K, void *fich_dev, void *rec_dev, void *stream);
/* The data channels (DCH) of K sliced frames, by class (classes_dev: uint8[K]); payload block p = 0 .. 4 is the frame bits
 * 240 + 144 p .. + 143.  Class 1 (header, terminator, data FR): DCH-a the first 72 bits of every block, DCH-b the 72 behind
 * them, 180 dibits each, coded dibit i the channel dibit 20 (i mod 9) + i / 9, each through iqa_ysf_fich's Viterbi decoder
 * to 176 bits and 4 tail bits.  Class 2 (V/D mode 1): DCH-a alone.  Class 3 (V/D mode 2): the first 40 bits of every block,
 * 100 dibits, coded dibit i the channel dibit 20 (i mod 5) + i / 5, to 96 bits and 4 tail bits.  Class 0 and every value over
 * 3: zeros.  info_dev: uint32[K][12]: DCH-a in words 0 .. 5, DCH-b in words 6 .. 11, the first bit the MSB of the block's
 * first word, zeros behind the block's bits.  rec_dev: int32[K][4]: the class (0 for a value over 3), the metric of DCH-a, of
 * DCH-b (channel bits changed; 0 where the block is not read), 0.  K <= 2^20.  K = 0 returns IQA_OK and touches no pointer. */
int iqa_ysf_decode(const void *bits_dev, const void *classes_dev, int64_t K, void *info_dev, void *rec_dev, void *stream);

/* ------------------------------------------------------------------------- *
 * LICH, SACCH, FACCH1 and CAC of an NXDN channel (--find-nxdn) *
 * ------------------------------------------------------------------------- */

#define IQA_NXDN_OFFSETS 192    /* o[i] = rint(i sps), i = 0 .. 191: the symbols of one frame behind the end of sync symbol 0 */
#define IQA_NXDN_WORDS 12       /* uint32 words of a sliced frame: symbol i the frame bits 2 i, 2 i + 1 */
#define IQA_NXDN_INFO 14        /* uint32 words of a frame's decoded blocks: SACCH 0 .. 1, FACCH1-a 2 .. 4, FACCH1-b 5 .. 7, CAC 8 .. 13 */
#define IQA_NXDN_RECORD 4       /* int32 values of a frame's decoded blocks */
#define IQA_NXDN_SACCH 1        /* the bits of a frame's class mask */
#define IQA_NXDN_FACCH1_A 2
#define IQA_NXDN_FACCH1_B 4
#define IQA_NXDN_CAC 8
/* The levels and the descrambled bits of K frame sync hits.  plane_dev: int32[n], iqa_ident_integrate's output at 4800 or 2400
 * symbols/s (|v| <= 64 * 65534).  hits_dev: int64[K][2], (m, s): m where sync symbol 0 ends, s the sign of the hit (negative:
 * -1, the same word with the spectrum inverted; else +1).  offsets (host): the IQA_NXDN_OFFSETS sample offsets of the symbols
 * 0 .. 191, ascending in steps of at most IQA_IDENT_MAX_SPS + 1, o[0] = 0.  valid = 0 if m + o[0] < 0, else the number of i
 * with m + o[i] < n.  The frame sync word 0xCDF59 holds inner levels (s_i in -3, -1, 1, 3; sum s_i = 0, sum s_i^2 = 74), so
 * the levels are the least squares fit of x_i = plane[m + o[i]], i = 0 .. 9: with P = sum x_i and Q = sum s_i x_i, Dc = 37 P
 * and A = s 15 Q, 370 times the DC and the outer level; both 0 where valid < 10.  Symbol i < valid reads as
 * d = s (370 plane[m + o[i]] - Dc): its first bit (d < 0), its second (3 |d| >= 2 A); from symbol 10 on the first bit is
 * inverted where the scrambler's bit is 1 (one bit per symbol, 0 0 1 0 0 1 1 1 0 and then b[k] = b[k - 5] ^ b[k - 9]); every
 * other bit is 0.  bits_dev: uint32[K][12], the first sent bit the MSB of word 0.  levels_dev: int64[K][3]: A, Dc, valid.
 * Every instant is checked against 0 .. n - 1 before it is read.  n <= 2^30, K <= 2^20.  n = 0 or K = 0 returns IQA_OK and
 * touches no pointer. */
int iqa_nxdn_slice(const void *plane_dev, int64_t n, const void *hits_dev, int64_t K, const int32_t offsets[IQA_NXDN_OFFSETS],
                   void *bits_dev, void *levels_dev, void *stream);
/* The blocks of K sliced frames, by class mask (classes_dev: uint8[K]): IQA_NXDN_SACCH the frame bits 36 .. 95 (36 steps,
 * coded bit j punctured where j mod 6 = 5, interleave 12 x 5), IQA_NXDN_FACCH1_A the bits 96 .. 239 and IQA_NXDN_FACCH1_B the
 * bits 240 .. 383 (96 steps, j mod 4 = 1, 9 x 16), IQA_NXDN_CAC alone the bits 36 .. 335 (175 steps, j mod 14 = 3 or 11,
 * 12 x 25); the p-th coded bit that is sent travels as channel bit C (p mod D) + p / D of its block.  Each block goes through
 * the 16-state Viterbi decoder of iqa_ysf_fich's code (g1 of step t the coded bit 2 t, g2 the bit 2 t + 1; the trellis starts
 * and ends in state 0; Hamming metric, a punctured bit counts 0 on every branch; on equal metrics the predecessor with the
 * smaller state index survives).  A mask over 15, or IQA_NXDN_CAC with another bit, reads nothing and is recorded as 0.
 * info_dev: uint32[K][14]: SACCH words 0 .. 1, FACCH1-a 2 .. 4, FACCH1-b 5 .. 7, CAC 8 .. 13, the first decoded bit the MSB of
 * the block's first word, zeros behind the block's bits and where nothing is read.  rec_dev: int32[K][4]: the mask, the metric
 * of the SACCH or the CAC, of FACCH1-a, of FACCH1-b (channel bits changed; 0 where the block is not read).  K <= 2^20.  K = 0
 * returns IQA_OK and touches no pointer. */
int iqa_nxdn_decode(const void *bits_dev, const void *classes_dev, int64_t K, void *info_dev, void *rec_dev, void *stream);

/* ------------------------------------------------------------------------- *
 * Carrier squelch of a run's targets (--squelch)       *
 * ------------------------------------------------------------------------- */

#define IQA_GATE_CELL 256              /* samples to a cell, counted on the absolute position */
#define IQA_GATE_MAX_SHIFT 30
#define IQA_GATE_MAX_FRAME (1 << 20)   /* samples to a frame (Lf), a multiple of IQA_GATE_CELL */
#define IQA_GATE_MAX_FRAMES (1 << 24)  /* frames of a run */
#define IQA_GATE_MAX_NUM 1024000       /* num_open = rint(1024 10^(open_db / 10)) at open_db = 30 */
/* Cells of iqa_gate_power for the samples pos .. pos + n - 1: (pos + n - 1) / 256 - pos / 256 + 1, one per cell c = m / 256
 * of the absolute position that the call touches; 0 for n <= 0. */
int64_t iqa_gate_cells(int64_t pos, int64_t n);
/* The power of a channel stream in integer cells.  z_dev: complex64[n], 8-byte aligned, z_dev[0] being sample pos.
 * q = clamp(rintf(ldexpf(x, sh)), -32767, 32767) per component (float32, half-even; NaN reads as 0, +-inf as +-32767),
 * |sh| <= IQA_GATE_MAX_SHIFT; p = qi^2 + qq^2 (< 2^31).  Every cell the call touches writes one entry of cells_dev
 * (int64[iqa_gate_cells(pos, n)]): the sum of p over the call's samples of the cell.  A cell cut by two calls gets a partial
 * sum from each; iqa_gate_add_cells adds them by cell number, so nothing depends on how the stream is cut into calls.
 * pos + n < 2^62.  n = 0 returns IQA_OK and touches no pointer. */
int iqa_gate_power(const void *z_dev, int64_t n, int64_t pos, int32_t sh, void *cells_dev, void *stream);
/* cells_dev[i] += part_dev[i], i < k (int64 each): a call's cells added to the run's at the call's first cell number. */
int iqa_gate_add_cells(const void *part_dev, int64_t k, void *cells_dev, void *stream);
/* From the cells of a stream of n samples (cells_dev: int64[ceil(n / 256)], added by cell number, each at most 256 (2^31 - 1))
 * to the state per frame, without a host round trip.  Lf: samples to a frame, a multiple of 256, <= IQA_GATE_MAX_FRAME;
 * F = max(1, n / Lf) <= IQA_GATE_MAX_FRAMES.  Frame f holds samples [f Lf, (f + 1) Lf), the last one runs to n.
 *   v_dev     int64[F]  16 E[f] / N[f], E the sum of the frame's cells and N its samples
 *   floor_dev int64[1]  max(1, the value of rank (F - 1) / 10 (0-based, ascending) among v)
 *   s_dev     uint8[F]  1 where 1024 v >= num_open floor, 0 where 1024 v < num_close floor, else s[f - 1] (s[-1] = 0)
 *   s2_dev    uint8[F]  s, without the runs of ones shorter than M frames
 *   g_dev     uint8[F]  1 iff some s2[f'] = 1 with max(0, f - H) <= f' <= min(F - 1, f + A)
 *   lo_dev, hi_dev int32[F]  (f0, f1 + 1) of the maximal run of ones [f0, f1] of g that holds f, or (-1, -1)
 * work_dev: int32[2 F].  1 <= num_close <= num_open <= IQA_GATE_MAX_NUM, M >= 1, H >= 0, A >= 0.  Three launches.  n = 0
 * returns IQA_OK and touches no pointer. */
int iqa_gate_decide(const void *cells_dev, int64_t n, int32_t Lf, int32_t F, int64_t num_open, int64_t num_close, int32_t M,
                    int32_t H, int32_t A, void *v_dev, void *floor_dev, void *s_dev, void *s2_dev, void *g_dev, void *lo_dev,
                    void *hi_dev, void *work_dev, void *stream);
/* The gated audio: for sample m, f = min(m / Lf, F - 1); out[m] = 0.0f where g[f] = 0, else audio[m] (k < R ? ramp[k] : 1.0f)
 * with k = min(m - lo[f] Lf, b - 1 - m) and b = hi[f] Lf, or n where hi[f] = F: one float32 multiply, the ramps inside the
 * transmission.  audio_dev, out_dev: float32[n], two buffers; ramp_dev: float32[R] (may be NULL at R = 0); g_dev, lo_dev,
 * hi_dev as iqa_gate_decide leaves them.  n = 0 returns IQA_OK and touches no pointer. */
int iqa_gate_apply(const void *audio_dev, int64_t n, int32_t Lf, int32_t F, const void *g_dev, const void *lo_dev,
                   const void *hi_dev, const void *ramp_dev, int32_t R, void *out_dev, void *stream);

/* ------------------------------------------------------------------------- *
 * Audio post-processing: automatic squelch (the reference's --audio-post)    *
 * ------------------------------------------------------------------------- */

/* ref: squelch.py apply_squelch :186-231 and its helpers :20-118, 164-183.  One call squelches a batch of files
 * ("segments"): every per-sample array of segment s lives in the workspace at samples [base, base + n), base a
 * multiple of IQA_SQ_TILE and ascending, so no workgroup straddles two files.  in_dev: float32 frames, segment s
 * interleaved [n][channels] at float offset in_off.  out_dev: same element offsets, float32 or (out_pcm16) int16 =
 * rint(y * 32767) saturated; segment s's result is the first (stop - start) * channels elements of its slot.
 * result_dev: iqa_squelch_result[n_segs].  segs (host) and segs_dev (device copy) hold the same table.
 * Percentiles (np.percentile, linear): the host gives each query's neighbouring order-statistic indices and the
 * float32 weight numpy computes (q_index[0..1] / q_gamma[0]: the noise floor; [2..3] / [1]: the 5th and [4..5] / [2]:
 * the 95th percentile of the adaptive score); the device selects those order statistics exactly and interpolates with
 * numpy's float32 _lerp.  Dilation reproduces the reference's int8 accumulation: a window count c sets a sample only
 * where (int8)(c mod 256) > 0.  Enqueues ~30 launches, no synchronisation. */
#define IQA_SQ_TILE 2048
typedef enum { IQA_SQ_ADAPTIVE = 0, IQA_SQ_STATIC = 1, IQA_SQ_TRANSIENT = 2 } iqa_sq_method;
typedef enum {
    IQA_SQ_STAGE_ENVELOPE_DB = 0, /* float32: _dbfs(_envelope(samples, window)) */
    IQA_SQ_STAGE_LEVEL = 1,       /* float32: adaptive: envelope - minimum.accumulate(envelope); transient: the dB
                                     difference of the short and long envelopes; static: unused */
    IQA_SQ_STAGE_THRESHOLD = 2,   /* float32: the per-sample threshold the mask compared against */
    IQA_SQ_STAGE_MASK = 3,        /* uint8: the mask before dilation */
    IQA_SQ_STAGE_DILATED = 4,     /* uint8: _dilate_mask */
    IQA_SQ_STAGE_GAIN = 5         /* float32: _smooth_gain */
} iqa_sq_stage;
typedef struct {
    int32_t method;      /* iqa_sq_method */
    int32_t auto_floor;  /* 0: segs[s].manual_floor_db */
    int32_t trim;        /* trim_silence */
    int32_t out_pcm16;
    double margin_db;           /* threshold_margin_db */
    double transient_margin_db;
} iqa_squelch_params;
typedef struct {
    int64_t n;        /* frames (>= the envelope window, >= the long window for "transient") */
    int64_t in_off;   /* float offset of the segment's frame 0 in in_dev / out_dev */
    int64_t base;     /* first workspace sample (multiple of IQA_SQ_TILE) */
    int32_t channels;
    int32_t window, short_window, long_window;  /* envelope windows in samples (>= 1) */
    int32_t hold;     /* dilation head = tail (<= 0: none) */
    int32_t fade;     /* gain fade (0: the dilated mask itself) */
    int32_t lead, trail;  /* trim margins in samples */
    double manual_floor_db;
    int64_t q_index[6];
    float q_gamma[3];
    int32_t reserved;
} iqa_squelch_seg;
typedef struct {
    double noise_floor_db, threshold_db;
    int64_t start, stop; /* the output is frames [start, stop) of samples * gain */
} iqa_squelch_result;

/* Workspace of iqa_squelch for `padded_samples` (= last base + n rounded up to IQA_SQ_TILE) and n_segs; -1 if invalid. */
int64_t iqa_squelch_workspace_bytes(int64_t padded_samples, int32_t n_segs);
/* Byte offset in that workspace of a per-sample stage array (iqa_sq_stage), valid after iqa_squelch; -1 if invalid. */
int64_t iqa_squelch_stage_offset(int64_t padded_samples, int32_t n_segs, int32_t stage);
int iqa_squelch(const iqa_squelch_params *params, const iqa_squelch_seg *segs, int32_t n_segs, const void *segs_dev,
                const void *in_dev, void *out_dev, void *result_dev, void *work_dev, int64_t work_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* IQA_HOTPATH_H */
