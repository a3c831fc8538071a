/*
 * rpf_engine.h -- C-ABI of the MI355X power-spectrum engine.
 *
 * This is the drop-in boundary for the FFT-and-accumulate worker of
 * rtl_power_fftw: everything `class Datastore` exposes to its two callers
 * (/root/reference/src/datastore.h:35-68, used from
 * /root/reference/src/acquisition.cxx:252-256,278-324,343-347,377-397 and
 * /root/reference/src/rtl_power_fftw.cxx:112,169,215), flattened to
 * `extern "C"` functions on an opaque handle, plain pointers and sizes.
 * No exceptions cross it; every call returns an int that is either RPF_OK or
 * one of the reference's own process exit codes
 * (/root/reference/src/exceptions.h:25-34), so the host turns a failure into
 * `throw RPFexception(rpf_last_error(e), (ReturnValue)rc)` unchanged.
 *
 * Threading contract (same as the reference, datastore.h:40-47): exactly one
 * producer thread calls begin/acquire/submit/unget/finish; the engine owns its
 * consumer thread and its HIP streams; rpf_get_* are valid after rpf_finish.
 *
 * The implementation (rtl-power-fftw_amd/csrc) is hand-written HIP for gfx950.
 * There is no CPU fallback: without a usable HIP device rpf_engine_create
 * fails with RPF_ERR_HARDWARE.
 */
#ifndef RPF_ENGINE_H
#define RPF_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPF_ABI_VERSION 2   /* 2: rpf_accumulate_device_hops, rpf_device_fused_hops, rpf_scan_reducer_*;
                               additive within 2: rpf_config::frame_step, rpf_frames_in, rpf_frame_span;
                               RPF_FLAG_SAMPLE_FORMAT, RPF_FLAG_CATCH_ALL, rpf_sample_bytes, rpf_sample_format;
                               RPF_FLAG_BIN_STATS, rpf_has_bin_stats, rpf_get_bin_stats, rpf_accumulate_device_stats;
                               rpf_accumulate_device_series, rpf_accumulate_series, rpf_series_launches;
                               rpf_accumulate_device_series_stats, rpf_accumulate_series_stats;
                               rpf_accumulate_device_excised, rpf_accumulate_excised;
                               rpf_engine_create_pfb, rpf_pfb_taps;
                               rpf_quantile_reset, rpf_quantile_append_device, rpf_quantile_append,
                               rpf_quantile_select_device, rpf_quantile_select, rpf_quantile_rows, rpf_quantile_max_rows;
                               rpf_accumulate_device_cross, rpf_accumulate_cross;
                               rpf_stft_device, rpf_stft;
                               rpf_correlate_device, rpf_correlate;
                               rpf_dedisperse_device, rpf_dedisperse, rpf_dedisperse_times;
                               rpf_fold_device, rpf_dedisperse_fold */

/* Return codes = ReturnValue of /root/reference/src/exceptions.h:25-34. */
#define RPF_OK 0
#define RPF_ERR_INVALID_ARGUMENT 3 /* ReturnValue::InvalidArgument */
#define RPF_ERR_INVALID_INPUT 5    /* ReturnValue::InvalidInput    */
#define RPF_ERR_ACQUISITION 6      /* ReturnValue::AcquisitionError */
#define RPF_ERR_HARDWARE 7         /* ReturnValue::HardwareError   */

typedef struct rpf_engine rpf_engine;

/* Mirrors the Params fields Datastore reads (datastore.cxx:23-34,67-76):
 * N, buffers, buf_length, window (+ the window values of AuxData). */
typedef struct rpf_config {
    uint32_t struct_size;     /* = sizeof(rpf_config), for ABI evolution          */
    int32_t N;                /* params.N: FFT bins, even (params.cxx:150-155)    */
    const float* window;      /* params.window ? N floats (copied) : NULL         */
    int32_t n_buffers;        /* params.buffers (default 5, params.h:42)          */
    int64_t buffer_capacity;  /* params.buf_length in bytes (params.h:43)         */
    int32_t device;           /* HIP device ordinal                               */
    uint32_t flags;           /* RPF_FLAG_*                                       */
    /* Appended within ABI 2 (struct_size tells the two forms apart: a config of
     * offsetof(rpf_config, frame_step) = 40 bytes, which ends at `flags`, means
     * frame_step = N).  Frame step S in complex samples, 1 <= S <= N; 0 = N.
     * Frame f is samples [f S, f S + N) = bytes [2 f S, 2 f S + 2N) of the stream:
     * S < N overlaps consecutive frames (Welch averaging).  Each frame is unpacked
     * as always -- -127, (-1)^n, window -- with n the index INSIDE the frame.  A
     * stream of B bytes holds frames(B) = B < 2N ? 0 : (B - 2N) / (2S) + 1 frames
     * (rpf_frames_in); every entry point counts frames that way.  S < 0 or S > N:
     * RPF_ERR_INVALID_ARGUMENT from rpf_engine_create, before any device is touched. */
    int32_t frame_step;
} rpf_config;

#define RPF_FLAG_NONE 0u
/* Stage raw bytes through VGPRs instead of LDS-DMA (debug / A-B measurement). */
#define RPF_FLAG_NO_LDS_DMA 1u
/* Sizes 16384..262144 (the four-step sizes): the fused persistent kernel -- ONE launch per acquisition, the
 * intermediate is handed from the column transforms to the row transforms inside each XCD's L2 instead of crossing
 * the fabric between two kernels.  It is what these sizes run by default on a 256-CU part (65536 ... 262144; 16384 and
 * 32768 default to the LDS mixed-radix kernels -- windowed runs of 32768 excepted, which are faster here -- so asking for
 * it is also asking for the four-step path) whenever
 * its eight workgroup teams assemble at rpf_engine_create; otherwise the engine keeps the two-kernel path.  A launch
 * whose teams do not assemble later (a CU held by someone else's kernel for seconds: another process on the device)
 * gives up, and the engine leaves the fused kernel for the rest of its life:
 *   - buffer-queue path (rpf_begin .. rpf_finish, rpf_accumulate): the acquisition does NOT fail -- like the
 *     reference's worker (datastore.cxx:48-96) this one has no failure path for it.  K3 leaves the accumulator alone,
 *     the worker runs the same staged bytes through the two-kernel path and rpf_finish returns RPF_OK with the spectrum
 *     that path gives (bit-identical to RPF_FLAG_NO_FOURSTEP_FUSED whenever every fused launch in flight gave up,
 *     else equal up to the order of the double additions);
 *   - device-resident entries (rpf_accumulate_device*, rpf_device_*; they return without synchronising): d_pwr_out of
 *     THAT launch is NaN-filled -- loud, never wrong -- and the next entry (or rpf_fused_status) that runs after the
 *     caller's stream has passed the launch notices and switches to the two-kernel path; see rpf_fused_status.
 *  */
#define RPF_FLAG_FOURSTEP_FUSED 2u
/* The four-step sizes on the two-kernel path (intermediate through HBM) even where the fused kernel is available
 * (A/B measurement, and the fallback's own tests). */
#define RPF_FLAG_NO_FOURSTEP_FUSED 8u
/* Sizes served by the LDS mixed-radix kernels (the tables csrc/mixed_plans.inc and
 * csrc/mixed_plans_split.inc: 500, 1000, 3000 ... 80000; 16384, 32768): use the kernel they would
 * get without them -- Bluestein, resp. the four-step pair for 16384 and 32768 (A/B measurement;
 * all are exact to the float32 bar). */
#define RPF_FLAG_NO_MIXED_RADIX 4u
/* Tuning: select kernel variant k for this N.  The shipped library contains only
 * variant 0 (one kernel per N x {window} x {staging}); any other k makes
 * rpf_engine_create fail with RPF_ERR_INVALID_ARGUMENT.  Experimental variants
 * exist only in the separate -DRPF_TUNING build used by tools/. */
#define RPF_FLAG_VARIANT(k) (((uint32_t)(k) & 0xffu) << 8)
/* Sample format of every stream the engine reads, in bits 16..19 of `flags` (zero = cu8, so a caller that never heard
 * of formats gets what it always got).  The sample is converted to float32 exactly (every value of the three integer
 * formats is a float32), (-1)^n is exact and the window multiplies once, with one rounding -- datastore.cxx:73-77 with
 * `v - 127` replaced by `v` for the signed formats.  Any other value: RPF_ERR_INVALID_ARGUMENT from
 * rpf_engine_create, before any device is touched.
 * cf32: the sample is the stored pair of IEEE float32 values, I then Q, little-endian, 8 bytes, x = v with no scaling,
 * clamping or screening: a stream in +-1.0 gives powers 2^-14 of the same signal at 8-bit full scale, and a NaN or an
 * Inf propagates into every bin of its frame and so into the sum.  A cf32 stream of int16 values gives the spectrum
 * of the cs16 stream of those values.  (3 is not a format: 4 is cf32.)
 * The LDS-resident kernel (powers of two 64 .. 8192) reads all four natively; at every other size a cs8 / cs16 / cf32
 * engine runs on the catch-all Stockham path (rpf_supported_n(N) holds for all four formats), which is several
 * times slower than the tuned kernel a cu8 engine gets at that size (README.md, "Sample formats"). */
#define RPF_FORMAT_CU8  0   /* unsigned 8-bit I,Q; x = v - 127   (the reference; the default) */
#define RPF_FORMAT_CS8  1   /* signed 8-bit I,Q;   x = v                                       */
#define RPF_FORMAT_CS16 2   /* signed 16-bit little-endian I,Q; x = v                          */
#define RPF_FORMAT_CF32 4   /* IEEE float32 little-endian I,Q;  x = v as stored                */
#define RPF_FLAG_SAMPLE_FORMAT(f) (((uint32_t)(f) & 0xfu) << 16)
/* Any N, any format on the catch-all Stockham path (A/B measurement, and the comparator of the format tests). */
#define RPF_FLAG_CATCH_ALL 16u
/* Per-bin statistics beside the power.  With re, im the float32 outputs of frame f's transform converted to double:
 *   p     = fma(im, im, re * re)                 the frame's power in the bin, correctly rounded (re * re is exact)
 *   S1[k] = the power accumulator, unchanged:    acc = fma(im, im, fma(re, re, acc))
 *   S2[k] = sum over the frames of p^2:          s2 = fma(p, p, s2)
 *   PK[k] = the largest p (peak hold), from 0
 * and across frame slots, workgroups, batches and launches S1 and S2 add in double, PK takes the maximum.  From them,
 * with M = repeats_done, the spectral kurtosis estimator SK[k] = (M+1)/(M-1) (M S2[k] / S1[k]^2 - 1) (NaN for M < 2 or
 * S1[k] = 0; rtl-power-fftw_amd/stats.py and host/datastore.h compute it): 1 for Gaussian noise, towards 0 for a steady
 * carrier, above 1 for anything intermittent.
 * An engine created with the flag keeps S2 and PK beside the power on the buffer-queue path (rpf_begin .. rpf_finish,
 * rpf_accumulate; rpf_get_bin_stats) and in rpf_accumulate_device_stats; rpf_get_power, rpf_accumulate and
 * rpf_accumulate_device keep their meaning and return S1.  Served natively by the LDS-resident kernel (powers of two
 * 64 .. 8192, every sample format, any frame step) with two more register accumulators per bin; at every other
 * size a stats engine runs on the catch-all Stockham path (README.md, "Per-bin statistics").  A NaN sample makes S1 and
 * S2 of every bin NaN and leaves PK the peak of the other frames (the maximum drops a NaN operand), on both paths.
 * Without the flag nothing changes: same kernels, same scratch, same results.
 * RPF_ERR_INVALID_ARGUMENT from rpf_engine_create, before any device is touched: together with RPF_FLAG_FOURSTEP_FUSED
 * or with RPF_FLAG_VARIANT(k), k != 0.  On a stats engine rpf_device_fused, rpf_device_fused_hops and rpf_device_reduce
 * return RPF_ERR_INVALID_ARGUMENT; rpf_accumulate_device_hops runs hop by hop (never the one-launch scan) and returns the
 * power alone; rpf_scan_reducer_* carry the power alone (a maximum beside RCCL's sum is not built). */
#define RPF_FLAG_BIN_STATS 32u

/* ABI version of the loaded library. */
int rpf_abi_version(void);
/* 1 if this build has a gfx950 kernel for N bins, else 0 (the supported set is
 * listed in DESIGN.md; an unsupported N makes rpf_engine_create fail with
 * RPF_ERR_INVALID_ARGUMENT rather than fall back to anything). */
int rpf_supported_n(int N);
/* Message of the last failure on this thread when no engine exists yet. */
const char* rpf_last_global_error(void);

/* Datastore::Datastore (datastore.cxx:23-34): buffer pool (pinned host memory
 * the producer fills directly), FFT plan (= twiddle tables on the device),
 * zeroed pwr[N] and queue_histogram[n_buffers+1]. */
int rpf_engine_create(const rpf_config* cfg, rpf_engine** out);
/* Polyphase filter bank (PFB) front end: an engine whose every frame is T N samples weighted by a prototype filter and
 * folded to N before the transform, which makes a channel flat-topped and isolates it from its neighbours.  Everything
 * that computes or checks it refers to this definition.
 *   Fold.  T = taps >= 1, h[0 .. T N) = coeffs (float32, copied).  The samples x are converted to float32 exactly, as the
 *     engine's format defines it (cu8: v - 127; cs8, cs16, cf32: v).  Output frame f, n in [0, N), I and Q separately:
 *         z = h[n] * x[f N + n]                                    (one float32 rounding)
 *         z = fmaf(h[t N + n], x[(f + t) N + n], z)   for t = 1 .. T-1, in increasing t
 *     with no contraction or reassociation beyond this (csrc/pfb_core.h).  The (-1)^n is not applied here.
 *   Spectrum.  What a RECTANGULAR cf32 engine of the same N computes from the frames z_f laid side by side (N is even, so
 *     (-1)^(tN+n) = (-1)^n and the cf32 kernels' own (-1)^n puts DC in the middle of the folded frame): bit for bit that,
 *     wherever the two launch the same grid on the same staging route.  Powers of two 64 .. 8192 run the LDS-resident
 *     kernel's cf32 form, every other even N the catch-all path, as a cf32 engine does; rpf_last_launch_info reports the
 *     transform launch.  The fold is one memory-bound launch (csrc/rpf_pfb.hip) per at most 64 MB of folded frames, in
 *     front of the unchanged transform; chunks after the first add into the output, so more than 64 MB of frames agree
 *     with the one-launch sum up to the grouping of the double additions.
 *   Frames.  Frame f spans the samples [f N, f N + T N): a stream of B bytes holds frames(B) = B < bTN ? 0 :
 *     (B - bTN) / (bN) + 1 frames and `frames` frames span bN (T - 1 + frames) bytes, b bytes per input sample.
 *     rpf_frames_in, rpf_frame_span, the frame quota of rpf_finish and every entry point count that way; the buffer queue
 *     carries up to a whole span from one staging slot to the next.  T = 1: one multiplication per sample.
 *   cfg is as for rpf_engine_create; its sample format is the INPUT format (all four), which rpf_sample_bytes and
 *     rpf_sample_format report.
 * RPF_ERR_INVALID_ARGUMENT before any device is touched: taps < 1, taps > 32 or taps x N > 2^26; coeffs NULL; cfg->window
 * non-NULL (the coefficients are the window); frame_step neither 0 nor N; RPF_FLAG_BIN_STATS; RPF_FLAG_FOURSTEP_FUSED; a
 * kernel variant other than 0.
 * On a PFB engine rpf_accumulate_device, the buffer queue (rpf_begin .. rpf_finish) and rpf_accumulate work;
 * rpf_accumulate_device_hops runs hop by hop, as on an engine with overlapped frames; rpf_device_fused,
 * rpf_device_fused_hops, rpf_device_reduce and the series, series-stats and excised entries return
 * RPF_ERR_INVALID_ARGUMENT.  An engine without PFB takes exactly the path it took. */
int rpf_engine_create_pfb(const rpf_config* cfg, int taps, const float* coeffs /* taps x N, copied */, rpf_engine** out);
/* T of a PFB engine, 0 for an engine without PFB, -1 for NULL. */
int rpf_pfb_taps(const rpf_engine* e);
/* Datastore::~Datastore (datastore.cxx:36-46). */
void rpf_engine_destroy(rpf_engine* e);
const char* rpf_last_error(const rpf_engine* e);

/* Start of Acquisition::run's worker section (acquisition.cxx:252-256):
 * pwr := 0, acquisition_finished := false, repeats_done := 0, start the
 * consumer.  `repeats` = params.repeats for this acquisition. */
int rpf_begin(rpf_engine* e, int64_t repeats);

/* acquisition.cxx:278-285: samples queue_histogram[#empty] and then blocks
 * until a buffer is free; returns it with its capacity. */
int rpf_buffer_acquire(rpf_engine* e, uint8_t** buf, size_t* capacity);
/* acquisition.cxx:302,320-323: buffer.resize(nbytes) + push_back to
 * occupied_buffers + notify.  nbytes even, <= capacity. */
int rpf_buffer_submit(rpf_engine* e, uint8_t* buf, size_t nbytes);
/* acquisition.cxx:310-314: failed readout, buffer goes back to the FRONT of
 * empty_buffers. */
int rpf_buffer_unget(rpf_engine* e, uint8_t* buf);

/* acquisition.cxx:343-347: acquisition_finished := true, notify, join.  On
 * return every submitted byte has been consumed per datastore.cxx:67-89
 * (frames may straddle buffers; frames beyond `repeats` and a trailing partial
 * frame are dropped) and pwr/repeats_done are final. */
int rpf_finish(rpf_engine* e, int64_t* repeats_done);

/* Datastore::pwr (datastore.h:53) -- raw accumulated |X|^2 per bin, bin N/2 =
 * DC; the DC interpolation of acquisition.cxx:377 is the caller's.  */
int rpf_get_power(const rpf_engine* e, double* out /* N */);
/* 1 if the engine was created with RPF_FLAG_BIN_STATS. */
int rpf_has_bin_stats(const rpf_engine* e);
/* S2 and PK of the last acquisition (RPF_FLAG_BIN_STATS), valid after rpf_finish like rpf_get_power; either pointer
 * may be NULL.  RPF_ERR_INVALID_ARGUMENT on an engine without the flag.  Bin N/2 = DC, no interpolation. */
int rpf_get_bin_stats(const rpf_engine* e, double* sum_sq /* N or NULL */, double* peak /* N or NULL */);
/* Datastore::repeats_done (datastore.h:38). */
int64_t rpf_get_repeats_done(const rpf_engine* e);
/* Datastore::queue_histogram (datastore.h:47), cumulative over the engine's
 * life like the reference's (never reset, datastore.cxx:24). */
int rpf_get_histogram(const rpf_engine* e, int* out /* n_buffers + 1 */);

/* Whole acquisition on one contiguous host stream, driven through the same
 * begin/acquire/submit/finish path in buffer_capacity-sized pieces. */
int rpf_accumulate(rpf_engine* e, const uint8_t* stream, size_t nbytes, int64_t repeats,
                   double* pwr_out /* N, host */, int64_t* repeats_done);

/* Replay without the copy into the pool: pin a caller-owned stream (hipHostRegister) so that rpf_accumulate on any part of
 * it hands the bytes to the consumer where they lie -- one H2D copy per staging slot instead of memcpy + copy per buffer
 * (measured: 9 -> 25 Gsample/s with the reference's default buffers).  Meant for a stream that is replayed more than once:
 * pinning costs ~4 ms per 82 MB and the FIRST copy out of freshly pinned memory runs at ~3 GB/s (the IOMMU mappings are
 * made then); rpf_accumulate never pins by itself.  The caller keeps the memory alive until rpf_stream_unregister or
 * rpf_engine_destroy (which unpins what is still registered).  RPF_ERR_HARDWARE if the runtime cannot pin the range (already
 * pinned memory, for one). */
int rpf_stream_register(rpf_engine* e, const void* stream, size_t nbytes);
int rpf_stream_unregister(rpf_engine* e, const void* stream);

/* Device-resident replay: the stream already sits in HBM (d_stream: even
 * address required, else RPF_ERR_INVALID_ARGUMENT; 16-byte aligned for the
 * LDS-DMA staging path, other alignments silently stage through VGPRs).  The
 * engine's device is made current for the call and the caller's restored.  Enqueues the fused kernel and the partial-sum reduce on
 * `hip_stream` (a hipStream_t; NULL = HIP's null stream) and returns
 * without synchronising (one exception: the two-kernel four-step and large Bluestein paths grow their intermediate to
 * what a launch needs -- a call that needs more than any before it synchronises `hip_stream` once, frees and
 * allocates); d_pwr_out[N] (device doubles, 16-byte aligned -- the reduce stores
 * bin pairs -- else RPF_ERR_INVALID_ARGUMENT; the same holds for every d_pwr_out below) is
 * overwritten with the sum over frames [0, min(repeats, rpf_frames_in(e, nbytes))).  Used by bench.py and the
 * full-size parity tests; does not touch the buffer queues. */
int rpf_accumulate_device(rpf_engine* e, const void* d_stream, size_t nbytes, int64_t repeats,
                          double* d_pwr_out, void* hip_stream, int64_t* repeats_done);

/* rpf_accumulate_device with the statistics (RPF_FLAG_BIN_STATS engines; else RPF_ERR_INVALID_ARGUMENT): d_out[3 x N]
 * = S1, S2, PK over the same frames, overwritten (zeros for a stream without a whole frame).  Same stream, alignment
 * and no-synchronise rules; K1 and ONE reduce launch for the three planes.  d_out[0 .. N) is bit for bit what
 * rpf_accumulate_device of the same engine writes. */
int rpf_accumulate_device_stats(rpf_engine* e, const void* d_stream, size_t nbytes, int64_t repeats,
                                double* d_out /* 3 x N: S1, S2, PK */, void* hip_stream, int64_t* repeats_done);

/* Cross-spectrum of two streams: Sab[k] = sum over the frames of A_f[k] conj(B_f[k]) beside Saa and Sbb, from FOUR power
 * spectra and the polarisation identity
 *     |A + B|^2 = |A|^2 + |B|^2 + 2 Re(A conj B),      |A + iB|^2 = |A|^2 + |B|^2 + 2 Im(A conj B)
 * with no transform kernel of its own.  Everything that computes or checks it refers to this definition.
 *   Inputs.  Two streams a and b in the engine's sample format, both of `nbytes` bytes, a multiple of b bytes per sample.
 *     The samples are converted to float32 exactly, as the format defines it (cu8: v - 127; cs8, cs16, cf32: v).  Frames,
 *     frame step, `repeats` and the dropped tail are those of rpf_accumulate_device on this engine: the frames used are
 *     [0, min(repeats, rpf_frames_in(e, nbytes))).
 *   Combined streams.  Sample by sample, I and Q as float32, one rounding per component and no contraction
 *     (csrc/cross_core.h):
 *         u = (aI + bI, aQ + bQ)   = a + b
 *         v = (aI - bQ, aQ + bI)   = a + i b
 *     exact for cu8, cs8 and cs16 (sums of 16-bit values are float32 integers), one float32 rounding for cf32.
 *   Four power planes.  Paa and Pbb are what rpf_accumulate_device of THIS engine writes for a and for b.  Puu and Pvv are
 *     what a cf32 engine with the same N, window, frame step, device and flags writes for u and v: bit for bit wherever
 *     the launches use the same grid and staging route, and with more than one chunk of scratch up to the grouping of the
 *     double additions.  A cf32 engine is its own cf32 engine.
 *   Output.  d_out[4 x N] (device doubles, 16-byte aligned, overwritten; zeros for a stream without a whole frame), bin
 *     N/2 = DC, computed in double, every operation rounded on its own, in exactly this order:
 *         C = Paa + Pbb;   out[0] = Paa;  out[1] = Pbb;  out[2] = 0.5 (Puu - C);  out[3] = 0.5 (Pvv - C)
 *     so that Sab = out[2] + i out[3], A and B being the transforms as the engine computes them: (-1)^n and the window
 *     applied, forward, unnormalised.
 *   Derived quantities (stats.coherence and stats.cross_phase; coherence and cross_phase of host/datastore.h):
 *         gamma^2 = (out[2]^2 + out[3]^2) / (out[0] out[1])    NaN where the denominator is 0; NOT clamped
 *         phase   = atan2(out[3], out[2])                      radians
 *   What a user must know.  gamma^2 of M frames is a biased estimate: identically 1 for M = 1 and about 1/M for unrelated
 *     streams.  Rounding can put it a few 1e-7 above 1.  The absolute error of Sab scales with Saa + Sbb, not with |Sab|:
 *     two streams whose levels differ by 40 dB carry about 100 times the relative error in gamma of two streams of equal
 *     level.  A NaN or an Inf in a cf32 stream propagates as it does for the power: into every bin of the planes that
 *     stream enters (a NaN in b: out[1], out[2] and out[3]).
 * The engine creates the cf32 engine at the first cross call (a windowed engine keeps its N window values on the host for
 * that), together with its scratch: two cf32 streams of at most 64 MB of whole frames each (at least one frame) and the
 * planes.  rpf_accumulate_device_cross puts every launch on `hip_stream` and returns without synchronising: this engine's
 * transform over a and over b; per chunk of scratch ONE combine launch (csrc/rpf_cross.hip, memory-bound: 2b bytes in and
 * 16 out per sample pair) and the cf32 engine's transform over u and over v, chunks after the first adding; one small
 * finishing launch into d_out.  It costs four transforms where a two-stream kernel would need two.  It does not touch
 * the buffer queues, pwr, repeats_done, the statistics or the quantile row store; *repeats_done (may be NULL) is the frame
 * count; rpf_last_launch_info reports the last transform launch, the cf32 engine's.  One cross call at a time per engine.
 * rpf_accumulate_cross is the same on two host streams, the counterpart of rpf_accumulate but not through the buffer
 * queues: both streams move through engine-owned device memory in pieces of whole frames (the pieces of
 * rpf_accumulate_series with one frame per integration), one piece of each at a time, every piece adds into the four
 * planes, the finishing launch runs once at the end and 4 x N doubles come back.  Synchronises before it returns.
 * RPF_ERR_INVALID_ARGUMENT, before any launch: a NULL argument; an engine created with RPF_FLAG_BIN_STATS; a PFB engine; a
 * kernel variant other than 0; a running acquisition; repeats < 0; nbytes that is no multiple of b; d_a or d_b that is no
 * multiple of b (each stream by the rules of rpf_accumulate_device: 16-byte aligned for the LDS-DMA path); d_out not
 * 16-byte aligned.  An engine that never makes a cross call takes exactly the path it took. */
int rpf_accumulate_device_cross(rpf_engine* e, const void* d_a, const void* d_b, size_t nbytes, int64_t repeats,
                                double* d_out /* 4 x N */, void* hip_stream, int64_t* repeats_done);
int rpf_accumulate_cross(rpf_engine* e, const uint8_t* a, const uint8_t* b, size_t nbytes, int64_t repeats,
                         double* out /* 4 x N, host */, int64_t* repeats_done);

/* Short-time Fourier transform: the complex spectrum of every frame, where every other entry ends in a sum of |X|^2.
 * Everything that computes or checks it refers to this definition.
 *   Frames.  F = min(max_frames, rpf_frames_in(e, nbytes)), max_frames >= 0; frame f starts at byte f b S of the stream (the
 *     engine's frame step; on a PFB engine frame f is the fold of the input frames f .. f + T - 1).
 *   Rows.  Row f is d_out[f N .. f N + N), interleaved float32 (re, im): F x N x 2 floats.  Rows < F are overwritten, rows
 *     >= F are not touched.  F = 0 makes no launch and is RPF_OK.  *frames_done = F (may be NULL).
 *   Values.  Row f is THE FLOAT32 TRANSFORM OF FRAME f EXACTLY AS THIS ENGINE COMPUTES IT BEFORE IT SQUARES: the engine's
 *     sample format converted exactly; (-1)^n and the window applied as one rounding; forward and unnormalised, so bin N/2
 *     is DC; on a PFB engine the folded frames.
 *   The tie to the power.  With re and im of a row converted to double, re re + im im (both squares are exact in double,
 *     so one rounding) is bit for bit what rpf_accumulate_device of the same engine writes for that frame alone (repeats =
 *     1, the pointer at the frame), on either staging route and on both kernel routes: the power kernels add
 *     fma(im, im, re re) to zero and every later addition adds zeros.  (An engine whose power comes from another family
 *     -- mixed radix, four-step, or the Bluestein kernels that serve cu8 below 64 bins -- is tied to the power of the
 *     catch-all engine of its configuration, whose rows it gives.)
 *   Routes.  N = 64 .. 8192 (the K1 sizes), any format, window, frame step and staging: K1's store kernels
 *     (csrc/k1_stft_body.inc), one launch; rpf_last_launch_info reports it.  Every other power of two up to 2^26, and any
 *     size with RPF_FLAG_CATCH_ALL: the catch-all Stockham transform, whatever family serves the size for power, in
 *     batches of frames, its last pass writing straight into the rows (no copy, no further kernel); overlapped frames go
 *     through the frame gather first.  An engine of another family creates its catch-all twin at the first call, as the
 *     cross entries create their cf32 engine.  A PFB engine: the fold per chunk of scratch, then the inner cf32 engine's
 *     route over the folded frames into the chunk's rows -- the channelizer.
 *   Nothing of the engine's state moves: queues, pwr, repeats_done, statistics, the quantile row store and the cross scratch
 *     stay as they are, and an engine that never calls these entries allocates nothing for them.
 * rpf_stft_device puts every launch on `hip_stream` and returns without synchronising; the stream follows
 * rpf_accumulate_device's rules (address a multiple of b; 16-byte aligned streams take the LDS-DMA route, other alignments
 * VGPR staging); d_out is 16-byte aligned.  rpf_stft is the same on a host stream into host rows: the stream moves through
 * engine-owned device memory in pieces of whole frames, as many as keep BOTH the input span and the rows (8 N bytes per
 * frame) within 64 MB and at least one (csrc/series_pieces.h, stft_pieces); it synchronises before it returns and
 * *frames_done counts the rows that came back.
 * RPF_ERR_INVALID_ARGUMENT, before any launch and with the output untouched: a NULL argument; N not a power of two
 * (Bluestein's spectrum lacks the final chirp, which |.|^2 discards); an engine created with RPF_FLAG_BIN_STATS; a kernel
 * variant other than 0; a running acquisition; max_frames < 0; nbytes or a stream address that is no multiple of b; d_out
 * not 16-byte aligned. */
int rpf_stft_device(rpf_engine* e, const void* d_stream, size_t nbytes, int64_t max_frames,
                    void* d_out /* F x N x (float re, float im) */, int64_t* frames_done, void* hip_stream);
int rpf_stft(rpf_engine* e, const uint8_t* stream, size_t nbytes, int64_t max_frames,
             void* out /* host, F x N x 2 floats */, int64_t* frames_done);

/* Correlator of up to eight streams: the visibility matrix V_ij[k] = sum over the frames of X_i,f[k] conj(X_j,f[k]) of
 * every pair at once, on the rows of rpf_stft_device.  Everything that computes or checks it refers to this definition.
 *   Inputs.  M = n_streams streams, 2 <= M <= 8, in the engine's sample format, each of `nbytes` bytes.  Frames, frame step,
 *     PFB folding, `repeats` and the dropped tail are those of rpf_stft_device on this engine: the frames used are [0, F),
 *     F = min(repeats, rpf_frames_in(e, nbytes)).  *frames_done = F (may be NULL); 0 where the call returns an error.
 *   Rows.  X_m,f is row f of rpf_stft_device of stream m on this engine: float32 (re, im), bin N/2 = DC.
 *   Per-frame term.  For a = X_i,f[k] and b = X_j,f[k], converted to double (csrc/correlate_core.h):
 *         t_re = fma(a.re, b.re, a.im b.im)        t_im = fma(a.im, b.re, -(a.re b.im))
 *     Each float32 x float32 product is exact in double, so each term is correctly rounded and equals numpy's
 *     ar br + ai bi and ai br - ar bi on float64 copies bit for bit, whatever contraction a compiler applies.  Swapping i
 *     and j negates t_im exactly; for i = j, t_re = fma(im, im, re re), the power of that frame, and t_im = +0.
 *   Sum.  V_ij[k] = sum over f of t, added in double, in an order fixed by N, M, F and the device, the same for every pair
 *     and independent of which stream is which: per chunk of C frames (below) the frame groups of correlate_groups, each
 *     summed from zero in frame order, then the groups added in their order, then the chunk added to the running sum of
 *     the chunks before it.  No floating-point atomics.
 *   Output.  d_out[M][M][2][N] doubles, 16-byte aligned, overwritten: ((i M + j) 2 + c) N + k, c = 0 re, 1 im.  For i > j the
 *     entry is the conjugate of (j, i) (re equal, im negated); the diagonal im is 0; F = 0 zeroes d_out.  For M = 2, V_01
 *     is Sab of rpf_accumulate_device_cross, A conj(B) with a = stream 0.
 *   Derived quantities (stats.coherence_matrix; coherence_pair of host/datastore.h):
 *         gamma^2_ij = (re^2 + im^2) / (V_ii V_jj)     NaN where the denominator is 0; NOT clamped
 *         phase_ij   = atan2(im, re)                    radians
 *     gamma^2 of F frames is biased as the cross entries' is: identically 1 for F = 1 and about 1/F for unrelated streams.
 *     A NaN in a cf32 stream m makes row m and column m NaN and leaves the other entries finite.
 * Per chunk of at most C = max(1, floor(64 MB / 8 N)) frames (2048 at 4096 bins, 1024 at 8192, 8 at 2^20): M launches of
 * the STFT route (stream m from byte f0 b S into rows block m), then the X-engine (csrc/rpf_correlate.hip: a lane per bin,
 * the pair sums in registers; with several frame groups one more launch adds their partial planes in order); after the
 * last chunk one finishing launch writes the Hermitian layout.  rpf_last_launch_info reports the last transform launch.
 * Made at the first call (and grown for a call with more streams than any before it): what rpf_stft_device makes; rows
 * scratch of M C frames (M x at most 64 MB); the X-engine's partial planes, G M^2 N doubles where G > 1 (at most 64 MB);
 * M^2 N running doubles (rpf_correlate: 3 M^2 N, the result included).  An engine that never correlates allocates
 * nothing for it.  Nothing else moves: queues, pwr, repeats_done, statistics, the quantile row store, the cross and the
 * STFT scratch stay as they are.
 * rpf_correlate_device puts every launch on `hip_stream` and returns without synchronising; every stream follows
 * rpf_stft_device's rules.  rpf_correlate is the same on M host streams: they move through engine-owned device memory
 * side by side, one piece of each at a time, in the pieces csrc/series_pieces.h gives with one frame per integration;
 * it synchronises before it returns.
 * RPF_ERR_INVALID_ARGUMENT, before any launch and with the output untouched: a NULL argument (the array, any element,
 * d_out); n_streams outside [2, 8]; N not a power of two (Bluestein's spectrum lacks the final chirp); an engine created
 * with RPF_FLAG_BIN_STATS; a kernel variant other than 0; a running acquisition; repeats < 0; nbytes or (device entry) a
 * stream address that is no multiple of b; d_out not 16-byte aligned (device entry).  PFB engines and overlapped frames
 * are served: their rows come from the STFT route unchanged. */
int rpf_correlate_device(rpf_engine* e, const void* const* d_streams, int n_streams, size_t nbytes, int64_t repeats,
                         double* d_out /* M x M x 2 x N */, void* hip_stream, int64_t* frames_done);
int rpf_correlate(rpf_engine* e, const uint8_t* const* streams, int n_streams, size_t nbytes, int64_t repeats,
                  double* out /* host */, int64_t* frames_done);

/* Incoherent dedispersion of the stored integrations: the DM-time plane, a second reader of the quantile entries' row
 * store.  Everything that computes or checks it refers to this definition.
 *   Rows.  The store holds K = rpf_quantile_rows(e) rows r[k][b] of N doubles, bin N/2 = DC, bit for bit what
 *     rpf_accumulate_device_series writes (rpf_quantile_append[_device] put them there).
 *   Inputs, on the host.  delays: D x N int32, delays[d N + b] >= 0, counted in integrations (rows).  weights: N doubles,
 *     or NULL for all ones.  D = n_trials, 1 <= D <= 4096.
 *   Times.  Dmax = the largest entry of the whole table; T = max(0, K - Dmax) (rpf_dedisperse_times).
 *   Output.  For every trial d < D and time t < T, in IEEE double with no contraction, every product and every sum
 *     rounded on its own:
 *         acc = +0.0
 *         for b = 0 ... N-1, ascending:   if weights[b] != 0:   acc = acc + weights[b] r[t + delays[d][b]][b]
 *         out[d T + t] = acc
 *     With weights == NULL the term is the row value itself.  A bin of weight 0 is NOT READ: that is how the DC spike or a
 *     flagged channel is left out.  A NaN in a row that some bin of non-zero weight reads makes exactly those outputs
 *     NaN.  The order is ascending in b for every output; no atomics, no cross-lane sums: the bits do not depend on the
 *     grid, the tiling or the route.  numpy gives the same bits with
 *         for b: acc = acc + w[b] * rows[delays[d, b] : delays[d, b] + T, b]          (dedisperse.reference)
 *   The store is read-only in this call: selecting quantiles before or after, appending more rows and dedispersing again,
 *     and a second identical call are all defined.
 *   The kernel knows no physics.  The delay table of a dispersion measure is built on the host, once in C++ (dm_delays of
 *     host/datastore.h) and once in Python (dedisperse.dm_delays), both by exactly this double-precision sequence,
 *     uncontracted, so the integers agree everywhere:
 *         f_b   = (fc + (b - N/2) (rate / N)) / 1e6          [MHz; fc the tuned frequency in Hz, rate in samples/s]
 *         inv_b = 1.0 / (f_b f_b);    ref = inv_(N-1);    t_row = (L S) / rate     [S the frame step, L frames per row]
 *         delays[d][b] = (int32) floor(((4.148808e3 dm_d) (inv_b - ref)) / t_row + 0.5)
 *     The highest bin is the reference, its delay 0.  Refused there: f_0 <= 0; a dm that is negative or not finite; a
 *     delay that does not fit int32.
 * How (csrc/rpf_dedisperse.hip over csrc/dedisperse_core.h): a workgroup owns 64 consecutive times x 16 trials and walks
 * the bins in blocks of 32, ascending; per block it stages rows [t0 + lo, t0 + 64 + hi) x 32 bins into LDS, lo and hi the
 * smallest and largest delay of the tile's trials over the block's bins of non-zero weight (computed here on the host
 * when the table is uploaded); a lane keeps its (trial, time) sums in registers.  A (tile, block) whose span exceeds the
 * LDS tile (hi - lo > 160) is read straight from the store: correct and slow.  One launch, no scratch.
 * rpf_dedisperse_device uploads the weights, the spans and the table into engine-owned memory (pinned and device, made at
 * the first call, grown for a larger table; an engine that never dedisperses allocates nothing), enqueues the copy and
 * the launch on `hip_stream` and returns without synchronising; d_out holds `capacity` doubles, of which D T are
 * written, and *times = T.  A call waits on the host for the launch of the call before it (the tables serve one call at
 * a time).  rpf_dedisperse is the same on the engine's stream into engine scratch, copied to `out`; it synchronises.
 * With T = 0 both return RPF_OK with *times = 0 and write nothing.  Nothing else of the engine moves: queues, pwr,
 * repeats_done, the store, the selection state, the cross, STFT and correlator scratch.
 * RPF_ERR_INVALID_ARGUMENT, before any device work, with the output untouched and *times = 0: a NULL e, delays,
 * d_out / out or times; n_trials < 1 or > 4096; a negative delay; a weight that is not finite; D T > capacity; d_out not
 * 16-byte aligned (device entry); a running acquisition; a PFB engine or an RPF_FLAG_BIN_STATS engine (the store's own
 * refusals).  rpf_dedisperse_times: T for this table and the rows stored now; -1 for a NULL argument, n_trials < 1 or a
 * negative delay. */
int rpf_dedisperse_device(rpf_engine* e, const int32_t* delays /* host, D x N */, const double* weights /* host, N, or NULL */,
                          int n_trials, double* d_out /* device, D x T, 16-byte aligned */, int64_t capacity /* doubles */,
                          void* hip_stream, int64_t* times /* T */);
int rpf_dedisperse(rpf_engine* e, const int32_t* delays, const double* weights, int n_trials, double* out /* host */,
                   int64_t capacity, int64_t* times);
int64_t rpf_dedisperse_times(const rpf_engine* e, const int32_t* delays, int n_trials);

/* Fold of a plane of time series at trial periods: profiles, hits and moments.  A reader of the D x T plane that
 * rpf_dedisperse_device writes (or of any D x T doubles).  Everything that computes or checks it refers to this definition.
 *   Input.  x[s][t]: D = n_series series of T doubles in device memory, pitch T.  steps[p]: P = n_periods unsigned 64-bit
 *     values on the host.  NB = phase_bins.
 *   Phase.  The kernel knows no physics: steps[p] is the phase advance per time in units of 2^-64 turn, and
 *         bin(p, t) = (((uint64(t) steps[p]) mod 2^64) >> 32) NB >> 32                 all in uint64, in [0, NB)
 *     Any steps[p] is legal; 0 puts every time into bin 0.
 *   Segments.  The fixed order is RPF_FOLD_SEGMENTS = 16 segments, the same for every T.  G = ceil(T / 16); segment g
 *     holds the times [min(T, g G), min(T, (g + 1) G)) and may be empty.
 *   Output.  All sums are IEEE double with no contraction, every sum and every product rounded on its own:
 *         part[g][s][p][b] = +0.0, then for t of segment g, ascending:   if bin(p, t) == b:  part += x[s][t]
 *         prof[s][p][b]    = +0.0, then for g = 0 ... 15, ascending:     prof += part[g][s][p][b]
 *         hits[p][b]       = the number of t < T with bin(p, t) == b                                        (int32)
 *         mom[s][0], mom[s][1] = the same two-level sums of x[s][t] and of x[s][t] x[s][t] over all t      (no bins)
 *     No atomics and no cross-lane sums of differently ordered terms: the bits depend on nothing but x, steps, NB and T.
 *     A NaN at time t reaches exactly the cells prof[s][p][bin(p, t)] of every p, and mom[s].  numpy gives the same bits
 *     with np.bincount(bins[lo:hi], weights=x[s, lo:hi], minlength=NB) per segment, the segments then added in order
 *     (fold.reference).
 *   Period to step, on the host, once in C++ (period_steps of host/datastore.h) and once in Python (fold.period_steps),
 *     both by exactly this double sequence:
 *         t_row = (L S) / rate;    pr = period_seconds / t_row           [S the frame step, L frames per row]
 *         refused unless pr is finite and pr >= 2
 *         steps = (uint64) ldexp(1.0 / pr, 64)                                 at most 2^63
 *     (row_period_steps takes pr itself, periods given in rows.)
 *   Statistic, on the host (fold.chi2 in Python, fold_chi2 of host/datastore.h), the reduced chi-square of a profile
 *     against a flat one:
 *         mu_s = mom[s][0] / T;    v_s = mom[s][1] / T - mu_s mu_s
 *         chi2[s][p] = sum over the b with hits > 0 of hits (prof / hits - mu_s)^2 / v_s / (n_used - 1)
 *     NaN where fewer than two bins have hits or v_s <= 0.
 * How (csrc/rpf_fold.hip over csrc/fold_core.h): a wave owns (series, 64 consecutive periods, segment), lane = period;
 * x[s][t] comes by scalar loads, every lane advances its 64-bit phase by steps[p] per time, and the wave's partial
 * profiles live in LDS as part[b][lane] (NB x 64 doubles), the sum of a lane's current bin in a register while the bin
 * stays.  The partials go to engine-owned scratch [g][s][p][b]; a second small launch adds the 16 segments in order.
 * The scratch is made at the first call and never exceeds 256 MB: where the partials of all series need more, the series
 * run in groups.  An engine that never folds allocates nothing.
 * rpf_fold_device uploads steps into engine-owned memory, enqueues on `hip_stream` and returns without synchronising; a
 * call waits on the host for the launches of the call before it (tables and scratch serve one call at a time).  d_prof
 * holds `capacity` doubles, of which D P NB are written; d_hits (P NB int32) and d_mom (D x 2 doubles) may be NULL.  It
 * touches nothing of the engine but its own tables and scratch, and works on any engine: it reads no store.
 * rpf_dedisperse_fold runs rpf_dedisperse_device into the engine's plane scratch on the engine's stream, folds that plane
 * where it lies (it never leaves the device), copies prof, hits and mom to the host and synchronises; *times = T of the
 * dedispersion.  It inherits every refusal of rpf_dedisperse.
 * With T = 0 both return RPF_OK and write nothing.
 * RPF_ERR_INVALID_ARGUMENT, before any device work, with the outputs untouched: a NULL e, series, steps or profile
 * pointer (rpf_dedisperse_fold: or times); D or P outside 1 ... 4096; NB outside 1 ... 128; T < 0 or T >= 2^31;
 * D P NB > capacity or > 2^24; d_series not 8-byte aligned, d_prof or d_mom not 16-byte aligned; a running acquisition. */
#define RPF_FOLD_SEGMENTS 16
int rpf_fold_device(rpf_engine* e, const double* d_series /* device, D x T */, int n_series, int64_t T,
                    const uint64_t* steps /* host, P */, int n_periods, int phase_bins,
                    double* d_prof /* device, D x P x NB, 16-byte aligned */, int64_t capacity /* doubles */,
                    int32_t* d_hits /* device, P x NB, or NULL */, double* d_mom /* device, D x 2, or NULL */, void* hip_stream);
int rpf_dedisperse_fold(rpf_engine* e, const int32_t* delays, const double* weights, int n_trials,
                        const uint64_t* steps, int n_periods, int phase_bins,
                        double* prof /* host */, int64_t capacity, int32_t* hits /* host or NULL */, double* mom /* host or NULL */,
                        int64_t* times);

/* The two halves of rpf_accumulate_device as separate enqueues, so that a
 * benchmark can bracket the dominant kernel alone with events on `hip_stream`:
 * _fused runs K1 (unpack+FFT+|X|^2) and leaves one partial spectrum per frame
 * slot in engine scratch; _reduce runs K3 over the scratch of the last _fused
 * call into d_pwr_out[N] (after rpf_device_fused_hops: all n_hops spectra, d_pwr_out[n_hops x N]). */
int rpf_device_fused(rpf_engine* e, const void* d_stream, size_t nbytes, int64_t repeats,
                     void* hip_stream, int64_t* repeats_done);
int rpf_device_reduce(rpf_engine* e, double* d_pwr_out, void* hip_stream);

/* A whole scan in one call: n_hops device-resident acquisitions (the reference's scan is a loop of
 * hops, /root/reference/src/rtl_power_fftw.cxx:133-174, each starting from a zeroed accumulator,
 * acquisition.cxx:252-254).  Hop h = the first min(repeats[h], rpf_frames_in(e, nbytes[h])) frames of
 * d_streams[h]; its spectrum goes to d_pwr_out[h*N .. h*N+N) (device doubles, overwritten; zeros
 * for a hop without a whole frame).  For the sizes the LDS-resident kernel serves (powers of two
 * 64 .. 8192) up to rpf_max_hops_per_launch() hops share ONE persistent kernel launch -- the
 * workgroups walk the hops' frames as one sequence and hand over / zero their register
 * accumulators at each hop boundary -- and ONE reduce launch, so a scan pays the per-launch
 * fixed cost once instead of once per hop; other sizes run hop by hop.  Same stream, alignment
 * and synchronisation rules as rpf_accumulate_device.  repeats_done: n_hops entries or NULL. */
int rpf_accumulate_device_hops(rpf_engine* e, const void* const* d_streams, const size_t* nbytes,
                               const int64_t* repeats, int n_hops, double* d_pwr_out /* n_hops x N */,
                               void* hip_stream, int64_t* repeats_done);
/* The fused-kernel half of it alone (n_hops <= rpf_max_hops_per_launch(), LDS-resident sizes
 * only, else RPF_ERR_INVALID_ARGUMENT); rpf_device_reduce then writes all n_hops spectra. */
int rpf_device_fused_hops(rpf_engine* e, const void* const* d_streams, const size_t* nbytes,
                          const int64_t* repeats, int n_hops, void* hip_stream, int64_t* repeats_done);
int rpf_max_hops_per_launch(void);

/* Spectrogram: the spectrum of one stream as it changes over time.  With F = rpf_frames_in(e, nbytes), L =
 * frames_per_spectrum >= 1 and the cap max_spectra >= 0: K = min(max_spectra, F / L) spectra (integer division: a
 * trailing group of fewer than L frames is dropped, as a trailing partial frame is); spectrum k is the sum of |X_f|^2
 * over the frames f in [k L, (k + 1) L), every frame unpacked, windowed and transformed exactly as
 * rpf_accumulate_device does it on this engine (format, frame step, window, (-1)^n).  Row k = d_out[k N .. k N + N)
 * (device doubles, 16-byte aligned), bin N/2 = DC; rows < K are overwritten, rows >= K are not touched;
 * *spectra_done = K (may be NULL).  Same stream, alignment and no-synchronise rules as rpf_accumulate_device.  K = 0 is
 * RPF_OK and launches nothing.
 * Powers of two 64 .. 8192 with the frames side by side (frame step N), all three sample formats, windowed or not,
 * either staging: ONE persistent launch walks all K spectra -- a workgroup stores the spectra that lie inside its share
 * of the frames straight into their rows and hands over the (at most two) it shares with its neighbours, which one
 * small fix-up launch then adds in workgroup order -- so the per-launch fixed cost is paid once, not K times, and
 * every row is bit-reproducible for a given grid, L and K.  (More than 2^31 / ceil(L / frames per workgroup) spectra:
 * the fewest launches that hold them.)  Every other engine -- another size, frame step S != N, RPF_FLAG_CATCH_ALL --
 * runs spectrum by spectrum through its single-acquisition path: row k is bit for bit what rpf_accumulate_device
 * writes for that slice of the stream (a fused four-step launch that gives up NaN-fills its own row), correct at every
 * size and fast at none.  rpf_series_launches tells the two apart.
 * RPF_ERR_INVALID_ARGUMENT: frames_per_spectrum < 1, max_spectra < 0, a misaligned stream or output, an engine created
 * with RPF_FLAG_BIN_STATS (its series entry is rpf_accumulate_device_series_stats, below). */
int rpf_accumulate_device_series(rpf_engine* e, const void* d_stream, size_t nbytes, int64_t frames_per_spectrum,
                                 int64_t max_spectra, double* d_out /* K x N */, void* hip_stream, int64_t* spectra_done);
/* The same calculation on a host stream, the counterpart of rpf_accumulate -- but not through the buffer queues: the
 * worker thread, pwr and repeats_done are not touched.  The stream moves through engine-owned device memory in pieces
 * that each hold a whole number of spectra (as many as fit in 64 MB; one, if a single spectrum is larger), the device
 * entry runs per piece on the engine's stream and each piece's rows are copied back, so device memory stays bounded for
 * any nbytes and K.  A stream pinned with rpf_stream_register is copied from where it lies.  Synchronises before it
 * returns.  Not while an acquisition is running. */
int rpf_accumulate_series(rpf_engine* e, const uint8_t* stream, size_t nbytes, int64_t frames_per_spectrum,
                          int64_t max_spectra, double* out /* K x N, host */, int64_t* spectra_done);
/* Time-resolved statistics: the series of an engine created with RPF_FLAG_BIN_STATS.  L, max_spectra, K, the frame
 * count and the dropped tail are those of rpf_accumulate_device_series; for every spectrum k the three planes
 * RPF_FLAG_BIN_STATS defines, over its L frames: row k = d_out[k 3N .. k 3N + 3N) = S1[N], S2[N], PK[N] (device doubles,
 * 16-byte aligned), bin N/2 = DC -- what rpf_accumulate_device_stats writes for that slice of the stream.  PK starts
 * from 0 in every row.  Rows < K are overwritten, rows >= K are not touched; K = 0 is RPF_OK and launches nothing.
 * SK of row k is the estimator above with M = L.
 * Powers of two 64 .. 8192, frame step N, all three formats, windowed or not, either staging: ONE persistent launch,
 * the series kernel with two more register accumulators per bin; a spectrum cut by a workgroup boundary leaves three
 * planes per segment and the fix-up launch adds S1 and S2 in workgroup order and takes the maximum of PK.  S1 is
 * computed by the operations of rpf_accumulate_device_series, in the same order for the same grid.  Every other engine
 * -- another size, frame step S != N, RPF_FLAG_CATCH_ALL -- runs spectrum by spectrum through
 * rpf_accumulate_device_stats' path, bit for bit.  rpf_series_launches tells the two apart.
 * RPF_ERR_INVALID_ARGUMENT: an engine created without RPF_FLAG_BIN_STATS, and what rpf_accumulate_device_series refuses. */
int rpf_accumulate_device_series_stats(rpf_engine* e, const void* d_stream, size_t nbytes, int64_t frames_per_spectrum,
                                       int64_t max_spectra, double* d_out /* K x 3 x N */, void* hip_stream,
                                       int64_t* spectra_done);
/* The same on a host stream, as rpf_accumulate_series: bounded pieces of whole spectra through engine-owned device
 * memory, not through the buffer queues; pwr, S2, PK and repeats_done of the engine are not touched.  Synchronises
 * before it returns.  Not while an acquisition is running. */
int rpf_accumulate_series_stats(rpf_engine* e, const uint8_t* stream, size_t nbytes, int64_t frames_per_spectrum,
                                int64_t max_spectra, double* out /* K x 3 x N, host */, int64_t* spectra_done);
/* The excised average: the power summed over the stream with the integrations that carried interference left out, bin
 * by bin (RPF_FLAG_BIN_STATS engines).  Everything that computes or checks it refers to this definition.
 *   Rows.  L = frames_per_spectrum >= 2, K = min(max_spectra, rpf_frames_in(e, nbytes) / L) as above; row k has the planes
 *     S1_k, S2_k, PK_k over the frames [k L, (k + 1) L), bit for bit the rows rpf_accumulate_device_series_stats writes
 *     for the same stream on the same engine (the same kernels run, one-launch route or spectrum by spectrum).
 *   Spectral kurtosis.  SK_k[b] = ((m + 1) / (m - 1)) * (m * S2 / (S1 * S1) - 1), m = (double)L, in IEEE double in exactly
 *     this order of operations -- the order of stats.spectral_kurtosis -- each operation rounded on its own: no
 *     contraction, no fast-math, a correctly rounded division (csrc/excise_core.h).  NaN where S1 = 0.
 *   Kept.  Integration k is kept in bin b iff sk_lo <= SK_k[b] && SK_k[b] <= sk_hi; a NaN compares false and is flagged.
 *     sk_lo and sk_hi are the caller's; -inf and +inf are allowed.
 *   Outputs.  d_out[3 x N] (device doubles, 16-byte aligned, overwritten; zeros for K = 0, and nothing else is launched):
 *       clean[b] = d_out[b]       sum of S1_k[b] over the kept k
 *       kept[b]  = d_out[N + b]   the number of kept k, as a double (an exact integer)
 *       total[b] = d_out[2N + b]  sum of S1_k[b] over all k < K
 *     d_mask (may be NULL): d_mask[k N + b] = 1 where (k, b) is flagged, else 0, for k < K; rows >= K are not touched.
 *     Bin N/2 = DC, no interpolation.
 *   Addition order.  Fixed for a given call -- no floating-point atomics, the same call twice gives the same bits -- and
 *     the same for clean and total: with nothing flagged clean == total bit for bit.  (Row k adds into accumulator
 *     k mod G of its bin in increasing k, and the G accumulators are added in a fixed order: csrc/excise_core.h.  The
 *     order differs from a sequential sum, so clean and total agree with one to a few ulp.)
 * The rows never leave HBM: the stream goes through the series kernels in pieces of whole rows -- as many as fit in
 * 64 MB of rows, at least one -- into engine-owned row scratch, and one launch per piece reads S1 and S2 of the piece
 * (16 N bytes per row; PK is not read) and updates the accumulators; one small launch at the end writes d_out.  So it
 * works at every size, frame step and format the engine serves and is fast where the series is; rpf_series_launches
 * reports the transform launches as for the series calls.  Same stream, alignment and no-synchronise rules as
 * rpf_accumulate_device (one exception of the same kind: a call that needs more row scratch than any before it
 * synchronises once to grow it).  One excised call at a time per engine: the scratch is the engine's.
 * The thresholds are the caller's business (stats.sk_limits, host/datastore.h sk_limits: 1 +- sigma sd of SK for
 * Gaussian noise and independent frames); nothing here is a calibrated false-alarm rate.
 * RPF_ERR_INVALID_ARGUMENT: an engine without RPF_FLAG_BIN_STATS, frames_per_spectrum < 2, sk_lo > sk_hi or a NaN
 * threshold, a misaligned d_out, and what rpf_accumulate_device_series_stats refuses. */
int rpf_accumulate_device_excised(rpf_engine* e, const void* d_stream, size_t nbytes, int64_t frames_per_spectrum,
                                  int64_t max_spectra, double sk_lo, double sk_hi,
                                  double* d_out /* 3 x N: clean, kept, total */, uint8_t* d_mask /* K x N or NULL */,
                                  void* hip_stream, int64_t* spectra_done);
/* The same on a host stream: the input moves in pieces as in rpf_accumulate_series_stats (no piece larger than the row
 * scratch holds), only 3 x N doubles and, if asked for, the mask come back.  Not through the buffer queues: the queues,
 * pwr, S2, PK and repeats_done of the engine are not touched.  Synchronises before it returns.  Not while an
 * acquisition is running. */
int rpf_accumulate_excised(rpf_engine* e, const uint8_t* stream, size_t nbytes, int64_t frames_per_spectrum,
                           int64_t max_spectra, double sk_lo, double sk_hi, double* out /* 3 x N, host */,
                           uint8_t* mask /* K x N or NULL, host */, int64_t* spectra_done);
/* Per-bin quantiles of the integrations: order statistics across time, where everything above is a sum.  Everything
 * that computes or checks them refers to this definition.
 *   Row store.  An engine keeps up to rpf_quantile_max_rows(e) = max(1, 2^27 / N) rows of N doubles, device-resident and
 *     engine-owned: 1 GiB at most.  It is allocated at the first append and grows by doubling; a growth synchronises once
 *     (the caller's stream and the engine's), moves the stored rows and frees the old block.
 *   Row.  What rpf_accumulate_device_series writes: the sum of |X_f|^2 over L = frames_per_spectrum consecutive frames,
 *     bin N/2 = DC.  An append adds K = min(max_spectra, rpf_frames_in(e, nbytes) / L) rows (a trailing partial group is
 *     dropped) after the rows stored so far; *appended = K (may be NULL).
 *   Selection.  Let v_(0) <= ... <= v_(K-1) be the K stored values of a bin in ascending order; a NaN counts as larger
 *     than every number, whatever its sign bit, as np.sort places it (-0.0 sorts below +0.0, which compare equal).  For
 *     0 <= q <= 1, in IEEE double with every operation rounded on its own and no contraction:
 *         h = q * (K - 1);  j = floor(h);  g = h - j;  a = v_(j);  b = v_(min(j + 1, K - 1))
 *         Q = (g == 0 || a == b) ? a : a + g * (b - a)
 *     so q = 0 is the minimum, q = 1 the maximum and q = 0.5 the median; a NaN among a, b with g != 0 gives NaN.  The
 *     output of quantile i is out[i N .. i N + N).  With no rows stored every output is NaN.  stats.quantiles states the
 *     same in numpy.
 *   The rows are not modified by a selection: selecting again with other q, or appending more rows and selecting again,
 *     is defined.  rpf_quantile_reset forgets the rows and keeps the allocation.
 * rpf_quantile_append_device runs the series once, straight into the store behind the rows it holds: the rows are bit for
 * bit those of rpf_accumulate_device_series for the same call on the same engine -- the one-launch route or spectrum by
 * spectrum, so every size, format, frame step and RPF_FLAG_CATCH_ALL works, and rpf_series_launches reports the route of
 * the last append.  Same stream, alignment and no-synchronise rules as rpf_accumulate_device_series (a growth excepted).
 * rpf_quantile_append moves a host stream in the pieces rpf_accumulate_series uses, so its rows are that call's rows bit
 * for bit; not through the buffer queues: the queues, pwr and repeats_done are not touched.  Synchronises before it returns.
 * rpf_quantile_select_device (q: nq values on the HOST, d_out: nq x N device doubles, 16-byte aligned) enqueues an
 * MSB-first radix select over order-preserving 64-bit keys (csrc/quantile_core.h, csrc/rpf_quantile.hip): 16 passes of
 * 4 bits count, per (quantile, bin), the stored values that share the digits chosen so far by their next digit; where
 * v_(j+1) is needed and the counts show no tie one further pass finds it as the smallest key above v_(j).  Exact,
 * read-only, integer counts and no floating-point atomics: the same bits for any grid.  It reads (16 + 1) K N 8 bytes
 * at most, all nq quantiles sharing each pass.  Returns without synchronising (its first call allocates the selection
 * state).  rpf_quantile_select is the same into host memory on the engine's stream, and synchronises.
 * Ordering between appends and selects is the caller's: the same stream, or synchronise.  One quantile call at a time per
 * engine: the store and the selection state are the engine's.
 * RPF_ERR_INVALID_ARGUMENT, before any device work and before the stream is touched: a NULL argument, a running
 * acquisition, frames_per_spectrum < 1, max_spectra < 0; a PFB engine; an engine with RPF_FLAG_BIN_STATS; an append that
 * would take the store over rpf_quantile_max_rows (nothing is appended: raise the frames per integration or cap
 * max_spectra); nq < 1 or nq > 8; a q that is NaN or outside [0, 1]; a misaligned d_stream or d_out, by the series' rules. */
int rpf_quantile_reset(rpf_engine* e);   /* rows = 0; keeps the allocation */
int rpf_quantile_append_device(rpf_engine* e, const void* d_stream, size_t nbytes, int64_t frames_per_spectrum,
                               int64_t max_spectra, void* hip_stream, int64_t* appended);
int rpf_quantile_append(rpf_engine* e, const uint8_t* stream, size_t nbytes, int64_t frames_per_spectrum,
                        int64_t max_spectra, int64_t* appended);
int rpf_quantile_select_device(rpf_engine* e, const double* q /* host */, int nq, double* d_out /* nq x N */, void* hip_stream);
int rpf_quantile_select(rpf_engine* e, const double* q, int nq, double* out /* nq x N, host */);
int64_t rpf_quantile_rows(const rpf_engine* e);       /* -1 for NULL */
int64_t rpf_quantile_max_rows(const rpf_engine* e);   /* -1 for NULL */
/* Transform-kernel launches the engine's last series call (either kind) enqueued: 1 on the one-launch path (whatever K is), K on the
 * spectrum-by-spectrum path, summed over the pieces of rpf_accumulate_series; 0 before any series call and for K = 0.
 * rpf_last_launch_info reports the geometry of the last of them. */
int rpf_series_launches(const rpf_engine* e);

/* Pure helpers on the engine's N and frame step S, so that callers never re-derive the formula:
 * frames(nbytes) = nbytes < 2N ? 0 : (nbytes - 2N) / (2S) + 1, and the bytes `frames` frames span,
 * 2N + 2S (frames - 1) (0 for no frame).  With S != N: rpf_accumulate_device_hops runs hop by hop
 * (the scan kernel reads frames side by side), rpf_device_fused_hops returns RPF_ERR_INVALID_ARGUMENT,
 * and so does rpf_device_fused on a size the LDS-resident K1 does not serve (rpf_accumulate_device is
 * the general entry point). */
int64_t rpf_frames_in(const rpf_engine* e, size_t nbytes);
size_t rpf_frame_span(const rpf_engine* e, int64_t frames);
/* Bytes per complex sample, b: 2 (cu8, cs8), 4 (cs16) or 8 (cf32), and the engine's RPF_FORMAT_*.  EVERY byte count of this
 * interface that is written 2N / 2S above is bN / bS: frames(nbytes) = nbytes < bN ? 0 : (nbytes - bN) / (bS) + 1,
 * the span bN + bS (frames - 1), the frame quota and the trailing partial frame of rpf_finish, the hop lengths of
 * rpf_accumulate_device_hops.  rpf_buffer_submit wants nbytes % b == 0 (a sample never straddles two buffers; frames
 * still may) and rpf_engine_create buffer_capacity % b == 0, else RPF_ERR_INVALID_ARGUMENT.  Device streams: address a
 * multiple of b, else RPF_ERR_INVALID_ARGUMENT; 16-byte aligned for the LDS-DMA path, other alignments stage through
 * VGPRs. */
int rpf_sample_bytes(const rpf_engine* e);
int rpf_sample_format(const rpf_engine* e);

/* Datastore::pwr as it sits in HBM after rpf_finish: copied (device to device, or peer to peer when
 * dst_device is another device) into d_dst[N]; synchronises hip_stream before returning. */
int rpf_copy_power_device(const rpf_engine* e, double* d_dst, void* hip_stream, int dst_device);

/* ---- multi-GPU scans in one process: the final reduce over RCCL / xGMI ----------------
 * One engine per device runs its share of a scan's hops (hop-major, frame-aligned); a scan reducer owns
 * one RCCL communicator over those devices (ncclCommInitAll; librccl.so is loaded with dlopen) and, on
 * every device, a block of max_hops x N doubles.  Per pass: _begin zeroes the blocks; after an engine's
 * rpf_finish, _deposit copies its accumulator into row `hop` of its device's block; _reduce issues ONE
 * ncclReduce(sum, ncclDouble, hops x N) onto the first device and one device-to-host copy.
 * rpf_scan_reducer_create fails with RPF_ERR_HARDWARE when RCCL is missing or refuses the device list
 * (e.g. one device listed twice); callers then add the per-device spectra on the host, which gives the
 * same sums up to the order of the additions. */
typedef struct rpf_scan_reducer rpf_scan_reducer;
int rpf_scan_reducer_create(const int* devices, int n_devices, int N, int max_hops, rpf_scan_reducer** out);
void rpf_scan_reducer_destroy(rpf_scan_reducer* r);
const char* rpf_scan_reducer_last_error(const rpf_scan_reducer* r);
int rpf_scan_reducer_begin(rpf_scan_reducer* r);
int rpf_scan_reducer_deposit(rpf_scan_reducer* r, int slot, int hop, const rpf_engine* e);
int rpf_scan_reducer_reduce(rpf_scan_reducer* r, int hops, double* host_out /* hops x N */);

/* Which four-step kernel this engine runs, and what became of its fused launches.
 *   *active            1: the fused persistent kernel is what the next launch runs; 0: the two-kernel path (or N is not
 *                      a four-step size)
 *   *launches_gave_up  fused launches whose teams did not assemble, over the engine's life.  Device-resident entries:
 *                      read it after synchronising the stream; a count that has grown means the spectrum of that
 *                      launch is NaN and must be asked for again (the engine is on the two-kernel path by then).
 *   *launches_recovered  of those, the ones the buffer-queue worker ran again on the two-kernel path
 * Any pointer may be NULL.  Not to be called while an acquisition is running.  NOT a pure query (hence no const): a call
 * that finds a device-resident launch to have given up retires the fused kernel for this engine then and there. */
int rpf_fused_status(rpf_engine* e, int* active, int64_t* launches_gave_up, int64_t* launches_recovered);

/* Launch geometry of the last fused-kernel launch (for DESIGN/bench reporting):
 * workgroups, threads per workgroup, frames per workgroup, LDS bytes. */
int rpf_last_launch_info(const rpf_engine* e, int* grid, int* block, int* frames_per_wg,
                         int* lds_bytes);

#ifdef __cplusplus
}
#endif
#endif /* RPF_ENGINE_H */
