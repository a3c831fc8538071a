// rpf_kernels.h -- internal C++ interface between the engine (rpf_engine.cpp)
// and the gfx950 kernels (rpf_kernels.hip).  Not part of the C-ABI.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <vector>

#include "excise_core.h"
#include "fft_core.h"
#include "hop_partition.h"
#include "pfb_core.h"
#include "quantile_core.h"
#include "series_partition.h"

namespace rpf {

struct LaunchInfo {
    int grid = 0;        // workgroups
    int block = 0;       // threads per workgroup
    int fpw = 0;         // frames processed concurrently by one workgroup
    int lds_bytes = 0;   // dynamic LDS per workgroup
    int slots = 0;       // partial spectra written (0: one per workgroup)
};

// Is there a fused kernel for N bins (tuning variant vid, 0 = default)?
bool kernel_supported(int N, int vid = 0);

// Persistent-grid geometry for N on `device`: li->grid is the number of
// workgroups that are simultaneously resident (occupancy x CU count).
// fmt: the sample format (fft_core.h kFmt*); the signed formats have variant 0 only and may come out with another
// grid than cu8 (cs16 stages twice the bytes in LDS) -- li says what was chosen.
// stats: the kernels with per-bin statistics (RPF_FLAG_BIN_STATS; variant 0 only), which may run at a lower occupancy.
hipError_t plan_launch(int N, int vid, bool window, bool use_dma, int device, LaunchInfo* li, int fmt = kFmtCu8,
                       bool stats = false);

// Fused unpack + FFT + |X|^2 accumulate over frames [0, nframes) of d_stream
// (frame f = bytes [pitch f, pitch f + bN); pitch 0 = bN; b = 2, or 4 for 16-bit samples: `fmt`; written for b = 2 below).  Writes one partial spectrum of N doubles
// per workgroup to d_partial (every workgroup writes, zeros included).
// `grid` is the number of workgroups to launch (<= the planned grid).  pitch: even, <= 2N; any pitch
// but 2N runs the strided instantiation (use_dma then also needs pitch % 16 == 0).
hipError_t launch_fft_accum(int N, int vid, bool window, bool use_dma, const uint8_t* d_stream,
                            long nframes, const cf* d_twiddles, const float* d_window,
                            double* d_partial, int grid, hipStream_t stream, LaunchInfo* li, long pitch = 0,
                            int fmt = kFmtCu8, bool stats = false);
// stats: workgroup w writes THREE planes of N doubles, d_partial[(3 w + plane) N ..): plane 0 the power sum S1 (the
// plain kernel's, instruction for instruction), plane 1 S2 = sum of the squared frame powers, plane 2 PK = the largest
// frame power.  d_partial then holds 3 x grid x N doubles.
// K3 for the statistics: d_out[plane * N + bin] for the three planes in ONE launch -- planes 0 and 1 summed over the
// slots exactly as launch_reduce sums them (same order, bit for bit), plane 2 their maximum; accumulate: combined with
// what d_out holds (+, +, max) instead of overwriting it.  Slot s, plane p lies at d_partial[(3 s + p) N ..).
hipError_t launch_reduce_stats(const double* d_partial, int nslots, int N, double* d_out, bool accumulate,
                               hipStream_t stream);
// The same over the hops of `hops` (hop_partition.h: frame f of hop h = bytes [2N f, 2N (f+1)) of
// hops.stream[h]) in ONE launch.  Workgroup w writes one partial spectrum of N doubles per hop it
// touches, at slot hops.slot_bias[h] + w of d_partial.  `grid` is what partition_hops returned
// for (li->fpw, the planned grid).
hipError_t launch_fft_accum_hops(int N, int vid, bool window, bool use_dma, const HopArgs& hops,
                                 const cf* d_twiddles, const float* d_window, double* d_partial, int grid,
                                 hipStream_t stream, LaunchInfo* li, int fmt = kFmtCu8);

// ---- a uniform series of spectra in ONE launch (rpf_kernels_series.hip, series_partition.h) ----
// Variant 0 of every K1 size, all three sample formats.
bool series_supported(int N, int fmt = kFmtCu8);
// The series kernel's resident grid (it may differ from plan_launch's: another kernel, its own register count).
hipError_t plan_series(int N, bool window, int device, LaunchInfo* li, int fmt = kFmtCu8);
// args from partition_series (+ stream, out), `grid` what it returned for (li->fpw, the planned grid).  Spectrum k =
// frames [k L, (k + 1) L) of args.stream (frames side by side) -> args.out[k N ..), overwritten; d_partial: scratch of
// 2 x grid x N doubles.  Two enqueues: the persistent kernel, then the fix-up of the spectra cut by workgroup
// boundaries (none with one workgroup).
hipError_t launch_fft_accum_series(int N, bool window, bool use_dma, const SeriesArgs& args, const cf* d_twiddles,
                                   const float* d_window, double* d_partial, int grid, hipStream_t stream,
                                   LaunchInfo* li, int fmt = kFmtCu8);

// The same with per-bin statistics (rpf_kernels_series_stats.hip; the kernels of RPF_FLAG_BIN_STATS engines): row k =
// args.out[3 k N ..) = S1[N], S2[N], PK[N] of spectrum k, what launch_fft_accum(stats) + launch_reduce_stats give for
// the slice; d_partial: 2 x grid x 3 x N doubles, slot s = three planes from d_partial[3 s N ..); the fix-up adds
// planes 0 and 1 in the plain fix-up's order and takes the maximum of plane 2.
bool series_stats_supported(int N, int fmt = kFmtCu8);
hipError_t plan_series_stats(int N, bool window, int device, LaunchInfo* li, int fmt = kFmtCu8);
hipError_t launch_fft_accum_series_stats(int N, bool window, bool use_dma, const SeriesArgs& args, const cf* d_twiddles,
                                         const float* d_window, double* d_partial, int grid, hipStream_t stream,
                                         LaunchInfo* li, int fmt = kFmtCu8);

// ---- the frames' spectra themselves (rpf_kernels_stft*.hip; include/rpf_engine.h, rpf_stft_device) ----
// Variant 0 of every K1 size, all four sample formats.
bool stft_supported(int N, int fmt = kFmtCu8);
// The store kernels' resident grid (kernels of their own, their own register counts).
hipError_t plan_stft(int N, bool window, int device, LaunchInfo* li, int fmt = kFmtCu8);
// d_out[f N .. f N + N) = the float32 transform of frame f = bytes [pitch f, pitch f + bN) of d_stream, f < nframes,
// overwritten; nothing else is written.  pitch as launch_fft_accum's (0 = bN; any other runs the strided kernel, and
// use_dma then also needs pitch % 16 == 0); d_out 16-byte aligned; `grid` <= the planned grid.
hipError_t launch_fft_stft(int N, bool window, bool use_dma, const uint8_t* d_stream, long nframes, const cf* d_twiddles,
                           const float* d_window, cf* d_out, int grid, hipStream_t stream, LaunchInfo* li, long pitch = 0,
                           int fmt = kFmtCu8);

// ---- the excised average over such rows (rpf_excise.hip, excise_core.h) ----
// d_state: excise_state_doubles(N) doubles, one accumulator triple per (row group, bin), owned by one call at a time.
size_t excise_state_doubles(int N);
// One piece: rows [k0, k0 + kc) of the call, d_rows[kc x 3 x N] as the series with statistics writes them (L >= 2 frames
// each), judged by sk_lo <= SK <= sk_hi and added into d_state; first: the call's first piece, d_state starts from zero.
// d_mask: the piece's kc x N bytes, 1 = flagged, or null.
hipError_t launch_excise_rows(const double* d_rows, int64_t kc, int64_t k0, int N, int64_t L, double sk_lo, double sk_hi,
                              double* d_state, uint8_t* d_mask, bool first, hipStream_t stream);
// After the last piece: d_out[3 x N] = clean, kept, total (16-byte aligned), the accumulators added in the fixed order.
hipError_t launch_excise_combine(const double* d_state, int N, double* d_out, hipStream_t stream);

// ---- per-bin quantiles of stored rows (rpf_quantile.hip, quantile_core.h) ----
// Bins whose selection state the workspace holds at a time (a call walks N in such chunks), and the workspace's size.
int quantile_chunk(int N);
size_t quantile_work_bytes(int N);
// d_out[q N + b] = the quantile of ranks (j[q], g[q]) over d_rows[0 .. K)[b], K x N doubles which are only read; d_work:
// quantile_work_bytes(N) bytes, owned by one call at a time (not read for K = 0: every output is then NaN).  j[q] < K.
hipError_t launch_quantile_select(const double* d_rows, int64_t K, int N, const QuantileRanks& ranks, void* d_work,
                                  double* d_out, hipStream_t stream);

// d_out[bin] = (accumulate ? d_out[bin] : 0) + sum_{s < nslots} d_partial[s*stride + bin],
// summed in a fixed order (deterministic).
// slot_stride = distance between partial spectra in elements (0: N).  N even.
// d_skip (may be null): a device word read when the kernel runs; non-zero = leave d_out untouched (the partial
// spectra are not a result: fourstep_fused_abort_word).
hipError_t launch_reduce(const double* d_partial, int nslots, int N, double* d_out,
                         bool accumulate, hipStream_t stream, size_t slot_stride = 0, const unsigned* d_skip = nullptr);
// The same for H hops in one launch: d_out[h*N + bin] from the slots [slots.begin[h], slots.begin[h+1]).
hipError_t launch_reduce_hops(const double* d_partial, const SlotRanges& slots, int H, int N, double* d_out,
                              bool accumulate, hipStream_t stream, size_t slot_stride = 0,
                              const unsigned* d_skip = nullptr);

// ---- mixed-radix path (KM, rpf_mixed.hip): the planned kernel for the sizes of mixed_plans.inc, its split form
// for those of mixed_plans_split.inc (the two tables are the list of sizes), the run-time Stockham kernel for every
// other even N <= 5120 with prime factors 2, 3, 5 only --
// variant: 0 = the shipped kernel of the size; others (tuning build only) = alternative plans
bool mixed_supported(int N, int variant = 0);
hipError_t plan_mixed(int N, int variant, bool windowed, int device, LaunchInfo* li);
// d_twN: master twiddles W_N^k; one partial spectrum of N doubles per workgroup
hipError_t launch_mixed(int N, int variant, const uint8_t* d_stream, long nframes, const cf* d_twN, const float* d_window,
                        double* d_partial, int grid, hipStream_t stream, LaunchInfo* li);

// ---- Bluestein path (KB in rpf_kernels.hip): any other even N <= 4096 ----------
bool bluestein_supported(int N);
hipError_t plan_bluestein(int N, int device, LaunchInfo* li);
// d_twM: master twiddles of length M = bluestein_length(N); d_g / d_bhat: bluestein_tables.h
hipError_t launch_bluestein(int N, const uint8_t* d_stream, long nframes, const cf* d_twM,
                            const cf* d_g, const cf* d_bhat, double* d_partial, int grid,
                            hipStream_t stream, LaunchInfo* li);

// ---- four-step path (rpf_fourstep.hip): N = N1 x N2, powers of two 16384..262144 --
bool fourstep_supported(int N);
size_t fourstep_scratch_bytes(int N);  // the LARGEST intermediate of one launch pair: 2 GB of complex floats, tile-major (rpf_fourstep.hip)
size_t fourstep_scratch_bytes_per_frame(int N);   // the engine grows its scratch to what its launches need, up to the above
int fourstep_partial_slots(int N);     // partial spectra written by K2b (frame groups)
int fourstep_sub_lengths(int N, int* n1, int* n2);
// Host tables in the kernels' lane order: step_tw[n2][.] = W_N^{n2 k1} (N entries),
// window_t[n2][n1] = window[N2 n1 + n2] (empty without a window).
void fourstep_tables(int N, const float* window, std::vector<cf>& step_tw, std::vector<float>& window_t);
hipError_t fourstep_prepare(int N, int device, LaunchInfo* li);
// Frames [0, nframes) -> d_partial[slots][N] (overwritten); K3 then sums the slots.
// d_tw_n1 / d_tw_n2: master twiddle tables of the two sub-transform lengths;
// d_twN / d_window: fourstep_tables' step_tw / window_t.
hipError_t launch_fourstep(int N, bool window, bool use_dma, const uint8_t* d_stream, long nframes,
                           const cf* d_tw_n1, const cf* d_tw_n2, const cf* d_twN, const float* d_window,
                           cf* d_scratch, size_t scratch_bytes, double* d_partial, int max_grid, hipStream_t stream);

// ---- fused four-step (rpf_fourstep.hip): one persistent kernel, Y stays in each XCD's L2 --------
size_t fourstep_fused_scratch_bytes(int N);   // 32 MB: two 2 MB rounds of Y per XCD
int fourstep_fused_slots(int N);              // partial spectra written: 8 teams x frames per round
size_t fourstep_fused_ctl_bytes();
// fails (hipErrorInvalidValue) unless the device has 256 CUs and one workgroup fits a CU
hipError_t fourstep_fused_prepare(int N, int device, int* grid);
// fault (tests only, rpf_debug_fused_fault): 1 = the launch finds 33 workgroups on XCD 0 (gives up at once);
// 2 = a squatter workgroup holds one CU's LDS until the launch has given up (the real failure: ~0.5 - 5 s)
hipError_t launch_fourstep_fused(int N, bool window, bool use_dma, const uint8_t* d_stream, long nframes,
                                 const cf* d_tw_n1, const cf* d_tw_n2, const cf* d_twN, const float* d_window,
                                 cf* d_scratch, double* d_partial, void* d_ctl, hipStream_t stream, int fault = 0);
// The launch's abort flag as a device word (K3's d_skip): valid from the launch until the next one on the same d_ctl.
const unsigned* fourstep_fused_abort_word(const void* d_ctl);
// After K3: what became of the fused launch.  If it raised its abort flag (teams did not assemble): *verdict = 1 and
// ++*aborts (words the host can read: pinned, mapped), and d_out (may be null: K3 was told to skip) is NaN-filled
// -- what a launch that gave up leaves must not look like a spectrum.
hipError_t launch_fused_verdict(const void* d_ctl, double* d_out, int N, unsigned* verdict, unsigned* aborts,
                                hipStream_t stream);
hipError_t fourstep_fused_aborted(const void* d_ctl, hipStream_t stream, bool* aborted);

// ---- large Bluestein path (rpf_fourstep.hip): even N in (4096, 131072], not a power of two --
bool bigblu_supported(int N);
int bigblu_lengths(int N, int* M, int* m1, int* m2);   // M = m1 * m2 = 2^ceil(log2(2N-1))
size_t bigblu_scratch_bytes(int N);    // two intermediates of 2 GB at most
size_t bigblu_scratch_bytes_per_frame(int N);
int bigblu_partial_slots(int N);       // partial spectra of M (not N) doubles each
hipError_t bigblu_prepare(int N, int device, LaunchInfo* li);
// Host tables (each M entries, in the kernels' lane order) from bluestein_tables.h's g (N) and bhat (M).
void bigblu_tables(int N, const cf* g, const cf* bhat, std::vector<cf>& g_t, std::vector<cf>& bhat_t,
                   std::vector<cf>& step_tw, std::vector<cf>& step_tw2);
// d_tw_m1 / d_tw_m2: master twiddles of lengths m1, m2; the rest: bigblu_tables' outputs.
hipError_t launch_bigblu(int N, bool use_dma, const uint8_t* d_stream, long nframes, const cf* d_tw_m1,
                         const cf* d_tw_m2, const cf* d_step_tw, const cf* d_step_tw2, const cf* d_g_t,
                         const cf* d_bhat_t, cf* d_scratch, size_t scratch_bytes, double* d_partial, int max_grid,
                         hipStream_t stream);

// ---- generic path (rpf_generic.hip): every other even N -- powers of two up to 2^26, others up to 2^23 --
bool generic_supported(int N);
int generic_length(int N);              // N, or Bluestein's M = 2^ceil(log2(2N-1))
int generic_batch(int N);
size_t generic_scratch_bytes(int N);
void generic_twiddle_tables(int N, std::vector<cf>& t0, std::vector<cf>& t1, int* h);
// d_pwr[N] = (accumulate ? d_pwr : 0) + sum over the frames; d_window: N floats or null (powers of two);
// d_g (N) / d_bhat (M): bluestein_tables.h's tables (other N).
hipError_t launch_generic(int N, const uint8_t* d_stream, long nframes, const float* d_window, const cf* d_g,
                          const cf* d_bhat, const cf* d_t0, const cf* d_t1, int h, cf* d_scratch, double* d_pwr,
                          bool accumulate, hipStream_t stream, int fmt = kFmtCu8, bool stats = false, cf* d_rows = nullptr);
// stats: d_pwr is three planes, d_pwr[plane * N + bin] = S1, S2, PK (launch_fft_accum), combined over the batches --
// and with what d_pwr holds when `accumulate` -- by +, +, max.
// d_rows (powers of two only; d_pwr, accumulate and stats are then not looked at): instead of squaring and summing, frame
// f's transform X goes to d_rows[f N .. f N + N) in natural order -- the batch loop writes the rows [done, done + nb) --
// by the Stockham transform's own last pass, which is given the rows as its destination: no kernel is added and none
// changes.

// ---- overlapped frames on the other kernel families (rpf_frames.hip) --------------------------------
// d_dst[f * frame_bytes .. (f+1) * frame_bytes) = d_src[f * pitch .. f * pitch + frame_bytes) for f < nframes:
// the frames of a stream with frame step S < N, laid side by side so that a kernel that addresses frames at 2N
// can run over them.  frame_bytes and pitch even; d_src, d_dst 2-byte aligned.
constexpr size_t kGatherBytes = static_cast<size_t>(64) << 20;   // gathered frames per chunk (the engine's scratch)
hipError_t launch_gather_frames(const uint8_t* d_src, long nframes, long pitch, long frame_bytes, uint8_t* d_dst,
                                hipStream_t stream);

// ---- polyphase filter bank front end (rpf_pfb.hip, pfb_core.h) ----------------------------------------
// d_z[f][n] (float32 I/Q, frames side by side, 16-byte aligned) = the fold of include/rpf_engine.h over the input
// frames f .. f + taps - 1 of d_src (frames of N samples of format `fmt` side by side; d_src a multiple of the sample's
// bytes) for f < nframes: nframes + taps - 1 input frames are read.  d_coeffs: taps x N floats, 8-byte aligned.
// taps 1, 2, 3, 4, 8: the sliding-window kernel; any other taps <= 32: the re-reading kernel.  In both a lane walks
// pfb_segment_frames(taps, fmt) output frames.
bool pfb_sliding(int taps);
int pfb_segment_frames(int taps, int fmt);
hipError_t launch_pfb_fold(const uint8_t* d_src, long nframes, int N, int taps, int fmt, const float* d_coeffs, float* d_z,
                           hipStream_t stream);

// ---- cross-spectrum front end (rpf_cross.hip, cross_core.h) ---------------------------------------------
// d_u = a + b and d_v = a + i b (float32 I/Q, 16-byte aligned) for the first `nsamples` complex samples of d_a and d_b
// (format `fmt`; each a multiple of the sample's bytes, read pair by pair where it is a multiple of the pair's).
hipError_t launch_cross_combine(const uint8_t* d_a, const uint8_t* d_b, long nsamples, int fmt, float* d_u, float* d_v,
                                hipStream_t stream);
// d_out[4 x N] = the finishing expression of include/rpf_engine.h over d_planes[4 x N] = Paa, Pbb, Puu, Pvv (not in place).
hipError_t launch_cross_finish(const double* d_planes, int N, double* d_out, hipStream_t stream);

// ---- correlator of up to eight streams (rpf_correlate.hip, correlate_core.h) ------------------------------------------
// The X-engine over rows [0, F) of M cf32 row blocks (block m at d_rows + 2 m stride floats, stride >= F N complex
// values): the M^2 running planes of correlate_plane at d_planes (accumulate: added to), through G frame groups
// (correlate_groups; G > 1 needs d_partial of G M^2 N doubles and adds a reduce launch).
hipError_t launch_correlate_xengine(const float* d_rows, long stride, int M, int N, long F, long G, double* d_partial,
                                    double* d_planes, bool accumulate, hipStream_t stream);
// d_out[M][M][2][N] (Hermitian; diagonal im 0) from the M^2 running planes (not in place).
hipError_t launch_correlate_finish(const double* d_planes, int M, int N, double* d_out, hipStream_t stream);

// ---- incoherent dedispersion of the stored integrations (rpf_dedisperse.hip, dedisperse_core.h) -----------------------
// d_out[D x T] = the sums of include/rpf_engine.h (rpf_dedisperse_device) over rows [0, K) of N doubles: d_delays[D x N]
// and d_weights[N] on the device, every delay in [0, K - T]; d_spans = DedispSpan[trial tiles x bin blocks], dedisperse_span
// of that table and those weights.  T < 1 launches nothing.
hipError_t launch_dedisperse(const double* d_rows, long K, int N, const int32_t* d_delays, const double* d_weights,
                             const void* d_spans, int D, long T, double* d_out, hipStream_t stream);

// ---- fold of a D x T plane at trial periods (rpf_fold.hip, fold_core.h) ------------------------------------------------
// d_prof[series x P x NB] (and d_hits[P x NB], d_mom[series x 2] where not NULL) = the sums of include/rpf_engine.h
// (rpf_fold_device) over d_x[series x T] for the steps d_steps[P] on the device.  d_scratch holds
// fold_scratch(series, P, NB).bytes, at most kFoldScratchBytes.  T < 1 launches nothing.
hipError_t launch_fold(const double* d_x, int series, long T, const uint64_t* d_steps, int P, int NB, void* d_scratch,
                       double* d_prof, int32_t* d_hits, double* d_mom, hipStream_t stream);

// Master twiddle table W_N^k = exp(-2 pi i k / N), k in [0,N), evaluated in
// long double and rounded once to float.
void make_twiddles(int N, std::vector<cf>& out);

}  // namespace rpf
