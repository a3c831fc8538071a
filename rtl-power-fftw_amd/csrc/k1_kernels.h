// k1_kernels.h -- the K1 kernel templates (fused unpack -> FFT -> |X|^2, rpf_kernels.hip's header comment), their
// dispatch table entry and its builder over the size table (k1_sizes.h), shared by the translation units that
// instantiate them (the list is at Variant, below).
#pragma once

#include <hip/hip_runtime.h>

#include <initializer_list>
#include <utility>

#include "k1_loader.h"
#include "k1_sizes.h"
#include "rpf_device_common.h"
#include "rpf_kernels.h"
#include "series_partition.h"
#include "stft_core.h"

namespace rpf {

namespace {

// Stage the raw bytes this wavefront will unpack in the iteration whose slot-0
// frame is `fb` (wave-local, a-major layout: fft_core.h raw_source).  P/8
// instructions per wave, each moving 64 lanes x 16 B = eight 128-byte rows.
// Frames past the end are clamped to the last frame (never accumulated) so that
// every iteration issues the same number of DMA instructions and the counted
// s_waitcnt vmcnt(N) at the top of the frame loop stays exact.
// IDX: the frame index type -- long in the single-acquisition kernel, int in the
// scan kernel (a hop's frames; one 64-bit multiply less per DMA instruction).
// pitch: bytes from one frame's start to the next -- a compile-time b N in every kernel but the strided ones, whose
// frames of a stream with frame step S < N (rpf_config::frame_step) lie b S apart (a kernel argument).
// FMT: the sample format (fft_core.h); 4-byte samples double the pieces and the frame, cf32's 8-byte samples double
// them again (P / 2 pieces: 8 at P = 16, under the 6-bit vmcnt field at every ring depth in use).
// BATCH > 0 (VGPR staging of the windowed cf32 kernels with statistics only, k1_body.inc): no more than BATCH 16-byte
// loads in flight, the pieces go to LDS batch by batch; 0, everywhere else: the compiler's own order, all at once.
template <class G, bool DMA, typename IDX, int FMT = kFmtCu8, int BATCH = 0>
__device__ __forceinline__ void stage_raw(const uint8_t* __restrict__ stream, IDX fb, IDX nframes, long pitch,
                                          uint8_t* wave_raw, int wave, int lane)
{
    constexpr int PIECES = G::P / 8 * (sample_bytes_of(FMT) / 2);
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
        const int j = i * 1024 + lane * 16;
        int slot, off;
        raw_source<G, FMT>(wave, j, &slot, &off);
        IDX f = fb + slot;
        f = f < nframes ? f : nframes - 1;
        const uint8_t* src = stream + static_cast<long>(f) * pitch + off;
        if constexpr (DMA) {
            // LDS address = wave-uniform base + 16 * lane (added by the hardware)
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(wave_raw + i * 1024), 16, 0, 0);
        } else {
            *reinterpret_cast<uint4*>(wave_raw + j) = *reinterpret_cast<const uint4*>(src);
            if constexpr (BATCH > 0) {
                if ((i + 1) % BATCH == 0) asm volatile("" ::: "memory");
            }
        }
    }
}

// ---- K1, one acquisition per launch ------------------------------------------------------
// Frame f -> workgroup (f / FPW) mod grid: at any moment the grid reads one contiguous window of
// the stream.  (The scan kernel below walks several acquisitions per launch; for a single one
// this plain form measured 1.2 us per launch faster on the same box -- A/B in
// profiles/r03_k1_fixed_cost.txt -- so rpf_accumulate / rpf_accumulate_device keep it.)
// STATS (RPF_FLAG_BIN_STATS, instantiated in rpf_kernels_stats*.hip only): two more double accumulators per bin, the
// sum of the squared powers and the largest power, and three partial planes per workgroup (k1_body.inc).
// LDW: loader waves (k1_loader.h).  The workgroup is launched with WG + 64 LDW threads; WG stays the threads that own
// frames.  The waves per SIMD the register budget must admit follow from the launched size (nine or ten waves: three).
template <class G, int WG, int OCC, bool WINDOW, bool DMA, int RAWD = 2, int ABL = 0, bool TWLDS = false,
          int FMT = kFmtCu8, bool STATS = false, int LDW = 0>
__global__ __launch_bounds__(WG + 64 * LDW, LDW ? (WG / 64 + LDW + 3) / 4 : OCC)
void fft_accum_kernel(const uint8_t* __restrict__ stream, long nframes, const cf* __restrict__ twN,
                      const float* __restrict__ window, double* __restrict__ partial)
{
    constexpr bool STRIDED = false;
    constexpr long pitch = static_cast<long>(sample_bytes_of(FMT)) * G::N;     // frames side by side (stage_raw)
#include "k1_body.inc"
}

// Overlapped frames (frame step S < N): frame f = bytes [f * pitch, f * pitch + 2N), pitch = 2S.  Frame f still goes
// to workgroup (f / FPW) mod grid, so neighbouring frames -- which share most of their bytes -- are staged by the
// same workgroup a few iterations apart and the shared bytes come back from L2.  A separate instantiation: the
// plain kernel keeps its compile-time 2N.
template <class G, int WG, int OCC, bool WINDOW, bool DMA, int RAWD = 2, int ABL = 0, bool TWLDS = false,
          int FMT = kFmtCu8, bool STATS = false>
__global__ __launch_bounds__(WG, OCC) void fft_accum_strided_kernel(const uint8_t* __restrict__ stream,
                                                                    long nframes, long pitch,
                                                                    const cf* __restrict__ twN,
                                                                    const float* __restrict__ window,
                                                                    double* __restrict__ partial)
{
    constexpr bool STRIDED = true;
    constexpr int LDW = 0;
#include "k1_body.inc"
}


// ---- K1, a scan of several acquisitions per launch -----------------------------------------
__device__ __forceinline__ void write_lane(int& v, int uniform_value, int lane_const)
{
    asm("v_writelane_b32 %0, %1, %2" : "+v"(v) : "s"(uniform_value), "n"(lane_const));
}

struct HopLanes {
    int v_nframes, v_begin, v_bias;
    unsigned v_stream_lo, v_stream_hi;
    // Scalar loads at constant offsets (a few s_load_dwordx16 through the scalar cache, the path
    // every kernel argument takes), then one v_writelane per entry.
    __device__ __forceinline__ void load(const HopArgs& a)
    {
        int nf = 0, bg = 0, bs = 0, lo = 0, hi = 0;
#pragma unroll
        for (int h = 0; h < kMaxHops; ++h) {
            const uintptr_t p = reinterpret_cast<uintptr_t>(a.stream[h]);
            write_lane(nf, a.nframes[h], h);
            write_lane(bg, a.it_begin[h], h);
            write_lane(bs, a.slot_bias[h], h);
            write_lane(lo, static_cast<int>(static_cast<unsigned>(p)), h);
            write_lane(hi, static_cast<int>(static_cast<unsigned>(p >> 32)), h);
        }
        write_lane(bg, a.it_begin[kMaxHops], kMaxHops);
        v_nframes = nf;
        v_begin = bg;
        v_bias = bs;
        v_stream_lo = static_cast<unsigned>(lo);
        v_stream_hi = static_cast<unsigned>(hi);
    }
    __device__ __forceinline__ int it_begin(int h) const { return __builtin_amdgcn_readlane(v_begin, h); }
    __device__ __forceinline__ int nframes(int h) const { return __builtin_amdgcn_readlane(v_nframes, h); }
    __device__ __forceinline__ int slot_bias(int h) const { return __builtin_amdgcn_readlane(v_bias, h); }
    __device__ __forceinline__ const uint8_t* stream(int h) const
    {
        const uintptr_t lo = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(v_stream_lo), h));
        const uintptr_t hi = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(v_stream_hi), h));
        return reinterpret_cast<const uint8_t*>(lo | (hi << 32));
    }
    // number of hop starts 1 .. kMaxHops at or before `it` (HopArgsView::hop_of)
    __device__ __forceinline__ int hop_of(int it) const
    {
        const int lane = static_cast<int>(__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)));
        const unsigned long long m = __builtin_amdgcn_ballot_w64(lane >= 1 && lane <= kMaxHops && v_begin <= it);
        return __builtin_popcountll(m);
    }
};

// the output rows of a series launch (k1_scan_body.inc; the scan kernel has none and never asks)
__device__ __forceinline__ double* series_rows(const HopArgs&) { return nullptr; }
__device__ __forceinline__ double* series_rows(const SeriesArgs& a) { return a.out; }

// One exchange slab per frame slot: the pass-1 store of frame f+1 waits (workgroup
// barrier at the top of the loop) until every wave has finished reading frame f's slab.
//
// RAWD: depth of the raw-byte ring = iterations staged ahead by LDS-DMA.  The HBM
// latency seen by a DMA under load is several frame times (measured ~3 us vs
// ~1 us of butterflies per frame), so one frame ahead leaves the workgroup idle
// most of the time; RAWD iterations ahead keep RAWD x 2N bytes per frame slot in flight.
//
// One launch walks the hops of `hops` (a single acquisition is H = 1): workgroup w owns the
// iterations [w I / G, (w + 1) I / G) of the launch's sequence and writes one partial spectrum
// per hop it touched (slot = slot_bias[h] + w), zeroing its register accumulators in between
// -- the reference's per-hop reset (acquisition.cxx:252-254) without a kernel boundary.
template <class G, int WG, int OCC, bool WINDOW, bool DMA, int RAWD = 2, int ABL = 0, bool TWLDS = false,
          int FMT = kFmtCu8>
__global__ __launch_bounds__(WG, OCC) void fft_accum_scan_kernel(const cf* __restrict__ twN,
                                                            const float* __restrict__ window,
                                                            double* __restrict__ partial,
                                                            const HopArgs hops)
{
    constexpr bool SERIES = false, STATS = false;
    using TABLE = HopLanes;
#include "k1_scan_body.inc"
}

// ---- K1, a uniform series of spectra per launch ---------------------------------------------
// The scan kernel's frame loop and hand-over over an arithmetic table (series_partition.h): spectrum k = the L frames
// from frame k L of one stream, as many spectra as the launch's 2^31 iterations hold.  A spectrum that lies inside one
// workgroup's range goes straight to its row of hops.out; one that is cut leaves its segments in the partial slots
// 2w / 2w + 1 for series_fixup_kernel.  Instantiated in rpf_kernels_series.hip only.
template <class G, int WG, int OCC, bool WINDOW, bool DMA, int RAWD = 2, int ABL = 0, bool TWLDS = false,
          int FMT = kFmtCu8>
__global__ __launch_bounds__(WG, OCC) void fft_accum_series_kernel(const cf* __restrict__ twN,
                                                              const float* __restrict__ window,
                                                              double* __restrict__ partial,
                                                              const SeriesArgs hops)
{
    constexpr bool SERIES = true, STATS = false;
    using TABLE = SeriesTable;
#include "k1_scan_body.inc"
}

// The series kernel with per-bin statistics (rpf_accumulate_device_series_stats): S2 and PK accumulated beside the
// power as in fft_accum_kernel's STATS form, zeroed at every spectrum; row k of hops.out and every partial slot are
// three planes of N, S1, S2, PK, handed over one after the other.  A kernel of its own name, so that the plain series
// kernels keep theirs.  Instantiated in rpf_kernels_series_stats.hip only.
template <class G, int WG, int OCC, bool WINDOW, bool DMA, int RAWD = 2, int ABL = 0, bool TWLDS = false,
          int FMT = kFmtCu8>
__global__ __launch_bounds__(WG, OCC) void fft_accum_series_stats_kernel(const cf* __restrict__ twN,
                                                                    const float* __restrict__ window,
                                                                    double* __restrict__ partial,
                                                                    const SeriesArgs hops)
{
    constexpr bool SERIES = true, STATS = true;
    using TABLE = SeriesTable;
#include "k1_scan_body.inc"
}

// ---- K1, the frames' spectra themselves (rpf_stft_device) ------------------------------------
// The plain kernel's frame loop with the spectrum stored where the plain kernel squares it: row f of `out` = the N
// float32 (re, im) of frame f in natural bin order (k1_stft_body.inc, stft_core.h).  The template arguments are the plain
// kernels' without the accumulate ones; one exchange slab per frame slot.  Kernels of their own names, instantiated in
// rpf_kernels_stft*.hip only: no other kernel moves.
typedef float stft_pair_t __attribute__((ext_vector_type(4)));   // two neighbouring bins: one 16-byte LDS read and store

template <class G, int WG, int OCC, bool WINDOW, bool DMA, int RAWD = 2, bool TWLDS = false, int FMT = kFmtCu8>
__global__ __launch_bounds__(WG, OCC) void fft_stft_kernel(const uint8_t* __restrict__ stream, long nframes,
                                                           const cf* __restrict__ twN,
                                                           const float* __restrict__ window, cf* __restrict__ out)
{
    constexpr long pitch = static_cast<long>(sample_bytes_of(FMT)) * G::N;     // frames side by side (stage_raw)
#include "k1_stft_body.inc"
}

template <class G, int WG, int OCC, bool WINDOW, bool DMA, int RAWD = 2, bool TWLDS = false, int FMT = kFmtCu8>
__global__ __launch_bounds__(WG, OCC) void fft_stft_strided_kernel(const uint8_t* __restrict__ stream, long nframes,
                                                                   long pitch, const cf* __restrict__ twN,
                                                                   const float* __restrict__ window,
                                                                   cf* __restrict__ out)
{
#include "k1_stft_body.inc"
}

}  // namespace

using SingleFn = void (*)(const uint8_t*, long, const cf*, const float*, double*);
using ScanFn = void (*)(const cf*, const float*, double*, const HopArgs);
using StridedFn = void (*)(const uint8_t*, long, long, const cf*, const float*, double*);
using SeriesFn = void (*)(const cf*, const float*, double*, const SeriesArgs);
using StftFn = void (*)(const uint8_t*, long, const cf*, const float*, cf*);
using StftStridedFn = void (*)(const uint8_t*, long, long, const cf*, const float*, cf*);

// One geometry of one size and the kernels instantiated for it, each as [window][dma]; a unit leaves the kernels it
// does not instantiate null (K1Kernels).
struct Variant {
    int N, vid, P;
    K1Geometry geo;
    int single_ldw[2][2];    // loader waves of single[window][dma]: its launch is geo.with_loader(...); no other kernel has any
    SingleFn single[2][2];   // one acquisition per launch
    ScanFn scan[2][2];       // several hops per launch
    StridedFn strided[2][2]; // one acquisition of overlapped frames (frame pitch a kernel argument)
    SeriesFn series[2][2];   // a uniform series of spectra per launch (kK1SeriesStats: of three-plane statistics)
    StftFn stft[2][2];       // the frames' spectra themselves, frames side by side (kK1Stft only)
    StftStridedFn stft_strided[2][2];   // ... of overlapped frames
};

// Variant 0 of every K1 size, one finder per translation unit so that the units compile side by side; each answers
// for its own sample formats and returns null for the others.  find_variant (rpf_kernels.hip) is the one entry the
// launch code uses and picks among the first six; the series kernels are looked up where they are launched.
// cf32 has no series kernel without statistics: its plain series run spectrum by spectrum (rpf_engine.cpp).  No form
// of any finder is null: every size x window x staging form is instantiated, none with scratch.
//   k1_variant                   rpf_kernels.hip                   cu8        single, scan, strided
//   k1_format_variant            rpf_kernels_formats.hip           cs8, cs16  single, scan, strided
//   k1_cf32_variant              rpf_kernels_cf32.hip              cf32       single, scan, strided
//   k1_stats_variant             rpf_kernels_stats.hip             cu8        single, strided with per-bin statistics
//   k1_stats_format_variant      rpf_kernels_stats_formats.hip     cs8, cs16  single, strided with per-bin statistics
//   k1_stats_cf32_variant        rpf_kernels_stats_cf32.hip        cf32       single, strided with per-bin statistics
//   k1_series_variant            rpf_kernels_series.hip            cu8, cs8, cs16 (null for cf32)  series
//   k1_series_stats_variant      rpf_kernels_series_stats.hip      cu8, cs8, cs16, and cf32 by way of the next
//                                                                             series with per-bin statistics
//   k1_series_stats_cf32_variant rpf_kernels_series_stats_cf32.hip cf32       series with per-bin statistics
//   k1_stft_variant              rpf_kernels_stft.hip              cu8        stft, stft_strided
//   k1_stft_format_variant       rpf_kernels_stft_formats.hip      cs8, cs16  stft, stft_strided
//   k1_stft_cf32_variant         rpf_kernels_stft_cf32.hip         cf32       stft, stft_strided
const Variant* k1_variant(int N, int fmt);
const Variant* k1_format_variant(int N, int fmt);
const Variant* k1_cf32_variant(int N, int fmt);
const Variant* k1_stats_variant(int N, int fmt);
const Variant* k1_stats_format_variant(int N, int fmt);
const Variant* k1_stats_cf32_variant(int N, int fmt);
const Variant* k1_series_variant(int N, int fmt);
const Variant* k1_series_stats_variant(int N, int fmt);
const Variant* k1_series_stats_cf32_variant(int N, int fmt);
const Variant* k1_stft_variant(int N, int fmt);
const Variant* k1_stft_format_variant(int N, int fmt);
const Variant* k1_stft_cf32_variant(int N, int fmt);

// The resident grid of kernels that share one launch geometry on `device`: for each kernel (null entries skipped) the
// dynamic-LDS attribute is set and its occupancy asked; *grid = max(the smallest, 1) x CUs.  rpf_kernels.hip.
hipError_t plan_resident_grid(std::initializer_list<const void*> kernels, const K1Geometry& geo, int device, int* grid);

// What a plan or a launch reports (li may be null).  `slots` is not K1's to set.
inline void fill_info(LaunchInfo* li, const K1Geometry& geo, int grid)
{
    if (!li) return;
    li->grid = grid;
    li->block = geo.WG;               // the threads that own frames, loader waves not counted
    li->fpw = geo.fpw;
    li->lds_bytes = geo.lds_bytes;
}

namespace {

// The kernels a Variant names: kK1Plain single, scan and strided; kK1Stats single and strided with STATS (a scan of
// a stats engine runs hop by hop); kK1Series the series kernel alone, with the geometry of the size's scan kernel;
// kK1SeriesStats the series kernel with statistics alone, with the geometry of the size's statistics kernels;
// kK1Stft the two store kernels alone, with the geometry of the size's plain kernels.
enum K1Kernels { kK1Plain, kK1Stats, kK1Series, kK1SeriesStats, kK1Stft };

// the [window][dma] instantiations of one kernel template; the arguments are its template arguments after TWLDS
#define RPF_K1_FORMS(KERNEL, ...)                                           \
    {{KERNEL<G, WG, OCC, false, false, RAWD, ABL, TWLDS, __VA_ARGS__>,       \
      KERNEL<G, WG, OCC, false, true, RAWD, ABL, TWLDS, __VA_ARGS__>},       \
     {KERNEL<G, WG, OCCW, true, false, RAWD, ABL, TWLDSW, __VA_ARGS__>,      \
      KERNEL<G, WG, OCCW, true, true, RAWD, ABL, TWLDSW, __VA_ARGS__>}}

// ... of the single-acquisition kernel, whose LDS-DMA entry without a window alone takes the loader waves
#define RPF_K1_SINGLE_FORMS(STATS)                                                                \
    {{fft_accum_kernel<G, WG, OCC, false, false, RAWD, ABL, TWLDS, FMT, STATS, 0>,                 \
      fft_accum_kernel<G, WG, OCC, false, true, RAWD, ABL, TWLDS, FMT, STATS, LDW>},               \
     {fft_accum_kernel<G, WG, OCCW, true, false, RAWD, ABL, TWLDSW, FMT, STATS, 0>,                \
      fft_accum_kernel<G, WG, OCCW, true, true, RAWD, ABL, TWLDSW, FMT, STATS, 0>}}
#define RPF_K1_SINGLE_LDW {{0, LDW}, {0, 0}}

// ... of a store kernel, whose template arguments are the plain kernels' without the accumulate ones
#define RPF_K1_STFT_FORMS(KERNEL)                                                \
    {{KERNEL<G, WG, OCC, false, false, RAWD, TWLDS, FMT>,                         \
      KERNEL<G, WG, OCC, false, true, RAWD, TWLDS, FMT>},                         \
     {KERNEL<G, WG, OCCW, true, false, RAWD, TWLDSW, FMT>,                        \
      KERNEL<G, WG, OCCW, true, true, RAWD, TWLDSW, FMT>}}

// The template arguments are K1Size's (k1_sizes.h) and the kernels' (above).  vid = tuning variant (0 = the default
// for this N).
template <int N, int P, int OCC, int OCCW = OCC, int RAWD = 2, int ABL = 0, bool TWLDS = false, int WGO = 0,
          int FMT = kFmtCu8, bool TWLDSW = TWLDS, K1Kernels KERNELS = kK1Plain, int LDW = 0>
Variant make_variant(int vid)
{
    using G = Geom<N, P>;
    constexpr K1Geometry geo = k1_geometry<G>(WGO, 1, RAWD, FMT, TWLDS || TWLDSW);
    constexpr int WG = geo.WG;
    if constexpr (KERNELS == kK1Stft)
        return Variant{N, vid, P, geo, {}, {}, {}, {}, {}, RPF_K1_STFT_FORMS(fft_stft_kernel),
                       RPF_K1_STFT_FORMS(fft_stft_strided_kernel)};
    else if constexpr (KERNELS == kK1Series)
        return Variant{N, vid, P, geo, {}, {}, {}, {}, RPF_K1_FORMS(fft_accum_series_kernel, FMT)};
    else if constexpr (KERNELS == kK1SeriesStats)
        return Variant{N, vid, P, geo, {}, {}, {}, {}, RPF_K1_FORMS(fft_accum_series_stats_kernel, FMT)};
    else if constexpr (KERNELS == kK1Stats)
        return Variant{N, vid, P, geo, RPF_K1_SINGLE_LDW, RPF_K1_SINGLE_FORMS(true), {},
                       RPF_K1_FORMS(fft_accum_strided_kernel, FMT, true), {}};
    else
        return Variant{N, vid, P, geo, RPF_K1_SINGLE_LDW, RPF_K1_SINGLE_FORMS(false),
                       RPF_K1_FORMS(fft_accum_scan_kernel, FMT), RPF_K1_FORMS(fft_accum_strided_kernel, FMT, false), {}};
}
#undef RPF_K1_FORMS
#undef RPF_K1_SINGLE_FORMS
#undef RPF_K1_SINGLE_LDW
#undef RPF_K1_STFT_FORMS

// Variant 0 of every row of the size table for one sample format and one set of kernels, and its look-up by N.
template <K1Kernels KERNELS, int FMT, int I>
Variant default_variant()
{
    constexpr K1Size s = k1_size(I, FMT, KERNELS == kK1Stats || KERNELS == kK1SeriesStats);
    static_assert(k1_geometry<Geom<s.N, s.P>>(s.WGO, 1, s.RAWD, FMT, s.TWLDS || s.TWLDSW).lds_bytes <= kLdsPerCU,
                  "a workgroup's LDS fits the CU");
    return make_variant<s.N, s.P, s.OCC, s.OCCW, s.RAWD, 0, s.TWLDS, s.WGO, FMT, s.TWLDSW, KERNELS, s.LDW>(0);
}
template <K1Kernels KERNELS, int FMT, int... I>
const Variant* find_default_variant(int N, std::integer_sequence<int, I...>)
{
    static const Variant table[] = {default_variant<KERNELS, FMT, I>()...};
    for (const Variant& v : table)
        if (v.N == N) return &v;
    return nullptr;
}
template <K1Kernels KERNELS, int FMT>
const Variant* find_default_variant(int N)
{
    return find_default_variant<KERNELS, FMT>(N, std::make_integer_sequence<int, kK1SizeCount>{});
}
// ... for the two signed formats, which share a unit wherever they are instantiated
template <K1Kernels KERNELS>
const Variant* find_signed_variant(int N, int fmt)
{
    return fmt == kFmtCs8    ? find_default_variant<KERNELS, kFmtCs8>(N)
           : fmt == kFmtCs16 ? find_default_variant<KERNELS, kFmtCs16>(N)
                             : nullptr;
}

}  // namespace

}  // namespace rpf
