// k1_kernels.h -- the K1 kernel templates (fused unpack -> FFT -> |X|^2, rpf_kernels.hip's header comment) and their
// dispatch table entry, shared by the translation units that instantiate them: rpf_kernels.hip (unsigned 8-bit
// samples, the default) and rpf_kernels_formats.hip (signed 8- and 16-bit samples).  Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include "rpf_device_common.h"
#include "rpf_kernels.h"

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
// FMT: the sample format (fft_core.h); 4-byte samples double the pieces and the frame.
template <class G, bool DMA, typename IDX, int FMT = kFmtCu8>
__device__ __forceinline__ void stage_raw(const uint8_t* __restrict__ stream, IDX fb, IDX nframes,
                                          uint8_t* wave_raw, int wave, int lane)
{
    constexpr int PIECES = G::P / 8 * (sample_bytes_of(FMT) / 2);
    constexpr int FRAME_BYTES = sample_bytes_of(FMT) * G::N;
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
        const int j = i * 1024 + lane * 16;
        int slot, off;
        raw_source<G, FMT>(wave, j, &slot, &off);
        IDX f = fb + slot;
        f = f < nframes ? f : nframes - 1;
        const uint8_t* src = stream + static_cast<long>(f) * FRAME_BYTES + off;
        if constexpr (DMA) {
            // LDS address = wave-uniform base + 16 * lane (added by the hardware)
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(wave_raw + i * 1024), 16, 0, 0);
        } else {
            *reinterpret_cast<uint4*>(wave_raw + j) = *reinterpret_cast<const uint4*>(src);
        }
    }
}

// The same at a run-time frame pitch (bytes from one frame's start to the next): the frames of a stream with frame
// step S < N (rpf_config::frame_step) lie 2S apart.  Only the strided K1 uses it.
template <class G, bool DMA, int FMT = kFmtCu8>
__device__ __forceinline__ void stage_raw_pitched(const uint8_t* __restrict__ stream, long fb, long nframes, long pitch,
                                                  uint8_t* wave_raw, int wave, int lane)
{
    constexpr int PIECES = G::P / 8 * (sample_bytes_of(FMT) / 2);
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
        const int j = i * 1024 + lane * 16;
        int slot, off;
        raw_source<G, FMT>(wave, j, &slot, &off);
        long f = fb + slot;
        f = f < nframes ? f : nframes - 1;
        const uint8_t* src = stream + f * pitch + off;
        if constexpr (DMA) {
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(wave_raw + i * 1024), 16, 0, 0);
        } else {
            *reinterpret_cast<uint4*>(wave_raw + j) = *reinterpret_cast<const uint4*>(src);
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
template <class G, int WG, int OCC, bool WINDOW, bool DMA, bool DBUF, int ACCB = 0, bool PF32 = false,
          int RAWD = 2, int ABL = 0, bool TWLDS = false, int FMT = kFmtCu8, bool STATS = false>
__global__ __launch_bounds__(WG, OCC) void fft_accum_kernel(const uint8_t* __restrict__ stream,
                                                            long nframes,
                                                            const cf* __restrict__ twN,
                                                            const float* __restrict__ window,
                                                            double* __restrict__ partial)
{
    constexpr bool STRIDED = false;
    constexpr long pitch = static_cast<long>(sample_bytes_of(FMT)) * G::N;     // (named by the discarded strided branches only)
#include "k1_body.inc"
}

// Overlapped frames (frame step S < N): frame f = bytes [f * pitch, f * pitch + 2N), pitch = 2S.  Frame f still goes
// to workgroup (f / FPW) mod grid, so neighbouring frames -- which share most of their bytes -- are staged by the
// same workgroup a few iterations apart and the shared bytes come back from L2.  A separate instantiation: the
// plain kernel keeps its compile-time 2N.
template <class G, int WG, int OCC, bool WINDOW, bool DMA, bool DBUF, int ACCB = 0, bool PF32 = false,
          int RAWD = 2, int ABL = 0, bool TWLDS = false, int FMT = kFmtCu8, bool STATS = false>
__global__ __launch_bounds__(WG, OCC) void fft_accum_strided_kernel(const uint8_t* __restrict__ stream,
                                                                    long nframes, long pitch,
                                                                    const cf* __restrict__ twN,
                                                                    const float* __restrict__ window,
                                                                    double* __restrict__ partial)
{
    constexpr bool STRIDED = true;
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

// DBUF: two slabs used alternately.  With one slab the pass-1 store of frame f+1
// must wait (workgroup barrier at the top of the loop) until every wave has
// finished reading frame f's slab; with two, the single barrier after the pass-1
// store orders both hazards and a frame costs one s_barrier instead of two, at
// the price of LDS (fewer resident workgroups).
//
// RAWD: depth of the raw-byte ring = iterations staged ahead by LDS-DMA.  The HBM
// latency seen by a DMA under load is several frame times (measured ~3 us vs
// ~1 us of butterflies per frame), so one frame ahead leaves the workgroup idle
// most of the time; RAWD iterations ahead keep RAWD x 2N bytes per frame slot in flight.
// ACCB > 0 (tuning variants): |X|^2 is first summed over ACCB frames in packed
// float32 (one v_pk_fma_f32 per bin instead of four half-rate f64 instructions)
// and only then folded into the f64 accumulators -- adds <= ~1e-7 relative error
// per batch, averaged down over the batches.  PF32: partial spectra leave as
// float32 (half the flush and K3 traffic; each partial is a sum over ~13 frames
// and there are hundreds of them, so the rounding averages out to ~1e-9).
//
// One launch walks the hops of `hops` (a single acquisition is H = 1): workgroup w owns the
// iterations [w I / G, (w + 1) I / G) of the launch's sequence and writes one partial spectrum
// per hop it touched (slot = slot_bias[h] + w), zeroing its register accumulators in between
// -- the reference's per-hop reset (acquisition.cxx:252-254) without a kernel boundary.
template <class G, int WG, int OCC, bool WINDOW, bool DMA, bool DBUF, int ACCB = 0, bool PF32 = false,
          int RAWD = 2, int ABL = 0, bool TWLDS = false, int FMT = kFmtCu8>
__global__ __launch_bounds__(WG, OCC) void fft_accum_scan_kernel(const cf* __restrict__ twN,
                                                            const float* __restrict__ window,
                                                            double* __restrict__ partial,
                                                            const HopArgs hops)
{
    constexpr int P = G::P, T = G::T, N = G::N, NPASS = G::NPASS;
    constexpr int FPW = WG / T;
    constexpr int NSLAB = DBUF ? 2 : 1;
    constexpr bool BLOCK_SYNC = (T > 64);
    static_assert(WG % T == 0 && WG % 64 == 0, "");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    cf* const slab_base = reinterpret_cast<cf*>(smem);                        // [NSLAB][FPW][LDS_CPX]
    uint8_t* const raw_base = smem + NSLAB * FPW * G::LDS_CPX * sizeof(cf);  // [WG/64][RAWD][128 P]

    const int tid = threadIdx.x;
    const int fs = tid / T, t = tid % T;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    constexpr int RAW_SLOT = raw_chunk_of(FMT) * P;   // bytes one wave stages per frame
    constexpr int PIECES = P / 8 * (sample_bytes_of(FMT) / 2);   // DMA instructions per wave per frame
    static_assert((RAWD - 1) * PIECES <= 63, "the counted wait below: vmcnt is a 6-bit field");
    uint8_t* const wave_raw = raw_base + wave * (RAWD * RAW_SLOT);

    // This workgroup's iterations: `count` of them, `step` apart from `first` on (hop_partition.h).
    // The host launches at most one workgroup per iteration (launch_fft_accum checks it), so
    // count >= 1 -- deliberately not tested here: a branch on q and r would put their scalar
    // load in front of the table loads instead of beside them.
    HopLanes tbl;
    tbl.load(hops);
    const int step = hops.step;
    int first, count;
    hop_share(static_cast<int>(blockIdx.x), hops.q, hops.r, step, &first, &count);

    // First thing: get the first iterations' bytes moving (HBM latency overlaps the constant
    // loads below).  The staging cursor `ahead` runs RAWD iterations in front of the compute
    // cursor, across hop boundaries; every iteration issues PIECES DMAs.  The frame loop sees
    // of it only a frame index that advances and a countdown: `ahead_run` stagings stay inside
    // the hop the cursor stands in (scans have step = 1, an interleaved single acquisition
    // never leaves its hop), then ahead_turn() moves the cursor on -- or, when nothing is left
    // to stage, parks it on the launch's iteration 0 with no advance: the same 2N FPW bytes
    // for every workgroup, an L2 hit, so the surplus (never read) stagings that keep the DMA
    // count per iteration constant cost no memory traffic.
    const int fstep = FPW * step;                  // frames between a workgroup's iterations
    HopCursor ahead;
    ahead.seek(tbl, first);
    int ahead_fb = (ahead.j - ahead.begin) * FPW, ahead_fstep = fstep;
    int ahead_left = count;                        // real iterations not staged yet
    auto run_length = [&](const HopCursor& c, int left) {
        const int in_hop = step == 1 ? c.end - c.j : left;
        return in_hop < left ? in_hop : left;
    };
    int ahead_run = run_length(ahead, ahead_left);
    ahead_left -= ahead_run;
    auto ahead_turn = [&]() {
        if (ahead_left > 0) {
            ahead.seek(tbl, ahead.end);            // (step == 1 here: the next hop starts where this one ended)
            ahead_fb = 0;
            ahead_run = run_length(ahead, ahead_left);
            ahead_left -= ahead_run;
        } else {
            ahead.seek(tbl, 0);
            ahead_fb = 0;
            ahead_fstep = 0;
            ahead_run = 0x7fffffff;
        }
    };
    auto stage_next = [&](uint8_t* dst) {
        stage_raw<G, DMA, int, FMT>(ahead.stream, ahead_fb, ahead.nframes, dst, wave, lane);
        ahead_fb += ahead_fstep;
        if (--ahead_run == 0) ahead_turn();
    };
    if constexpr (!(ABL & 8)) {
#pragma unroll
        for (int d = 0; d < RAWD; ++d) stage_next(wave_raw + d * RAW_SLOT);
    }

    // Loop-invariant per-thread constants: twiddles, sign, window.
    cf tw[NPASS - 1][P - 1];
    load_twiddles<G, 1, TWLDS>(t, twN, tw);
    cf* const twtable = reinterpret_cast<cf*>(raw_base + (WG / 64) * RAWD * RAW_SLOT);
    if constexpr (TWLDS) {
        fill_twlds<G, 1>(tid, WG, twN, twtable);
        exchange_sync<true>();
    }
    const float sgn = (t & 1) ? -1.0f : 1.0f;
    float wsgn[P];
    if constexpr (WINDOW) {
#pragma unroll
        for (int a = 0; a < P; ++a) wsgn[a] = window[t + T * a] * sgn;
    }
    double acc[P];
    float acc32[ACCB > 0 ? P : 1];

    PhaseClock clk;
    clk.start();
    HopCursor cur;
    cur.seek(tbl, first);
    int it = 0;                                    // iterations done: ring slot and slab parity
    while (true) {
        // ---- one segment: this workgroup's iterations inside hop cur.h ------------------------
        const int seg = run_length(cur, count - it);
#pragma unroll
        for (int a = 0; a < P; ++a) acc[a] = 0.0;
        if constexpr (ACCB > 0) {
#pragma unroll
            for (int a = 0; a < P; ++a) acc32[a] = 0.0f;
        }
        int fb = (cur.j - cur.begin) * FPW;        // slot-0 frame of the iteration, within the hop
        for (int n = seg; n > 0; --n, ++it, fb += fstep) {
            const bool active = (fb + fs) < cur.nframes;
            cf* const slab = slab_base + ((DBUF ? (it & 1) : 0) * FPW + fs) * G::LDS_CPX;
            uint8_t* const ring_slot = wave_raw + (it % RAWD) * RAW_SLOT;
            cf x[P];

            // this iteration's bytes have landed: every iteration issues exactly PIECES DMA
            // instructions per wave, so all but the newest (RAWD-1) iterations' worth are done
            if constexpr (DMA && !(ABL & 8))
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"((RAWD - 1) * PIECES) : "memory");
            exchange_sync<false>();
            RPF_STAMP(clk, 0);                   // waiting for the staged bytes
            phase_unpack<G, WINDOW, FMT>(ring_slot + sample_bytes_of(FMT) * lane, sgn, wsgn, x);
            // The slot is refilled next: its ds_read_u16 must have RETURNED first (a DMA
            // that hits in L2/MALL can land before queued LDS reads execute -- seen as
            // sporadic 1e-3 errors), so wait for this wave's LDS reads, not just issue.
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            exchange_sync<false>();
            RPF_STAMP(clk, 1);                   // unpack
            // the slot has been consumed: refill it with the iteration RAWD ahead
            if constexpr (!(ABL & 8)) stage_next(ring_slot);
            RPF_STAMP(clk, 3);                   // DMA issue

            // single slab: every wave must be done with the previous frame's slab
            if constexpr (!DBUF) exchange_sync<BLOCK_SYNC>();
            RPF_STAMP(clk, 2);                       // top-of-frame barrier
            middle_passes<G, 1, ABL, TWLDS>(t, x, tw, slab, clk, twtable);   // stamps 4J..4J+3
            if constexpr (!(ABL & 4)) phase_fetch<G, NPASS>(t, x, slab);
            asm volatile("" : "+v"(x[0]));
            RPF_STAMP(clk, 12);                      // last fetch
            if constexpr (!(ABL & 2)) phase_last<G>(x);
            RPF_STAMP(clk, 13);                      // last butterfly
            if constexpr (ACCB > 0) {
                if (active) {
#pragma unroll
                    for (int a = 0; a < P; ++a)
                        acc32[a] = __builtin_fmaf(x[a].x, x[a].x, __builtin_fmaf(x[a].y, x[a].y, acc32[a]));
                }
                if ((it % ACCB) == ACCB - 1) {
#pragma unroll
                    for (int a = 0; a < P; ++a) {
                        acc[a] += static_cast<double>(acc32[a]);
                        acc32[a] = 0.0f;
                    }
                }
            } else if constexpr (ABL & 1) {
#pragma unroll
                for (int a = 0; a < P; ++a) asm volatile("" ::"v"(x[a]));
            } else {
                if (active) phase_accumulate(x, acc, P);
            }
            RPF_STAMP(clk, 14);                      // accumulate
        }
        if constexpr (ACCB > 0) {
#pragma unroll
            for (int a = 0; a < P; ++a) acc[a] += static_cast<double>(acc32[a]);
        }

        // ---- hand the segment over: one partial spectrum (the FPW frame slots summed) ----------
        // The accumulators go through the slab (free between frames; the raw ring with its
        // in-flight prefetches is not touched) so that the bin-scattered registers leave as
        // fully coalesced 512-byte rows: stage at a padded bin index (one spare double per
        // 16, conflict-free for the stride-16 bin pattern of bin_of), then stream out.
        exchange_sync<true>();
        double* const stage = reinterpret_cast<double*>(smem);          // [FPW][N + N/16]
        constexpr int SN = N + N / 16;
        static_assert(sizeof(double) * SN <= sizeof(cf) * G::LDS_CPX, "the stage stays inside the slab");
        // (opaque copies of the thread indices: the hand-over runs once per hop, its sixteen
        // stage addresses must not be hoisted into registers that live across the frame loop)
        int ft = t, ftid = tid, ffs = fs;
        asm volatile("" : "+v"(ft), "+v"(ftid), "+v"(ffs));
#pragma unroll
        for (int a = 0; a < P; ++a) {
            const int bin = bin_of<G>(ft, a);
            stage[ffs * SN + bin + (bin >> 4)] = acc[a];
        }
        exchange_sync<true>();
        const size_t slot = static_cast<size_t>(tbl.slot_bias(cur.h) + static_cast<int>(blockIdx.x));
        if constexpr (PF32) {
            for (int bin = ftid; bin < N; bin += WG) {
                double v = 0.0;
#pragma unroll
                for (int k = 0; k < FPW; ++k) v += stage[k * SN + bin + (bin >> 4)];
                reinterpret_cast<float*>(partial)[slot * N + bin] = static_cast<float>(v);
            }
        } else {
            // two neighbouring bins per lane = one 16-byte store: an 8-byte-per-lane store tail is
            // issue-bound at ~7 B/clk/CU (MI355X_MICROARCH.md), and every workgroup ends in one.
            // Written through (store_partial2), as K1's flush.
            for (int bin = 2 * ftid; bin < N; bin += 2 * WG) {
                partial2_t v = {0.0, 0.0};
#pragma unroll
                for (int k = 0; k < FPW; ++k) {
                    v.x += stage[k * SN + bin + (bin >> 4)];
                    v.y += stage[k * SN + bin + 1 + (bin >> 4)];
                }
                store_partial2(partial + slot * N + bin, v);
            }
        }
        if (it >= count) break;
        // next hop: the slab is reused by its first frame once every wave has read the stage
        exchange_sync<true>();
        cur.seek(tbl, cur.end);                    // (a segment that is not the last ends with its hop)
    }
    clk.publish(lane);
    if constexpr (DMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // trailing (repeated) prefetches
}

}  // namespace

using SingleFn = void (*)(const uint8_t*, long, const cf*, const float*, double*);
using ScanFn = void (*)(const cf*, const float*, double*, const HopArgs);
using StridedFn = void (*)(const uint8_t*, long, long, const cf*, const float*, double*);

struct Variant {
    int N, vid, P, WG, fpw, lds_bytes;
    bool partial_f32;
    SingleFn single[2][2];   // [window][dma]: one acquisition per launch
    ScanFn scan[2][2];       // several hops per launch
    StridedFn strided[2][2]; // one acquisition of overlapped frames (frame pitch a kernel argument)
};

// The instantiations for the signed sample formats (rpf_kernels_formats.hip): variant 0 of every K1 size, or null.
const Variant* find_format_variant(int N, int fmt);
// The instantiations with per-bin statistics (rpf_kernels_stats.hip: cu8; rpf_kernels_stats_formats.hip: cs8, cs16):
// variant 0 of every K1 size, the single-acquisition and strided kernels only (scan entries null), or null.
const Variant* find_stats_variant(int N, int fmt);
const Variant* find_stats_format_variant(int N, int fmt);

namespace {


// OCC (OCCW for the windowed kernels) = waves per SIMD the register budget
// must admit (= resident workgroups per CU x WG/256).  vid = tuning variant
// (0 = the default for this N).
template <int N, int P, int OCC, int OCCW = OCC, bool DBUF = false, int ACCB = 0, bool PF32 = false,
          int RAWD = 2, int ABL = 0, bool TWLDS = false, int WGO = 0, int FMT = kFmtCu8>
Variant make_variant(int vid)
{
    using G = Geom<N, P>;
    constexpr int WG = WGO ? WGO : (G::T >= 256 ? G::T : 256);   // WGO: several frames per workgroup
    constexpr int FPW = WG / G::T;
    constexpr int LDS = FPW * ((DBUF ? 2 : 1) * G::LDS_CPX * (int)sizeof(cf) + RAWD * sample_bytes_of(FMT) * N) +
                        (TWLDS ? twlds_entries<G>() * (int)sizeof(cf) : 0);
    return Variant{N, vid, P, WG, FPW, LDS, PF32,
                   {{fft_accum_kernel<G, WG, OCC, false, false, DBUF, ACCB, PF32, RAWD, ABL, TWLDS, FMT>,
                     fft_accum_kernel<G, WG, OCC, false, true, DBUF, ACCB, PF32, RAWD, ABL, TWLDS, FMT>},
                    {fft_accum_kernel<G, WG, OCCW, true, false, DBUF, ACCB, PF32, RAWD, ABL, TWLDS, FMT>,
                     fft_accum_kernel<G, WG, OCCW, true, true, DBUF, ACCB, PF32, RAWD, ABL, TWLDS, FMT>}},
                   {{fft_accum_scan_kernel<G, WG, OCC, false, false, DBUF, ACCB, PF32, RAWD, ABL, TWLDS, FMT>,
                     fft_accum_scan_kernel<G, WG, OCC, false, true, DBUF, ACCB, PF32, RAWD, ABL, TWLDS, FMT>},
                    {fft_accum_scan_kernel<G, WG, OCCW, true, false, DBUF, ACCB, PF32, RAWD, ABL, TWLDS, FMT>,
                     fft_accum_scan_kernel<G, WG, OCCW, true, true, DBUF, ACCB, PF32, RAWD, ABL, TWLDS, FMT>}},
                   {{fft_accum_strided_kernel<G, WG, OCC, false, false, DBUF, ACCB, PF32, RAWD, ABL, TWLDS, FMT>,
                     fft_accum_strided_kernel<G, WG, OCC, false, true, DBUF, ACCB, PF32, RAWD, ABL, TWLDS, FMT>},
                    {fft_accum_strided_kernel<G, WG, OCCW, true, false, DBUF, ACCB, PF32, RAWD, ABL, TWLDS, FMT>,
                     fft_accum_strided_kernel<G, WG, OCCW, true, true, DBUF, ACCB, PF32, RAWD, ABL, TWLDS, FMT>}}};
}

}  // namespace

}  // namespace rpf
