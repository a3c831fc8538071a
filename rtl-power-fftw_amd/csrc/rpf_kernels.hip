// rpf_kernels.hip -- gfx950 (CDNA4) kernels of the power-spectrum engine.
//
// K1  fft_accum_kernel   fused  u8-IQ unpack -> (-1)^n -> window -> FFT -> |X|^2 (f64)
//                        replaces the body of Datastore::fftThread
//                        (/root/reference/src/datastore.cxx:66-89).
// K3  reduce_kernel      deterministic sum of the per-workgroup partial spectra
//                        into pwr[N] (Datastore::pwr, datastore.h:53).
//
// K1 layout.  One frame (N complex samples = 2N bytes of HBM) is owned by
// T = N/P threads holding P points each; a 256-thread (or T-thread, if larger)
// workgroup runs WG/T frames side by side and walks the stream persistently
// (frame f -> workgroup (f / FPW) mod grid).  Per frame:
//   1. the 2N raw bytes arrive in LDS by LDS-DMA (global_load_lds_dwordx4,
//      16 B per lane, fully coalesced, no VGPR round trip), issued one frame
//      ahead so the HBM latency hides under the previous frame's butterflies;
//   2. each thread picks its P samples (stride T) out of LDS with ds_read_u16,
//      converts (v_cvt_f32_ubyteN), removes the 127 offset, applies (-1)^n and
//      the window -- all exact except the single window rounding;
//   3. radix-P butterflies in registers, twiddles held in registers for the
//      whole kernel, one padded LDS exchange between passes (bank-conflict
//      free, fft_core.h); exchanges that stay inside a wavefront need no
//      s_barrier;
//   4. |X|^2 is added in double into P per-thread register accumulators that
//      live for the whole kernel; they are written once, at the end, as one
//      partial spectrum per frame slot.
// HBM traffic per frame is therefore exactly the 2N input bytes; the kernel is
// bound by VALU + LDS, not by HBM (DESIGN.md has the numbers).  No MFMA.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <type_traits>

#include <algorithm>

#include "bluestein_tables.h"
#include "k1_kernels.h"

namespace rpf {

namespace {

// KB  bluestein_kernel -- any even N <= 4096 that is not one of K1's powers of two
// (bluestein_tables.h).  G = Geom<M, P> with M = 2^ceil(log2(2N-1)); per frame:
//   a[n] = (v[n] - 127) * g[n] for n < N, zero-padded to M      (g carries (-1)^n, window, chirp)
//   A = FFT_M(a);  z = conj(A * bhat);  c = FFT_M(z)            (= conj of the circular convolution)
//   pwr[k] += |c[k]|^2 for k < N                                (|X[k]| = |c[k]|)
// The two transforms reuse K1's passes; between them the spectrum goes through
// the slab once more (digit-reversed -> natural order).  Samples are read
// straight from HBM as coalesced u16 loads (frames are only 4-byte aligned).
template <class G, int WG, int OCC, bool TWLDS>
__global__ __launch_bounds__(WG, OCC) void bluestein_kernel(const uint8_t* __restrict__ stream,
                                                            long nframes, int N,
                                                            const cf* __restrict__ twM,
                                                            const cf* __restrict__ g,
                                                            const cf* __restrict__ bhat,
                                                            double* __restrict__ partial)
{
    constexpr int P = G::P, T = G::T, M = G::N, NPASS = G::NPASS;
    constexpr int FPW = WG / T;
    constexpr bool BLOCK_SYNC = (T > 64);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int fs = tid / T, t = tid % T;
    cf* const slab = reinterpret_cast<cf*>(smem) + fs * G::LDS_CPX;

    cf tw[NPASS - 1][P - 1];
    load_twiddles<G, 1, TWLDS>(t, twM, tw);
    cf* const twtable = reinterpret_cast<cf*>(smem) + FPW * G::LDS_CPX;
    if constexpr (TWLDS) {
        fill_twlds<G, 1>(tid, WG, twM, twtable);
        exchange_sync<true>();
    }
    PhaseClock noclk;
    double acc[P];
#pragma unroll
    for (int a = 0; a < P; ++a) acc[a] = 0.0;

    const long stride = static_cast<long>(gridDim.x) * FPW;
    for (long fb = static_cast<long>(blockIdx.x) * FPW; fb < nframes; fb += stride) {
        const bool active = (fb + fs) < nframes;
        const uint8_t* const frame = stream + (fb + fs) * 2 * static_cast<long>(N);
        cf x[P];
#pragma unroll
        for (int a = 0; a < P; ++a) {
            const int n = t + T * a;
            x[a] = cf{0.0f, 0.0f};
            if (active && n < N) {
                const uint32_t iq = *reinterpret_cast<const uint16_t*>(frame + 2 * n);
                const cf v = iq_plus_2p23(iq) - (kTwo23 + 127.0f);
                x[a] = cmul(v, g[n]);
            }
        }
        exchange_sync<BLOCK_SYNC>();             // previous frame's slab reads are done
        middle_passes<G, 1, 0, TWLDS>(t, x, tw, slab, noclk, twtable);
        phase_fetch<G, NPASS>(t, x, slab);
        phase_last<G>(x);
        exchange_sync<BLOCK_SYNC>();             // ... before the slab is rewritten in another order
#pragma unroll
        for (int a = 0; a < P; ++a) {
            const int j = bin_of<G>(t, a);
            cf z = cmul(x[a], bhat[j]);
            z.y = -z.y;
            slab[G::slot(j)] = z;
        }
        exchange_sync<BLOCK_SYNC>();
        phase_fetch<G, 1>(t, x, slab);           // natural order: lane t gets elements t + T a
        middle_passes<G, 1, 0, TWLDS>(t, x, tw, slab, noclk, twtable);   // its pass-1 store rewrites exactly those slots
        phase_fetch<G, NPASS>(t, x, slab);
        phase_last<G>(x);
        if (active) phase_accumulate(x, acc, P);
    }

    // partial spectrum: only the first N of the M convolution outputs are bins
    exchange_sync<true>();
    double* const stage = reinterpret_cast<double*>(smem);
    constexpr int SM = M + M / 16;
#pragma unroll
    for (int a = 0; a < P; ++a) {
        const int bin = bin_of<G>(t, a);
        stage[fs * SM + bin + (bin >> 4)] = acc[a];
    }
    exchange_sync<true>();
    double* out = partial + static_cast<size_t>(blockIdx.x) * N;
    for (int bin = tid; bin < N; bin += WG) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < FPW; ++k) v += stage[k * SM + bin + (bin >> 4)];
        out[bin] = v;
    }
}

// K3.  out[hop][bin] = (accumulate ? out[hop][bin] : 0) + the partial spectra of the hop's slot
// range, in a fixed order (bit-reproducible for a given grid): thread (g, b) sums the slots
// g, g+GROUPS, g+2 GROUPS, ... of the bin pair b -- 16-byte loads, UNROLL of them in flight -- then
// the GROUPS group sums are added in group order.  blockIdx.y = hop.
// skip (may be null): a device word; non-zero = the partial spectra are not a result (the fused four-step
// kernel gave up) and `out` is left as it is.
// RPF_REDUCE_LOAD (A/B builds): cache policy of K3's partial-spectrum loads, 0 plain, 1 nt.
#ifndef RPF_REDUCE_LOAD
#define RPF_REDUCE_LOAD 0
#endif
template <typename V>
__device__ __forceinline__ V load_partial2(const V* p)
{
#if RPF_REDUCE_LOAD == 1
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}

template <typename PT, int PAIRS, int GROUPS, int UNROLL>
__global__ __launch_bounds__(PAIRS* GROUPS) void reduce_kernel(
    const PT* __restrict__ partial, const SlotRanges slots, int N, double* __restrict__ out,
    int accumulate, size_t stride, const unsigned* __restrict__ skip)
{
    typedef PT pt2 __attribute__((ext_vector_type(2)));
    typedef double d2 __attribute__((ext_vector_type(2)));
    __shared__ d2 red[GROUPS][PAIRS + 1];
    if (skip != nullptr && *skip != 0) return;
    const int hop = blockIdx.y;
    const int first = slots.begin[hop], nslots = slots.begin[hop + 1] - first;
    const int b = threadIdx.x % PAIRS, g = threadIdx.x / PAIRS;
    const int bin = blockIdx.x * (2 * PAIRS) + 2 * b;            // N is even: a pair never straddles the end
    d2 s = {0.0, 0.0};
    if (bin < N) {
        const PT* p = partial + static_cast<size_t>(first) * stride + bin;
        int sl = g;
        for (; sl + (UNROLL - 1) * GROUPS < nslots; sl += UNROLL * GROUPS) {
            pt2 v[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
                v[u] = load_partial2(reinterpret_cast<const pt2*>(p + static_cast<size_t>(sl + u * GROUPS) * stride));
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                s.x += v[u].x;
                s.y += v[u].y;
            }
        }
        for (; sl < nslots; sl += GROUPS) {
            const pt2 v = load_partial2(reinterpret_cast<const pt2*>(p + static_cast<size_t>(sl) * stride));
            s.x += v.x;
            s.y += v.y;
        }
    }
    red[g][b] = s;
    __syncthreads();
    if (g == 0 && bin < N) {
        double* o = out + static_cast<size_t>(hop) * N + bin;
        d2 tot = {0.0, 0.0};
        if (accumulate) tot = *reinterpret_cast<const d2*>(o);
#pragma unroll
        for (int k = 0; k < GROUPS; ++k) {
            tot.x += red[k][b].x;
            tot.y += red[k][b].y;
        }
        *reinterpret_cast<d2*>(o) = tot;
    }
}

}  // namespace

// ---------------------------------------------------------------- dispatch --
// (Defined ahead of the tables below: kernels are emitted in the order their tables are first named, and the
// instruction stream of bluestein_kernel<Geom<8192, 16>> was seen to differ when K1's came after it.)
const Variant* k1_variant(int N, int fmt)
{
    return fmt == kFmtCu8 ? find_default_variant<kK1Plain, kFmtCu8>(N) : nullptr;
}

namespace {

#ifdef RPF_TUNING
#include "k1_tuning.inc"
#endif

// Variant 0 of a size is the size table's (k1_sizes.h), from the unit that instantiates the format's kernels
// (k1_kernels.h); any other variant is one of the tuning build's experiments (cu8 without statistics only).
const Variant* find_variant(int N, int vid, int fmt = kFmtCu8, bool stats = false)
{
    if (vid == 0) {
        if (fmt == kFmtCu8) return stats ? k1_stats_variant(N, fmt) : k1_variant(N, fmt);
        if (fmt == kFmtCf32) return stats ? k1_stats_cf32_variant(N, fmt) : k1_cf32_variant(N, fmt);
        return stats ? k1_stats_format_variant(N, fmt) : k1_format_variant(N, fmt);
    }
#ifdef RPF_TUNING
    if (!stats && fmt == kFmtCu8)
        for (const Variant& v : kTuningVariants)
            if (v.N == N && v.vid == vid) return &v;
#endif
    return nullptr;
}

using BluesteinFn = void (*)(const uint8_t*, long, int, const cf*, const cf*, const cf*, double*);
struct BluesteinVariant {
    int M;
    K1Geometry geo;
    BluesteinFn fn;
};
template <int M, int P, int OCC, bool TWLDS = false>
BluesteinVariant make_bluestein()
{
    using G = Geom<M, P>;
    constexpr K1Geometry geo = k1_geometry<G>(0, 1, 0, kFmtCu8, TWLDS);      // one slab per frame slot, no raw ring
    return BluesteinVariant{M, geo, bluestein_kernel<G, geo.WG, OCC, TWLDS>};
}
const BluesteinVariant kBluestein[] = {
    make_bluestein<64, 8, 4>(),    make_bluestein<128, 8, 4>(),   make_bluestein<256, 8, 4>(),
    // P = 8 up to M = 1024; from M = 2048 on, 16 points per lane with the pass-2/3
    // twiddles in an LDS table (one pass and one exchange less per transform; with
    // register twiddles two inlined 16-point transforms spill even at 256 VGPRs).
    // Measured: M = 4096 +24 %, 2048 +6 %, 1024 +-0, 512 -6 %.
    make_bluestein<512, 8, 4>(),   make_bluestein<1024, 8, 2>(),  make_bluestein<2048, 16, 2, true>(),
    make_bluestein<4096, 16, 2, true>(),  make_bluestein<8192, 16, 2, true>(),
};
const BluesteinVariant* find_bluestein(int M)
{
    for (const BluesteinVariant& v : kBluestein)
        if (v.M == M) return &v;
    return nullptr;
}

}  // namespace

bool kernel_supported(int N, int vid) { return find_variant(N, vid) != nullptr; }

#ifdef RPF_PHASE_TIMING
extern "C" int rpf_debug_phase_cycles(unsigned long long* out16, unsigned long long* waves, int reset)
{
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_phase_cycles), sizeof(unsigned long long) * kPhaseSlots) != hipSuccess) return 1;
    if (hipMemcpyFromSymbol(waves, HIP_SYMBOL(g_phase_waves), sizeof(unsigned long long)) != hipSuccess) return 1;
    if (reset) {
        unsigned long long z[kPhaseSlots] = {0};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_phase_cycles), z, sizeof(z));
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_phase_waves), z, sizeof(unsigned long long));
    }
    return 0;
}

// the seam marks of the K1 launches since the last reset (RPF_SEAM_MARK): out[kSeamWgs][kSeamMarks]
extern "C" int rpf_debug_seam_marks(unsigned long long* out, int* nwgs, int reset)
{
    *nwgs = kSeamWgs;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_seam_marks), sizeof(g_seam_marks)) != hipSuccess) return 1;
    if (reset) {
        static unsigned long long z[kSeamWgs][kSeamMarks];
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_seam_marks), z, sizeof(z));
    }
    return 0;
}
#endif

hipError_t plan_resident_grid(std::initializer_list<const void*> kernels, const K1Geometry& geo, int device, int* grid)
{
    int per_cu = 1 << 30;
    for (const void* fn : kernels) {
        if (!fn) continue;
        hipError_t err = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, geo.lds_bytes);
        if (err != hipSuccess) return err;
        int n = 0;
        err = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, geo.launched, geo.lds_bytes);
        if (err != hipSuccess) return err;
        per_cu = std::min(per_cu, n);
    }
    hipDeviceProp_t prop;
    hipError_t err = hipGetDeviceProperties(&prop, device);
    if (err != hipSuccess) return err;
    *grid = std::max(per_cu, 1) * prop.multiProcessorCount;
    return hipSuccess;
}

hipError_t plan_launch(int N, int vid, bool window, bool use_dma, int device, LaunchInfo* li, int fmt, bool stats)
{
    const Variant* v = find_variant(N, vid, fmt, stats);
    if (!v) return hipErrorInvalidValue;
    const int w = window ? 1 : 0, d = use_dma ? 1 : 0;
    int grid = 0, grid1 = 0;
    // the single-acquisition, scan and strided instantiations share one grid (the statistics kernels have no scan
    // form): the smaller of what the single kernel admits at its launched size, loader waves included, and the others
    hipError_t err = plan_resident_grid({reinterpret_cast<const void*>(v->single[w][d])},
                                        v->geo.with_loader(v->single_ldw[w][d]), device, &grid1);
    if (err != hipSuccess) return err;
    err = plan_resident_grid({reinterpret_cast<const void*>(v->scan[w][d]),
                              reinterpret_cast<const void*>(v->strided[w][d])}, v->geo, device, &grid);
    if (err != hipSuccess) return err;
    fill_info(li, v->geo, std::min(grid, grid1));
    return hipSuccess;
}

hipError_t launch_fft_accum(int N, int vid, bool window, bool use_dma, const uint8_t* d_stream,
                            long nframes, const cf* d_twiddles, const float* d_window,
                            double* d_partial, int grid, hipStream_t stream, LaunchInfo* li, long pitch, int fmt, bool stats)
{
    const Variant* v = find_variant(N, vid, fmt, stats);
    const long sb = sample_bytes_of(fmt);
    if (!v || grid < 1 || pitch < 0 || pitch > sb * N || (pitch % sb)) return hipErrorInvalidValue;
    if (pitch == 0 || pitch == sb * N)
        hipLaunchKernelGGL(v->single[window ? 1 : 0][use_dma ? 1 : 0], dim3(grid),
                           dim3(v->geo.with_loader(v->single_ldw[window ? 1 : 0][use_dma ? 1 : 0]).launched),
                           v->geo.lds_bytes, stream, d_stream, nframes, d_twiddles, d_window, d_partial);
    else
        hipLaunchKernelGGL(v->strided[window ? 1 : 0][use_dma ? 1 : 0], dim3(grid), dim3(v->geo.launched), v->geo.lds_bytes,
                           stream, d_stream, nframes, pitch, d_twiddles, d_window, d_partial);
    fill_info(li, v->geo, grid);
    return hipGetLastError();
}

hipError_t launch_fft_accum_hops(int N, int vid, bool window, bool use_dma, const HopArgs& hops,
                                 const cf* d_twiddles, const float* d_window, double* d_partial, int grid,
                                 hipStream_t stream, LaunchInfo* li, int fmt)
{
    const Variant* v = find_variant(N, vid, fmt);
    if (!v || grid < 1 || hops.H < 1 || hops.H > kMaxHops || grid > hops.total) return hipErrorInvalidValue;
    hipLaunchKernelGGL(v->scan[window ? 1 : 0][use_dma ? 1 : 0], dim3(grid), dim3(v->geo.launched), v->geo.lds_bytes, stream,
                       d_twiddles, d_window, d_partial, hops);
    fill_info(li, v->geo, grid);
    return hipGetLastError();
}

bool bluestein_supported(int N)
{
    return N >= 2 && N % 2 == 0 && N <= 4096 && !kernel_supported(N, 0) &&
           find_bluestein(bluestein_length(N)) != nullptr;
}

hipError_t plan_bluestein(int N, int device, LaunchInfo* li)
{
    const BluesteinVariant* v = bluestein_supported(N) ? find_bluestein(bluestein_length(N)) : nullptr;
    if (!v) return hipErrorInvalidValue;
    int grid = 0;
    hipError_t err = plan_resident_grid({reinterpret_cast<const void*>(v->fn)}, v->geo, device, &grid);
    if (err != hipSuccess) return err;
    fill_info(li, v->geo, grid);
    return hipSuccess;
}

hipError_t launch_bluestein(int N, const uint8_t* d_stream, long nframes, const cf* d_twM,
                            const cf* d_g, const cf* d_bhat, double* d_partial, int grid,
                            hipStream_t stream, LaunchInfo* li)
{
    const BluesteinVariant* v = bluestein_supported(N) ? find_bluestein(bluestein_length(N)) : nullptr;
    if (!v || grid < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(v->fn, dim3(grid), dim3(v->geo.WG), v->geo.lds_bytes, stream, d_stream, nframes, N, d_twM,
                       d_g, d_bhat, d_partial);
    fill_info(li, v->geo, grid);
    return hipGetLastError();
}

namespace {
template <typename PT, int PAIRS, int GROUPS, int UNROLL>
void launch_reduce_shape(const PT* d_partial, const SlotRanges& slots, int H, int N, double* d_out, bool accumulate,
                         hipStream_t stream, size_t stride, const unsigned* d_skip = nullptr)
{
    const dim3 blocks((N + 2 * PAIRS - 1) / (2 * PAIRS), H);
    hipLaunchKernelGGL((reduce_kernel<PT, PAIRS, GROUPS, UNROLL>), blocks, dim3(PAIRS * GROUPS), 0, stream, d_partial,
                       slots, N, d_out, accumulate ? 1 : 0, stride, d_skip);
}
}  // namespace

hipError_t launch_reduce_hops(const double* d_partial, const SlotRanges& slots, int H, int N, double* d_out,
                              bool accumulate, hipStream_t stream, size_t slot_stride, const unsigned* d_skip)
{
    if (H < 1 || H > kMaxHops) return hipErrorInvalidValue;
    const size_t stride = slot_stride ? slot_stride : static_cast<size_t>(N);
    // one block shape: seven were measured in situ behind K1 within 0.3 us of each other (profiles/r03_k3_shapes.txt)
    launch_reduce_shape<double, 8, 16, 8>(d_partial, slots, H, N, d_out, accumulate, stream, stride, d_skip);
    return hipGetLastError();
}

hipError_t launch_reduce(const double* d_partial, int nslots, int N, double* d_out,
                         bool accumulate, hipStream_t stream, size_t slot_stride, const unsigned* d_skip)
{
    SlotRanges one;
    one.begin[0] = 0;
    for (int h = 1; h <= kMaxHops; ++h) one.begin[h] = nslots;
    return launch_reduce_hops(d_partial, one, 1, N, d_out, accumulate, stream, slot_stride, d_skip);
}

void make_twiddles(int N, std::vector<cf>& out)
{
    out.resize(N);
    const long double two_pi = 6.283185307179586476925286766559005768L;
    for (int k = 0; k < N; ++k) {
        const long double a = two_pi * static_cast<long double>(k) / static_cast<long double>(N);
        out[k].x = static_cast<float>(cosl(a));
        out[k].y = static_cast<float>(-sinl(a));
    }
}

}  // namespace rpf
