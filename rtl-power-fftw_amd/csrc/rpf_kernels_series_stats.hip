// rpf_kernels_series_stats.hip -- K1 for a uniform series of per-bin statistics
// (rpf_accumulate_device_series_stats): fft_accum_series_stats_kernel (k1_kernels.h, k1_scan_body.inc under STATS) for
// variant 0 of every K1 size x {plain, windowed} x {LDS-DMA, VGPR staging} x {cu8, cs8, cs16} (cf32: the unit beside
// this one, rpf_kernels_series_stats_cf32.hip, behind the same finder), and the fix-up kernel
// that combines the segments of the spectra a workgroup boundary cuts, plane by plane.  A translation unit of its own,
// as rpf_kernels_series.hip: it compiles beside the others and none of their kernels moves.
#include "k1_kernels.h"

namespace rpf {

namespace {

// series_fixup_kernel (rpf_kernels_series.hip) with a plane dimension: blockIdx.z = plane, rows and partial slots are
// kStatsPlanes x N doubles, plane p at p N.  The same blocks leave, the same thread (g, b) takes the same segments in
// the same order; planes 0 and 1 add (plane 0 bit for bit as the plain fix-up adds the same segments), plane 2 takes
// the maximum (stats_combine; every segment's peak is >= 0, so starting from 0 is starting from nothing).
template <int PAIRS, int GROUPS>
__global__ __launch_bounds__(PAIRS* GROUPS) void series_stats_fixup_kernel(const double* __restrict__ partial,
                                                                           const SeriesArgs a, int N)
{
    typedef double d2 __attribute__((ext_vector_type(2)));
    __shared__ d2 red[GROUPS][PAIRS + 1];
    const int bnd = static_cast<int>(blockIdx.y) + 1;
    const int plane = static_cast<int>(blockIdx.z);
    int lo, hi;
    hop_range(bnd, a.q, a.r, &lo, &hi);
    const int k = series_div(lo, a.magic, a.shift);
    if (k * a.ips == lo) return;                                  // the boundary separates two spectra
    int wa, wb;
    series_spectrum_wgs(k, a, &wa, &wb);
    if (wa != bnd - 1) return;                                    // an earlier boundary's block writes this row
    const int nseg = wb - wa + 1;
    const size_t stride = static_cast<size_t>(kStatsPlanes) * N;
    const int b = threadIdx.x % PAIRS, g = threadIdx.x / PAIRS;
    const int bin = blockIdx.x * (2 * PAIRS) + 2 * b;             // N is even: a pair never straddles the end
    d2 s = {0.0, 0.0};
    if (bin < N) {
        for (int j = g; j < nseg; j += GROUPS) {
            const size_t slot = static_cast<size_t>(2 * (wa + j) + (j == 0 ? 1 : 0));
            const d2 v = *reinterpret_cast<const d2*>(partial + slot * stride + static_cast<size_t>(plane) * N + bin);
            s.x = stats_combine(plane, s.x, v.x);
            s.y = stats_combine(plane, s.y, v.y);
        }
    }
    red[g][b] = s;
    __syncthreads();
    if (g == 0 && bin < N) {
        d2 tot = {0.0, 0.0};
#pragma unroll
        for (int j = 0; j < GROUPS; ++j) {
            tot.x = stats_combine(plane, tot.x, red[j][b].x);
            tot.y = stats_combine(plane, tot.y, red[j][b].y);
        }
        *reinterpret_cast<d2*>(a.out + static_cast<size_t>(k) * stride + static_cast<size_t>(plane) * N + bin) = tot;
    }
}

}  // namespace

const Variant* k1_series_stats_variant(int N, int fmt)
{
    // (cf32: the kernels of rpf_kernels_series_stats_cf32.hip; plan, launch and fix-up below are format-free)
    if (fmt == kFmtCf32) return k1_series_stats_cf32_variant(N, fmt);
    return fmt == kFmtCu8 ? find_default_variant<kK1SeriesStats, kFmtCu8>(N) : find_signed_variant<kK1SeriesStats>(N, fmt);
}

bool series_stats_supported(int N, int fmt) { return k1_series_stats_variant(N, fmt) != nullptr; }

hipError_t plan_series_stats(int N, bool window, int device, LaunchInfo* li, int fmt)
{
    const Variant* v = k1_series_stats_variant(N, fmt);
    if (!v) return hipErrorInvalidValue;
    const int w = window ? 1 : 0;
    int grid = 0;
    // the two staging forms share one grid
    hipError_t err = plan_resident_grid({reinterpret_cast<const void*>(v->series[w][0]),
                                         reinterpret_cast<const void*>(v->series[w][1])}, v->geo, device, &grid);
    if (err != hipSuccess) return err;
    fill_info(li, v->geo, grid);
    return hipSuccess;
}

hipError_t launch_fft_accum_series_stats(int N, bool window, bool use_dma, const SeriesArgs& args, const cf* d_twiddles,
                                         const float* d_window, double* d_partial, int grid, hipStream_t stream,
                                         LaunchInfo* li, int fmt)
{
    const Variant* v = k1_series_stats_variant(N, fmt);
    if (!v || grid < 1 || grid > args.total || args.K < 1 || !args.stream || !args.out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(v->series[window ? 1 : 0][use_dma ? 1 : 0], dim3(grid), dim3(v->geo.WG), v->geo.lds_bytes, stream,
                       d_twiddles, d_window, d_partial, args);
    fill_info(li, v->geo, grid);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess || grid < 2) return err;       // one workgroup: every spectrum is complete
    constexpr int PAIRS = 8, GROUPS = 16;
    const dim3 blocks((N + 2 * PAIRS - 1) / (2 * PAIRS), grid - 1, kStatsPlanes);
    hipLaunchKernelGGL((series_stats_fixup_kernel<PAIRS, GROUPS>), blocks, dim3(PAIRS * GROUPS), 0, stream, d_partial, args, N);
    return hipGetLastError();
}

}  // namespace rpf
