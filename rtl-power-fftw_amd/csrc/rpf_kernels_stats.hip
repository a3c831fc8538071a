// rpf_kernels_stats.hip -- K1 with per-bin statistics (k1_kernels.h, kK1Stats) for unsigned 8-bit samples, and K3 for
// the statistics.  A translation unit of its own, as rpf_kernels_formats.hip: the plain kernels of rpf_kernels.hip are
// not compiled here and do not change.
#include "k1_kernels.h"

namespace rpf {

namespace {

// K3 for the statistics: reduce_kernel's (rpf_kernels.hip) thread layout and summation order -- thread (g, b) takes
// the slots g, g + GROUPS, ... of bin pair b, UNROLL 16-byte loads in flight, then the GROUPS group results in group
// order -- so that planes 0 and 1 come out bit for bit as launch_reduce would sum them; plane 2 takes the maximum.
// blockIdx.y = plane.
template <int PAIRS, int GROUPS, int UNROLL>
__global__ __launch_bounds__(PAIRS* GROUPS) void reduce_stats_kernel(const double* __restrict__ partial, int nslots, int N,
                                                                     double* __restrict__ out, int accumulate)
{
    typedef double d2 __attribute__((ext_vector_type(2)));
    __shared__ d2 red[GROUPS][PAIRS + 1];
    const int plane = blockIdx.y;
    const size_t stride = static_cast<size_t>(kStatsPlanes) * N;
    const int b = threadIdx.x % PAIRS, g = threadIdx.x / PAIRS;
    const int bin = blockIdx.x * (2 * PAIRS) + 2 * b;            // N is even: a pair never straddles the end
    d2 s = {0.0, 0.0};
    if (bin < N) {
        const double* p = partial + static_cast<size_t>(plane) * N + bin;
        int sl = g;
        for (; sl + (UNROLL - 1) * GROUPS < nslots; sl += UNROLL * GROUPS) {
            d2 v[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
                v[u] = *reinterpret_cast<const d2*>(p + static_cast<size_t>(sl + u * GROUPS) * stride);
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                s.x = stats_combine(plane, s.x, v[u].x);
                s.y = stats_combine(plane, s.y, v[u].y);
            }
        }
        for (; sl < nslots; sl += GROUPS) {
            const d2 v = *reinterpret_cast<const d2*>(p + static_cast<size_t>(sl) * stride);
            s.x = stats_combine(plane, s.x, v.x);
            s.y = stats_combine(plane, s.y, v.y);
        }
    }
    red[g][b] = s;
    __syncthreads();
    if (g == 0 && bin < N) {
        double* o = out + static_cast<size_t>(plane) * N + bin;
        d2 tot = {0.0, 0.0};
        if (accumulate) tot = *reinterpret_cast<const d2*>(o);
#pragma unroll
        for (int k = 0; k < GROUPS; ++k) {
            tot.x = stats_combine(plane, tot.x, red[k][b].x);
            tot.y = stats_combine(plane, tot.y, red[k][b].y);
        }
        *reinterpret_cast<d2*>(o) = tot;
    }
}

}  // namespace

hipError_t launch_reduce_stats(const double* d_partial, int nslots, int N, double* d_out, bool accumulate,
                               hipStream_t stream)
{
    if (nslots < 0 || N < 2 || (N & 1)) return hipErrorInvalidValue;
    constexpr int PAIRS = 8, GROUPS = 16, UNROLL = 8;             // launch_reduce's shape
    const dim3 blocks((N + 2 * PAIRS - 1) / (2 * PAIRS), kStatsPlanes);
    hipLaunchKernelGGL((reduce_stats_kernel<PAIRS, GROUPS, UNROLL>), blocks, dim3(PAIRS * GROUPS), 0, stream, d_partial,
                       nslots, N, d_out, accumulate ? 1 : 0);
    return hipGetLastError();
}

const Variant* k1_stats_variant(int N, int fmt)
{
    return fmt == kFmtCu8 ? find_default_variant<kK1Stats, kFmtCu8>(N) : nullptr;
}

}  // namespace rpf
