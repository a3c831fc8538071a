// rpf_correlate.hip -- the kernels of the correlator of up to eight streams (include/rpf_engine.h, rpf_correlate_device).
//
// correlate_xengine<M>: the X-engine.  Reads the cf32 rows of M streams that the store kernels left (block m holds rows
// [0, F) of stream m, `stride` complex values apart) and forms every pair's per-frame term (correlate_core.h) in double.
// A lane owns one bin and a workgroup is one wave of 64 consecutive bins, so a wave reads 512 contiguous bytes per
// stream row and frame.  The M(M+1)/2 re and M(M-1)/2 im sums live in registers (64 doubles at M = 8).  The grid is
// bins x frame groups (correlate_groups): with one group a lane writes, or adds, its sums straight into the running
// planes; with several it writes partial planes that correlate_reduce adds in the order of the groups.  No LDS, no
// atomics: the order of every sum is fixed by N, M and F, and is the same for every pair.
//
// correlate_reduce: running plane p (+)= the partial planes of groups 0, 1, ..., G - 1, added in that order.
// correlate_finish: the Hermitian M x M x 2 x N layout from the running planes, one (cell, bin) per lane.
//
// Format-free and memory-bound; no scratch in any instantiation (profiles/correlate_resources.txt).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "correlate_core.h"
#include "rpf_kernels.h"

namespace rpf {

namespace {

constexpr int kCorrelateWG = 256;       // the reduce and the finish
constexpr int kReduceLoads = 8;         // the reduce's partial planes in flight per lane

template <int M>
__global__ __launch_bounds__(kCorrelateBins) void correlate_xengine_kernel(const float2* __restrict__ rows, long stride, int N,
                                                                           long F, long G, double* __restrict__ partial,
                                                                           double* __restrict__ planes, int accumulate)
{
    constexpr int kRe = M * (M + 1) / 2, kIm = M * (M - 1) / 2;
    const int k = blockIdx.x * kCorrelateBins + threadIdx.x;
    if (k >= N) return;
    const long g = blockIdx.y;
    const long f1 = correlate_group_begin(F, G, g + 1);
    double re[kRe], im[kIm > 0 ? kIm : 1];
#pragma unroll
    for (int r = 0; r < kRe; ++r) re[r] = 0.0;
#pragma unroll
    for (int q = 0; q < kIm; ++q) im[q] = 0.0;
    const float2* p = rows + k;
#pragma unroll 2
    for (long f = correlate_group_begin(F, G, g); f < f1; ++f) {
        float2 x[M];
#pragma unroll
        for (int m = 0; m < M; ++m) x[m] = p[m * stride + f * N];
        int r = 0, q = 0;
#pragma unroll
        for (int i = 0; i < M; ++i) {
#pragma unroll
            for (int j = i; j < M; ++j) {
                double t_re, t_im;
                correlate_term(x[i].x, x[i].y, x[j].x, x[j].y, t_re, t_im);
                re[r++] += t_re;
                if (j > i) im[q++] += t_im;
            }
        }
    }
    const long n = N;
    int r = 0, q = 0;
#pragma unroll
    for (int i = 0; i < M; ++i) {
#pragma unroll
        for (int j = i; j < M; ++j) {
            const int pr = correlate_plane(M, i, j, 0);
            if (G == 1) {
                double* d = planes + pr * n + k;
                *d = accumulate ? *d + re[r] : re[r];
            } else {
                partial[(g * M * M + pr) * n + k] = re[r];
            }
            ++r;
            if (j > i) {
                const int pi = correlate_plane(M, i, j, 1);
                if (G == 1) {
                    double* d = planes + pi * n + k;
                    *d = accumulate ? *d + im[q] : im[q];
                } else {
                    partial[(g * M * M + pi) * n + k] = im[q];
                }
                ++q;
            }
        }
    }
}

__global__ __launch_bounds__(kCorrelateWG) void correlate_reduce_kernel(const double* __restrict__ partial, int planes_count, int N,
                                                                        long G, double* __restrict__ planes, int accumulate)
{
    const int k = blockIdx.x * kCorrelateWG + threadIdx.x;
    if (k >= N) return;
    const long n = N, p = blockIdx.y, stride = static_cast<long>(planes_count) * n;
    const double* src = partial + p * n + k;
    double s = src[0];
    long g = 1;
    // eight loads in flight, the additions still one after the other in group order: few lanes (M^2 N) walk G partials
    for (; g + kReduceLoads <= G; g += kReduceLoads) {
        double v[kReduceLoads];
#pragma unroll
        for (int u = 0; u < kReduceLoads; ++u) v[u] = src[(g + u) * stride];
#pragma unroll
        for (int u = 0; u < kReduceLoads; ++u) s += v[u];
    }
    for (; g < G; ++g) s += src[g * stride];
    double* d = planes + p * n + k;
    *d = accumulate ? *d + s : s;
}

__global__ __launch_bounds__(kCorrelateWG) void correlate_finish_kernel(const double* __restrict__ planes, int M, int N,
                                                                        double* __restrict__ out)
{
    const int k = blockIdx.x * kCorrelateWG + threadIdx.x;
    if (k >= N) return;
    const int cell = blockIdx.y, i = cell / M, j = cell % M;
    const long n = N;
    double re, im;
    if (i <= j) {
        re = planes[correlate_plane(M, i, j, 0) * n + k];
        im = i < j ? planes[correlate_plane(M, i, j, 1) * n + k] : 0.0;
    } else {
        re = planes[correlate_plane(M, j, i, 0) * n + k];
        im = -planes[correlate_plane(M, j, i, 1) * n + k];
    }
    out[(2 * static_cast<long>(cell)) * n + k] = re;
    out[(2 * static_cast<long>(cell) + 1) * n + k] = im;
}

}  // namespace

hipError_t launch_correlate_xengine(const float* d_rows, long stride, int M, int N, long F, long G, double* d_partial,
                                    double* d_planes, bool accumulate, hipStream_t stream)
{
    if (F < 1) return hipSuccess;
    if (!d_rows || !d_planes || N < 1 || G < 1 || G > F || (G > 1 && !d_partial) || stride < F * N || G > 65535)
        return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>(correlate_bin_blocks(N)), static_cast<unsigned>(G)), block(kCorrelateBins);
    const float2* rows = reinterpret_cast<const float2*>(d_rows);
    const int acc = accumulate ? 1 : 0;
#define RPF_XENGINE(MM) \
    case MM: hipLaunchKernelGGL((correlate_xengine_kernel<MM>), grid, block, 0, stream, rows, stride, N, F, G, d_partial, d_planes, acc); break
    switch (M) {
        RPF_XENGINE(2);
        RPF_XENGINE(3);
        RPF_XENGINE(4);
        RPF_XENGINE(5);
        RPF_XENGINE(6);
        RPF_XENGINE(7);
        RPF_XENGINE(8);
        default: return hipErrorInvalidValue;
    }
#undef RPF_XENGINE
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess || G == 1) return rc;
    hipLaunchKernelGGL(correlate_reduce_kernel, dim3((N + kCorrelateWG - 1) / kCorrelateWG, M * M), dim3(kCorrelateWG), 0, stream,
                       d_partial, M * M, N, G, d_planes, acc);
    return hipGetLastError();
}

hipError_t launch_correlate_finish(const double* d_planes, int M, int N, double* d_out, hipStream_t stream)
{
    if (!d_planes || !d_out || N < 1 || M < kCorrelateMinStreams || M > kCorrelateMaxStreams) return hipErrorInvalidValue;
    hipLaunchKernelGGL(correlate_finish_kernel, dim3((N + kCorrelateWG - 1) / kCorrelateWG, M * M), dim3(kCorrelateWG), 0, stream,
                       d_planes, M, N, d_out);
    return hipGetLastError();
}

}  // namespace rpf
