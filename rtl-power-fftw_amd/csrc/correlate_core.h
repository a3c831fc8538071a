// correlate_core.h -- what the correlator of up to eight streams (include/rpf_engine.h, rpf_correlate_device) states
// once: the per-frame term, the pair -> plane map of the running sums, the frame-group partition of the X-engine and the
// chunk rule of the rows scratch.
//
// Plain C++: the kernels (rpf_correlate.hip), the engine (rpf_engine.cpp) and the CPU tests
// (tests/emul/correlate_emul.cpp) share what is below, so they cannot drift.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RPF_CORR_HD __host__ __device__ __forceinline__
#else
#define RPF_CORR_HD inline
#endif

namespace rpf {

constexpr int kCorrelateMinStreams = 2;
constexpr int kCorrelateMaxStreams = 8;
constexpr size_t kCorrelateChunkBytes = static_cast<size_t>(64) << 20;     // rows of ONE stream per chunk
constexpr size_t kCorrelatePartialBytes = static_cast<size_t>(64) << 20;   // the X-engine's partial planes, at most
constexpr int kCorrelateBins = 64;                  // bins of one X-engine workgroup: one wave, a lane per bin
constexpr int64_t kCorrelateTargetWaves = 4096;     // 256 CUs x 16 waves: the X-engine's grid where N alone does not fill it
constexpr int64_t kCorrelateMinGroupFrames = 64;    // a frame group sums at least this many frames (where F allows)

// The term of frame f at bin k for a = X_i,f[k] and b = X_j,f[k] (float32 values, converted to double): both products
// of float32 values are exact in double, so each fma rounds once and t equals numpy's ar*br + ai*bi and ai*br - ar*bi on
// float64 copies bit for bit, whatever contraction a compiler applies.
RPF_CORR_HD void correlate_term(float ar, float ai, float br, float bi, double& re, double& im)
{
    const double a_re = ar, a_im = ai, b_re = br, b_im = bi;
    re = std::fma(a_re, b_re, a_im * b_im);
    im = std::fma(a_im, b_re, -(a_re * b_im));
}

// The M x M running planes of N doubles each: Re V_ij of i <= j in plane i M + j (the upper triangle and the diagonal),
// Im V_ij of i < j in plane j M + i (the lower triangle).  A bijection onto the M^2 planes.  c = 0: re, 1: im.
RPF_CORR_HD int correlate_plane(int M, int i, int j, int c)
{
    return c == 0 ? i * M + j : j * M + i;
}

// Frames per chunk of the rows scratch: as many rows of 8 N bytes as fit 64 MB, at least one (2048 at 4096 bins).
inline int64_t correlate_chunk_frames(int N)
{
    return std::max<int64_t>(1, static_cast<int64_t>(kCorrelateChunkBytes / (sizeof(float) * 2 * static_cast<size_t>(N))));
}

// X-engine workgroups along the bins.
RPF_CORR_HD int64_t correlate_bin_blocks(int N) { return (N + kCorrelateBins - 1) / kCorrelateBins; }

// Frame groups G of an X-engine launch over F frames of M streams: one where the bins alone give kCorrelateTargetWaves
// workgroups; else enough to reach that many, but at least kCorrelateMinGroupFrames frames per group and partial planes
// of at most kCorrelatePartialBytes.  1 <= G <= max(F, 1); fixed for a given N, M and F.
inline int64_t correlate_groups(int N, int M, int64_t F)
{
    const int64_t blocks = correlate_bin_blocks(N);
    int64_t g = (kCorrelateTargetWaves + blocks - 1) / blocks;
    g = std::min(g, std::max<int64_t>(1, F / kCorrelateMinGroupFrames));
    const size_t group_bytes = sizeof(double) * static_cast<size_t>(M) * static_cast<size_t>(M) * static_cast<size_t>(N);
    g = std::min(g, std::max<int64_t>(1, static_cast<int64_t>(kCorrelatePartialBytes / group_bytes)));
    return std::max<int64_t>(1, g);
}

// Group g of G sums frames [correlate_group_begin(F, G, g), correlate_group_begin(F, G, g + 1)).
RPF_CORR_HD int64_t correlate_group_begin(int64_t F, int64_t G, int64_t g) { return g * F / G; }

}  // namespace rpf
