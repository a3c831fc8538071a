// rpf_pfb.hip -- the fold of the polyphase filter bank front end (include/rpf_engine.h, rpf_engine_create_pfb).
//
// Output frame f of the chunk, column n:  z = sum over t < T of h[tN + n] x[(f + t)N + n]  (pfb_core.h has the exact
// expression), written as float32 I/Q frames side by side -- a cf32 stream the unchanged transform of a rectangular
// cf32 engine then reads.  Memory-bound: b bytes in and 8 bytes out per complex sample.
//
// A lane owns one PAIR of adjacent complex samples of the row (N is even): it loads 4 (8-bit formats), 8 (cs16) or 16
// (cf32) bytes per input frame and stores 16 bytes per output frame; consecutive lanes own consecutive pairs, so a
// wavefront reads 256 B .. 1 KB and writes 1 KB of each row in one piece.  The rows are a whole number of pairs long,
// so the base address alone decides the access width: a stream that starts at a multiple of the pair's bytes is read
// pair by pair (ALIGNED), any other (an odd sample offset) sample by sample -- the widest access that divides the base
// address, the row bytes and the pitch, as rpf_frames.hip picks it.  The output is engine scratch, 16-byte aligned.
//
//   sliding form (T = 1, 2, 3, 4, 8): the lane walks a segment of pfb_segment_frames() consecutive output frames with
//     its T coefficient pairs and the last T converted input frames in registers; the frame loop is unrolled by T so
//     the ring index is a compile-time constant.  Inside a segment every input byte is loaded once; a segment loads
//     the T - 1 halo frames before its first new one again, which its neighbour has just brought into L2.
//   re-reading form (every other T <= 32, run-time T): each output from T loads; the reuse comes from L2.
//
// No LDS, no scratch (profiles/pfb_resources.txt).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "pfb_core.h"
#include "rpf_kernels.h"

namespace rpf {

namespace {

constexpr int kPfbWG = 256;

// The raw bytes of one pair of complex samples.
template <int FMT>
struct PairRaw {
    static constexpr int kBytes = 4 * pfb_value_bytes(FMT);
    union {
        uint8_t b[kBytes];
        uint16_t h[kBytes / 2];
        uint32_t w[kBytes >= 4 ? kBytes / 4 : 1];
    };
};

// ALIGNED: p is a multiple of the pair's bytes -- one access; else p is a multiple of the sample's bytes -- two.
template <int FMT, bool ALIGNED>
__device__ __forceinline__ void load_pair(const uint8_t* __restrict__ p, float (&x)[4])
{
    PairRaw<FMT> raw;
    if constexpr (FMT == kPfbCf32) {
        if constexpr (ALIGNED) {
            const uint4 v = *reinterpret_cast<const uint4*>(p);
            raw.w[0] = v.x; raw.w[1] = v.y; raw.w[2] = v.z; raw.w[3] = v.w;
        } else {
            const uint2 a = *reinterpret_cast<const uint2*>(p), c = *reinterpret_cast<const uint2*>(p + 8);
            raw.w[0] = a.x; raw.w[1] = a.y; raw.w[2] = c.x; raw.w[3] = c.y;
        }
    } else if constexpr (FMT == kPfbCs16) {
        if constexpr (ALIGNED) {
            const uint2 v = *reinterpret_cast<const uint2*>(p);
            raw.w[0] = v.x; raw.w[1] = v.y;
        } else {
            raw.w[0] = *reinterpret_cast<const uint32_t*>(p);
            raw.w[1] = *reinterpret_cast<const uint32_t*>(p + 4);
        }
    } else {
        if constexpr (ALIGNED) {
            raw.w[0] = *reinterpret_cast<const uint32_t*>(p);
        } else {
            raw.h[0] = *reinterpret_cast<const uint16_t*>(p);
            raw.h[1] = *reinterpret_cast<const uint16_t*>(p + 2);
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) x[c] = pfb_value<FMT>(raw.b + c * pfb_value_bytes(FMT));
}

// Thread g of the launch: pair g % (N/2) of segment g / (N/2); segment s = output frames [s L, min((s + 1) L, nframes)).
// Input frames [0, nframes + T - 1) are read, output frames [0, nframes) written.
template <int FMT, int T, bool ALIGNED>
__global__ __launch_bounds__(kPfbWG) void pfb_fold_sliding_kernel(const uint8_t* __restrict__ src, long nframes, int N,
                                                                  const float* __restrict__ coeffs, float4* __restrict__ dst,
                                                                  int L)
{
    const long half = N / 2;
    const long g = static_cast<long>(blockIdx.x) * kPfbWG + threadIdx.x;
    const long seg = g / half, p = g - seg * half;
    const long f0 = seg * L;
    if (f0 >= nframes) return;
    const long f1 = min(f0 + static_cast<long>(L), nframes);
    constexpr long kPair = PairRaw<FMT>::kBytes;
    const long row = half * kPair;
    const uint8_t* in = src + f0 * row + p * kPair;
    float4* out = dst + f0 * half + p;
    float h[T][2];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const float2 c = *reinterpret_cast<const float2*>(coeffs + static_cast<long>(t) * N + 2 * p);
        h[t][0] = c.x;
        h[t][1] = c.y;
    }
    // input frame f + t of the output frame f = f0 + j sits in ring[(j + t) % T]
    float ring[T][4];
#pragma unroll
    for (int t = 0; t + 1 < T; ++t) {
        load_pair<FMT, ALIGNED>(in, ring[t]);
        in += row;
    }
    for (long f = f0; f < f1; f += T) {
#pragma unroll
        for (int u = 0; u < T; ++u) {
            if (f + u < f1) {
                load_pair<FMT, ALIGNED>(in, ring[(u + T - 1) % T]);
                in += row;
                float z[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    z[c] = pfb_first(h[0][c >> 1], ring[u % T][c]);
#pragma unroll
                    for (int t = 1; t < T; ++t) z[c] = pfb_next(h[t][c >> 1], ring[(u + t) % T][c], z[c]);
                }
                *out = make_float4(z[0], z[1], z[2], z[3]);
                out += half;
            }
        }
    }
}

// The same thread-to-output mapping; every output frame reads its T input frames and coefficient rows again.
template <int FMT, bool ALIGNED>
__global__ __launch_bounds__(kPfbWG) void pfb_fold_reread_kernel(const uint8_t* __restrict__ src, long nframes, int N, int T,
                                                                 const float* __restrict__ coeffs, float4* __restrict__ dst,
                                                                 int L)
{
    const long half = N / 2;
    const long g = static_cast<long>(blockIdx.x) * kPfbWG + threadIdx.x;
    const long seg = g / half, p = g - seg * half;
    const long f0 = seg * L;
    if (f0 >= nframes) return;
    const long f1 = min(f0 + static_cast<long>(L), nframes);
    constexpr long kPair = PairRaw<FMT>::kBytes;
    const long row = half * kPair;
    const float* const hp = coeffs + 2 * p;
    for (long f = f0; f < f1; ++f) {
        const uint8_t* in = src + f * row + p * kPair;
        float x[4], z[4];
        load_pair<FMT, ALIGNED>(in, x);
        float2 c = *reinterpret_cast<const float2*>(hp);
#pragma unroll
        for (int k = 0; k < 4; ++k) z[k] = pfb_first(k >> 1 ? c.y : c.x, x[k]);
        for (int t = 1; t < T; ++t) {
            in += row;
            load_pair<FMT, ALIGNED>(in, x);
            c = *reinterpret_cast<const float2*>(hp + static_cast<long>(t) * N);
#pragma unroll
            for (int k = 0; k < 4; ++k) z[k] = pfb_next(k >> 1 ? c.y : c.x, x[k], z[k]);
        }
        dst[f * half + p] = make_float4(z[0], z[1], z[2], z[3]);
    }
}

template <int FMT, bool ALIGNED>
hipError_t launch_fmt(const uint8_t* d_src, long nframes, int N, int taps, const float* d_coeffs, float* d_z,
                      hipStream_t stream)
{
    const int L = pfb_segment_frames(taps, FMT);
    const long segments = (nframes + L - 1) / L;
    const long threads = segments * (N / 2);
    const long blocks = (threads + kPfbWG - 1) / kPfbWG;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>(blocks)), block(kPfbWG);
    float4* const z = reinterpret_cast<float4*>(d_z);
#define RPF_PFB_SLIDING(T)                                                                                       \
    case T:                                                                                                      \
        hipLaunchKernelGGL((pfb_fold_sliding_kernel<FMT, T, ALIGNED>), grid, block, 0, stream, d_src, nframes, N, \
                           d_coeffs, z, L);                                                                      \
        break
    switch (taps) {
        RPF_PFB_SLIDING(1);
        RPF_PFB_SLIDING(2);
        RPF_PFB_SLIDING(3);
        RPF_PFB_SLIDING(4);
        RPF_PFB_SLIDING(8);
        default:
            hipLaunchKernelGGL((pfb_fold_reread_kernel<FMT, ALIGNED>), grid, block, 0, stream, d_src, nframes, N, taps,
                               d_coeffs, z, L);
    }
#undef RPF_PFB_SLIDING
    return hipGetLastError();
}

template <int FMT>
hipError_t launch_aligned(const uint8_t* d_src, long nframes, int N, int taps, const float* d_coeffs, float* d_z,
                          hipStream_t stream)
{
    const uintptr_t addr = reinterpret_cast<uintptr_t>(d_src);
    constexpr uintptr_t kPair = PairRaw<FMT>::kBytes;
    if (addr % (kPair / 2)) return hipErrorInvalidValue;          // not even a whole sample
    return addr % kPair == 0 ? launch_fmt<FMT, true>(d_src, nframes, N, taps, d_coeffs, d_z, stream)
                             : launch_fmt<FMT, false>(d_src, nframes, N, taps, d_coeffs, d_z, stream);
}

}  // namespace

bool pfb_sliding(int taps) { return taps == 1 || taps == 2 || taps == 3 || taps == 4 || taps == 8; }

// Short segments: a lane's frames are a serial chain of loads, and what limits the fold is how many lanes are in flight,
// not the halo rows, which a neighbouring lane reads at about the same time and L2 serves
// (profiles/pfb_segment_lengths.txt: 4, 8, 16, 32, 64 frames measured; 8 is fastest from 2- and 4-byte samples, 16 from
// cf32, for either form and every T measured).
int pfb_segment_frames(int taps, int fmt)
{
    (void)taps;
    return fmt == kPfbCf32 ? 16 : 8;
}

hipError_t launch_pfb_fold(const uint8_t* d_src, long nframes, int N, int taps, int fmt, const float* d_coeffs, float* d_z,
                           hipStream_t stream)
{
    if (nframes < 1) return hipSuccess;
    if (!d_src || !d_coeffs || !d_z || N < 2 || (N & 1) || taps < 1 || taps > kPfbMaxTaps ||
        (reinterpret_cast<uintptr_t>(d_z) & 15) || (reinterpret_cast<uintptr_t>(d_coeffs) & 7))
        return hipErrorInvalidValue;
    switch (fmt) {
        case kPfbCu8: return launch_aligned<kPfbCu8>(d_src, nframes, N, taps, d_coeffs, d_z, stream);
        case kPfbCs8: return launch_aligned<kPfbCs8>(d_src, nframes, N, taps, d_coeffs, d_z, stream);
        case kPfbCs16: return launch_aligned<kPfbCs16>(d_src, nframes, N, taps, d_coeffs, d_z, stream);
        case kPfbCf32: return launch_aligned<kPfbCf32>(d_src, nframes, N, taps, d_coeffs, d_z, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace rpf
