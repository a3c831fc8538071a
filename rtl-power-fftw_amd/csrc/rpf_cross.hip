// rpf_cross.hip -- the two kernels of the cross-spectrum front end (include/rpf_engine.h, rpf_accumulate_device_cross).
//
// cross_combine: u = a + b and v = a + i b, sample by sample (cross_core.h has the exact expression), written as two
// cf32 streams the unchanged transform of a cf32 engine then reads.  Elementwise over samples: it knows nothing of
// frames, N or the frame step.  Memory-bound: 2b bytes in and 16 bytes out per sample pair of the two streams.
//
// A lane owns one PAIR of adjacent complex samples, as the PFB fold does (rpf_pfb.hip): it loads 4 (8-bit formats), 8
// (cs16) or 16 (cf32) bytes of each stream and stores 16 bytes of u and 16 of v; consecutive lanes own consecutive
// pairs, so a wavefront reads 256 B .. 1 KB of each input and writes 1 KB of each output in one piece.  A stream that
// starts at a multiple of the pair's bytes is read pair by pair (ALIGNED), any other (an odd sample offset) sample by
// sample; the two streams are judged separately.  An odd sample count leaves one last sample to a lane of its own.
// One pair per lane and no loop: what limits a kernel of this shape is how many lanes are in flight
// (profiles/pfb_segment_lengths.txt), and a stream of 2^28 samples is 2^27 lanes.
//
// cross_finish: out = Paa, Pbb, 0.5 (Puu - C), 0.5 (Pvv - C) with C = Paa + Pbb, one bin per lane.
//
// No LDS, no scratch (profiles/cross_resources.txt).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cross_core.h"
#include "rpf_kernels.h"

namespace rpf {

namespace {

constexpr int kCrossWG = 256;

// One complex sample at p (a multiple of the sample's bytes): 2, 4 or 8 bytes in one access.
template <int FMT>
__device__ __forceinline__ void load_sample(const uint8_t* __restrict__ p, float (&x)[2])
{
    constexpr int vb = pfb_value_bytes(FMT);
    union {
        uint8_t b[2 * vb];
        uint16_t h;
        uint32_t w[2];
    } raw;
    if constexpr (vb == 1) {
        raw.h = *reinterpret_cast<const uint16_t*>(p);
    } else if constexpr (vb == 2) {
        raw.w[0] = *reinterpret_cast<const uint32_t*>(p);
    } else {
        const uint2 v = *reinterpret_cast<const uint2*>(p);
        raw.w[0] = v.x;
        raw.w[1] = v.y;
    }
    x[0] = pfb_value<FMT>(raw.b);
    x[1] = pfb_value<FMT>(raw.b + vb);
}

// Two adjacent samples at p.  ALIGNED: p is a multiple of the pair's bytes -- one access; else two.
template <int FMT, bool ALIGNED>
__device__ __forceinline__ void load_pair(const uint8_t* __restrict__ p, float (&x)[4])
{
    constexpr int vb = pfb_value_bytes(FMT);
    if constexpr (ALIGNED) {
        union {
            uint8_t b[4 * vb];
            uint32_t w[vb];
        } raw;
        if constexpr (vb == 1) {
            raw.w[0] = *reinterpret_cast<const uint32_t*>(p);
        } else if constexpr (vb == 2) {
            const uint2 v = *reinterpret_cast<const uint2*>(p);
            raw.w[0] = v.x;
            raw.w[1] = v.y;
        } else {
            const uint4 v = *reinterpret_cast<const uint4*>(p);
            raw.w[0] = v.x;
            raw.w[1] = v.y;
            raw.w[2] = v.z;
            raw.w[3] = v.w;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = pfb_value<FMT>(raw.b + c * vb);
    } else {
        float lo[2], hi[2];
        load_sample<FMT>(p, lo);
        load_sample<FMT>(p + 2 * vb, hi);
        x[0] = lo[0];
        x[1] = lo[1];
        x[2] = hi[0];
        x[3] = hi[1];
    }
}

// Lane g: samples 2g and 2g + 1 of the `nsamples` (the last lane of an odd count: sample 2g alone).
template <int FMT, bool ALIGNED_A, bool ALIGNED_B>
__global__ __launch_bounds__(kCrossWG) void cross_combine_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                                 long nsamples, float* __restrict__ u, float* __restrict__ v)
{
    constexpr long kSample = 2 * pfb_value_bytes(FMT);
    const long g = static_cast<long>(blockIdx.x) * kCrossWG + threadIdx.x;
    const long s0 = 2 * g;
    if (s0 >= nsamples) return;
    if (s0 + 1 < nsamples) {
        float xa[4], xb[4], lo_u[2], lo_v[2], hi_u[2], hi_v[2];
        load_pair<FMT, ALIGNED_A>(a + s0 * kSample, xa);
        load_pair<FMT, ALIGNED_B>(b + s0 * kSample, xb);
        cross_combine_sample(xa[0], xa[1], xb[0], xb[1], lo_u, lo_v);
        cross_combine_sample(xa[2], xa[3], xb[2], xb[3], hi_u, hi_v);
        reinterpret_cast<float4*>(u)[g] = make_float4(lo_u[0], lo_u[1], hi_u[0], hi_u[1]);
        reinterpret_cast<float4*>(v)[g] = make_float4(lo_v[0], lo_v[1], hi_v[0], hi_v[1]);
    } else {
        float xa[2], xb[2], su[2], sv[2];
        load_sample<FMT>(a + s0 * kSample, xa);
        load_sample<FMT>(b + s0 * kSample, xb);
        cross_combine_sample(xa[0], xa[1], xb[0], xb[1], su, sv);
        reinterpret_cast<float2*>(u)[s0] = make_float2(su[0], su[1]);
        reinterpret_cast<float2*>(v)[s0] = make_float2(sv[0], sv[1]);
    }
}

__global__ __launch_bounds__(kCrossWG) void cross_finish_kernel(const double* __restrict__ planes, int N, double* __restrict__ out)
{
    const int k = blockIdx.x * kCrossWG + threadIdx.x;
    if (k >= N) return;
    double r[kCrossPlanes];
    cross_finish_bin(planes[k], planes[N + k], planes[2 * static_cast<long>(N) + k], planes[3 * static_cast<long>(N) + k], r);
#pragma unroll
    for (int p = 0; p < kCrossPlanes; ++p) out[static_cast<long>(p) * N + k] = r[p];
}

template <int FMT>
hipError_t launch_combine_fmt(const uint8_t* d_a, const uint8_t* d_b, long nsamples, float* d_u, float* d_v, hipStream_t stream)
{
    constexpr uintptr_t kPair = 4 * pfb_value_bytes(FMT);
    const uintptr_t pa = reinterpret_cast<uintptr_t>(d_a), pb = reinterpret_cast<uintptr_t>(d_b);
    if (pa % (kPair / 2) || pb % (kPair / 2)) return hipErrorInvalidValue;          // not even a whole sample
    const long lanes = (nsamples + 1) / 2;
    const long blocks = (lanes + kCrossWG - 1) / kCrossWG;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>(blocks)), block(kCrossWG);
    const bool al_a = pa % kPair == 0, al_b = pb % kPair == 0;
#define RPF_CROSS_COMBINE(A, B) \
    hipLaunchKernelGGL((cross_combine_kernel<FMT, A, B>), grid, block, 0, stream, d_a, d_b, nsamples, d_u, d_v)
    if (al_a && al_b) RPF_CROSS_COMBINE(true, true);
    else if (al_a) RPF_CROSS_COMBINE(true, false);
    else if (al_b) RPF_CROSS_COMBINE(false, true);
    else RPF_CROSS_COMBINE(false, false);
#undef RPF_CROSS_COMBINE
    return hipGetLastError();
}

}  // namespace

hipError_t launch_cross_combine(const uint8_t* d_a, const uint8_t* d_b, long nsamples, int fmt, float* d_u, float* d_v,
                                hipStream_t stream)
{
    if (nsamples < 1) return hipSuccess;
    if (!d_a || !d_b || !d_u || !d_v || (reinterpret_cast<uintptr_t>(d_u) & 15) || (reinterpret_cast<uintptr_t>(d_v) & 15))
        return hipErrorInvalidValue;
    switch (fmt) {
        case kPfbCu8: return launch_combine_fmt<kPfbCu8>(d_a, d_b, nsamples, d_u, d_v, stream);
        case kPfbCs8: return launch_combine_fmt<kPfbCs8>(d_a, d_b, nsamples, d_u, d_v, stream);
        case kPfbCs16: return launch_combine_fmt<kPfbCs16>(d_a, d_b, nsamples, d_u, d_v, stream);
        case kPfbCf32: return launch_combine_fmt<kPfbCf32>(d_a, d_b, nsamples, d_u, d_v, stream);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_cross_finish(const double* d_planes, int N, double* d_out, hipStream_t stream)
{
    if (!d_planes || !d_out || N < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cross_finish_kernel, dim3((N + kCrossWG - 1) / kCrossWG), dim3(kCrossWG), 0, stream, d_planes, N, d_out);
    return hipGetLastError();
}

}  // namespace rpf
