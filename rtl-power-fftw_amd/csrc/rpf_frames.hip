// rpf_frames.hip -- the frame gather of overlapped frames (rpf_config::frame_step S < N).
//
// K1 addresses frames at a run-time pitch itself (fft_accum_strided_kernel).  Every other kernel family (KM and its
// split form, four-step, Bluestein, large Bluestein, catch-all) reads frame f at byte 2N f; for those the engine copies
// the overlapped frames side by side into a bounded device scratch -- frame f of the chunk to bytes [2N f, 2N (f+1)) --
// and runs the size's unchanged kernel over it (rpf_engine.cpp, launch_frames).  A pure copy: HBM-bound, one read of
// each frame's 2N bytes (the overlap comes back from L2) and one write.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "rpf_kernels.h"

namespace rpf {

namespace {

constexpr int kGatherWG = 256;

// V: the widest access (16, 8, 4 or 2 bytes) that divides both base addresses, the pitch and the frame length -- every
// access of the launch is then naturally aligned.  x: chunks of V inside a frame, y: frames; grid-stride in both.
template <typename V>
__global__ __launch_bounds__(kGatherWG) void gather_frames_kernel(const uint8_t* __restrict__ src, long nframes,
                                                                  long pitch, long per_frame, uint8_t* __restrict__ dst)
{
    const V* const s = reinterpret_cast<const V*>(src);
    V* const d = reinterpret_cast<V*>(dst);
    const long pitch_v = pitch / static_cast<long>(sizeof(V));
    for (long f = blockIdx.y; f < nframes; f += gridDim.y) {
        const V* const sf = s + f * pitch_v;
        V* const df = d + f * per_frame;
        for (long k = static_cast<long>(blockIdx.x) * kGatherWG + threadIdx.x; k < per_frame;
             k += static_cast<long>(gridDim.x) * kGatherWG)
            df[k] = sf[k];
    }
}

template <typename V>
void launch_typed(const uint8_t* d_src, long nframes, long pitch, long frame_bytes, uint8_t* d_dst, hipStream_t stream)
{
    const long per_frame = frame_bytes / static_cast<long>(sizeof(V));
    // enough workgroups to cover a large frame across the device, and the rest of ~2048 across frames
    const long gx = std::min<long>((per_frame + kGatherWG - 1) / kGatherWG, 256);
    const long gy = std::min<long>(nframes, std::max<long>(1, 2048 / gx));
    hipLaunchKernelGGL(gather_frames_kernel<V>, dim3(static_cast<unsigned>(gx), static_cast<unsigned>(gy)),
                       dim3(kGatherWG), 0, stream, d_src, nframes, pitch, per_frame, d_dst);
}

}  // namespace

hipError_t launch_gather_frames(const uint8_t* d_src, long nframes, long pitch, long frame_bytes, uint8_t* d_dst,
                                hipStream_t stream)
{
    if (nframes < 1) return hipSuccess;
    if (!d_src || !d_dst || pitch < 2 || frame_bytes < 2 || (pitch & 1) || (frame_bytes & 1)) return hipErrorInvalidValue;
    const uintptr_t bits = reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_dst) |
                           static_cast<uintptr_t>(pitch) | static_cast<uintptr_t>(frame_bytes);
    if (bits & 1) return hipErrorInvalidValue;
    if ((bits & 15) == 0)
        launch_typed<uint4>(d_src, nframes, pitch, frame_bytes, d_dst, stream);
    else if ((bits & 7) == 0)
        launch_typed<uint2>(d_src, nframes, pitch, frame_bytes, d_dst, stream);
    else if ((bits & 3) == 0)
        launch_typed<uint32_t>(d_src, nframes, pitch, frame_bytes, d_dst, stream);
    else
        launch_typed<uint16_t>(d_src, nframes, pitch, frame_bytes, d_dst, stream);
    return hipGetLastError();
}

}  // namespace rpf
