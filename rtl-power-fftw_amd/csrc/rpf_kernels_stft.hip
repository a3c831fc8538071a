// rpf_kernels_stft.hip -- K1's store kernels (rpf_stft_device): fft_stft_kernel and fft_stft_strided_kernel
// (k1_kernels.h, k1_stft_body.inc) for variant 0 of every K1 size x {plain, windowed} x {LDS-DMA, VGPR staging}, cu8
// here, cs8 and cs16 in rpf_kernels_stft_formats.hip, cf32 in rpf_kernels_stft_cf32.hip, with the geometry of the size's
// plain kernels; and the launch code of all three.  Translation units of their own: they compile beside the others
// and none of their kernels moves.
#include "k1_kernels.h"

namespace rpf {

const Variant* k1_stft_variant(int N, int fmt)
{
    return fmt == kFmtCu8 ? find_default_variant<kK1Stft, kFmtCu8>(N) : nullptr;
}

namespace {

const Variant* find_stft_variant(int N, int fmt)
{
    return fmt == kFmtCu8 ? k1_stft_variant(N, fmt) : fmt == kFmtCf32 ? k1_stft_cf32_variant(N, fmt) : k1_stft_format_variant(N, fmt);
}

}  // namespace

bool stft_supported(int N, int fmt) { return find_stft_variant(N, fmt) != nullptr; }

hipError_t plan_stft(int N, bool window, int device, LaunchInfo* li, int fmt)
{
    const Variant* v = find_stft_variant(N, fmt);
    if (!v) return hipErrorInvalidValue;
    const int w = window ? 1 : 0;
    int grid = 0;
    // the plain and the strided kernel in both staging forms share one grid
    hipError_t err = plan_resident_grid({reinterpret_cast<const void*>(v->stft[w][0]), reinterpret_cast<const void*>(v->stft[w][1]),
                                         reinterpret_cast<const void*>(v->stft_strided[w][0]),
                                         reinterpret_cast<const void*>(v->stft_strided[w][1])}, v->geo, device, &grid);
    if (err != hipSuccess) return err;
    fill_info(li, v->geo, grid);
    return hipSuccess;
}

hipError_t launch_fft_stft(int N, bool window, bool use_dma, const uint8_t* d_stream, long nframes, const cf* d_twiddles,
                           const float* d_window, cf* d_out, int grid, hipStream_t stream, LaunchInfo* li, long pitch, int fmt)
{
    const Variant* v = find_stft_variant(N, fmt);
    const long sb = sample_bytes_of(fmt);
    if (!v || grid < 1 || nframes < 1 || !d_stream || !d_out || pitch < 0 || pitch > sb * N || (pitch % sb))
        return hipErrorInvalidValue;
    if (pitch == 0 || pitch == sb * N)
        hipLaunchKernelGGL(v->stft[window ? 1 : 0][use_dma ? 1 : 0], dim3(grid), dim3(v->geo.WG), v->geo.lds_bytes, stream,
                           d_stream, nframes, d_twiddles, d_window, d_out);
    else
        hipLaunchKernelGGL(v->stft_strided[window ? 1 : 0][use_dma ? 1 : 0], dim3(grid), dim3(v->geo.WG), v->geo.lds_bytes,
                           stream, d_stream, nframes, pitch, d_twiddles, d_window, d_out);
    fill_info(li, v->geo, grid);
    return hipGetLastError();
}

}  // namespace rpf
