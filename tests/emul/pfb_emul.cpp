// TEST-ONLY host build of the polyphase fold, for tests/test_pfb.py and tests/test_gpu_pfb.py: csrc/pfb_core.h's
// conversion and inner expression -- the same text the kernels compile -- walked frame by frame exactly as
// include/rpf_engine.h defines the fold: z = h[n] x[fN + n], then z = fmaf(h[tN + n], x[(f + t)N + n], z) in increasing
// t, I and Q separately.  Built with -ffp-contract=off; the fused multiply-add is std::fmaf's (__builtin_fmaf).
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../rtl-power-fftw_amd/csrc/pfb_core.h"

using namespace rpf;

namespace {

template <int FMT>
void fold(const uint8_t* stream, long long frames, int N, int taps, const float* h, float* z)
{
    constexpr size_t vb = pfb_value_bytes(FMT);
    const size_t row = 2 * static_cast<size_t>(N);                    // values (I and Q) per frame
    for (long long f = 0; f < frames; ++f)
        for (size_t v = 0; v < row; ++v) {
            const uint8_t* p = stream + (static_cast<size_t>(f) * row + v) * vb;
            float acc = pfb_first(h[v >> 1], pfb_value<FMT>(p));
            for (int t = 1; t < taps; ++t)
                acc = pfb_next(h[static_cast<size_t>(t) * N + (v >> 1)], pfb_value<FMT>(p + static_cast<size_t>(t) * row * vb), acc);
            z[static_cast<size_t>(f) * row + v] = acc;
        }
}

}  // namespace

extern "C" {

int rpf_emul_pfb_max_taps(void) { return kPfbMaxTaps; }

// z[frames x N x 2] (float32 I, Q) from the stream's first frames + taps - 1 input frames of N samples of `fmt`
// (RPF_FORMAT_*).  Returns 0, or -1 for a bad argument.
int rpf_emul_pfb_fold(const void* stream, long long frames, int N, int taps, int fmt, const float* h, float* z)
{
    if (!stream || !h || !z || frames < 0 || N < 2 || (N & 1) || taps < 1 || taps > kPfbMaxTaps) return -1;
    const uint8_t* s = static_cast<const uint8_t*>(stream);
    switch (fmt) {
        case kPfbCu8: fold<kPfbCu8>(s, frames, N, taps, h, z); return 0;
        case kPfbCs8: fold<kPfbCs8>(s, frames, N, taps, h, z); return 0;
        case kPfbCs16: fold<kPfbCs16>(s, frames, N, taps, h, z); return 0;
        case kPfbCf32: fold<kPfbCf32>(s, frames, N, taps, h, z); return 0;
        default: return -1;
    }
}

}  // extern "C"
