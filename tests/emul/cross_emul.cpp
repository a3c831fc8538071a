// TEST-ONLY host build of the cross-spectrum front end, for tests/test_cross.py and tests/test_gpu_cross.py:
// csrc/cross_core.h's two expressions -- the same text the kernels compile -- walked sample by sample and bin by bin
// exactly as include/rpf_engine.h defines them (rpf_accumulate_device_cross).  Built with -ffp-contract=off.
#include <cstddef>
#include <cstdint>

#include "../../rtl-power-fftw_amd/csrc/cross_core.h"

using namespace rpf;

namespace {

template <int FMT>
void combine(const uint8_t* a, const uint8_t* b, long long nsamples, float* u, float* v)
{
    constexpr size_t vb = pfb_value_bytes(FMT);
    for (long long s = 0; s < nsamples; ++s) {
        const uint8_t* pa = a + static_cast<size_t>(s) * 2 * vb;
        const uint8_t* pb = b + static_cast<size_t>(s) * 2 * vb;
        float su[2], sv[2];
        cross_combine_sample(pfb_value<FMT>(pa), pfb_value<FMT>(pa + vb), pfb_value<FMT>(pb), pfb_value<FMT>(pb + vb), su, sv);
        u[2 * s] = su[0];
        u[2 * s + 1] = su[1];
        v[2 * s] = sv[0];
        v[2 * s + 1] = sv[1];
    }
}

}  // namespace

extern "C" {

// u, v [nsamples x 2] (float32 I, Q) from the first nsamples complex samples of a and b in `fmt` (RPF_FORMAT_*).
// Returns 0, or -1 for a bad argument.
int rpf_emul_cross_combine(const void* a, const void* b, long long nsamples, int fmt, float* u, float* v)
{
    if (!a || !b || !u || !v || nsamples < 0) return -1;
    const uint8_t* pa = static_cast<const uint8_t*>(a);
    const uint8_t* pb = static_cast<const uint8_t*>(b);
    switch (fmt) {
        case kPfbCu8: combine<kPfbCu8>(pa, pb, nsamples, u, v); return 0;
        case kPfbCs8: combine<kPfbCs8>(pa, pb, nsamples, u, v); return 0;
        case kPfbCs16: combine<kPfbCs16>(pa, pb, nsamples, u, v); return 0;
        case kPfbCf32: combine<kPfbCf32>(pa, pb, nsamples, u, v); return 0;
        default: return -1;
    }
}

// out[4 x N] = the finishing expression over planes[4 x N] = Paa, Pbb, Puu, Pvv.
int rpf_emul_cross_finish(const double* planes, int N, double* out)
{
    if (!planes || !out || N < 1) return -1;
    const size_t n = static_cast<size_t>(N);
    for (size_t k = 0; k < n; ++k) {
        double r[kCrossPlanes];
        cross_finish_bin(planes[k], planes[n + k], planes[2 * n + k], planes[3 * n + k], r);
        for (int p = 0; p < kCrossPlanes; ++p) out[p * n + k] = r[p];
    }
    return 0;
}

}  // extern "C"
