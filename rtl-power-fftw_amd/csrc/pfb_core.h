// pfb_core.h -- the sample conversion and the inner expression of the polyphase fold (include/rpf_engine.h,
// rpf_engine_create_pfb): z = h[n] x[fN + n], then z = fmaf(h[tN + n], x[(f + t)N + n], z) for t = 1 .. T-1 in
// increasing t, I and Q separately, every step rounded once, nothing contracted or reassociated beyond that.
//
// Plain C++: the kernels (rpf_pfb.hip) and the CPU tests (tests/emul/pfb_emul.cpp) share what is below, so the two
// cannot drift.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define RPF_PFB_HD __host__ __device__ __forceinline__
#else
#define RPF_PFB_HD inline
#endif

namespace rpf {

// the sample formats, by the numbers of RPF_FORMAT_* (fft_core.h's kFmt* are the same numbers)
constexpr int kPfbCu8 = 0, kPfbCs8 = 1, kPfbCs16 = 2, kPfbCf32 = 4;
constexpr int kPfbMaxTaps = 32;
constexpr int pfb_value_bytes(int fmt) { return fmt == kPfbCf32 ? 4 : fmt == kPfbCs16 ? 2 : 1; }   // one of I, Q

// One stored value (I or Q) as the engine's float32, exactly: cu8 is v - 127; cs8, cs16 and cf32 are v.
template <int FMT>
RPF_PFB_HD float pfb_value(const uint8_t* p)
{
    if constexpr (FMT == kPfbCu8) {
        return static_cast<float>(static_cast<int>(p[0]) - 127);
    } else if constexpr (FMT == kPfbCs8) {
        return static_cast<float>(static_cast<int8_t>(p[0]));
    } else if constexpr (FMT == kPfbCs16) {
        return static_cast<float>(static_cast<int16_t>(static_cast<uint16_t>(p[0]) | (static_cast<uint16_t>(p[1]) << 8)));
    } else {
        static_assert(FMT == kPfbCf32, "");
        float v;
        __builtin_memcpy(&v, p, 4);
        return v;
    }
}

// tap 0: one multiplication, one rounding
RPF_PFB_HD float pfb_first(float h, float x)
{
#pragma clang fp contract(off)
    return h * x;
}

// tap t >= 1: one fused multiply-add, one rounding
RPF_PFB_HD float pfb_next(float h, float x, float z) { return __builtin_fmaf(h, x, z); }

}  // namespace rpf
