// quantile_core.h -- the per-element steps of the per-bin quantiles (include/rpf_engine.h, rpf_quantile_select_device):
// the order-preserving map from a double to a 64-bit key and back, the digit order of the radix select, the step that
// narrows a (quantile, bin) by one digit from the digit counts, and the rank and interpolation expression.
//
// Selection.  A (quantile, bin) carries a key prefix and a rank r: the r-th smallest (from 0) of the stored keys that
// share the prefix is the key looked for.  It starts with an empty prefix and r = j.  A pass counts, by their next
// digit -- kQuantileDigitBits bits, most significant first -- the keys that share the prefix; the digit whose
// cumulative count first exceeds r joins the prefix and r drops by the count below it.  After kQuantilePasses passes
// the prefix is the key of v_(j).  The last pass also tells whether v_(j+1) is the same key (more keys left in the
// digit than r + 1): if not, it is the smallest key above the prefix, which one further pass finds as a minimum.
// Counts are integers and a minimum has no order, so the result does not depend on how the rows are split over
// lanes, workgroups or launches.
//
// Plain C++: the kernels (rpf_quantile.hip), the engine and the CPU tests (tests/emul/quantile_emul.cpp) share what is
// below.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define RPF_QUANTILE_HD __host__ __device__ __forceinline__
#else
#define RPF_QUANTILE_HD inline
#endif

namespace rpf {

constexpr int kQuantileMaxQ = 8;                                  // quantiles per selection
constexpr int kQuantileDigitBits = 4;
constexpr int kQuantileDigits = 1 << kQuantileDigitBits;          // counters per (quantile, bin) and pass
constexpr int kQuantilePasses = 64 / kQuantileDigitBits;          // counting passes; one more finds v_(j+1)
constexpr uint64_t kQuantileNanKey = ~static_cast<uint64_t>(0);   // every NaN: above +inf
constexpr uint32_t kQuantileNoAbove = ~static_cast<uint32_t>(0);  // rank word after the last pass: b needs no search

// Ascending keys for ascending doubles: a negative number has all its bits flipped, any other its sign bit, so
// -inf < ... < -0.0 < +0.0 < ... < +inf in unsigned order; a NaN of either sign is all ones, above everything.
// Integer operations only: a subnormal keeps its place whatever the floating-point mode.
RPF_QUANTILE_HD uint64_t quantile_key(uint64_t bits)
{
    const uint64_t sign = static_cast<uint64_t>(1) << 63;
    if ((bits & ~sign) > (static_cast<uint64_t>(0x7ff) << 52)) return kQuantileNanKey;
    return (bits & sign) ? ~bits : bits | sign;
}

// The inverse; the NaN key gives the quiet NaN 0x7fff...f.
RPF_QUANTILE_HD uint64_t quantile_unkey(uint64_t key)
{
    const uint64_t sign = static_cast<uint64_t>(1) << 63;
    return (key & sign) ? key & ~sign : ~key;
}

RPF_QUANTILE_HD uint64_t quantile_bits(double v)
{
    union { double d; uint64_t u; } x;
    x.d = v;
    return x.u;
}

RPF_QUANTILE_HD double quantile_double(uint64_t bits)
{
    union { double d; uint64_t u; } x;
    x.u = bits;
    return x.d;
}

// Pass p (0 .. kQuantilePasses - 1) looks at the bits [shift, shift + kQuantileDigitBits), most significant first.
RPF_QUANTILE_HD int quantile_shift(int pass) { return 64 - kQuantileDigitBits * (pass + 1); }
// The bits above them: what a key must share with the prefix to be counted (none in pass 0).
RPF_QUANTILE_HD uint64_t quantile_prefix_mask(int pass)
{
    return pass == 0 ? 0 : ~static_cast<uint64_t>(0) << (quantile_shift(pass) + kQuantileDigitBits);
}
RPF_QUANTILE_HD bool quantile_matches(uint64_t key, uint64_t prefix, uint64_t prefix_mask) { return ((key ^ prefix) & prefix_mask) == 0; }
RPF_QUANTILE_HD int quantile_digit(uint64_t key, int shift) { return static_cast<int>((key >> shift) & (kQuantileDigits - 1)); }

// One (quantile, bin) narrowed by a pass's counts, counts[d * stride] for digit d: the digit joins the prefix, the rank
// drops by the keys below it.  Returns the keys left in the chosen digit.  (The counts of the keys that share the
// prefix add up to more than the rank, by induction from j < K; the last digit is taken if they ever did not.)
RPF_QUANTILE_HD uint32_t quantile_narrow(const uint32_t* counts, size_t stride, int shift, uint64_t& prefix, uint32_t& rank)
{
    uint32_t below = 0, in_digit = 0;
    int d = 0;
    for (; d < kQuantileDigits; ++d) {
        in_digit = counts[static_cast<size_t>(d) * stride];
        if (rank < below + in_digit || d == kQuantileDigits - 1) break;
        below += in_digit;
    }
    prefix |= static_cast<uint64_t>(d) << shift;
    rank -= below;
    return in_digit;
}

// h = q (K - 1), j = floor(h), g = h - j: IEEE double, every operation rounded on its own.  K >= 1, 0 <= q <= 1.
RPF_QUANTILE_HD void quantile_rank(double q, int64_t K, int64_t& j, double& g)
{
#pragma clang fp contract(off)
    const double h = q * static_cast<double>(K - 1);
    j = static_cast<int64_t>(h);                  // h >= 0: truncation is the floor
    if (j > K - 1) j = K - 1;
    g = h - static_cast<double>(j);
}

// Q = (g == 0 || a == b) ? a : a + g (b - a), no contraction.  A NaN among a, b with g != 0 gives NaN.
RPF_QUANTILE_HD double quantile_interp(double a, double b, double g)
{
#pragma clang fp contract(off)
    if (g == 0.0 || a == b) return a;
    const double d = b - a;
    const double gd = g * d;
    return a + gd;
}

// What a selection is asked for, by value in the kernels' arguments: the ranks are the same in every bin.
struct QuantileRanks {
    int nq;
    uint32_t j[kQuantileMaxQ];
    double g[kQuantileMaxQ];
};

}  // namespace rpf
