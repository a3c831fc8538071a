// excise_core.h -- the per-element step and the addition order of the excised average (include/rpf_engine.h,
// rpf_accumulate_device_excised): the rows of a series of statistics, S1[N] S2[N] PK[N] each, are judged bin by bin with
// the spectral kurtosis of the row, and S1 is summed over the rows that pass.
//
// Order of the additions.  Row k of the CALL (not of the piece it arrives in) belongs to row group k mod G,
// G = excise_groups(N).  Every (group, bin) keeps one accumulator triple and takes its rows in increasing k, so what an
// accumulator holds after the last row does not depend on how the rows were cut into pieces.  The combine then adds the
// G accumulators of a bin in a fixed order: lane j of kExciseLanes takes the groups j, j + kExciseLanes, ... in
// increasing order, and the lanes' sums are added in lane order.  clean and total go through the same additions in the
// same order, so with nothing flagged they are equal bit for bit.
//
// Plain C++: the kernels (rpf_excise.hip), the engine and the CPU tests (tests/emul/excise_emul.cpp) share what is below.
#pragma once

#if defined(__HIPCC__)
#define RPF_EXCISE_HD __host__ __device__ __forceinline__
#else
#define RPF_EXCISE_HD inline
#endif

namespace rpf {

constexpr int kExcisePlanes = 3;         // the output's planes: clean, kept, total
constexpr int kExciseLanes = 32;         // lanes of the combine (above)
constexpr int kExciseGroupBins = 1 << 18;   // G N stays near this: enough (group, bin pair) threads for every CU at any N

// Row groups for N bins: 4096 at N = 64, 32 at N = 8192, 1 from 2^18 bins up (the accumulators then are the output).
RPF_EXCISE_HD int excise_groups(int N)
{
    const int g = kExciseGroupBins / N;
    return g < 1 ? 1 : g;
}

struct ExciseAcc {
    double clean, kept, total;
};

// SK of a row's bin from its S1 and S2 over m frames, (m+1)/(m-1) (m S2 / S1^2 - 1): IEEE double, every operation
// rounded on its own, in the order stats.spectral_kurtosis (and host/datastore.h) evaluates it -- no contraction into
// fused multiply-adds, a correctly rounded division, no reciprocal approximation.  NaN where S1 = 0.
RPF_EXCISE_HD double excise_sk(double s1, double s2, double m)
{
#pragma clang fp contract(off)
    if (s1 == 0.0) return __builtin_nan("");
    const double scale = (m + 1.0) / (m - 1.0);
    const double sq = s1 * s1;
    const double ms2 = m * s2;
    const double ratio = ms2 / sq;
    const double excess = ratio - 1.0;
    return scale * excess;
}

// Kept: sk_lo <= SK <= sk_hi.  A NaN compares false: flagged.
RPF_EXCISE_HD bool excise_keeps(double sk, double sk_lo, double sk_hi) { return sk_lo <= sk && sk <= sk_hi; }

// One row's bin into its accumulators; returns the mask byte (1 = flagged).  A flagged row leaves clean and kept as
// they are (nothing is added, not even a zero).
RPF_EXCISE_HD unsigned char excise_step(ExciseAcc& a, double s1, double s2, double m, double sk_lo, double sk_hi)
{
#pragma clang fp contract(off)
    const bool keep = excise_keeps(excise_sk(s1, s2, m), sk_lo, sk_hi);
    a.total = a.total + s1;
    a.clean = keep ? a.clean + s1 : a.clean;
    a.kept = keep ? a.kept + 1.0 : a.kept;
    return keep ? 0 : 1;
}

// Two partial results of one bin (the combine's additions).
RPF_EXCISE_HD ExciseAcc excise_add(const ExciseAcc& a, const ExciseAcc& b)
{
    return ExciseAcc{a.clean + b.clean, a.kept + b.kept, a.total + b.total};
}

}  // namespace rpf
