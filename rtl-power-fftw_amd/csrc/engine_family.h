// engine_family.h -- which kernel family serves an engine: the enumerator rpf_engine keeps and the one rule that
// picks it (rpf_engine.cpp, check_config).  Plain C++11, no HIP: tests/emul/engine_family_emul.cpp compiles it alone and
// tests/test_engine_family.py walks its whole input space.
#pragma once

namespace rpf {

enum class Family {
    K1,            // the LDS-resident kernel (rpf_kernels*.hip), at any frame step
    Mixed,         // the LDS mixed-radix kernels (rpf_mixed*.hip): planned, split and run-time Stockham forms
    FourStep,      // K2a/K2b or the fused persistent kernel (rpf_fourstep.hip)
    Bluestein,     // the chirp-z kernel of the small sizes (rpf_kernels.hip)
    BigBluestein,  // the large (four-step) Bluestein path (rpf_fourstep.hip)
    Generic,       // the catch-all Stockham path (rpf_generic.hip): every format, every size
    // No transform: select_family's "No gfx950 kernel for N bins", and what the outer engine of a polyphase filter bank
    // has -- it owns the queues and the fold, its inner engine has a family of its own.  So a PFB engine is not K1; the
    // entries that ask is_k1() (launch_frames, rpf_device_fused, both hop entries, series_native) look at `taps` first,
    // and what a PFB engine would answer there never decides anything.
    None,
};

// What the rule reads: the configuration, and what this build has at N as plain bools (the *_supported functions).
struct FamilyQuery {
    int N;
    int variant;            // RPF_FLAG_VARIANT(k); 0 = the shipped kernels
    bool cu8;               // the sample format is cu8
    bool stats;             // RPF_FLAG_BIN_STATS
    bool windowed;          // a window is given
    bool flag_catch_all, flag_no_mixed_radix, flag_fourstep_fused;
    bool k1_v0;             // kernel_supported(N, 0)
    bool k1;                // kernel_supported(N, variant)
    bool mixed;             // mixed_supported(N, variant)
    bool fourstep, bluestein, bigblu;     // (at most one of the three at any N)
    bool generic;           // generic_supported(N)
};

// The first family of this list that applies serves the engine.
inline Family select_family(const FamilyQuery& q)
{
    const bool shipped = q.variant == 0;            // every family but K1 and Mixed has its shipped kernels only
    const Family generic = shipped && q.generic ? Family::Generic : Family::None;
    // The catch-all path is the one that reads every format at every N: it takes the engines that ask for it and the
    // signed formats on every size K1 does not serve, whatever family that size runs on with cu8.
    // ... and so do the statistics: a stats engine at any size K1 does not serve runs there.
    // (cf32 with statistics included: K1 has every size x window x staging form of it, rpf_kernels_stats_cf32.hip.)
    if (q.flag_catch_all || ((!q.cu8 || q.stats) && !q.k1_v0)) return generic;
    // 32768 is served twice, by the split form 2 x 16384 and by the four-step kernels.  Plain runs are faster on the
    // former (0.37 against 0.22 Tsample/s); WINDOWED runs are not: the 16384-point plan has no registers left for the
    // window values next to its two-deep section pipeline (0.175, it was 0.27 before round 3's section sums), the
    // four-step kernels multiply them in as they unpack (0.21 - 0.22).  profiles/r04_sizes.txt.
    const bool windowed_32768 = q.N == 32768 && q.windowed && shipped;
    // (asking for the fused four-step kernel is asking for the four-step path)
    if (q.mixed && !windowed_32768 && !q.flag_no_mixed_radix && !q.flag_fourstep_fused) return Family::Mixed;
    if (shipped && q.bluestein) return Family::Bluestein;
    if (shipped && q.bigblu) return Family::BigBluestein;
    if (shipped && q.fourstep) return Family::FourStep;
    if (q.k1 && (q.cu8 || shipped)) return Family::K1;          // (the tuning variants of K1 are cu8 kernels)
    return generic;
}

}  // namespace rpf
