// fold_core.h -- what the fold of a D x T plane at trial periods (include/rpf_engine.h, rpf_fold_device) states once:
// the bin rule, the segment rule, which wave owns which (series, periods, segment), the LDS index of a wave's partial
// profiles, the scratch layout and the series groups.
//
// Plain C++: the kernel (rpf_fold.hip), the engine (rpf_engine.cpp) and the CPU emulator (tests/emul/fold_emul.cpp)
// share what is below, so they cannot drift.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/rpf_engine.h"

#if defined(__HIPCC__)
#define RPF_FOLD_HD __host__ __device__ __forceinline__
#else
#define RPF_FOLD_HD inline
#endif

namespace rpf {

constexpr int kFoldSegments = RPF_FOLD_SEGMENTS;      // the fixed order: 16 segments whatever T
constexpr int kFoldMaxSeries = 4096;
constexpr int kFoldMaxPeriods = 4096;
constexpr int kFoldMaxBins = 128;
constexpr int64_t kFoldMaxCells = static_cast<int64_t>(1) << 24;         // D P NB of one call
constexpr int kFoldLanes = 64;                        // a wave: 64 consecutive periods, lane = period
constexpr size_t kFoldScratchBytes = static_cast<size_t>(256) << 20;     // the engine's scratch never exceeds this
static_assert(kFoldSegments == 16, "the order of the sums is part of the definition");

// bin(p, t) of the definition from the phase (t steps[p]) mod 2^64: its upper 32 bits times NB, upper 32 bits of that.
RPF_FOLD_HD uint32_t fold_bin_of_phase(uint64_t phase, uint32_t NB)
{
    return static_cast<uint32_t>(((phase >> 32) * static_cast<uint64_t>(NB)) >> 32);
}
// The phase at time t: the product wraps, and so does adding `step` once per time, so the two are equal.
RPF_FOLD_HD uint64_t fold_phase(uint64_t step, int64_t t) { return static_cast<uint64_t>(t) * step; }
RPF_FOLD_HD uint32_t fold_bin(uint64_t step, int64_t t, uint32_t NB) { return fold_bin_of_phase(fold_phase(step, t), NB); }

// Segment g of T times is [fold_segment_begin(T, g), fold_segment_begin(T, g + 1)); G = ceil(T / 16); may be empty.
RPF_FOLD_HD int64_t fold_segment_begin(int64_t T, int g)
{
    const int64_t G = (T + kFoldSegments - 1) / kFoldSegments, at = static_cast<int64_t>(g) * G;
    return at < T ? at : T;
}

// acc + x and acc + x x, every product and every sum rounded on its own, on the host and the device.
RPF_FOLD_HD double fold_add(double acc, double x)
{
#pragma clang fp contract(off)
    return acc + x;
}
RPF_FOLD_HD double fold_add_square(double acc, double x)
{
#pragma clang fp contract(off)
    const double q = x * x;
    return acc + q;
}

// The tile partition: wave (chunk, g, s) owns periods [chunk 64, chunk 64 + 64) of series s over segment g.
RPF_FOLD_HD int fold_period_chunks(int P) { return (P + kFoldLanes - 1) / kFoldLanes; }
// Where the partial sum of phase bin `bin` of lane `lane` lies in the wave's LDS, in doubles: a pitch of 64 doubles, so
// lane i of each 32-lane half of a ds_read_b64 touches dwords 128 bin + 2 i and + 1, banks 2 i and 2 i + 1 whatever bin
// each lane holds: conflict-free (tools/lds_bank_model.py's rules).
RPF_FOLD_HD int fold_lds_index(int bin, int lane) { return bin * kFoldLanes + lane; }
RPF_FOLD_HD size_t fold_lds_bytes(int NB) { return sizeof(double) * static_cast<size_t>(NB) * kFoldLanes; }

// The scratch of one group of `series` series, in bytes from its (256-byte aligned) start:
//   part  [16][series][P][NB] doubles, then mom partials [16][series][2] doubles, then hit partials [16][P][NB] int32.
struct FoldScratch {
    size_t part_at, mom_at, hits_at, bytes;
};
RPF_FOLD_HD FoldScratch fold_scratch(int series, int P, int NB)
{
    const size_t cells = static_cast<size_t>(P) * NB;
    FoldScratch f;
    f.part_at = 0;
    f.mom_at = sizeof(double) * kFoldSegments * series * cells;
    f.hits_at = f.mom_at + sizeof(double) * kFoldSegments * series * 2;
    f.bytes = f.hits_at + sizeof(int32_t) * kFoldSegments * cells;
    return f;
}
// The series of one group: the most whose scratch fits kFoldScratchBytes, at least 1 (one series of 4096 x 128 cells
// needs 96 MB), at most D.
RPF_FOLD_HD int fold_group_series(int D, int P, int NB)
{
    const size_t cells = static_cast<size_t>(P) * NB;
    const size_t fixed = sizeof(int32_t) * kFoldSegments * cells, each = sizeof(double) * kFoldSegments * (cells + 2);
    const size_t fit = (kFoldScratchBytes - fixed) / each;
    return fit < static_cast<size_t>(D) ? static_cast<int>(fit) : D;
}

}  // namespace rpf
