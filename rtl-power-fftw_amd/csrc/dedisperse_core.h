// dedisperse_core.h -- what the incoherent dedispersion of the stored integrations (include/rpf_engine.h,
// rpf_dedisperse_device) states once: the term and its order, T, the tile partition, the per-(trial tile, bin block)
// span rule, which lane owns which (trial, time), and the LDS index.
//
// Plain C++: the kernel (rpf_dedisperse.hip), the engine (rpf_engine.cpp) and the CPU emulator
// (tests/emul/dedisperse_emul.cpp) share what is below, so they cannot drift.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RPF_DD_HD __host__ __device__ __forceinline__
#else
#define RPF_DD_HD inline
#endif

namespace rpf {

constexpr int kDedispMaxTrials = 4096;
constexpr int kDedispTT = 64;        // times of a tile: the lanes of one wave, time fastest across lanes
constexpr int kDedispDT = 16;        // trials of a tile
constexpr int kDedispBC = 32;        // bins of a block: a staged row is 256 contiguous bytes of a store row
constexpr int kDedispWG = 256;       // lanes of a workgroup: kDedispWG / kDedispTT waves, each kDedispPerLane trials of the tile
constexpr int kDedispSubs = kDedispWG / kDedispTT;          // 4
constexpr int kDedispPerLane = kDedispDT / kDedispSubs;     // 4 accumulators per lane
// The LDS tile: kDedispRows rows of kDedispPitch doubles (59136 bytes, two workgroups per CU).  The pitch is odd, so
// the 32 lanes that a ds_read_b64 serves together (one bin at 32 consecutive rows) touch dwords 2 (row pitch + c), whose
// banks (dword mod 64) are all different: conflict-free (tools/lds_bank_model.py's rules).
constexpr int kDedispPitch = kDedispBC + 1;
constexpr int kDedispRows = 224;
static_assert(kDedispDT % kDedispSubs == 0 && kDedispWG % kDedispTT == 0 && (kDedispPitch & 1) == 1, "tile geometry");
static_assert(sizeof(double) * kDedispRows * kDedispPitch <= 65536, "the tile is static LDS");

// acc + w r, the product and the sum each rounded on its own (never one fused operation), on the host and the device.
RPF_DD_HD double dedisperse_term(double acc, double w, double r)
{
#pragma clang fp contract(off)
    const double p = w * r;
    return acc + p;
}

// T: the times every trial can form from K rows when the largest delay of the table is dmax.
RPF_DD_HD int64_t dedisperse_times(int64_t K, int64_t dmax) { return K > dmax ? K - dmax : 0; }

RPF_DD_HD int64_t dedisperse_time_tiles(int64_t T) { return (T + kDedispTT - 1) / kDedispTT; }
RPF_DD_HD int dedisperse_trial_tiles(int D) { return (D + kDedispDT - 1) / kDedispDT; }
RPF_DD_HD int dedisperse_bin_blocks(int N) { return (N + kDedispBC - 1) / kDedispBC; }

// Lane `lane` of a workgroup owns time t0 + dedisperse_lane_time(lane) and, for j < kDedispPerLane, trial
// d0 + dedisperse_lane_trial(lane, j) of its tile: a wave is 64 consecutive times of one trial at a time.
RPF_DD_HD int dedisperse_lane_time(int lane) { return lane % kDedispTT; }
RPF_DD_HD int dedisperse_lane_trial(int lane, int j) { return lane / kDedispTT + j * kDedispSubs; }

// The span of (trial tile, bin block): the smallest and the largest delay of the tile's trials (those below D) over the
// block's bins of non-zero weight.  hi < lo: no such bin, the block adds nothing and is skipped.
struct DedispSpan {
    int32_t lo, hi;
};

inline DedispSpan dedisperse_span(const int32_t* delays, const double* weights, int N, int D, int tile, int block)
{
    DedispSpan s{INT32_MAX, -1};
    const int d1 = std::min(D, (tile + 1) * kDedispDT), b1 = std::min(N, (block + 1) * kDedispBC);
    for (int d = tile * kDedispDT; d < d1; ++d)
        for (int b = block * kDedispBC; b < b1; ++b) {
            if (weights[b] == 0.0) continue;
            const int32_t v = delays[static_cast<size_t>(d) * N + b];
            s.lo = std::min(s.lo, v);
            s.hi = std::max(s.hi, v);
        }
    return s;
}

RPF_DD_HD bool dedisperse_span_empty(DedispSpan s) { return s.hi < s.lo; }
// The block is staged through LDS where rows [t0 + lo, t0 + kDedispTT + hi) fit the tile; else every lane reads the
// store directly (correct and slow).
RPF_DD_HD bool dedisperse_span_fits(DedispSpan s)
{
    return static_cast<int64_t>(s.hi) - s.lo + kDedispTT <= kDedispRows;
}
// Rows a staged block holds for the time tile at t0: [t0 + lo, min(t0 + kDedispTT + hi, K)); at least one for t0 < T.
RPF_DD_HD int64_t dedisperse_staged_rows(DedispSpan s, int64_t t0, int64_t K)
{
    const int64_t end = t0 + kDedispTT + s.hi;
    return (end < K ? end : K) - (t0 + s.lo);
}
// Where row `row` of the staged rows (0 = store row t0 + lo) and bin `col` of the block lies in the tile, in doubles.
RPF_DD_HD int dedisperse_lds_index(int row, int col) { return row * kDedispPitch + col; }

}  // namespace rpf
