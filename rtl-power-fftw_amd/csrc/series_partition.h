// series_partition.h -- how ONE persistent launch of the fused kernel walks a uniform series of K spectra of L frames
// each, cut from one contiguous stream (rpf_accumulate_device_series): the scan of hop_partition.h with an arithmetic
// table in place of the 16-entry one.  Every "hop" k has the same L frames and starts at frame k L, so with
// ips = ceil(L / FPW) iterations per spectrum
//   hop_of(it) = it / ips      it_begin(k) = k ips      nframes(k) = L      stream(k) = base + k L bN
// and K is bounded by nothing but the 2^31 iterations of one launch.  The quotient is a multiply and a shift by
// constants the host works out (series_magic), exact for every iteration below 2^31.
//
// Workgroup w of G owns the contiguous iterations [lo_w, hi_w) (hop_range).  A spectrum whose iterations all lie in one
// workgroup's range is COMPLETE: that workgroup stores it straight into its output row.  Any other spectrum spans
// workgroups; each of them holds one SEGMENT of it and leaves it in a partial slot, and a fix-up kernel adds the
// segments in workgroup order.  A range cuts at most two spectra -- its first (begun by a predecessor: slot 2w) and its
// last (finished by a successor: slot 2w + 1; a range inside one spectrum writes slot 2w alone) -- so the scratch is
// 2 G spectra whatever K is.
//
// Plain C++: the engine, both kernels and the CPU tests (tests/emul/series_emul.cpp) share what is below.
#pragma once

#include <cstdint>

#include "hop_partition.h"

namespace rpf {

struct SeriesArgs {
    int K;                               // spectra in this launch
    int L;                               // frames per spectrum
    int ips;                             // iterations per spectrum = ceil(L / fpw)
    int total;                           // iterations in the launch = K ips = q grid + r
    int q, r;
    unsigned magic;                      // it / ips = (it * magic) >> shift for 0 <= it < 2^31 (series_magic)
    int shift;
    static constexpr int step = 1;       // (the scan body's name for the distance between a workgroup's iterations)
    long spectrum_bytes;                 // L bN: from one spectrum's first frame to the next one's
    const uint8_t* stream;               // first byte of spectrum 0
    double* out;                         // row k = out[k N .. k N + N)
};

// magic = ceil(2^(31 + l) / d), l = ceil(log2 d): floor(n / d) = (n * magic) >> (31 + l) for every 0 <= n < 2^31
// (Granlund & Montgomery: the error of the multiplier, < 2^l / d / 2^(31 + l) per unit of n, adds up to less than 1 / d).
// magic < 2^32 and the product < 2^63.
RPF_HOP_HD void series_magic(int d, unsigned* magic, int* shift)
{
    int l = 0;
    while ((static_cast<int64_t>(1) << l) < d) ++l;
    const uint64_t p = static_cast<uint64_t>(1) << (31 + l);
    *magic = static_cast<unsigned>((p + static_cast<uint64_t>(d) - 1) / static_cast<uint64_t>(d));
    *shift = 31 + l;
}
RPF_HOP_HD int series_div(int n, unsigned magic, int shift)
{
    return static_cast<int>((static_cast<uint64_t>(static_cast<unsigned>(n)) * magic) >> shift);
}

// The TABLE of HopCursor::seek (hop_partition.h) for a series: arithmetic on wave-uniform values.
struct SeriesTable {
    int ips, L, shift;
    unsigned magic;
    long spectrum_bytes;
    const uint8_t* base;
    RPF_HOP_HD void load(const SeriesArgs& a)
    {
        ips = a.ips;
        L = a.L;
        shift = a.shift;
        magic = a.magic;
        spectrum_bytes = a.spectrum_bytes;
        base = a.stream;
    }
    RPF_HOP_HD int hop_of(int it) const { return series_div(it, magic, shift); }
    RPF_HOP_HD int it_begin(int h) const { return h * ips; }
    RPF_HOP_HD int nframes(int) const { return L; }
    RPF_HOP_HD const uint8_t* stream(int h) const { return base + static_cast<long>(h) * spectrum_bytes; }
    RPF_HOP_HD int slot_bias(int) const { return 0; }   // (HopLanes' slot rule; named by the scan body's other branch only)
};

// Fills *a (all but stream and out, which are the caller's) for K spectra of L frames on a grid of at most max_grid
// workgroups running fpw frames each.  Returns the grid to launch, 0 for K = 0, or -1 if the arguments do not fit
// (K ips must stay below 2^31: series_max_spectra).
inline int partition_series(int64_t K, int64_t L, int fpw, int max_grid, long frame_bytes, SeriesArgs* a)
{
    if (K < 0 || L < 1 || fpw < 1 || max_grid < 1 || L > INT32_MAX - fpw) return -1;
    const int64_t ips = (L + fpw - 1) / fpw;
    if (K * ips > INT32_MAX) return -1;
    a->K = static_cast<int>(K);
    a->L = static_cast<int>(L);
    a->ips = static_cast<int>(ips);
    a->total = static_cast<int>(K * ips);
    const int grid = a->total < max_grid ? a->total : max_grid;
    a->q = grid ? a->total / grid : 0;
    a->r = grid ? a->total % grid : 0;
    series_magic(a->ips, &a->magic, &a->shift);
    a->spectrum_bytes = static_cast<long>(L) * frame_bytes;
    return grid;
}
// the most spectra of L frames one launch takes
inline int64_t series_max_spectra(int64_t L, int fpw) { return INT32_MAX / ((L + fpw - 1) / fpw); }

// first and last spectrum workgroup w touches
RPF_HOP_HD void series_range_spectra(int w, const SeriesArgs& a, int* first, int* last)
{
    int lo, hi;
    hop_range(w, a.q, a.r, &lo, &hi);
    *first = series_div(lo, a.magic, a.shift);
    *last = series_div(hi - 1, a.magic, a.shift);
}
// Does the segment [seg_lo, seg_hi) of iterations hold all of its spectrum, whose iterations are [begin, end)?
RPF_HOP_HD bool series_segment_complete(int seg_lo, int seg_hi, int begin, int end) { return seg_lo == begin && seg_hi == end; }
// ... and if not, its partial slot: 2w if the spectrum began before the workgroup's range, else 2w + 1
RPF_HOP_HD int series_segment_slot(int w, int seg_lo, int begin) { return 2 * w + (seg_lo == begin ? 1 : 0); }

// all iterations of spectrum k inside workgroup w's range?
RPF_HOP_HD bool series_complete(int w, int k, const SeriesArgs& a)
{
    int lo, hi;
    hop_range(w, a.q, a.r, &lo, &hi);
    return k * a.ips >= lo && (k + 1) * a.ips <= hi;
}
// Partial slot of workgroup w's segment of spectrum k (which its range overlaps); -1: complete, no slot.
RPF_HOP_HD int series_slot(int w, int k, const SeriesArgs& a)
{
    int lo, hi;
    hop_range(w, a.q, a.r, &lo, &hi);
    const int begin = k * a.ips, end = begin + a.ips;
    const int seg_lo = begin > lo ? begin : lo, seg_hi = end < hi ? end : hi;
    if (series_segment_complete(seg_lo, seg_hi, begin, end)) return -1;
    return series_segment_slot(w, seg_lo, begin);
}
// The workgroup whose range holds iteration `it` (< total): the first r ranges have q + 1 iterations, the rest q.
RPF_HOP_HD int series_wg_of(int it, int q, int r)
{
    const int head = r * (q + 1);
    return it < head ? it / (q + 1) : r + (it - head) / q;
}
// The workgroups [*wa, *wb] that hold spectrum k, in closed form.
RPF_HOP_HD void series_spectrum_wgs(int k, const SeriesArgs& a, int* wa, int* wb)
{
    *wa = series_wg_of(k * a.ips, a.q, a.r);
    *wb = series_wg_of((k + 1) * a.ips - 1, a.q, a.r);
}

}  // namespace rpf
