// TEST-ONLY host build of the series walk with per-bin statistics, for tests/test_series_stats.py: the partition of
// series_partition.h walked as k1_scan_body.inc walks it under SERIES && STATS -- three accumulators per frame slot
// (sum, sum of squares, maximum from 0), a three-plane hand-over per segment -- and the fix-up's blocks with a plane
// dimension (rpf_kernels_series_stats.hip).  Everything about WHERE a segment goes calls the header's own functions.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../rtl-power-fftw_amd/csrc/series_partition.h"

using namespace rpf;

namespace {
constexpr int kPlanes = 3;
// fft_core.h's stats_combine: planes 0 and 1 add, plane 2 takes the maximum
double combine(int plane, double a, double b) { return plane == 2 ? (a > b ? a : b) : a + b; }
}  // namespace

extern "C" {

// power[f]: float64 stand-ins for the frames' powers (at least K L of them).  rows[K x 3] (pre-filled by the caller):
// row k = sum, sum of squares, maximum of its L frames.  frame_owner[f] counts how often frame f was accumulated,
// row_writes[3 k + p] and slot_writes[3 s + p] how often plane p of row k / of partial slot s (of 2 grid) was written.
// An inactive frame slot leaves all three accumulators alone.  Returns the grid, or -1.
int rpf_emul_series_stats_walk(long long K, long long L, int fpw, int max_grid, const double* power, double* rows,
                               int* frame_owner, int* row_writes, int* slot_writes)
{
    SeriesArgs a{};
    const int grid = partition_series(K, L, fpw, max_grid, 2 * 64, &a);
    if (grid < 1) return grid;
    SeriesTable tbl;
    tbl.load(a);
    std::vector<double> partial(2 * static_cast<size_t>(grid) * kPlanes, 0.0);
    for (int w = 0; w < grid; ++w) {
        int first, count;
        hop_share(w, a.q, a.r, a.step, &first, &count);
        HopCursor cur;
        cur.seek(tbl, first);
        int it = 0;
        while (true) {
            const int in_hop = cur.end - cur.j, left = count - it;
            const int seg = in_hop < left ? in_hop : left;
            std::vector<double> acc(static_cast<size_t>(fpw) * kPlanes, 0.0);       // [plane][frame slot], all from 0
            int fb = (cur.j - cur.begin) * fpw;
            for (int n = seg; n > 0; --n, ++it, fb += fpw)
                for (int fs = 0; fs < fpw; ++fs)
                    if (fb + fs < cur.nframes) {
                        const long long f = static_cast<long long>(cur.h) * a.L + fb + fs;
                        const double p = power[f];
                        acc[0 * fpw + fs] += p;
                        acc[1 * fpw + fs] += p * p;
                        acc[2 * fpw + fs] = combine(2, acc[2 * fpw + fs], p);
                        frame_owner[f]++;
                    }
            const bool complete = series_segment_complete(cur.j, first + it, cur.begin, cur.end);
            const int slot = complete ? -1 : series_segment_slot(w, cur.j, cur.begin);
            for (int plane = 0; plane < kPlanes; ++plane) {
                double v = 0.0;
                for (int fs = 0; fs < fpw; ++fs) v = combine(plane, v, acc[plane * fpw + fs]);
                if (complete) {
                    rows[static_cast<size_t>(cur.h) * kPlanes + plane] = v;
                    row_writes[static_cast<size_t>(cur.h) * kPlanes + plane]++;
                } else {
                    partial[static_cast<size_t>(slot) * kPlanes + plane] = v;
                    slot_writes[static_cast<size_t>(slot) * kPlanes + plane]++;
                }
            }
            if (it >= count) break;
            cur.seek(tbl, cur.end);
        }
    }
    for (int bnd = 1; bnd < grid; ++bnd) {            // series_stats_fixup_kernel, blockIdx.y = bnd - 1, blockIdx.z = plane
        int lo, hi;
        hop_range(bnd, a.q, a.r, &lo, &hi);
        const int k = series_div(lo, a.magic, a.shift);
        if (k * a.ips == lo) continue;
        int wa, wb;
        series_spectrum_wgs(k, a, &wa, &wb);
        if (wa != bnd - 1) continue;
        for (int plane = 0; plane < kPlanes; ++plane) {
            double tot = 0.0;
            for (int j = 0; j <= wb - wa; ++j)
                tot = combine(plane, tot, partial[static_cast<size_t>(2 * (wa + j) + (j == 0 ? 1 : 0)) * kPlanes + plane]);
            rows[static_cast<size_t>(k) * kPlanes + plane] = tot;
            row_writes[static_cast<size_t>(k) * kPlanes + plane]++;
        }
    }
    return grid;
}

}  // extern "C"
