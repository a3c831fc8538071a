// TEST-ONLY host build of the series partition (series_partition.h), for tests/test_series.py.  Everything here calls
// the header's own functions -- the ones the engine, the series kernel and the fix-up kernel call -- so that the
// brute-force checks in Python are checks of the shipped arithmetic.
#include <cstdint>
#include <cstddef>
#include <vector>

#include "../../rtl-power-fftw_amd/csrc/series_partition.h"

using namespace rpf;

extern "C" {

// partition_series; out8 = K, L, ips, total, q, r, shift, magic (as int64)
int rpf_emul_series_partition(long long K, long long L, int fpw, int max_grid, long long* out8)
{
    SeriesArgs a{};
    const int grid = partition_series(K, L, fpw, max_grid, 2 * 64, &a);
    if (grid < 0) return grid;
    const long long v[8] = {a.K, a.L, a.ips, a.total, a.q, a.r, a.shift, static_cast<long long>(a.magic)};
    for (int i = 0; i < 8; ++i) out8[i] = v[i];
    return grid;
}

long long rpf_emul_series_max_spectra(long long L, int fpw) { return series_max_spectra(L, fpw); }

// the division-free quotient at the n given iterations, for the divisor ips
void rpf_emul_series_div(int ips, const int* it, int n, int* out)
{
    unsigned magic;
    int shift;
    series_magic(ips, &magic, &shift);
    for (int i = 0; i < n; ++i) out[i] = series_div(it[i], magic, shift);
}

static SeriesArgs args_of(long long K, long long L, int fpw, int max_grid, int* grid)
{
    SeriesArgs a{};
    *grid = partition_series(K, L, fpw, max_grid, 2 * 64, &a);
    return a;
}

// per workgroup: lo, hi, first and last spectrum (4 ints each)
int rpf_emul_series_ranges(long long K, long long L, int fpw, int max_grid, int* out4)
{
    int grid;
    const SeriesArgs a = args_of(K, L, fpw, max_grid, &grid);
    for (int w = 0; w < grid; ++w) {
        hop_range(w, a.q, a.r, &out4[4 * w], &out4[4 * w + 1]);
        series_range_spectra(w, a, &out4[4 * w + 2], &out4[4 * w + 3]);
    }
    return grid;
}

int rpf_emul_series_complete(long long K, long long L, int fpw, int max_grid, int w, int k)
{
    int grid;
    const SeriesArgs a = args_of(K, L, fpw, max_grid, &grid);
    return series_complete(w, k, a) ? 1 : 0;
}
int rpf_emul_series_slot(long long K, long long L, int fpw, int max_grid, int w, int k)
{
    int grid;
    const SeriesArgs a = args_of(K, L, fpw, max_grid, &grid);
    return series_slot(w, k, a);
}
void rpf_emul_series_spectrum_wgs(long long K, long long L, int fpw, int max_grid, int k, int* wa, int* wb)
{
    int grid;
    const SeriesArgs a = args_of(K, L, fpw, max_grid, &grid);
    series_spectrum_wgs(k, a, wa, wb);
}

// The kernel's walk with float64 stand-ins for the frames' powers: power[f] for the frames of the stream (at least
// K L of them).  Every workgroup walks its range with HopCursor over SeriesTable exactly as k1_scan_body.inc does -- one
// accumulator per frame slot, a hand-over at the end of every segment, the frame slots summed in slot order --, a
// complete segment goes to rows[k], a cut one to partial[slot]; then the fix-up's blocks (one per workgroup boundary)
// add the segments of the spectra they own in workgroup order.  rows[K] must be pre-filled by the caller; frame_owner
// [f] counts how often frame f was accumulated; slot_writes[2 grid] how often each partial slot was written.
// Returns the grid, or -1.
int rpf_emul_series_walk(long long K, long long L, int fpw, int max_grid, const double* power, double* rows,
                         int* frame_owner, int* slot_writes)
{
    int grid;
    const SeriesArgs a = args_of(K, L, fpw, max_grid, &grid);
    if (grid < 1) return grid;
    SeriesTable tbl;
    tbl.load(a);
    std::vector<double> partial(2 * static_cast<size_t>(grid), 0.0);
    for (int w = 0; w < grid; ++w) {
        int first, count;
        hop_share(w, a.q, a.r, a.step, &first, &count);
        HopCursor cur;
        cur.seek(tbl, first);
        int it = 0;
        while (true) {
            const int in_hop = cur.end - cur.j, left = count - it;
            const int seg = in_hop < left ? in_hop : left;
            std::vector<double> acc(fpw, 0.0);
            int fb = (cur.j - cur.begin) * fpw;
            for (int n = seg; n > 0; --n, ++it, fb += fpw)
                for (int fs = 0; fs < fpw; ++fs)
                    if (fb + fs < cur.nframes) {
                        const long long f = static_cast<long long>(cur.h) * a.L + fb + fs;   // (stream(h) = base + h L bN)
                        acc[fs] += power[f];
                        frame_owner[f]++;
                    }
            double v = 0.0;
            for (int fs = 0; fs < fpw; ++fs) v += acc[fs];
            if (series_segment_complete(cur.j, first + it, cur.begin, cur.end)) {
                rows[cur.h] = v;
            } else {
                const int slot = series_segment_slot(w, cur.j, cur.begin);
                partial[slot] = v;
                slot_writes[slot]++;
            }
            if (it >= count) break;
            cur.seek(tbl, cur.end);
        }
    }
    for (int bnd = 1; bnd < grid; ++bnd) {            // series_fixup_kernel, blockIdx.y = bnd - 1
        int lo, hi;
        hop_range(bnd, a.q, a.r, &lo, &hi);
        const int k = series_div(lo, a.magic, a.shift);
        if (k * a.ips == lo) continue;
        int wa, wb;
        series_spectrum_wgs(k, a, &wa, &wb);
        if (wa != bnd - 1) continue;
        double tot = 0.0;
        for (int j = 0; j <= wb - wa; ++j) tot += partial[2 * (wa + j) + (j == 0 ? 1 : 0)];
        rows[k] = tot;
    }
    return grid;
}

}  // extern "C"
