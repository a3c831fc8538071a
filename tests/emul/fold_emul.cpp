// TEST-ONLY host build of the fold's core, for tests/test_fold.py and tests/test_gpu_fold.py: csrc/fold_core.h -- the same
// text the kernel and the engine compile -- behind a C interface, and a walk of the kernel's partition (csrc/rpf_fold.hip:
// wave by wave, lane by lane, the LDS cells, the register that holds the current bin's sum, the scratch layout, the
// groups of series and the second level) on the CPU.  Built with -ffp-contract=off.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../rtl-power-fftw_amd/csrc/fold_core.h"

using namespace rpf;

extern "C" {

int rpf_emul_fold_segments(void) { return kFoldSegments; }
int rpf_emul_fold_lanes(void) { return kFoldLanes; }
int rpf_emul_fold_max_bins(void) { return kFoldMaxBins; }
int rpf_emul_fold_max_series(void) { return kFoldMaxSeries; }
int rpf_emul_fold_max_periods(void) { return kFoldMaxPeriods; }
long long rpf_emul_fold_max_cells(void) { return kFoldMaxCells; }
long long rpf_emul_fold_scratch_cap(void) { return static_cast<long long>(kFoldScratchBytes); }
int rpf_emul_fold_lds_index(int bin, int lane) { return fold_lds_index(bin, lane); }
long long rpf_emul_fold_lds_bytes(int NB) { return static_cast<long long>(fold_lds_bytes(NB)); }
unsigned rpf_emul_fold_bin(unsigned long long step, long long t, unsigned NB) { return fold_bin(step, t, NB); }
long long rpf_emul_fold_segment_begin(long long T, int g) { return fold_segment_begin(T, g); }
int rpf_emul_fold_group_series(int D, int P, int NB) { return fold_group_series(D, P, NB); }
long long rpf_emul_fold_scratch_bytes(int series, int P, int NB) { return static_cast<long long>(fold_scratch(series, P, NB).bytes); }

// The kernel's walk over x[D x T]: prof[D x P x NB], hits[P x NB], mom[D x 2].  per_group < 1: the engine's groups of series
// (fold_group_series); else that many series per group, so that a test reaches more than one group at a small size.
// *disorder counts additions that did not come in ascending t for their cell, LDS indices outside the wave's cells, cells
// of a lane touched by another lane, and scratch cells written twice or never.  Returns the groups, or -1 for a bad argument.
long long rpf_emul_fold(const double* x, int D, long long T, const unsigned long long* steps, int P, int NB, int per_group,
                        double* prof, int32_t* hits, double* mom, long long* disorder)
{
    if (!x || !steps || !prof || !hits || !mom || D < 1 || D > kFoldMaxSeries || P < 1 || P > kFoldMaxPeriods || NB < 1 ||
        NB > kFoldMaxBins || T < 0)
        return -1;
    if (per_group < 1) per_group = fold_group_series(D, P, NB);
    long long bad = 0, groups = 0;
    const size_t cells = static_cast<size_t>(P) * NB;
    const int chunks = fold_period_chunks(P), lds_cells = static_cast<int>(fold_lds_bytes(NB) / sizeof(double));
    std::vector<double> cell(lds_cells);
    std::vector<int32_t> count(lds_cells);
    std::vector<long long> last(lds_cells);
    for (int s0 = 0; s0 < D; s0 += per_group, ++groups) {
        const int series = std::min(per_group, D - s0);
        const FoldScratch at = fold_scratch(series, P, NB);
        if (per_group == fold_group_series(D, P, NB) && at.bytes > kFoldScratchBytes) ++bad;
        std::vector<unsigned char> scratch(at.bytes);
        double* const part = reinterpret_cast<double*>(scratch.data() + at.part_at);
        double* const mom_part = reinterpret_cast<double*>(scratch.data() + at.mom_at);
        int32_t* const hit_part = reinterpret_cast<int32_t*>(scratch.data() + at.hits_at);
        std::vector<char> written(static_cast<size_t>(kFoldSegments) * series * cells, 0);
        for (int s = 0; s < series; ++s)
            for (int chunk = 0; chunk < chunks; ++chunk)
                for (int g = 0; g < kFoldSegments; ++g) {
                    const int p0 = chunk * kFoldLanes;
                    const int64_t lo = fold_segment_begin(T, g), hi = fold_segment_begin(T, g + 1);
                    const double* xs = x + static_cast<size_t>(s0 + s) * T;
                    std::fill(cell.begin(), cell.end(), 0.0);
                    std::fill(count.begin(), count.end(), 0);
                    std::fill(last.begin(), last.end(), -1);
                    for (int lane = 0; lane < kFoldLanes; ++lane) {
                        const int p = p0 + lane;
                        const uint64_t step = p < P ? steps[p] : 0;
                        uint64_t phase = fold_phase(step, lo);
                        uint32_t cur = fold_bin_of_phase(phase, NB);
                        double sum = 0.0, m0 = 0.0, m1 = 0.0;
                        int32_t n = 0;
                        auto index = [&](uint32_t bin) {
                            const int i = fold_lds_index(static_cast<int>(bin), lane);
                            if (i < 0 || i >= lds_cells || i % kFoldLanes != lane) {
                                ++bad;
                                return 0;
                            }
                            return i;
                        };
                        for (int64_t t = lo; t < hi; ++t) {
                            const uint32_t bin = fold_bin_of_phase(phase, NB);
                            if (bin != fold_bin(step, t, NB)) ++bad;          // the advanced phase is the product's
                            if (bin != cur) {
                                cell[index(cur)] = sum;
                                count[index(cur)] = n;
                                sum = cell[index(bin)];
                                n = count[index(bin)];
                                cur = bin;
                            }
                            if (t <= last[index(cur)]) ++bad;
                            last[index(cur)] = t;
                            sum = fold_add(sum, xs[t]);
                            ++n;
                            m0 = fold_add(m0, xs[t]);
                            m1 = fold_add_square(m1, xs[t]);
                            phase += step;
                        }
                        cell[index(cur)] = sum;
                        count[index(cur)] = n;
                        if (chunk == 0 && lane == 0) {
                            mom_part[(static_cast<size_t>(g) * series + s) * 2] = m0;
                            mom_part[(static_cast<size_t>(g) * series + s) * 2 + 1] = m1;
                        }
                    }
                    // out through LDS, transposed
                    const size_t out = (static_cast<size_t>(g) * series + s) * cells;
                    for (int lane = 0; lane < kFoldLanes; ++lane)
                        for (int i = lane; i < NB * kFoldLanes; i += kFoldLanes) {
                            const int pl = i / NB, b = i - pl * NB;
                            if (p0 + pl >= P) continue;
                            const size_t to = out + static_cast<size_t>(p0 + pl) * NB + b;
                            if (written[to]++) ++bad;
                            part[to] = cell[fold_lds_index(b, pl)];
                            // (the hits are the same walk of a plane of ones, one launch per call: series 0 of group 0 here)
                            if (s0 == 0 && s == 0) hit_part[(static_cast<size_t>(g) * P + p0 + pl) * NB + b] = count[fold_lds_index(b, pl)];
                        }
                }
        for (char w : written) bad += w != 1;
        // the second level
        const size_t series_cells = cells * series;
        for (size_t i = 0; i < series_cells; ++i) {
            double acc = 0.0;
            for (int g = 0; g < kFoldSegments; ++g) acc = fold_add(acc, part[g * series_cells + i]);
            prof[s0 * cells + i] = acc;
        }
        for (size_t i = 0; i < 2 * static_cast<size_t>(series); ++i) {
            double acc = 0.0;
            for (int g = 0; g < kFoldSegments; ++g) acc = fold_add(acc, mom_part[g * 2 * series + i]);
            mom[2 * static_cast<size_t>(s0) + i] = acc;
        }
        if (s0 == 0)
            for (size_t i = 0; i < cells; ++i) {
                int32_t n = 0;
                for (int g = 0; g < kFoldSegments; ++g) n += hit_part[g * cells + i];
                hits[i] = n;
            }
    }
    if (disorder) *disorder = bad;
    return groups;
}

}  // extern "C"
