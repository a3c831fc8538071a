// TEST-ONLY host build of the dedisperser's core, for tests/test_dedisperse.py and tests/test_gpu_dedisperse.py:
// csrc/dedisperse_core.h -- the same text the kernel and the engine compile -- behind a C interface, and a walk of the
// kernel's tiles, blocks, spans and LDS indices (csrc/rpf_dedisperse.hip, lane by lane) on the CPU.  Built with
// -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "../../rtl-power-fftw_amd/csrc/dedisperse_core.h"

using namespace rpf;

extern "C" {

int rpf_emul_dedisperse_tt(void) { return kDedispTT; }
int rpf_emul_dedisperse_dt(void) { return kDedispDT; }
int rpf_emul_dedisperse_bc(void) { return kDedispBC; }
int rpf_emul_dedisperse_rows(void) { return kDedispRows; }
int rpf_emul_dedisperse_pitch(void) { return kDedispPitch; }
int rpf_emul_dedisperse_max_trials(void) { return kDedispMaxTrials; }
int rpf_emul_dedisperse_lds_index(int row, int col) { return dedisperse_lds_index(row, col); }
long long rpf_emul_dedisperse_times(long long K, long long dmax) { return dedisperse_times(K, dmax); }

// (tile, block) pairs of this table that are not empty (*pairs) and, returned, those of them read straight from the store.
long long rpf_emul_dedisperse_direct_pairs(const int32_t* delays, const double* weights, int N, int D, long long* pairs)
{
    if (!delays || N < 1 || D < 1) return -1;
    std::vector<double> ones(N, 1.0);
    const double* w = weights ? weights : ones.data();
    long long all = 0, direct = 0;
    for (int tile = 0; tile < dedisperse_trial_tiles(D); ++tile)
        for (int blk = 0; blk < dedisperse_bin_blocks(N); ++blk) {
            const DedispSpan sp = dedisperse_span(delays, w, N, D, tile, blk);
            if (dedisperse_span_empty(sp)) continue;
            ++all;
            direct += !dedisperse_span_fits(sp);
        }
    if (pairs) *pairs = all;
    return direct;
}

// The kernel's walk over rows[K x N]: out[D x T].  visits[D x T] (may be NULL) counts the terms every output took;
// *disorder counts terms that did not come in ascending b for their output, reads of an LDS cell that the block did not
// stage, and LDS indices outside the tile.  Returns T, or -1 for a bad argument.
long long rpf_emul_dedisperse(const double* rows, long long K, int N, const int32_t* delays, const double* weights, int D,
                              double* out, int32_t* visits, long long* disorder, long long* direct_terms)
{
    if (!rows || !delays || !out || K < 0 || N < 1 || D < 1 || D > kDedispMaxTrials) return -1;
    std::vector<double> ones(N, 1.0);
    const double* w = weights ? weights : ones.data();
    int32_t dmax = 0;
    for (size_t i = 0; i < static_cast<size_t>(D) * N; ++i) {
        if (delays[i] < 0) return -1;
        dmax = std::max(dmax, delays[i]);
    }
    const int64_t T = dedisperse_times(K, dmax);
    const int nblocks = dedisperse_bin_blocks(N);
    std::vector<DedispSpan> spans(static_cast<size_t>(dedisperse_trial_tiles(D)) * nblocks);
    for (int tile = 0; tile < dedisperse_trial_tiles(D); ++tile)
        for (int blk = 0; blk < nblocks; ++blk) spans[tile * nblocks + blk] = dedisperse_span(delays, w, N, D, tile, blk);
    std::vector<int32_t> last(static_cast<size_t>(D) * T, -1);
    long long bad = 0, direct = 0;
    const int cells_in_tile = kDedispRows * kDedispPitch;
    std::vector<double> tile(cells_in_tile);
    std::vector<char> staged_cell(cells_in_tile);
    for (int64_t bx = 0; bx < dedisperse_time_tiles(T); ++bx)
        for (int by = 0; by < dedisperse_trial_tiles(D); ++by) {
            const int64_t t0 = bx * kDedispTT;
            const int d0 = by * kDedispDT;
            std::vector<double> acc(static_cast<size_t>(kDedispWG) * kDedispPerLane, 0.0);
            for (int blk = 0; blk < nblocks; ++blk) {
                const DedispSpan sp = spans[by * nblocks + blk];
                if (dedisperse_span_empty(sp)) continue;
                const int c0 = blk * kDedispBC, bc = std::min(kDedispBC, N - c0);
                const bool staged = dedisperse_span_fits(sp);
                if (staged) {
                    std::fill(staged_cell.begin(), staged_cell.end(), 0);
                    const int64_t r0 = t0 + sp.lo, cells = dedisperse_staged_rows(sp, t0, K) * kDedispBC;
                    for (int lane = 0; lane < kDedispWG; ++lane)
                        for (int64_t i = lane; i < cells; i += kDedispWG) {
                            const int row = static_cast<int>(i / kDedispBC), col = static_cast<int>(i % kDedispBC);
                            if (col >= bc) continue;
                            const int at = dedisperse_lds_index(row, col);
                            if (at < 0 || at >= cells_in_tile || r0 + row >= K) {
                                ++bad;
                                continue;
                            }
                            tile[at] = rows[(r0 + row) * N + c0 + col];
                            staged_cell[at] = 1;
                        }
                }
                for (int lane = 0; lane < kDedispWG; ++lane) {
                    const int lt = dedisperse_lane_time(lane);
                    const int64_t t = t0 + lt;
                    for (int j = 0; j < kDedispPerLane; ++j) {
                        const int d = d0 + dedisperse_lane_trial(lane, j);
                        if (d >= D || t >= T) continue;      // (the kernel's lanes at t >= T run on, their sums never stored)
                        const int32_t* dl = delays + static_cast<size_t>(d) * N + c0;
                        for (int c = 0; c < bc; ++c) {
                            const double wb = w[c0 + c];
                            if (wb == 0.0) continue;
                            double r;
                            if (staged) {
                                const int at = dedisperse_lds_index(lt - sp.lo + dl[c], c);
                                if (at < 0 || at >= cells_in_tile || !staged_cell[at]) {
                                    ++bad;
                                    continue;
                                }
                                r = tile[at];
                            } else {
                                r = rows[(t + dl[c]) * N + c0 + c];
                                ++direct;
                            }
                            double& a = acc[static_cast<size_t>(lane) * kDedispPerLane + j];
                            a = dedisperse_term(a, wb, r);
                            int32_t& seen = last[static_cast<size_t>(d) * T + t];
                            if (c0 + c <= seen) ++bad;
                            seen = c0 + c;
                            if (visits) ++visits[static_cast<size_t>(d) * T + t];
                        }
                    }
                }
            }
            for (int lane = 0; lane < kDedispWG; ++lane)
                for (int j = 0; j < kDedispPerLane; ++j) {
                    const int d = d0 + dedisperse_lane_trial(lane, j);
                    const int64_t t = t0 + dedisperse_lane_time(lane);
                    if (d < D && t < T) out[static_cast<size_t>(d) * T + t] = acc[static_cast<size_t>(lane) * kDedispPerLane + j];
                }
        }
    if (disorder) *disorder = bad;
    if (direct_terms) *direct_terms = direct;
    return T;
}

}  // extern "C"
