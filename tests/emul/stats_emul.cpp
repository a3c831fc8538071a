// TEST-ONLY host build of K1 with per-bin statistics (k1_body.inc with STATS; tests/test_spectral_stats.py): the
// frame loop of fft_emul.cpp's run() with phase_accumulate_stats in place of phase_accumulate, for a grid of
// `groups` workgroups of `slots` frame slots each (frame f -> workgroup (f / slots) mod groups, slot f mod slots, as
// the kernel deals them), the flush's combine of the frame slots and the reduce's combine of the workgroups' partial
// planes (stats_combine: +, +, max), all in the kernels' order.  Also hands out the per-frame spectra the
// accumulators saw, so that a test can restate the definitions on exactly those numbers.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../rtl-power-fftw_amd/csrc/fft_core.h"

namespace {

using rpf::cf;

template <class G, int J>
void load_tw(int t, const std::vector<cf>& twN, cf (*tw)[G::P - 1])
{
    if constexpr (J < G::NPASS) {
        for (int r = 1; r < G::P; ++r) tw[J - 1][r - 1] = twN[rpf::twiddle_index<G, J>(t, r)];
        load_tw<G, J + 1>(t, twN, tw);
    }
}

template <class G, int J>
void middle(std::vector<std::vector<cf>>& regs, std::vector<cf>& slab, const std::vector<std::vector<cf>>& tws)
{
    if constexpr (J < G::NPASS) {
        constexpr int P = G::P, T = G::T;
        for (int t = 0; t < T; ++t) {
            if constexpr (J > 1) rpf::phase_fetch<G, J>(t, regs[t].data(), slab.data());
        }
        for (int t = 0; t < T; ++t) {
            rpf::phase_butterfly_twiddle<G>(regs[t].data(), tws[t].data() + (J - 1) * (P - 1));
            rpf::phase_store<G, J>(t, regs[t].data(), slab.data());
        }
        middle<G, J + 1>(regs, slab, tws);
    }
}

// out: 3 x N (S1, S2, PK); spectra (may be null): nframes x N x 2 floats, frame-major, in bin order
template <int N, int P>
int run(const float* window, const uint8_t* stream, long nframes, int slots, int groups, double* out, float* spectra)
{
    using G = rpf::Geom<N, P>;
    constexpr int T = G::T;
    if (slots < 1 || groups < 1) return -2;
    std::vector<cf> twN(N);
    const long double two_pi = 6.283185307179586476925286766559005768L;
    for (int k = 0; k < N; ++k) {
        long double a = two_pi * k / N;
        twN[k] = {(float)cosl(a), (float)(-sinl(a))};
    }
    std::vector<std::vector<cf>> tws(T, std::vector<cf>((G::NPASS - 1) * (P - 1)));
    for (int t = 0; t < T; ++t) load_tw<G, 1>(t, twN, reinterpret_cast<cf(*)[P - 1]>(tws[t].data()));
    std::vector<std::vector<cf>> regs(T, std::vector<cf>(P));
    std::vector<cf> slab(G::LDS_CPX);
    for (auto& c : slab) c = {NAN, NAN};
    // the register accumulators of every (workgroup, frame slot, thread): [plane][register]
    const size_t lanes = static_cast<size_t>(groups) * slots * T;
    std::vector<double> acc(lanes * P, 0.0), s2(lanes * P, 0.0), pk(lanes * P, 0.0);

    constexpr int WAVES = T >= 64 ? T / 64 : 1;
    std::vector<uint8_t> raw(WAVES * rpf::kRawChunk * P);
    for (long f = 0; f < nframes; ++f) {
        const uint8_t* frame = stream + (size_t)f * 2 * N;
        for (int w = 0; w < WAVES; ++w)
            for (int j = 0; j < rpf::kRawChunk * P; ++j) {
                int slot, off;
                rpf::raw_source<G>(w, j, &slot, &off);
                raw[w * rpf::kRawChunk * P + j] = slot == 0 ? frame[off] : 0;
            }
        for (int t = 0; t < T; ++t) {
            const float sgn = (t & 1) ? -1.0f : 1.0f;
            float wsgn[P];
            if (window)
                for (int a = 0; a < P; ++a) wsgn[a] = window[t + T * a] * sgn;
            const uint8_t* lane_raw = raw.data() + (t / 64) * rpf::kRawChunk * P + 2 * (t % 64);
            if (window) rpf::phase_unpack<G, true>(lane_raw, sgn, wsgn, regs[t].data());
            else rpf::phase_unpack<G, false>(lane_raw, sgn, wsgn, regs[t].data());
        }
        middle<G, 1>(regs, slab, tws);
        const size_t wg = static_cast<size_t>((f / slots) % groups), fs = static_cast<size_t>(f % slots);
        for (int t = 0; t < T; ++t) {
            rpf::phase_fetch<G, G::NPASS>(t, regs[t].data(), slab.data());
            rpf::phase_last<G>(regs[t].data());
            const size_t at = ((wg * slots + fs) * T + t) * P;
            rpf::phase_accumulate_stats(regs[t].data(), &acc[at], &s2[at], &pk[at], P);
            if (spectra)
                for (int a = 0; a < P; ++a) {
                    float* o = spectra + (static_cast<size_t>(f) * N + rpf::bin_of<G>(t, a)) * 2;
                    o[0] = regs[t][a].x;
                    o[1] = regs[t][a].y;
                }
        }
    }
    // the flush: the frame slots of a workgroup combine from 0 in slot order; the reduce: the workgroups' partial
    // planes in workgroup order
    for (int plane = 0; plane < rpf::kStatsPlanes; ++plane) {
        const std::vector<double>& src = plane == 0 ? acc : plane == 1 ? s2 : pk;
        for (int t = 0; t < T; ++t)
            for (int a = 0; a < P; ++a) {
                double tot = 0.0;
                for (int wg = 0; wg < groups; ++wg) {
                    double v = 0.0;
                    for (int k = 0; k < slots; ++k)
                        v = rpf::stats_combine(plane, v, src[((static_cast<size_t>(wg) * slots + k) * T + t) * P + a]);
                    tot = rpf::stats_combine(plane, tot, v);
                }
                out[static_cast<size_t>(plane) * N + rpf::bin_of<G>(t, a)] = tot;
            }
    }
    return 0;
}

}  // namespace

extern "C" {
// The geometries the shipped statistics kernels use (k1_stats_table.h): P = 8 for 64 and 512, 16 for the rest.
int rpf_emul_stats(int N, const float* window, const uint8_t* stream, long nframes, int slots, int groups, double* out,
                   float* spectra)
{
    switch (N) {
        case 64: return run<64, 8>(window, stream, nframes, slots, groups, out, spectra);
        case 128: return run<128, 16>(window, stream, nframes, slots, groups, out, spectra);
        case 512: return run<512, 8>(window, stream, nframes, slots, groups, out, spectra);
        case 1024: return run<1024, 16>(window, stream, nframes, slots, groups, out, spectra);
        case 4096: return run<4096, 16>(window, stream, nframes, slots, groups, out, spectra);
        case 8192: return run<8192, 16>(window, stream, nframes, slots, groups, out, spectra);
    }
    return -1;
}
int rpf_emul_stats_p(int N) { return N == 64 || N == 512 ? 8 : 16; }
}
