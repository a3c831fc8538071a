// TEST-ONLY host build of the short-time Fourier transform's plain-C++ parts, for tests/test_stft.py:
// csrc/stft_core.h's staging index map over fft_core.h's geometry at every row of the K1 size table (k1_sizes.h) -- the
// same functions the store kernels compile (k1_stft_body.inc) -- and csrc/series_pieces.h's piece rule of rpf_stft.
#include <hip/hip_runtime.h>

#include <utility>

#include "../../rtl-power-fftw_amd/csrc/k1_sizes.h"
#include "../../rtl-power-fftw_amd/csrc/series_pieces.h"
#include "../../rtl-power-fftw_amd/csrc/stft_core.h"

using namespace rpf;

namespace {

// what the kernels of row I do with a row, lane by lane
template <int I>
struct Row {
    static constexpr K1Size s = k1_size(I, kFmtCu8, false);
    using G = Geom<s.N, s.P>;
    static void geometry(int* out)
    {
        out[0] = G::N;
        out[1] = G::P;
        out[2] = G::T;
        out[3] = G::LDS_CPX;
        out[4] = stft_read_rounds<G>();
        out[5] = stft_store_conflicts(G::N);
        out[6] = stft_read_conflicts(G::N);
    }
    // store[(t P + a) 2 ..] = bin, staging index of register a of lane t
    static void stores(int* out)
    {
        for (int t = 0; t < G::T; ++t)
            for (int a = 0; a < G::P; ++a) {
                const int bin = bin_of<G>(t, a);
                out[2 * (t * G::P + a)] = bin;
                out[2 * (t * G::P + a) + 1] = stft_stage_index<G>(bin);
            }
    }
    // read[(t R + i) 2 ..] = first bin of the pair lane t takes in round i, and its staging index
    static void reads(int* out)
    {
        constexpr int R = stft_read_rounds<G>();
        for (int t = 0; t < G::T; ++t)
            for (int i = 0; i < R; ++i) {
                const int bin = stft_read_bin<G>(t, i);
                out[2 * (t * R + i)] = bin;
                out[2 * (t * R + i) + 1] = stft_stage_index<G>(bin);
            }
    }
};

template <int... I>
int dispatch(int row, int what, int* out, std::integer_sequence<int, I...>)
{
    int rc = -1;
    auto one = [&](auto tag) {
        constexpr int K = decltype(tag)::value;
        if (K != row) return;
        if (what == 0) Row<K>::geometry(out);
        else if (what == 1) Row<K>::stores(out);
        else Row<K>::reads(out);
        rc = 0;
    };
    (one(std::integral_constant<int, I>{}), ...);
    return rc;
}

}  // namespace

extern "C" {

int rpf_emul_stft_rows(void) { return kK1SizeCount; }

// what = 0: out[7] = N, P, T, slab size in complex values, read rounds, stated store and read conflict degrees;
// 1: out[2 N] = (bin, staging index) per (lane, register); 2: out[N] = (first bin, staging index) per (lane, round).
// Returns 0, or -1 past the table's end.
int rpf_emul_stft_map(int row, int what, int* out)
{
    if (!out || what < 0 || what > 2) return -1;
    return dispatch(row, what, out, std::make_integer_sequence<int, kK1SizeCount>{});
}

// rpf_stft's pieces: frame and pitch in bytes, N bins, F frames; out3 = frames per piece, a full piece's input bytes,
// the byte hop between frames.
void rpf_emul_stft_pieces(long long frame, long long pitch, int N, long long F, long long* out3)
{
    const FrameBytes fb{static_cast<size_t>(frame), static_cast<size_t>(pitch)};
    const SeriesPieces p = stft_pieces(fb, 8 * static_cast<size_t>(N), F);
    out3[0] = p.per_piece;
    out3[1] = static_cast<long long>(p.bytes);
    out3[2] = static_cast<long long>(p.hop);
}

}  // extern "C"
