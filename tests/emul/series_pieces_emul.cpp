// TEST-ONLY export of csrc/series_pieces.h, the piece plan of a host call of the series family, for
// tests/test_series_pieces.py, which compiles this file itself (the header is plain C++: a second or two).
#include "../../rtl-power-fftw_amd/csrc/series_pieces.h"

// b bytes per sample, N bins, frame step S, taps (0 = no PFB), K integrations of L frames, an input budget in bytes and
// a cap on the rows of a piece (0 = none); out3 = per_piece, a full piece's bytes, the byte hop between integrations.
extern "C" void rpf_emul_series_pieces(int b, int N, int S, int taps, long long L, long long K, long long budget,
                                       long long row_cap, long long* out3)
{
    const rpf::FrameBytes fb{static_cast<size_t>(b) * N * (taps > 1 ? taps : 1), static_cast<size_t>(b) * S};
    const rpf::SeriesPieces p = rpf::series_pieces(fb, L, K, static_cast<size_t>(budget), row_cap > 0 ? row_cap : INT64_MAX);
    out3[0] = p.per_piece;
    out3[1] = static_cast<long long>(p.bytes);
    out3[2] = static_cast<long long>(p.hop);
}
