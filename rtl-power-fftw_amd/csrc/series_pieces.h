// series_pieces.h -- how a HOST stream of K integrations of L frames is cut into pieces by the series family's host
// entries (rpf_accumulate_series[_stats], rpf_accumulate_excised, rpf_quantile_append) and by the CLI's file reader,
// which does not know K: whole integrations, as many as span at most a budget of input bytes and, where the rows are
// bounded too, at most row_cap of them -- but at least one, however large it is.  Frame f of a stream is bytes
// [f pitch, f pitch + frame): frame = b N (b T N on a PFB engine), pitch = b S; with overlapped frames (pitch < frame) a
// piece's last bytes are the next piece's first.  Plain C++11, shared by the engine, the C++ host
// (host/datastore.h, host/piece_reader.h) and the CPU tests (tests/emul/series_pieces_emul.cpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace rpf {

constexpr size_t kSeriesPieceBytes = static_cast<size_t>(64) << 20;      // the input budget of a piece

struct FrameBytes {
    size_t frame, pitch;
    // whole frames in nbytes, and the bytes `frames` frames span
    int64_t frames_in(size_t nbytes) const { return nbytes < frame ? 0 : static_cast<int64_t>((nbytes - frame) / pitch + 1); }
    size_t span(int64_t frames) const { return frames < 1 ? 0 : frame + pitch * static_cast<size_t>(frames - 1); }
};

struct SeriesPieces {
    int64_t per_piece;   // integrations in every piece but the last
    size_t bytes;        // input of a full piece = span(per_piece L)
    size_t hop;          // from one integration's first byte to the next one's = L pitch: piece i starts at i per_piece hop
};

inline SeriesPieces series_pieces(const FrameBytes& fb, int64_t L, int64_t K = INT64_MAX, size_t budget = kSeriesPieceBytes,
                                  int64_t row_cap = INT64_MAX)
{
    const int64_t fit = fb.frames_in(budget) / L;
    const int64_t per_piece = std::min(std::min(K, std::max<int64_t>(1, row_cap)), std::max<int64_t>(1, fit));
    return {per_piece, fb.span(per_piece * L), static_cast<size_t>(L) * fb.pitch};
}

// rpf_stft's pieces (one frame per "integration"): a frame leaves a row of row_bytes = 8 N bytes, usually more than it
// brought, so a piece takes as many whole frames as keep BOTH its input span and its rows within the budget -- and at
// least one.  With a frame step of one sample the rows, not the input, are the bound.
inline SeriesPieces stft_pieces(const FrameBytes& fb, size_t row_bytes, int64_t F = INT64_MAX, size_t budget = kSeriesPieceBytes)
{
    return series_pieces(fb, 1, F, budget, static_cast<int64_t>(budget / row_bytes));
}

}  // namespace rpf
