// piece_reader.h -- a file (or stdin) handed out in the pieces of csrc/series_pieces.h, whole integrations of L frames
// in one buffer: fill(), the engine call on data() with per_piece() as its cap, consume(what it credited), until that
// says false or the engine credits nothing.  --series, --series-stats, --excise, --quantile, --cross and --stft read their
// input so.
#ifndef RPF_HOST_PIECE_READER_H
#define RPF_HOST_PIECE_READER_H

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "datastore.h"      // (RPFexception; csrc/series_pieces.h)

namespace rpf_host {

class PieceReader {
public:
  // path "-": stdin.  Frame f of the file is bytes [f pitch_bytes, f pitch_bytes + frame_bytes).
  // row_cap: at most so many integrations in a piece (--stft: the rows a piece leaves are bounded too, stft_pieces).
  PieceReader(const std::string& path, int64_t frame_bytes, int64_t pitch_bytes, int64_t L,
              int64_t budget = static_cast<int64_t>(rpf::kSeriesPieceBytes), int64_t row_cap = INT64_MAX)
    : frames_{static_cast<size_t>(frame_bytes), static_cast<size_t>(pitch_bytes)}, L_(L),
      pieces_(rpf::series_pieces(frames_, L, INT64_MAX, static_cast<size_t>(budget), row_cap)),
      file_(path == "-" ? stdin : std::fopen(path.c_str(), "rb")), bytes_(file_ ? pieces_.bytes : 0) {
    if (!file_) throw RPFexception("Could not open " + path + ".", ReturnValue::InvalidInput);
  }
  ~PieceReader() { if (file_ != stdin) std::fclose(file_); }
  PieceReader(const PieceReader&) = delete;
  PieceReader& operator=(const PieceReader&) = delete;

  int64_t per_piece() const { return pieces_.per_piece; }     // integrations a full buffer holds
  const uint8_t* data() const { return bytes_.data(); }
  // Reads until the buffer is full or the file has ended; returns the bytes it holds.
  size_t fill() {
    while (!ended_ && have_ < bytes_.size()) {
      const size_t got = std::fread(bytes_.data() + have_, 1, bytes_.size() - have_, file_);
      if (got == 0) ended_ = true;
      have_ += got;
    }
    return have_;
  }
  // The engine took `done` integrations: the next one moves to the front, with the bytes it shares with the last one
  // (overlapped frames) and whatever was read beyond.  False: the file has ended and less than one integration is left.
  bool consume(int64_t done) {
    const size_t used = std::min(have_, static_cast<size_t>(done) * pieces_.hop);    // (have_: a pitch above the frame)
    std::memmove(bytes_.data(), bytes_.data() + used, have_ - used);
    have_ -= used;
    return !(ended_ && have_ < frames_.span(L_));
  }

private:
  rpf::FrameBytes frames_;
  int64_t L_;
  rpf::SeriesPieces pieces_;
  std::FILE* file_;
  std::vector<uint8_t> bytes_;
  size_t have_ = 0;
  bool ended_ = false;
};

}  // namespace rpf_host
#endif  // RPF_HOST_PIECE_READER_H
