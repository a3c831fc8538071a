// datastore.h -- C++11 host-side counterpart of the reference's `class Datastore`
// (/root/reference/src/datastore.h:35-68) over the C-ABI of include/rpf_engine.h.
//
// A maintainer of rtl_power_fftw swaps the reference's datastore.{h,cxx} for this
// header and links librpf_engine.so; Acquisition::run keeps its structure, the
// mutex/deque hand-off of acquisition.cxx:278-285,310-314,320-323,343-347
// becomes acquire()/unget()/submit()/finish() (INTEGRATION.md shows the diff).
// Errors surface as RPFexception with the reference's own ReturnValue codes.
#ifndef RPF_HOST_DATASTORE_H
#define RPF_HOST_DATASTORE_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rpf_engine.h"
#include "../csrc/series_pieces.h"

namespace rpf_host {

// exceptions.h:25-34
enum class ReturnValue {
  Success = 0, NoDeviceFound = 1, InvalidDeviceIndex = 2, InvalidArgument = 3,
  TCLAPerror = 4, InvalidInput = 5, AcquisitionError = 6, HardwareError = 7
};

// exceptions.h:39-47
class RPFexception : public std::runtime_error {
public:
  explicit RPFexception(const std::string& what, ReturnValue retval_)
    : runtime_error(what), retval(retval_) {}
  ReturnValue returnValue() const { return retval; }
private:
  ReturnValue retval;
};

// The Params fields the hot path reads (params.h:33-66), same names and defaults.
struct Params {
  int N = 512;
  int buffers = 5;
  int buf_length = 16384 * 100;
  bool window = false;
  int64_t repeats = buf_length / (2 * N);
  // Frame step S in complex samples (rpf_config::frame_step, --frame-overlap): frame f = samples [f S, f S + N).
  // 0 = N, frames side by side as in the reference.
  int frame_step = 0;
  int64_t step() const { return frame_step > 0 ? frame_step : N; }
  // What one complex sample of the stream is (RPF_FORMAT_*, --format): cu8, the reference's, unless told otherwise.
  int sample_format = RPF_FORMAT_CU8;
  int64_t sample_bytes() const { return sample_format == RPF_FORMAT_CF32 ? 8 : sample_format == RPF_FORMAT_CS16 ? 4 : 2; }
  // Polyphase filter bank front end (rpf_engine_create_pfb, --pfb): T taps, 0 = none; pfb_coeffs: T x N values, empty =
  // pfb_coefficients(N, T), the default prototype.  A frame then spans T N samples and the step is N.
  int pfb_taps = 0;
  std::vector<float> pfb_coeffs;
  int64_t span_samples() const { return static_cast<int64_t>(N) * std::max(pfb_taps, 1); }
  // frame f of a stream is bytes [f bS, f bS + b span), b bytes per sample, span = N (T N with PFB): the bytes `frames`
  // frames span (rpf_frame_span) and the frames a stream of nbytes holds (rpf_frames_in) by the engine's own formulas
  rpf::FrameBytes frame_bytes() const { return {static_cast<size_t>(sample_bytes() * span_samples()), static_cast<size_t>(sample_bytes() * step())}; }
  int64_t frame_span(int64_t frames) const { return static_cast<int64_t>(frame_bytes().span(frames)); }
  int64_t frames_in(int64_t nbytes) const { return nbytes < 0 ? 0 : frame_bytes().frames_in(static_cast<size_t>(nbytes)); }
  // a sample budget of r0 side-by-side frames as frames at step S: floor((r0 - 1) N / S) + 1 (r0 at S = N); with a PFB
  // of T taps r0 - (T - 1), at least one
  int64_t frames_for_budget(int64_t r0) const {
    if (r0 < 1) return r0;
    if (pfb_taps > 1) return std::max<int64_t>(r0 - (pfb_taps - 1), 1);
    return (r0 - 1) * N / step() + 1;
  }
  int sample_rate = 2000000;
  int64_t cfreq = 1420405752;
  bool linear = false;
  bool baseline = false;
  int device = 0;          // additive: HIP device ordinal
  // Per-bin statistics beside the power (RPF_FLAG_BIN_STATS, --stats): Datastore::sum_sq, Datastore::peak.
  bool bin_stats = false;
};

// The default PFB prototype h[0 .. T N): sinc((j - (TN-1)/2) / N) (0.54 - 0.46 cos(2 pi j / (TN-1))), computed in double,
// scaled so that the sum of h^2 is N and rounded to float32 once -- the formula of pfb.py's coefficients().
inline std::vector<float> pfb_coefficients(int N, int taps) {
  if (taps < 1 || taps > 32 || N < 2 || N % 2 != 0)
    throw RPFexception("pfb_coefficients: taps must be in 1 .. 32 and N a positive even number.", ReturnValue::InvalidArgument);
  const size_t M = static_cast<size_t>(taps) * static_cast<size_t>(N);
  const double pi = 3.14159265358979323846;
  std::vector<double> h(M);
  double sum_sq = 0;
  for (size_t j = 0; j < M; ++j) {
    const double x = (static_cast<double>(j) - static_cast<double>(M - 1) / 2.0) / N;
    const double y = pi * (x == 0 ? 1.0e-20 : x);
    h[j] = std::sin(y) / y * (0.54 - 0.46 * std::cos(2.0 * pi * static_cast<double>(j) / static_cast<double>(M - 1)));
    sum_sq += h[j] * h[j];
  }
  const double scale = std::sqrt(N / sum_sq);
  std::vector<float> out(M);
  for (size_t j = 0; j < M; ++j) out[j] = static_cast<float>(h[j] * scale);
  return out;
}

// The spectral kurtosis estimator (Nita & Gary) from S1 = sum of the frame powers and S2 = sum of their squares over
// M frames: SK = (M+1)/(M-1) (M S2 / S1^2 - 1), in double, in exactly this order of operations (stats.py's
// spectral_kurtosis does the same ones); NaN for M < 2 or S1 = 0.
inline double spectral_kurtosis(double s1, double s2, int64_t M) {
  if (M < 2 || s1 == 0.0) return std::nan("");
  const double m = static_cast<double>(M);
  return ((m + 1.0) / (m - 1.0)) * (m * s2 / (s1 * s1) - 1.0);
}

// Thresholds for the excised average (rpf_accumulate_excised): 1 -+ sigma sd with sd^2 = 4 M^2 / ((M-1)(M+2)(M+3)), the
// variance of SK for Gaussian noise and M independent frames; the lower limit not below 0.  The same operations as
// stats.py's sk_limits.  SK is skewed to the right, so 3 sigma flags a fraction of a per cent of clean data: a starting
// point, not a calibrated false-alarm rate.
inline void sk_limits(int64_t M, double sigma, double& lo, double& hi) {
  if (M < 2)
    throw RPFexception("sk_limits: M must be at least 2, got " + std::to_string(M) + ".", ReturnValue::InvalidArgument);
  const double m = static_cast<double>(M);
  const double sd = std::sqrt(4.0 * m * m / ((m - 1.0) * (m + 2.0) * (m + 3.0)));
  const double d = sigma * sd;
  lo = std::max(1.0 - d, 0.0);
  hi = 1.0 + d;
}

// The magnitude-squared coherence of two streams from one bin of the four planes of rpf_accumulate_cross (Saa, Sbb,
// Re Sab, Im Sab): (re^2 + im^2) / (Saa Sbb), in double, in exactly this order of operations (stats.py's coherence does
// the same ones); NaN where Saa Sbb = 0; not clamped.  And arg Sab in radians (stats.py's cross_phase).
inline double coherence(double saa, double sbb, double re, double im) {
  const double den = saa * sbb;
  if (den == 0.0) return std::nan("");
  return (re * re + im * im) / den;
}
inline double cross_phase(double re, double im) { return std::atan2(im, re); }
// The same for the pair (i, j) of the correlator (rpf_correlate): (re^2 + im^2) / (V_ii V_jj) from one bin of V_ij and
// of the two autos (stats.py's coherence_matrix does the same operations); NaN where V_ii V_jj = 0; not clamped.
inline double coherence_pair(double vii, double vjj, double re, double im) { return coherence(vii, vjj, re, im); }

// The delay table of the dispersion measures `dms` [pc cm^-3] for rpf_dedisperse (include/rpf_engine.h has the
// sequence; dedisperse.py's dm_delays does the same operations, so the integers agree): D x N int32, in integrations of
// L frames at step S, the highest bin the reference.  The one product that feeds a sum goes through a volatile, so no
// compiler can fuse the two.
inline std::vector<int32_t> dm_delays(const std::vector<double>& dms, double fc, double rate, int N, int64_t L, int64_t S) {
  if (N < 1 || L < 1 || S < 1 || !(rate > 0))
    throw RPFexception("dm_delays: N, L, the frame step and the rate must be positive.", ReturnValue::InvalidArgument);
  std::vector<double> inv(N);
  for (int b = 0; b < N; ++b) {
    volatile double off = static_cast<double>(b - N / 2) * (rate / static_cast<double>(N));
    const double f = (fc + off) / 1e6;
    if (b == 0 && !(f > 0))
      throw RPFexception("dm_delays: the lowest bin's frequency must be positive, got " + std::to_string(f) + " MHz.",
                         ReturnValue::InvalidArgument);
    inv[b] = 1.0 / (f * f);
  }
  const double ref = inv[N - 1], t_row = (static_cast<double>(L) * static_cast<double>(S)) / rate;
  std::vector<int32_t> out(dms.size() * static_cast<size_t>(N));
  for (size_t d = 0; d < dms.size(); ++d) {
    if (!(dms[d] >= 0) || std::isinf(dms[d]))
      throw RPFexception("dm_delays: a dispersion measure must be finite and not negative, got " + std::to_string(dms[d]) + ".",
                         ReturnValue::InvalidArgument);
    const double k = 4.148808e3 * dms[d];
    for (int b = 0; b < N; ++b) {
      const double v = std::floor((k * (inv[b] - ref)) / t_row + 0.5);
      if (!(v < 2147483648.0))
        throw RPFexception("dm_delays: the delay of DM " + std::to_string(dms[d]) + " at bin " + std::to_string(b) +
                           " does not fit 32 bits.", ReturnValue::InvalidArgument);
      out[d * N + b] = static_cast<int32_t>(v);
    }
  }
  return out;
}

// The steps of rpf_fold_device (include/rpf_engine.h has the sequence; fold.py's row_period_steps and period_steps do the
// same operations, so the integers agree): the phase advance per row, in units of 2^-64 turn, of periods given in rows ...
inline std::vector<uint64_t> row_period_steps(const std::vector<double>& periods_rows) {
  std::vector<uint64_t> out;
  for (double pr : periods_rows) {
    if (!std::isfinite(pr) || !(pr >= 2.0))
      throw RPFexception("period_steps: a period must be finite and at least two rows; got " + std::to_string(pr) + " rows.",
                         ReturnValue::InvalidArgument);
    out.push_back(static_cast<uint64_t>(std::ldexp(1.0 / pr, 64)));       // at most 2^63
  }
  return out;
}
// ... and of periods in seconds, for rows of L frames at step S of a stream at `rate` samples/s.
inline std::vector<uint64_t> period_steps(const std::vector<double>& periods_s, double rate, int N, int64_t L, int64_t S) {
  if (N < 1 || L < 1 || S < 1 || !(rate > 0))
    throw RPFexception("period_steps: N, L, the frame step and the rate must be positive.", ReturnValue::InvalidArgument);
  const double t_row = (static_cast<double>(L) * static_cast<double>(S)) / rate;
  std::vector<double> rows;
  for (double v : periods_s) rows.push_back(v / t_row);
  return row_period_steps(rows);
}

// The reduced chi-square of every folded profile against a flat one (include/rpf_engine.h; fold.py's chi2): prof D x P x NB,
// hits P x NB, mom D x 2, T the times folded; D x P values, NaN where fewer than two bins have hits or the variance is
// not positive.
inline std::vector<double> fold_chi2(const std::vector<double>& prof, const std::vector<int32_t>& hits, const std::vector<double>& mom,
                                     size_t D, size_t P, size_t NB, int64_t T) {
  std::vector<double> out(D * P, std::nan(""));
  if (T < 1) return out;
  for (size_t s = 0; s < D; ++s) {
    const double mu = mom[2 * s] / static_cast<double>(T), var = mom[2 * s + 1] / static_cast<double>(T) - mu * mu;
    for (size_t p = 0; p < P; ++p) {
      int used = 0;
      double sum = 0;
      for (size_t b = 0; b < NB; ++b) {
        const int32_t h = hits[p * NB + b];
        if (h <= 0) continue;
        const double dev = prof[(s * P + p) * NB + b] / h - mu;
        sum += h * dev * dev / var;
        ++used;
      }
      if (used >= 2 && var > 0) out[s * P + p] = sum / (used - 1);
    }
  }
  return out;
}

// A filled/empty hand-off buffer: what `Buffer&` is in acquisition.cxx:283,302-304
// (data()/size()/resize()), backed by engine-owned pinned memory.
class Buffer {
public:
  uint8_t* data() { return ptr_; }
  const uint8_t* data() const { return ptr_; }
  size_t size() const { return size_; }
  size_t capacity() const { return capacity_; }
  void resize(size_t n) {
    if (n > capacity_)
      throw RPFexception("Buffer::resize beyond buf_length", ReturnValue::InvalidArgument);
    size_ = n;
  }
private:
  friend class Datastore;
  uint8_t* ptr_ = nullptr;
  size_t size_ = 0, capacity_ = 0;
};

class Datastore {
public:
  const Params& params;
  int64_t repeats_done = 0;          // datastore.h:38
  std::vector<double> pwr;           // datastore.h:53 (valid after finish())
  std::vector<double> sum_sq, peak;  // params.bin_stats: S2 and PK of the acquisition (valid after finish()), else empty

  // datastore.cxx:23-34
  // device_override >= 0: HIP device for this instance (one Datastore per device in a
  // multi-device scan) instead of params.device
  Datastore(const Params& params_, std::vector<float>& window_values, int device_override = -1)
    : params(params_), pwr(params_.N) {
    if (params.window && (int)window_values.size() != params.N)
      throw RPFexception("Error reading window function. Expected " + std::to_string(params.N)
                         + " values, found " + std::to_string(window_values.size()) + ".",
                         ReturnValue::InvalidInput);
    rpf_config cfg;
    cfg.struct_size = sizeof(cfg);
    cfg.N = params.N;
    cfg.window = params.window ? window_values.data() : nullptr;
    cfg.n_buffers = params.buffers;
    cfg.buffer_capacity = params.buf_length;
    cfg.device = device_override >= 0 ? device_override : params.device;
    cfg.flags = RPF_FLAG_NONE | RPF_FLAG_SAMPLE_FORMAT(params.sample_format) | (params.bin_stats ? RPF_FLAG_BIN_STATS : 0u);
    if (params.bin_stats) {
      sum_sq.assign(params.N, 0.0);
      peak.assign(params.N, 0.0);
    }
    cfg.frame_step = params.frame_step;
    int rc;
    if (params.pfb_taps != 0) {
      if (!params.pfb_coeffs.empty() && params.pfb_coeffs.size() != static_cast<size_t>(std::max(params.pfb_taps, 0)) * params.N)
        throw RPFexception("Error reading PFB coefficients. Expected " + std::to_string(static_cast<int64_t>(params.pfb_taps) * params.N)
                           + " values, found " + std::to_string(params.pfb_coeffs.size()) + ".", ReturnValue::InvalidInput);
      const bool in_range = params.pfb_taps >= 1 && params.pfb_taps <= 32;
      const std::vector<float> h = !params.pfb_coeffs.empty() ? params.pfb_coeffs
                                   : in_range ? pfb_coefficients(params.N, params.pfb_taps) : std::vector<float>(1);
      rc = rpf_engine_create_pfb(&cfg, params.pfb_taps, h.data(), &engine_);
    } else {
      rc = rpf_engine_create(&cfg, &engine_);
    }
    if (rc != RPF_OK) throw RPFexception(rpf_last_global_error(), (ReturnValue)rc);
  }
  // datastore.cxx:36-46
  ~Datastore() { rpf_engine_destroy(engine_); }
  Datastore(const Datastore&) = delete;
  Datastore(Datastore&&) = delete;
  Datastore& operator=(const Datastore&) = delete;
  Datastore& operator=(Datastore&&) = delete;

  // acquisition.cxx:252-256: zero pwr, repeats_done = 0, start the worker
  void begin() { begin(params.repeats); }
  // the same for a shard of an acquisition (multi-device scans: this device's share of the frames)
  void begin(int64_t repeats) { check(rpf_begin(engine_, repeats)); repeats_done = 0; }
  // acquisition.cxx:278-285
  Buffer acquire() {
    Buffer b;
    check(rpf_buffer_acquire(engine_, &b.ptr_, &b.capacity_));
    b.size_ = b.capacity_;
    return b;
  }
  // acquisition.cxx:310-314
  void unget(Buffer& b) { check(rpf_buffer_unget(engine_, b.ptr_)); }
  // acquisition.cxx:320-323
  void submit(Buffer& b) { check(rpf_buffer_submit(engine_, b.ptr_, b.size_)); }
  // acquisition.cxx:343-347; pwr and repeats_done are final afterwards
  void finish() {
    check(rpf_finish(engine_, &repeats_done));
    check(rpf_get_power(engine_, pwr.data()));
    if (params.bin_stats) check(rpf_get_bin_stats(engine_, sum_sq.data(), peak.data()));
    // 65536 ... 262144 bins: a launch of the persistent four-step kernel that could not get the whole device (another
    // process on it) gives up; the engine has run those bytes through its two-kernel path and keeps to it -- the
    // acquisition is complete and right, the operator is told once why the rest of the run is a few per cent slower
    int64_t gave_up = 0;
    if (rpf_fused_status(engine_, nullptr, &gave_up, nullptr) == RPF_OK && gave_up > fused_gave_up_) {
      if (fused_gave_up_ == 0)
        std::cerr << "Note: the device was busy; the FFT worker left its single-launch kernel for the two-kernel path "
                     "(results are unaffected)." << std::endl;
      fused_gave_up_ = gave_up;
    }
  }
  // Spectrogram (rpf_accumulate_series): consecutive spectra of frames_per_spectrum frames of a host stream, row k of
  // `rows` (resized to K x N) = frames [k L, (k + 1) L).  Not through the buffer queues: pwr and repeats_done stay.
  // Returns K = min(max_spectra, frames / L).
  int64_t accumulate_series(const uint8_t* stream, size_t nbytes, int64_t frames_per_spectrum, int64_t max_spectra,
                            std::vector<double>& rows) {
    return series_rows(rpf_accumulate_series, 1, stream, nbytes, frames_per_spectrum, max_spectra, rows);
  }
  // The same on a stream resident in HBM (rpf_accumulate_device_series): d_out = K x N device doubles, asynchronous
  // on hip_stream.
  int64_t accumulate_device_series(const void* d_stream, size_t nbytes, int64_t frames_per_spectrum, int64_t max_spectra,
                                   double* d_out, void* hip_stream = nullptr) {
    int64_t done = 0;
    check(rpf_accumulate_device_series(engine_, d_stream, nbytes, frames_per_spectrum, max_spectra, d_out, hip_stream, &done));
    return done;
  }
  // Time-resolved statistics (rpf_accumulate_series_stats, params.bin_stats): as accumulate_series, row k of `rows`
  // (resized to K x 3 x N) = S1[N], S2[N], PK[N] of frames [k L, (k + 1) L); spectral_kurtosis with M = L per row.
  int64_t accumulate_series_stats(const uint8_t* stream, size_t nbytes, int64_t frames_per_spectrum, int64_t max_spectra,
                                  std::vector<double>& rows) {
    return series_rows(rpf_accumulate_series_stats, 3, stream, nbytes, frames_per_spectrum, max_spectra, rows);
  }
  // The same on a stream resident in HBM (rpf_accumulate_device_series_stats): d_out = K x 3 x N device doubles,
  // asynchronous on hip_stream.
  int64_t accumulate_device_series_stats(const void* d_stream, size_t nbytes, int64_t frames_per_spectrum,
                                         int64_t max_spectra, double* d_out, void* hip_stream = nullptr) {
    int64_t done = 0;
    check(rpf_accumulate_device_series_stats(engine_, d_stream, nbytes, frames_per_spectrum, max_spectra, d_out, hip_stream,
                                             &done));
    return done;
  }
  // The excised average (rpf_accumulate_excised, params.bin_stats; include/rpf_engine.h has the definition): `out`
  // (resized to 3 x N) = clean, kept, total over the K integrations of frames_per_spectrum frames, an integration kept
  // in a bin iff sk_lo <= SK <= sk_hi; mask: NULL, or resized to K x N bytes, 1 = flagged.  Returns K.
  int64_t accumulate_excised(const uint8_t* stream, size_t nbytes, int64_t frames_per_spectrum, int64_t max_spectra,
                             double sk_lo, double sk_hi, std::vector<double>& out, std::vector<uint8_t>* mask = nullptr) {
    out.assign(static_cast<size_t>(3) * params.N, 0.0);
    if (mask) mask->assign(row_capacity(nbytes, frames_per_spectrum, max_spectra) * params.N, 0);
    int64_t done = 0;
    check(rpf_accumulate_excised(engine_, stream, nbytes, frames_per_spectrum, max_spectra, sk_lo, sk_hi, out.data(),
                                 mask ? mask->data() : nullptr, &done));
    if (mask) mask->resize(static_cast<size_t>(done) * params.N);
    return done;
  }
  // The same on a stream resident in HBM (rpf_accumulate_device_excised): d_out = 3 x N device doubles, d_mask = K x N
  // device bytes or NULL, asynchronous on hip_stream.
  int64_t accumulate_device_excised(const void* d_stream, size_t nbytes, int64_t frames_per_spectrum, int64_t max_spectra,
                                    double sk_lo, double sk_hi, double* d_out, uint8_t* d_mask = nullptr,
                                    void* hip_stream = nullptr) {
    int64_t done = 0;
    check(rpf_accumulate_device_excised(engine_, d_stream, nbytes, frames_per_spectrum, max_spectra, sk_lo, sk_hi, d_out,
                                        d_mask, hip_stream, &done));
    return done;
  }
  // The frames' spectra themselves (rpf_stft; include/rpf_engine.h has the definition): row f of `rows` (resized to F x N
  // x 2 floats, interleaved re, im) = the float32 transform of frame f of a host stream, F = min(max_frames, frames).  Not
  // through the buffer queues: pwr and repeats_done stay.  Returns F.
  int64_t stft(const uint8_t* stream, size_t nbytes, int64_t max_frames, std::vector<float>& rows) {
    const int64_t fit = std::max<int64_t>(0, std::min(max_frames, static_cast<int64_t>(rpf_frames_in(engine_, nbytes))));
    rows.assign(static_cast<size_t>(fit) * params.N * 2, 0.0f);
    int64_t done = 0;
    float none[2];
    check(rpf_stft(engine_, stream, nbytes, max_frames, rows.empty() ? none : rows.data(), &done));
    return done;
  }
  // The same on a stream resident in HBM (rpf_stft_device): d_out = F x N x 2 device floats, 16-byte aligned,
  // asynchronous on hip_stream.
  int64_t stft_device(const void* d_stream, size_t nbytes, int64_t max_frames, void* d_out, void* hip_stream = nullptr) {
    int64_t done = 0;
    check(rpf_stft_device(engine_, d_stream, nbytes, max_frames, d_out, &done, hip_stream));
    return done;
  }
  // Cross-spectrum of two host streams of nbytes each (rpf_accumulate_cross; include/rpf_engine.h has the definition):
  // `planes` (resized to 4 x N) = Saa, Sbb, Re Sab, Im Sab over the first min(repeats, frames) frames; coherence and
  // cross_phase above take one bin of them.  Not through the buffer queues: pwr and repeats_done stay.  Returns the frames.
  int64_t accumulate_cross(const uint8_t* a, const uint8_t* b, size_t nbytes, int64_t repeats, std::vector<double>& planes) {
    planes.assign(static_cast<size_t>(4) * params.N, 0.0);
    int64_t done = 0;
    check(rpf_accumulate_cross(engine_, a, b, nbytes, repeats, planes.data(), &done));
    return done;
  }
  // The same on two streams resident in HBM (rpf_accumulate_device_cross): d_out = 4 x N device doubles, asynchronous
  // on hip_stream.
  int64_t accumulate_device_cross(const void* d_a, const void* d_b, size_t nbytes, int64_t repeats, double* d_out,
                                  void* hip_stream = nullptr) {
    int64_t done = 0;
    check(rpf_accumulate_device_cross(engine_, d_a, d_b, nbytes, repeats, d_out, hip_stream, &done));
    return done;
  }
  // Visibilities of M host streams of nbytes each (rpf_correlate; include/rpf_engine.h has the definition): `out`
  // (resized to M x M x 2 x N) = V_ij re and im over the first min(repeats, frames) frames; coherence_pair and
  // cross_phase above take one bin of them.  Not through the buffer queues: pwr and repeats_done stay.  Returns the frames.
  int64_t correlate(const std::vector<const uint8_t*>& streams, size_t nbytes, int64_t repeats, std::vector<double>& out) {
    const size_t M = streams.size();
    out.assign(2 * M * M * static_cast<size_t>(params.N), 0.0);
    int64_t done = 0;
    check(rpf_correlate(engine_, streams.data(), static_cast<int>(M), nbytes, repeats, out.data(), &done));
    return done;
  }
  // The same on streams resident in HBM (rpf_correlate_device): d_out = M x M x 2 x N device doubles, asynchronous on
  // hip_stream.
  int64_t correlate_device(const std::vector<const void*>& d_streams, size_t nbytes, int64_t repeats, double* d_out,
                           void* hip_stream = nullptr) {
    int64_t done = 0;
    check(rpf_correlate_device(engine_, d_streams.data(), static_cast<int>(d_streams.size()), nbytes, repeats, d_out,
                               hip_stream, &done));
    return done;
  }
  // Per-bin quantiles of the integrations (rpf_quantile_*; include/rpf_engine.h has the definition): the engine keeps the
  // rows of the series in HBM, appended call by call, and selects order statistics of every bin from them.
  void quantile_reset() { check(rpf_quantile_reset(engine_)); }
  int64_t quantile_rows() const { return rpf_quantile_rows(engine_); }
  int64_t quantile_max_rows() const { return rpf_quantile_max_rows(engine_); }
  // the rows accumulate_series would return for this call, appended to the store; returns how many
  int64_t quantile_append(const uint8_t* stream, size_t nbytes, int64_t frames_per_spectrum, int64_t max_spectra) {
    int64_t done = 0;
    check(rpf_quantile_append(engine_, stream, nbytes, frames_per_spectrum, max_spectra, &done));
    return done;
  }
  // the same on a stream resident in HBM (rpf_quantile_append_device), asynchronous on hip_stream
  int64_t quantile_append_device(const void* d_stream, size_t nbytes, int64_t frames_per_spectrum, int64_t max_spectra,
                                 void* hip_stream = nullptr) {
    int64_t done = 0;
    check(rpf_quantile_append_device(engine_, d_stream, nbytes, frames_per_spectrum, max_spectra, hip_stream, &done));
    return done;
  }
  // the quantiles q (each in [0, 1], at most 8) of the stored rows: `out` (resized to q.size() x N), plane i = q[i]
  void quantile_select(const std::vector<double>& q, std::vector<double>& out) {
    out.assign(std::max<size_t>(q.size(), 1) * params.N, 0.0);
    check(rpf_quantile_select(engine_, q.data(), static_cast<int>(q.size()), out.data()));
    out.resize(q.size() * params.N);
  }
  // the same into d_out = q.size() x N device doubles (rpf_quantile_select_device), asynchronous on hip_stream
  void quantile_select_device(const std::vector<double>& q, double* d_out, void* hip_stream = nullptr) {
    check(rpf_quantile_select_device(engine_, q.data(), static_cast<int>(q.size()), d_out, hip_stream));
  }
  // Incoherent dedispersion of the stored rows (rpf_dedisperse; include/rpf_engine.h has the definition): delays = D x N
  // (dm_delays above makes a DM table), weights = N values or empty for all ones; `out` (resized to D x T) = the
  // DM-time plane.  The store is only read.  Returns T.
  int64_t dedisperse(const std::vector<int32_t>& delays, const std::vector<double>& weights, std::vector<double>& out) {
    const int D = static_cast<int>(delays.size() / static_cast<size_t>(params.N));
    const int64_t T = std::max<int64_t>(rpf_dedisperse_times(engine_, delays.data(), D), 0);
    out.assign(std::max<size_t>(static_cast<size_t>(D) * static_cast<size_t>(T), 1), 0.0);
    int64_t times = 0;
    check(rpf_dedisperse(engine_, delays.data(), weights.empty() ? nullptr : weights.data(), D, out.data(),
                         static_cast<int64_t>(D) * T, &times));
    out.resize(static_cast<size_t>(D) * static_cast<size_t>(times));
    return times;
  }
  // rpf_dedisperse_fold: the same plane, folded on the device at `steps` (period_steps above) into NB phase bins; prof
  // (D x P x NB), hits (P x NB) and mom (D x 2) are resized.  Returns T.
  int64_t dedisperse_fold(const std::vector<int32_t>& delays, const std::vector<double>& weights, const std::vector<uint64_t>& steps,
                          int NB, std::vector<double>& prof, std::vector<int32_t>& hits, std::vector<double>& mom) {
    const int D = static_cast<int>(delays.size() / static_cast<size_t>(params.N)), P = static_cast<int>(steps.size());
    const size_t cells = static_cast<size_t>(P) * static_cast<size_t>(std::max(NB, 0));
    prof.assign(std::max<size_t>(cells * D, 1), 0.0);
    hits.assign(std::max<size_t>(cells, 1), 0);
    mom.assign(2 * static_cast<size_t>(std::max(D, 1)), 0.0);
    int64_t times = 0;
    check(rpf_dedisperse_fold(engine_, delays.data(), weights.empty() ? nullptr : weights.data(), D, steps.data(), P, NB,
                              prof.data(), static_cast<int64_t>(cells * D), hits.data(), mom.data(), &times));
    prof.resize(cells * D);
    hits.resize(cells);
    return times;
  }
  // the same into d_out = `capacity` device doubles (rpf_dedisperse_device), asynchronous on hip_stream
  int64_t dedisperse_device(const std::vector<int32_t>& delays, const std::vector<double>& weights, double* d_out,
                            int64_t capacity, void* hip_stream = nullptr) {
    int64_t times = 0;
    check(rpf_dedisperse_device(engine_, delays.data(), weights.empty() ? nullptr : weights.data(),
                                static_cast<int>(delays.size() / static_cast<size_t>(params.N)), d_out, capacity, hip_stream, &times));
    return times;
  }
  // transform launches of the last series call: 1 = the one-launch path
  int series_launches() const { return rpf_series_launches(engine_); }
  // the engine behind this Datastore (multi-device scans hand it to the scan reducer)
  const rpf_engine* engine() const { return engine_; }
  // datastore.cxx:98-103
  void printQueueHistogram() const {
    std::vector<int> h(params.buffers + 1);
    rpf_get_histogram(engine_, h.data());
    std::cerr << "Buffer queue histogram: ";
    for (auto size : h) std::cerr << size << " ";
    std::cerr << std::endl;
  }

private:
  void check(int rc) const {
    if (rc != RPF_OK) throw RPFexception(rpf_last_error(engine_), (ReturnValue)rc);
  }
  // Rows a host call of the series family can return, at least one (what the engine refuses, it refuses on a buffer).
  size_t row_capacity(size_t nbytes, int64_t frames_per_spectrum, int64_t max_spectra) const {
    const int64_t fit = frames_per_spectrum >= 1 ? rpf_frames_in(engine_, nbytes) / frames_per_spectrum : 0;
    return static_cast<size_t>(std::max<int64_t>(1, std::min(fit, std::max<int64_t>(max_spectra, 0))));
  }
  // accumulate_series and accumulate_series_stats: `entry` into rows of `planes` x N doubles
  typedef int (*SeriesEntry)(rpf_engine*, const uint8_t*, size_t, int64_t, int64_t, double*, int64_t*);
  int64_t series_rows(SeriesEntry entry, int planes, const uint8_t* stream, size_t nbytes, int64_t frames_per_spectrum,
                      int64_t max_spectra, std::vector<double>& rows) {
    const size_t row = static_cast<size_t>(planes) * params.N;
    rows.assign(row_capacity(nbytes, frames_per_spectrum, max_spectra) * row, 0.0);
    int64_t done = 0;
    check(entry(engine_, stream, nbytes, frames_per_spectrum, max_spectra, rows.data(), &done));
    rows.resize(static_cast<size_t>(done) * row);
    return done;
  }
  rpf_engine* engine_ = nullptr;
  int64_t fused_gave_up_ = 0;
};

}  // namespace rpf_host
#endif  // RPF_HOST_DATASTORE_H
