// host_capi.cpp -- TEST SHIM: C entry points onto the CPU-only pieces of the C++
// host (option parsing, unit parsing, Plan, aux-file parsing, spectrum writer)
// so that tests/ can drive them through ctypes and compare with the oracle's
// restatements and the man page.  Not needed by the CLI itself.
#include <algorithm>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "acquisition.h"
#include "aux_data.h"
#include "options.h"
#include "piece_reader.h"
#include "sample_source.h"
#include "scan_plan.h"
#include "units.h"

using namespace rpf_host;

namespace {
std::string g_text;
int copy_out(const std::string& s, char* out, size_t cap)
{
    if (s.size() + 1 > cap) return -1;
    std::memcpy(out, s.c_str(), s.size() + 1);
    return static_cast<int>(s.size());
}

// What `call` returns, or -(the reference's exit code) of what it throws with the message in `msg`.
template <class Call>
long long or_exit_code(char* msg, size_t cap, Call call)
{
    try {
        return call();
    } catch (RPFexception& e) {
        copy_out(e.what(), msg, cap);
        return -static_cast<long long>(e.returnValue());
    }
}

// The shims that need a device run `call` on a Datastore of their own without a window: what it returns (as above) and
// the launches of its last series call.
template <class Call>
long long on_datastore(int N, int sample_format, int frame_step, bool bin_stats, int* launches, char* msg, size_t cap, Call call)
{
    return or_exit_code(msg, cap, [&]() -> long long {
        Params params;
        params.N = N;
        params.sample_format = sample_format;
        params.frame_step = frame_step;
        params.bin_stats = bin_stats;
        std::vector<float> no_window;
        Datastore data(params, no_window);
        const long long done = call(data);
        if (launches) *launches = data.series_launches();
        return done;
    });
}
}  // namespace

extern "C" {

long long rpf_host_parse_frequency(const char* s) { return parse_frequency(s); }
double rpf_host_parse_time(const char* s) { return parse_time(s); }

// Parses argv; on success fills the numeric fields and returns 0, else returns the
// reference's exit code and puts the message in `msg`.
int rpf_host_parse(int argc, const char* const* argv, int* N, int* buffers, int* buf_length,
                   long long* repeats, int* sample_rate, long long* cfreq, long long* startfreq,
                   long long* stopfreq, int* flags, double* integration_time, char* msg, size_t cap)
{
    try {
        Options o = parse_command_line(argc, argv);
        *N = o.N; *buffers = o.buffers; *buf_length = o.buf_length; *repeats = o.repeats;
        *sample_rate = o.sample_rate; *cfreq = o.cfreq; *startfreq = o.startfreq; *stopfreq = o.stopfreq;
        *integration_time = o.integration_time;
        *flags = (o.window ? 1 : 0) | (o.baseline ? 2 : 0) | (o.linear ? 4 : 0) | (o.endless ? 8 : 0) |
                 (o.strict_time ? 16 : 0) | (o.matrixMode ? 32 : 0) | (o.freq_hopping_isSet ? 64 : 0) |
                 (o.talkless ? 128 : 0) | (o.buf_length_isSet ? 256 : 0) | (o.integration_time_isSet ? 512 : 0) |
                 (o.session_duration_isSet ? 1024 : 0) | (o.show_help ? 2048 : 0) | (o.show_version ? 4096 : 0);
        return 0;
    } catch (RPFexception& e) {
        copy_out(e.what(), msg, cap);
        return static_cast<int>(e.returnValue());
    }
}

// Overlapped frames on top of a parsed command line and the Plan at `samplerate` (the -t conversion needs the rate):
// frame step S, repeats R (sample budgets of -t and the default converted to frames at step S) and the complex
// samples one acquisition reads (frame_span(R) / 2).  0 or the reference's exit code (message in `msg`).
int rpf_host_parse_frames(int argc, const char* const* argv, int samplerate, int* N, int* step, long long* repeats,
                          long long* samples_per_acq, char* msg, size_t cap)
{
    try {
        Options o = parse_command_line(argc, argv);
        Plan plan(o, samplerate);
        *N = o.N;
        *step = static_cast<int>(o.step());
        *repeats = o.repeats;
        *samples_per_acq = o.frame_span(o.repeats) / o.sample_bytes();
        return 0;
    } catch (RPFexception& e) {
        copy_out(e.what(), msg, cap);
        return static_cast<int>(e.returnValue());
    }
}

// Plan on top of a parsed command line: returns hop count (<= cap) or -code.
int rpf_host_plan(int argc, const char* const* argv, int samplerate, long long* repeats, int* buf_length,
                  long long* freqs, int cap)
{
    try {
        Options o = parse_command_line(argc, argv);
        Plan plan(o, samplerate);
        *repeats = o.repeats;
        *buf_length = o.buf_length;
        int n = 0;
        for (auto f : plan.freqs_to_tune) {
            if (n >= cap) return -1;
            freqs[n++] = f;
        }
        return n;
    } catch (RPFexception& e) {
        return -static_cast<int>(e.returnValue());
    }
}

// The default PFB prototype (datastore.h's pfb_coefficients) into out[taps x N]; 0, or the exit code of a bad argument.
int rpf_host_pfb_coefficients(int N, int taps, float* out)
{
    try {
        const std::vector<float> h = pfb_coefficients(N, taps);
        std::copy(h.begin(), h.end(), out);
        return 0;
    } catch (RPFexception& e) {
        return static_cast<int>(e.returnValue());
    }
}

// Params' byte formulas with a PFB of `taps` taps (0 = none) and b = 2, 4 or 8 bytes per sample (format cu8, cs16, cf32).
long long rpf_host_pfb_frames_in(int N, int taps, int sample_bytes, long long nbytes)
{
    Params p;
    p.N = N;
    p.pfb_taps = taps;
    p.sample_format = sample_bytes == 8 ? RPF_FORMAT_CF32 : sample_bytes == 4 ? RPF_FORMAT_CS16 : RPF_FORMAT_CU8;
    return p.frames_in(nbytes);
}

long long rpf_host_pfb_frame_span(int N, int taps, int sample_bytes, long long frames)
{
    Params p;
    p.N = N;
    p.pfb_taps = taps;
    p.sample_format = sample_bytes == 8 ? RPF_FORMAT_CF32 : sample_bytes == 4 ? RPF_FORMAT_CS16 : RPF_FORMAT_CU8;
    return p.frame_span(frames);
}

long long rpf_host_next_read_size(long long total, long long done, int buf_length)
{
    return next_read_size(total, done, buf_length);
}

// Aux parser on in-memory text: kind 0 = float column, 1 = double column.
int rpf_host_read_column(const char* text, int kind, double* out, int cap)
{
    std::istringstream in(text);
    int n = 0;
    if (kind == 0) {
        for (float v : read_value_column<float>(in)) { if (n >= cap) return -1; out[n++] = v; }
    } else {
        for (double v : read_value_column<double>(in)) { if (n >= cap) return -1; out[n++] = v; }
    }
    return n;
}

// AuxData with both inputs on "stdin" (text): baseline first, then window.
int rpf_host_aux_from_stdin(int N, int want_window, int want_baseline, const char* text, float* window,
                            double* baseline, char* msg, size_t cap)
{
    Options o;
    o.N = N;
    o.window = want_window != 0;
    o.baseline = want_baseline != 0;
    o.window_file = "-";
    o.baseline_file = "-";
    std::istringstream in(text);
    try {
        AuxData aux(o, in);
        for (size_t i = 0; i < aux.window_values.size(); ++i) window[i] = aux.window_values[i];
        for (size_t i = 0; i < aux.baseline_values.size(); ++i) baseline[i] = aux.baseline_values[i];
        return 0;
    } catch (RPFexception& e) {
        copy_out(e.what(), msg, cap);
        return static_cast<int>(e.returnValue());
    }
}

long rpf_host_format_text(double* pwr, int N, long long repeats_done, long long tuned_freq, int samplerate,
                          int linear, const double* baseline, char* out, size_t cap)
{
    std::vector<double> p(pwr, pwr + N), b;
    if (baseline) b.assign(baseline, baseline + N);
    std::ostringstream os;
    write_spectrum_text(os, p, N, repeats_done, tuned_freq, samplerate, linear != 0, baseline ? &b : nullptr);
    std::memcpy(pwr, p.data(), sizeof(double) * N);
    return copy_out(os.str(), out, cap);
}

// The --stats writer (write_spectrum_text_stats); pwr and peak come back with their DC bins interpolated.
long rpf_host_format_text_stats(double* pwr, const double* sum_sq, double* peak, int N, long long repeats_done,
                                long long tuned_freq, int samplerate, int linear, const double* baseline, char* out,
                                size_t cap)
{
    std::vector<double> p(pwr, pwr + N), s2(sum_sq, sum_sq + N), pk(peak, peak + N), b;
    if (baseline) b.assign(baseline, baseline + N);
    std::ostringstream os;
    write_spectrum_text_stats(os, p, s2, pk, N, repeats_done, tuned_freq, samplerate, linear != 0, baseline ? &b : nullptr);
    std::memcpy(pwr, p.data(), sizeof(double) * N);
    std::memcpy(peak, pk.data(), sizeof(double) * N);
    return copy_out(os.str(), out, cap);
}

// The text header with (stats != 0) or without the statistics columns named.
long rpf_host_format_header(const char* start_stamp, const char* end_stamp, int stats, char* out, size_t cap)
{
    std::ostringstream os;
    write_text_header(os, start_stamp, end_stamp, stats != 0);
    return copy_out(os.str(), out, cap);
}

// The text header of the --excise block (cross == 0) or of the --cross block.
long rpf_host_format_header_mode(const char* start_stamp, const char* end_stamp, int cross, char* out, size_t cap)
{
    std::ostringstream os;
    if (cross) write_text_header_cross(os, start_stamp, end_stamp);
    else write_text_header_excised(os, start_stamp, end_stamp);
    return copy_out(os.str(), out, cap);
}

// datastore.h's spectral_kurtosis, element by element.
void rpf_host_spectral_kurtosis(const double* s1, const double* s2, long long M, double* out, int n)
{
    for (int i = 0; i < n; ++i) out[i] = spectral_kurtosis(s1[i], s2[i], M);
}

// datastore.h's coherence and cross_phase over planes[4 x n] = Saa, Sbb, Re Sab, Im Sab, element by element.
void rpf_host_coherence(const double* planes, int n, double* out)
{
    for (int i = 0; i < n; ++i) out[i] = coherence(planes[i], planes[n + i], planes[2 * n + i], planes[3 * n + i]);
}

void rpf_host_cross_phase(const double* planes, int n, double* out)
{
    for (int i = 0; i < n; ++i) out[i] = cross_phase(planes[2 * n + i], planes[3 * n + i]);
}

// The --cross writer (write_spectrum_text_cross) over planes[4 x N].
long rpf_host_format_text_cross(const double* planes, int N, long long frames, long long tuned_freq, int samplerate,
                                int linear, const double* baseline, char* out, size_t cap)
{
    std::vector<double> p(planes, planes + 4 * static_cast<size_t>(N)), b;
    if (baseline) b.assign(baseline, baseline + N);
    std::ostringstream os;
    write_spectrum_text_cross(os, p, N, frames, tuned_freq, samplerate, linear != 0, baseline ? &b : nullptr);
    return copy_out(os.str(), out, cap);
}

// The --correlate header for M streams (write_text_header_correlate).
long rpf_host_format_header_correlate(const char* start_stamp, const char* end_stamp, int M, char* out, size_t cap)
{
    std::ostringstream os;
    write_text_header_correlate(os, start_stamp, end_stamp, M);
    return copy_out(os.str(), out, cap);
}

// datastore.h's coherence_pair, element by element over n bins of the two autos and of V_ij.
void rpf_host_coherence_pair(const double* vii, const double* vjj, const double* re, const double* im, int n, double* out)
{
    for (int i = 0; i < n; ++i) out[i] = coherence_pair(vii[i], vjj[i], re[i], im[i]);
}

// The --correlate writer (write_spectrum_text_correlate) over vis[M x M x 2 x N].
long rpf_host_format_text_correlate(const double* vis, int M, int N, long long frames, long long tuned_freq, int samplerate,
                                    int linear, const double* baseline, char* out, size_t cap)
{
    std::vector<double> v(vis, vis + 2 * static_cast<size_t>(M) * M * N), b;
    if (baseline) b.assign(baseline, baseline + N);
    std::ostringstream os;
    write_spectrum_text_correlate(os, v, M, N, frames, tuned_freq, samplerate, linear != 0, baseline ? &b : nullptr);
    return copy_out(os.str(), out, cap);
}

void rpf_host_format_matrix(double* pwr, int N, long long repeats_done, int samplerate, int linear,
                            const double* baseline, float* row_out)
{
    std::vector<double> p(pwr, pwr + N), b;
    if (baseline) b.assign(baseline, baseline + N);
    std::vector<float> row;
    spectrum_matrix_row(p, N, repeats_done, samplerate, linear != 0, baseline ? &b : nullptr, row);
    std::memcpy(row_out, row.data(), sizeof(float) * N);
    std::memcpy(pwr, p.data(), sizeof(double) * N);
}

// rpf_host::Datastore's two series calls (needs a device, unlike the rest of this shim): spectra of L frames of a
// host stream through accumulate_series into out[cap_rows x N]; device != 0: the stream is first copied to the GPU by
// the caller (d_stream, d_out device pointers) and accumulate_device_series runs on the null stream.  Returns K, or
// -(the reference's exit code) with the message in `msg`.
long long rpf_host_accumulate_series(int N, int sample_format, int frame_step, const unsigned char* stream, size_t nbytes,
                                     long long L, long long max_spectra, double* out, long long cap_rows, int device_resident,
                                     int* launches, char* msg, size_t cap)
{
    return on_datastore(N, sample_format, frame_step, false, launches, msg, cap, [&](Datastore& data) -> long long {
        if (device_resident) return data.accumulate_device_series(stream, nbytes, L, std::min(max_spectra, cap_rows), out);
        std::vector<double> rows;
        const long long done = data.accumulate_series(stream, nbytes, L, std::min(max_spectra, cap_rows), rows);
        std::memcpy(out, rows.data(), sizeof(double) * rows.size());
        return done;
    });
}

// rpf_host::Datastore's two STFT calls: the rows of a host stream through stft into out[cap_rows x N x 2 floats];
// device_resident != 0: stream and out are device pointers and stft_device runs on the null stream.  Returns F, or
// -(the reference's exit code) with the message in `msg`.
long long rpf_host_stft(int N, int sample_format, int frame_step, const unsigned char* stream, size_t nbytes,
                        long long max_frames, float* out, long long cap_rows, int device_resident, char* msg, size_t cap)
{
    return on_datastore(N, sample_format, frame_step, false, nullptr, msg, cap, [&](Datastore& data) -> long long {
        if (device_resident) return data.stft_device(stream, nbytes, std::min(max_frames, cap_rows), out);
        std::vector<float> rows;
        const long long done = data.stft(stream, nbytes, std::min(max_frames, cap_rows), rows);
        std::memcpy(out, rows.data(), sizeof(float) * rows.size());
        return done;
    });
}

// The same for the two series calls with statistics, on a Datastore with params.bin_stats: out[cap_rows x 3 x N].
long long rpf_host_accumulate_series_stats(int N, int sample_format, int frame_step, const unsigned char* stream,
                                           size_t nbytes, long long L, long long max_spectra, double* out, long long cap_rows,
                                           int device_resident, int* launches, char* msg, size_t cap)
{
    return on_datastore(N, sample_format, frame_step, true, launches, msg, cap, [&](Datastore& data) -> long long {
        if (device_resident) return data.accumulate_device_series_stats(stream, nbytes, L, std::min(max_spectra, cap_rows), out);
        std::vector<double> rows;
        const long long done = data.accumulate_series_stats(stream, nbytes, L, std::min(max_spectra, cap_rows), rows);
        std::memcpy(out, rows.data(), sizeof(double) * rows.size());
        return done;
    });
}

// datastore.h's sk_limits; 0, or -(exit code) with the message in `msg`.
int rpf_host_sk_limits(long long M, double sigma, double* lo, double* hi, char* msg, size_t cap)
{
    return static_cast<int>(or_exit_code(msg, cap, [&]() -> long long { sk_limits(M, sigma, *lo, *hi); return 0; }));
}

// rpf_host::Datastore's two excised calls on a Datastore with params.bin_stats (needs a device): out[3 x N], mask
// (cap_rows x N bytes, or NULL); device_resident != 0: stream, out and mask are device pointers and
// accumulate_device_excised runs on the null stream.  Returns K, or -(exit code) with the message in `msg`.
long long rpf_host_accumulate_excised(int N, int sample_format, int frame_step, const unsigned char* stream, size_t nbytes,
                                      long long L, long long max_spectra, double sk_lo, double sk_hi, double* out,
                                      unsigned char* mask, long long cap_rows, int device_resident, int* launches, char* msg,
                                      size_t cap)
{
    return on_datastore(N, sample_format, frame_step, true, launches, msg, cap, [&](Datastore& data) -> long long {
        if (device_resident)
            return data.accumulate_device_excised(stream, nbytes, L, std::min(max_spectra, cap_rows), sk_lo, sk_hi, out, mask);
        std::vector<double> res;
        std::vector<uint8_t> flags;
        const long long done = data.accumulate_excised(stream, nbytes, L, std::min(max_spectra, cap_rows), sk_lo, sk_hi, res,
                                                       mask ? &flags : nullptr);
        std::memcpy(out, res.data(), sizeof(double) * res.size());
        if (mask) std::memcpy(mask, flags.data(), flags.size());
        return done;
    });
}

// The excised block's writer (write_spectrum_text_excised).
long rpf_host_format_text_excised(const double* clean, const double* kept, const double* total, int N, long long K,
                                  long long L, long long tuned_freq, int samplerate, int linear, const double* baseline,
                                  char* out, size_t cap)
{
    std::vector<double> c(clean, clean + N), k(kept, kept + N), t(total, total + N), b;
    if (baseline) b.assign(baseline, baseline + N);
    std::ostringstream os;
    write_spectrum_text_excised(os, c, k, t, N, K, L, tuned_freq, samplerate, linear != 0, baseline ? &b : nullptr);
    return copy_out(os.str(), out, cap);
}

// rpf_host::Datastore's quantile calls (needs a device): the host stream cut into `pieces` parts of whole integrations,
// each appended (quantile_append), then ONE quantile_select of q[nq] into out[nq x N]; rows_out: quantile_rows() before
// the select.  Returns the rows appended, or -(exit code) with the message in `msg`.
long long rpf_host_accumulate_quantiles(int N, int sample_format, int frame_step, const unsigned char* stream, size_t nbytes,
                                        long long L, int pieces, const double* q, int nq, double* out, long long* rows_out,
                                        int* launches, char* msg, size_t cap)
{
    return on_datastore(N, sample_format, frame_step, false, launches, msg, cap, [&](Datastore& data) -> long long {
        const Params& params = data.params;
        data.quantile_reset();
        const long long total = L >= 1 ? params.frames_in(static_cast<int64_t>(nbytes)) / L : 0;
        const long long per_piece = std::max<long long>(1, (total + std::max(pieces, 1) - 1) / std::max(pieces, 1));
        const size_t hop = static_cast<size_t>(std::max<long long>(L, 0)) * params.sample_bytes() * params.step();
        long long done = 0;
        do {
            const long long got = data.quantile_append(stream + static_cast<size_t>(done) * hop,
                                                       nbytes - static_cast<size_t>(done) * hop, L, per_piece);
            if (got == 0) break;
            done += got;
        } while (done < total);
        if (rows_out) *rows_out = data.quantile_rows();
        if (launches) *launches = data.series_launches();      // (also if the select below is refused)
        std::vector<double> planes;
        data.quantile_select(std::vector<double>(q, q + std::max(nq, 0)), planes);
        std::memcpy(out, planes.data(), sizeof(double) * planes.size());
        return done;
    });
}

// Walks a file as the CLI's series modes do (piece_reader.h), crediting every piece min(per_piece, whole integrations
// held) as the series entries do.  Piece i: out4[4 i ..] = the file offset of its first byte, the bytes held, the
// integrations credited and where in `bytes` the first frame_span(credited L) bytes handed over were copied.  Returns
// the pieces (at most cap_pieces and cap_bytes), or -(exit code) with the message in `msg`.
long long rpf_host_piece_walk(const char* path, long long frame_bytes, long long pitch_bytes, long long L, long long budget,
                              long long* per_piece, long long* out4, int cap_pieces, unsigned char* bytes, size_t cap_bytes,
                              char* msg, size_t cap)
{
    return or_exit_code(msg, cap, [&]() -> long long {
        PieceReader in(path, frame_bytes, pitch_bytes, L, budget);
        const rpf::FrameBytes fb{static_cast<size_t>(frame_bytes), static_cast<size_t>(pitch_bytes)};
        *per_piece = in.per_piece();
        long long offset = 0;
        size_t copied = 0;
        int n = 0;
        for (bool more = true; more; ++n) {
            const size_t have = in.fill();
            const long long done = std::min<long long>(in.per_piece(), fb.frames_in(have) / L);
            if (done == 0) break;
            const size_t handed = fb.span(done * L);
            if (n >= cap_pieces || copied + handed > cap_bytes) return -1;
            std::memcpy(bytes + copied, in.data(), handed);
            const long long v[4] = {offset, static_cast<long long>(have), done, static_cast<long long>(copied)};
            std::copy(v, v + 4, out4 + 4 * n);
            copied += handed;
            offset += done * L * pitch_bytes;
            more = in.consume(done);
        }
        return n;
    });
}

// The --quantile header and block writers.
long rpf_host_format_text_quantiles(const double* planes, const double* q, int nq, int N, long long L, long long tuned_freq,
                                    int samplerate, int linear, const double* baseline, char* out, size_t cap)
{
    std::vector<double> p(planes, planes + static_cast<size_t>(nq) * N), qs(q, q + nq), b;
    if (baseline) b.assign(baseline, baseline + N);
    std::ostringstream os;
    write_text_header_quantiles(os, "a", "b", qs);
    write_spectrum_text_quantiles(os, p, qs, N, L, tuned_freq, samplerate, linear != 0, baseline ? &b : nullptr);
    return copy_out(os.str(), out, cap);
}

// The --quantile options of a parsed command line: frames, and the list into q[cap_q]; returns the number of quantiles
// (0 without --quantile), or -(exit code) with the message in `msg`.
int rpf_host_parse_quantiles(int argc, const char* const* argv, long long* frames, double* q, int cap_q, char* msg, size_t cap)
{
    return static_cast<int>(or_exit_code(msg, cap, [&]() -> long long {
        Options o = parse_command_line(argc, argv);
        *frames = o.quantile_frames;
        int n = 0;
        for (double v : o.quantiles)
            if (n < cap_q) q[n++] = v;
        return n;
    }));
}

// The --dedisperse options of a parsed command line: frames, and the trials of --dm into dms[cap_dms]; returns the number
// of trials (0 without --dedisperse), or -(exit code) with the message in `msg`.
int rpf_host_parse_dedisperse(int argc, const char* const* argv, long long* frames, double* dms, int cap_dms, char* msg, size_t cap)
{
    return static_cast<int>(or_exit_code(msg, cap, [&]() -> long long {
        Options o = parse_command_line(argc, argv);
        *frames = o.dedisperse_frames;
        int n = 0;
        for (double v : o.dms)
            if (n < cap_dms) dms[n++] = v;
        return n;
    }));
}

// datastore.h's dm_delays into out[n_dms x N]; 0, or -(exit code) with the message in `msg`.
int rpf_host_dm_delays(const double* dms, int n_dms, double fc, double rate, int N, long long L, long long step, int* out,
                       char* msg, size_t cap)
{
    return static_cast<int>(or_exit_code(msg, cap, [&]() -> long long {
        const std::vector<int32_t> d = dm_delays(std::vector<double>(dms, dms + n_dms), fc, rate, N, L, step);
        std::copy(d.begin(), d.end(), out);
        return 0;
    }));
}

// The --dedisperse header and block of one trial (write_text_header_dedisperse, write_text_dedisperse).
long rpf_host_format_text_dedisperse(const double* trial, long long T, long long nb, long long L, long long step, int samplerate,
                                     int linear, double dm, long long largest_delay, char* out, size_t cap)
{
    std::ostringstream os;
    write_text_header_dedisperse(os, "a", "b", dm, largest_delay);
    write_text_dedisperse(os, trial, T, nb, L, step, samplerate, linear != 0);
    return copy_out(os.str(), out, cap);
}

// The --fold options of a parsed command line: the trial periods into periods[cap_periods] and *phase_bins; returns the
// number of periods (0 without --fold), or -(exit code) with the message in `msg`.
int rpf_host_parse_fold(int argc, const char* const* argv, double* periods, int cap_periods, long long* phase_bins, char* msg,
                        size_t cap)
{
    return static_cast<int>(or_exit_code(msg, cap, [&]() -> long long {
        Options o = parse_command_line(argc, argv);
        *phase_bins = o.phase_bins;
        int n = 0;
        for (double v : o.fold_periods)
            if (n < cap_periods) periods[n++] = v;
        return n;
    }));
}

// datastore.h's period_steps (in_rows = 0: periods in seconds) or row_period_steps (in_rows != 0) into out[n]; 0, or
// -(exit code) with the message in `msg`.
int rpf_host_period_steps(const double* periods, int n, int in_rows, double rate, int N, long long L, long long step,
                          unsigned long long* out, char* msg, size_t cap)
{
    return static_cast<int>(or_exit_code(msg, cap, [&]() -> long long {
        const std::vector<double> v(periods, periods + n);
        const std::vector<uint64_t> s = in_rows ? row_period_steps(v) : period_steps(v, rate, N, L, step);
        std::copy(s.begin(), s.end(), out);
        return 0;
    }));
}

// datastore.h's fold_chi2 into out[D x P].
void rpf_host_fold_chi2(const double* prof, const int* hits, const double* mom, int D, int P, int NB, long long T, double* out)
{
    const size_t cells = static_cast<size_t>(P) * NB;
    const std::vector<double> c = fold_chi2(std::vector<double>(prof, prof + cells * D), std::vector<int32_t>(hits, hits + cells),
                                            std::vector<double>(mom, mom + 2 * static_cast<size_t>(D)), D, P, NB, T);
    std::copy(c.begin(), c.end(), out);
}

// The two --fold blocks (write_text_fold_plane, then write_text_fold_profile of cell (d, p)).
long rpf_host_format_text_fold(const double* dms, int D, const double* periods, int P, int NB, long long T, const double* chi2,
                               int d, int p, const double* prof, const int* hits, long long nb, int linear, char* out, size_t cap)
{
    std::ostringstream os;
    const std::vector<double> c(chi2, chi2 + static_cast<size_t>(D) * P);
    write_text_fold_plane(os, "a", "b", std::vector<double>(dms, dms + D), std::vector<double>(periods, periods + P), NB, T, c);
    write_text_fold_profile(os, "a", "b", dms[d], periods[p], c[static_cast<size_t>(d) * P + p], prof, hits, NB, nb, linear != 0);
    return copy_out(os.str(), out, cap);
}

void rpf_host_synthetic(unsigned long long seed, unsigned long long first, unsigned long long n, unsigned char* out)
{
    SyntheticSource::generate(seed, first, n, out);
}

}  // extern "C"
