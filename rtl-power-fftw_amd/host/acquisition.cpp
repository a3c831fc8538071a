#include "acquisition.h"

#include <chrono>
#include <cmath>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <sstream>

#include "interrupts.h"
#include "scan_plan.h"

namespace rpf_host {

Acquisition::Acquisition(const Options& options, AuxData& aux, SampleSource& source, Datastore& data,
                         ScanMetadata& meta, int actual_samplerate, int64_t freq)
    : options_(options), aux_(aux), source_(source), data_(data), meta_(meta),
      actual_samplerate_(actual_samplerate), freq_(freq)
{
    shard_.repeats = options.repeats;
}

Acquisition::Acquisition(const Options& options, AuxData& aux, SampleSource& source, Datastore& data,
                         ScanMetadata& meta, int actual_samplerate, int64_t freq, const Shard& shard)
    : options_(options), aux_(aux), source_(source), data_(data), meta_(meta),
      actual_samplerate_(actual_samplerate), freq_(freq), shard_(shard), sharded_(true)
{
}

std::string Acquisition::utc_now()
{
    const time_t now = std::time(nullptr);
    char text[80];
    // gmtime_r: several acquisitions run side by side under --gpus a,b,... and std::gmtime hands every caller the same
    // static struct tm (ThreadSanitizer found the race, profiles/r04_tsan.txt)
    struct tm parts;
    gmtime_r(&now, &parts);
    std::strftime(text, sizeof(text), "%Y-%m-%d %X UTC", &parts);
    return text;
}

void Acquisition::run()
{
    // Tune, up to three tries (acquisition.cxx:229-249)
    bool tuned = false;
    for (int attempt = 1; attempt <= 3 && !tuned; ++attempt) {
        if (chatty()) std::cerr << "Tuning to " << freq_ << " Hz (try " << attempt << ")" << std::endl;
        try {
            source_.set_frequency(freq_);
            tuned_freq_ = source_.frequency();
            tuned = tuned_freq_ != 0;
        } catch (const RPFexception&) {
        }
    }
    if (!tuned) throw TuneError(freq_);
    if (chatty()) std::cerr << "Device tuned to: " << tuned_freq_ << " Hz" << std::endl;
    if (sharded_ && !source_.position(shard_.hop_base, static_cast<uint64_t>(options_.sample_bytes()) * static_cast<uint64_t>(options_.step()) *
                                                          static_cast<uint64_t>(shard_.first_frame)))
        throw RPFexception("This sample source cannot be split across devices.", ReturnValue::InvalidArgument);

    data_.begin(shard_.repeats);                                // :252-256

    start_stamp_ = utc_now();
    if (!sharded_) {
        std::time(&meta_.scanBeg);
        if (meta_.cntTimeStamps == 0) {
            meta_.firstAcqTimestamp = utc_now();
            meta_.cntTimeStamps++;
        }
    }
    if (chatty()) std::cerr << "Acquisition started at " << start_stamp_ << std::endl;

    using clock = std::chrono::steady_clock;
    const clock::time_point deadline =
        clock::now() + std::chrono::milliseconds(static_cast<int64_t>(options_.integration_time * 1000));

    const int64_t data_total = options_.frame_span(shard_.repeats);     // :273 (2N x repeats at frame step N)
    int64_t data_read = 0;
    while (data_read < data_total) {
        Buffer buffer = data_.acquire();                        // :278-285
        const int64_t wanted = next_read_size(data_total, data_read, options_.buf_length);
        buffer.resize(static_cast<size_t>(wanted));             // :302
        const bool ok = source_.read(buffer);                   // :304
        device_readouts_++;
        if (!ok) {
            std::cerr << "Error: dropped samples." << std::endl;
            data_.unget(buffer);                                // :310-314
            if (!source_.retry_after_short_read()) break;       // a finite replay has nothing more to give
        } else {
            successful_readouts_++;
            data_read += static_cast<int64_t>(buffer.size());   // == wanted, except for the last read of a replay
            data_.submit(buffer);                               // :320-323
            if (source_.exhausted()) break;                     // the replay ended inside this buffer
        }
        if (options_.strict_time && clock::now() >= deadline) break;                      // :326-327
        if (interrupts && checkInterrupt(InterruptState::FinishNow)) break;               // :330-331
    }

    end_stamp_ = utc_now();
    if (!sharded_) {
        std::time(&meta_.scanEnd);
        meta_.lastAcqTimestamp = utc_now();
        meta_.sumScanDur += static_cast<float>(std::difftime(meta_.scanEnd, meta_.scanBeg));
        meta_.avgScanDur = meta_.sumScanDur / meta_.metaRows;
    }
    if (chatty()) std::cerr << "Acquisition done at " << end_stamp_ << std::endl;

    data_.finish();                                             // :343-347
}

void print_acquisition_summary(int N, int64_t repeats_done, int64_t device_readouts, int64_t successful_readouts,
                               int actual_samplerate)
{
    std::cerr << "Actual number of (complex) samples collected: " << static_cast<int64_t>(N) * repeats_done
              << std::endl;
    std::cerr << "Actual number of device readouts: " << device_readouts << std::endl;
    std::cerr << "Number of successful readouts: " << successful_readouts << std::endl;
    std::cerr << "Actual number of averaged spectra: " << repeats_done << std::endl;
    std::cerr << "Effective integration time: " << static_cast<double>(N) * repeats_done / actual_samplerate
              << " seconds" << std::endl;
}

void Acquisition::print_summary() const
{
    print_acquisition_summary(options_.N, data_.repeats_done, device_readouts_, successful_readouts_,
                              actual_samplerate_);
}

namespace {

// The '#' lines that precede a text block; `titles` names the columns after the frequency.
void write_titled_header(std::ostream& out, const std::string& start_stamp, const std::string& end_stamp,
                         const std::string& titles)
{
    out << "# rtl-power-fftw output" << std::endl;
    out << "# Acquisition start: " << start_stamp << std::endl;
    out << "# Acquisition end: " << end_stamp << std::endl;
    out << "#" << std::endl;
    out << "# frequency [Hz]" << titles << std::endl;
}

// value of bin i after normalisation (acquisition.cxx:392-399): successive
// divisions in this order, then optional dB and baseline
inline double bin_value(const std::vector<double>& pwr, int i, int N, int64_t repeats_done, int samplerate,
                        bool linear, const std::vector<double>* baseline)
{
    const double p = pwr[i] / repeats_done / N / samplerate;
    const double b = baseline ? (*baseline)[i] : 0;
    return (linear ? p : 10 * std::log10(p)) - b;
}

inline void interpolate_dc(std::vector<double>& pwr, int N)
{
    pwr[N / 2] = (pwr[N / 2 - 1] + pwr[N / 2 + 1]) / 2;         // :377
}

// One line per bin: its frequency, then what columns(i) writes (" " and a value, per column), in six digits; the blank
// line that ends a block (:428-432).
template <class Columns>
void write_rows(std::ostream& out, int N, int64_t tuned_freq, int samplerate, Columns columns)
{
    // digits needed to tell neighbouring bins apart, plus two (:380-383; samplerate/N is an int division)
    const int freq_digits = static_cast<int>(
        std::ceil(std::floor(std::log10(static_cast<double>(tuned_freq))) - std::log10(samplerate / N) + 1 + 2));
    for (int i = 0; i < N; ++i) {
        const double freq = tuned_freq + (i - N / 2.0) * samplerate / N;
        out << std::setprecision(freq_digits) << freq << std::setprecision(6);
        columns(i);
        out << std::endl;
    }
    out << std::endl;
    out.flush();
}

// Plane c of planes[.. x N] on its own, its DC bin the mean of its neighbours.
std::vector<std::vector<double>> split_planes(const std::vector<double>& planes, size_t count, int N)
{
    std::vector<std::vector<double>> plane(count);
    for (size_t c = 0; c < count; ++c) {
        plane[c].assign(planes.begin() + c * N, planes.begin() + (c + 1) * N);
        interpolate_dc(plane[c], N);
    }
    return plane;
}

}  // namespace

void write_text_header(std::ostream& out, const std::string& start_stamp, const std::string& end_stamp)
{
    write_text_header(out, start_stamp, end_stamp, false);
}

void write_text_header(std::ostream& out, const std::string& start_stamp, const std::string& end_stamp, bool stats)
{
    write_titled_header(out, start_stamp, end_stamp, std::string(" power spectral density [dB/Hz]") +
                                                         (stats ? " peak hold [dB/Hz] spectral kurtosis" : ""));
}

void write_text_header_excised(std::ostream& out, const std::string& start_stamp, const std::string& end_stamp)
{
    write_titled_header(out, start_stamp, end_stamp, " power spectral density [dB/Hz] kept fraction");
}

void write_text_header_quantiles(std::ostream& out, const std::string& start_stamp, const std::string& end_stamp,
                                 const std::vector<double>& q)
{
    std::ostringstream titles;
    for (double v : q) titles << " quantile " << std::setprecision(6) << v << " [dB/Hz]";
    write_titled_header(out, start_stamp, end_stamp, titles.str());
}

void write_text_header_cross(std::ostream& out, const std::string& start_stamp, const std::string& end_stamp)
{
    write_titled_header(out, start_stamp, end_stamp,
                        " power spectral density a [dB/Hz] power spectral density b [dB/Hz] coherence phase [rad]");
}

void write_text_header_correlate(std::ostream& out, const std::string& start_stamp, const std::string& end_stamp, int M)
{
    std::ostringstream titles;
    for (int m = 0; m < M; ++m) titles << " power spectral density " << m << " [dB/Hz]";
    for (int i = 0; i < M; ++i)
        for (int j = i + 1; j < M; ++j) titles << " coherence " << i << "-" << j << " phase " << i << "-" << j << " [rad]";
    write_titled_header(out, start_stamp, end_stamp, titles.str());
}

void write_spectrum_text(std::ostream& out, std::vector<double>& pwr, int N, int64_t repeats_done,
                         int64_t tuned_freq, int samplerate, bool linear, const std::vector<double>* baseline)
{
    interpolate_dc(pwr, N);
    write_rows(out, N, tuned_freq, samplerate,
               [&](int i) { out << " " << bin_value(pwr, i, N, repeats_done, samplerate, linear, baseline); });
}

void write_spectrum_text_stats(std::ostream& out, std::vector<double>& pwr, const std::vector<double>& sum_sq,
                               std::vector<double>& peak, int N, int64_t repeats_done, int64_t tuned_freq,
                               int samplerate, bool linear, const std::vector<double>* baseline)
{
    // the kurtosis of every bin from the sums as accumulated; its DC bin, like the other two columns', is the mean
    // of its neighbours
    std::vector<double> sk(N);
    for (int i = 0; i < N; ++i) sk[i] = spectral_kurtosis(pwr[i], sum_sq[i], repeats_done);
    interpolate_dc(sk, N);
    interpolate_dc(pwr, N);
    interpolate_dc(peak, N);
    write_rows(out, N, tuned_freq, samplerate, [&](int i) {
        out << " " << bin_value(pwr, i, N, repeats_done, samplerate, linear, baseline) << " "
            << bin_value(peak, i, N, 1, samplerate, linear, baseline) << " " << sk[i];
    });
}

void write_spectrum_text_excised(std::ostream& out, const std::vector<double>& clean, const std::vector<double>& kept,
                                 const std::vector<double>& total, int N, int64_t K, int64_t L, int64_t tuned_freq,
                                 int samplerate, bool linear, const std::vector<double>* baseline)
{
    // every bin's mean over ITS kept integrations (bins differ in how many that is), so the usual division by the
    // number of frames happens here, bin by bin, and bin_value divides by 1
    std::vector<double> mean(N);
    const double l = static_cast<double>(L);
    for (int i = 0; i < N; ++i)
        mean[i] = kept[i] > 0 ? clean[i] / (kept[i] * l) : total[i] / (static_cast<double>(K) * l);
    interpolate_dc(mean, N);
    write_rows(out, N, tuned_freq, samplerate, [&](int i) {
        out << " " << bin_value(mean, i, N, 1, samplerate, linear, baseline) << " " << kept[i] / static_cast<double>(K);
    });
}

void write_spectrum_text_quantiles(std::ostream& out, const std::vector<double>& planes, const std::vector<double>& q, int N,
                                   int64_t L, int64_t tuned_freq, int samplerate, bool linear,
                                   const std::vector<double>* baseline)
{
    const std::vector<std::vector<double>> columns = split_planes(planes, q.size(), N);
    write_rows(out, N, tuned_freq, samplerate, [&](int i) {
        for (const std::vector<double>& column : columns) out << " " << bin_value(column, i, N, L, samplerate, linear, baseline);
    });
}

void write_spectrum_text_cross(std::ostream& out, const std::vector<double>& planes, int N, int64_t frames, int64_t tuned_freq,
                               int samplerate, bool linear, const std::vector<double>* baseline)
{
    // the DC bin of each of the four planes is the mean of its neighbours; coherence and phase come from those
    const std::vector<std::vector<double>> plane = split_planes(planes, 4, N);
    write_rows(out, N, tuned_freq, samplerate, [&](int i) {
        out << " " << bin_value(plane[0], i, N, frames, samplerate, linear, baseline) << " "
            << bin_value(plane[1], i, N, frames, samplerate, linear, baseline) << " "
            << coherence(plane[0][i], plane[1][i], plane[2][i], plane[3][i]) << " " << cross_phase(plane[2][i], plane[3][i]);
    });
}

void write_spectrum_text_correlate(std::ostream& out, const std::vector<double>& vis, int M, int N, int64_t frames,
                                   int64_t tuned_freq, int samplerate, bool linear, const std::vector<double>* baseline)
{
    // the DC bin of every plane is the mean of its neighbours; coherence and phase come from those
    const std::vector<std::vector<double>> plane = split_planes(vis, static_cast<size_t>(2 * M * M), N);
    auto re = [&](int i, int j) -> const std::vector<double>& { return plane[2 * (i * M + j)]; };
    auto im = [&](int i, int j) -> const std::vector<double>& { return plane[2 * (i * M + j) + 1]; };
    write_rows(out, N, tuned_freq, samplerate, [&](int k) {
        for (int m = 0; m < M; ++m) out << " " << bin_value(re(m, m), k, N, frames, samplerate, linear, baseline);
        for (int i = 0; i < M; ++i)
            for (int j = i + 1; j < M; ++j)
                out << " " << coherence_pair(re(i, i)[k], re(j, j)[k], re(i, j)[k], im(i, j)[k]) << " "
                    << cross_phase(re(i, j)[k], im(i, j)[k]);
    });
}

void write_text_header_dedisperse(std::ostream& out, const std::string& start_stamp, const std::string& end_stamp, double dm,
                                  int64_t largest_delay)
{
    out << "# rtl-power-fftw output" << std::endl;
    out << "# Acquisition start: " << start_stamp << std::endl;
    out << "# Acquisition end: " << end_stamp << std::endl;
    out << "# DM " << std::setprecision(6) << dm << " pc cm^-3, largest delay " << largest_delay << " integrations" << std::endl;
    out << "#" << std::endl;
    out << "# time [s] power [median units]" << std::endl;
}

void write_text_dedisperse(std::ostream& out, const double* trial, int64_t T, int64_t nb, int64_t L, int64_t step, int samplerate,
                           bool linear)
{
    for (int64_t t = 0; t < T; ++t) {
        const double time = static_cast<double>(t * L * step) / samplerate, p = trial[t] / static_cast<double>(nb);
        out << std::setprecision(9) << time << std::setprecision(6) << " " << (linear ? p : 10 * std::log10(p)) << std::endl;
    }
    out << std::endl;
    out.flush();
}

void write_text_fold_plane(std::ostream& out, const std::string& start_stamp, const std::string& end_stamp,
                           const std::vector<double>& dms, const std::vector<double>& periods, int NB, int64_t T,
                           const std::vector<double>& chi2)
{
    out << "# rtl-power-fftw output" << std::endl;
    out << "# Acquisition start: " << start_stamp << std::endl;
    out << "# Acquisition end: " << end_stamp << std::endl;
    out << "# fold: " << dms.size() << " DMs x " << periods.size() << " periods, " << NB << " phase bins, " << T << " times" << std::endl;
    out << "#" << std::endl;
    out << "# DM [pc cm^-3] period [s] reduced chi2" << std::endl;
    for (size_t d = 0; d < dms.size(); ++d) {
        for (size_t p = 0; p < periods.size(); ++p)
            out << std::setprecision(6) << dms[d] << " " << std::setprecision(9) << periods[p] << " " << std::setprecision(6)
                << chi2[d * periods.size() + p] << std::endl;
        out << std::endl;
    }
    out << std::endl;
    out.flush();
}

void write_text_fold_profile(std::ostream& out, const std::string& start_stamp, const std::string& end_stamp, double dm,
                             double period, double chi2, const double* prof, const int32_t* hits, int NB, int64_t nb, bool linear)
{
    out << "# rtl-power-fftw output" << std::endl;
    out << "# Acquisition start: " << start_stamp << std::endl;
    out << "# Acquisition end: " << end_stamp << std::endl;
    out << "# DM " << std::setprecision(6) << dm << " pc cm^-3, period " << std::setprecision(9) << period << " s, reduced chi2 "
        << std::setprecision(6) << chi2 << std::endl;
    out << "#" << std::endl;
    out << "# phase [turns] power [median units] hits" << std::endl;
    for (int b = 0; b < NB; ++b) {
        const double p = prof[b] / (static_cast<double>(hits[b]) * static_cast<double>(nb));
        out << std::setprecision(6) << (b + 0.5) / NB << " ";
        if (hits[b] == 0)
            out << "nan";
        else
            out << (linear ? p : 10 * std::log10(p));
        out << " " << hits[b] << std::endl;
    }
    out << std::endl;
    out.flush();
}

void spectrum_matrix_row(std::vector<double>& pwr, int N, int64_t repeats_done, int samplerate, bool linear,
                         const std::vector<double>* baseline, std::vector<float>& row)
{
    interpolate_dc(pwr, N);
    row.resize(N);
    for (int i = 0; i < N; ++i)
        row[i] = static_cast<float>(bin_value(pwr, i, N, repeats_done, samplerate, linear, baseline));
}

void Acquisition::write_data(std::ostream& out) const
{
    const std::vector<double>* baseline = options_.baseline ? &aux_.baseline_values : nullptr;
    if (!options_.matrixMode) {
        write_text_header(out, start_stamp_, end_stamp_, options_.bin_stats);
        if (options_.bin_stats)
            write_spectrum_text_stats(out, data_.pwr, data_.sum_sq, data_.peak, options_.N, data_.repeats_done, tuned_freq_,
                                      actual_samplerate_, options_.linear, baseline);
        else
            write_spectrum_text(out, data_.pwr, options_.N, data_.repeats_done, tuned_freq_, actual_samplerate_,
                                options_.linear, baseline);
        return;
    }
    append_matrix_row(options_, meta_, data_.pwr, data_.repeats_done, tuned_freq_, actual_samplerate_, baseline);
}

void append_matrix_row(const Options& options, ScanMetadata& meta, std::vector<double>& pwr, int64_t repeats_done,
                       int64_t tuned_freq, int samplerate, const std::vector<double>* baseline)
{
    std::vector<float> row;
    spectrum_matrix_row(pwr, options.N, repeats_done, samplerate, options.linear, baseline, row);
    std::ofstream bin(options.bin_file, std::ios::out | std::ios::app | std::ios::binary);
    bin.write(reinterpret_cast<const char*>(row.data()), static_cast<std::streamsize>(row.size() * 4));
    if (meta.metaRows == 1) meta.metaCols += options.N;
    if (tuned_freq >= options.finalfreq) meta.metaRows++;
}

}  // namespace rpf_host
