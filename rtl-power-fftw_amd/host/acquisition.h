// acquisition.h -- one data acquisition at one frequency: the producer loop of
// Acquisition::run (/root/reference/src/acquisition.cxx:222-348) over the
// engine's hand-off calls, the stderr summary (:350-358) and the spectrum
// writer (:360-433; text for gnuplot or float32 matrix rows).
#ifndef RPF_HOST_ACQUISITION_H
#define RPF_HOST_ACQUISITION_H

#include <cstdint>
#include <ctime>
#include <exception>
#include <ostream>
#include <string>

#include "aux_data.h"
#include "datastore.h"
#include "options.h"
#include "sample_source.h"

namespace rpf_host {

// Matrix-mode bookkeeping that the reference keeps in globals
// (/root/reference/src/metadata.h:28-33, rtl_power_fftw.cxx:39-48).
struct ScanMetadata {
    int metaRows = 1;
    int metaCols = 0;
    float avgScanDur = 0.0f;
    float sumScanDur = 0.0f;
    time_t scanEnd = 0, scanBeg = 0;
    int tunfreq = 0;
    int startFreq = 0, endFreq = 0, stepFreq = 0;
    std::string firstAcqTimestamp, lastAcqTimestamp;
    int cntTimeStamps = 0;
};

// acquisition.h:62-76 of the reference: tuning failed after three attempts.
class TuneError : public std::exception {
public:
    explicit TuneError(int64_t freq_) : freq(freq_) {}
    const char* what() const noexcept override { return "Could not tune to the given frequency."; }
    int64_t frequency() const { return freq; }
private:
    int64_t freq;
};

// One device's share of an acquisition in a multi-device scan:
// `repeats` frames starting `first_frame` frames into the hop whose bytes begin
// `hop_base` bytes into a sequential replay.
struct Shard {
    int64_t repeats = 0;
    int64_t first_frame = 0;
    uint64_t hop_base = 0;
};

class Acquisition {
public:
    Acquisition(const Options& options, AuxData& aux, SampleSource& source, Datastore& data,
                ScanMetadata& meta, int actual_samplerate, int64_t freq);
    // The same for a shard: quiet (the scan's main thread reports in hop order) and
    // without touching the scan-wide metadata.
    Acquisition(const Options& options, AuxData& aux, SampleSource& source, Datastore& data,
                ScanMetadata& meta, int actual_samplerate, int64_t freq, const Shard& shard);
    void run();
    void print_summary() const;
    void write_data(std::ostream& out) const;

    int64_t tuned_freq() const { return tuned_freq_; }
    const std::string& start_stamp() const { return start_stamp_; }
    const std::string& end_stamp() const { return end_stamp_; }
    int64_t device_readouts() const { return device_readouts_; }
    int64_t successful_readouts() const { return successful_readouts_; }
    static std::string utc_now();

private:
    bool chatty() const { return !sharded_ && (!options_.talkless || options_.outcnt == 0); }

    const Options& options_;
    AuxData& aux_;
    SampleSource& source_;
    Datastore& data_;
    ScanMetadata& meta_;
    int actual_samplerate_;
    int64_t freq_;
    Shard shard_;
    bool sharded_ = false;
    int64_t tuned_freq_ = 0;
    std::string start_stamp_, end_stamp_;
    int64_t device_readouts_ = 0;
    int64_t successful_readouts_ = 0;
};

// stderr summary of one acquisition (acquisition.cxx:350-358)
void print_acquisition_summary(int N, int64_t repeats_done, int64_t device_readouts, int64_t successful_readouts,
                               int actual_samplerate);
// The five '#' lines that precede a text spectrum (acquisition.cxx:411-419)
void write_text_header(std::ostream& out, const std::string& start_stamp, const std::string& end_stamp);

// Text/matrix rendering of one accumulated spectrum (acquisition.cxx:377-432).
// Mutates pwr[N/2] (DC interpolation) exactly like the reference.
void write_spectrum_text(std::ostream& out, std::vector<double>& pwr, int N, int64_t repeats_done,
                         int64_t tuned_freq, int samplerate, bool linear, const std::vector<double>* baseline);
// The same with the statistics columns of --stats: after the power column the peak hold, PK / N / samplerate (no
// division by repeats_done) through the power column's linear / dB / baseline handling and precision, and the
// spectral kurtosis (datastore.h), dimensionless: never dB, no baseline, "nan" where undefined.  The DC bin of both
// is the mean of its neighbours, as the power's.  Mutates pwr[N/2] and peak[N/2]; sum_sq is left alone.
void write_spectrum_text_stats(std::ostream& out, std::vector<double>& pwr, const std::vector<double>& sum_sq,
                               std::vector<double>& peak, int N, int64_t repeats_done, int64_t tuned_freq,
                               int samplerate, bool linear, const std::vector<double>* baseline);
// `stats`: the last '#' line names the two columns of --stats too
void write_text_header(std::ostream& out, const std::string& start_stamp, const std::string& end_stamp, bool stats);
// --excise: the header with "kept fraction" as the third column's name, and the block.  Power column: the mean over
// the kept integrations, clean[b] / (kept[b] L) -- where none was kept, the unexcised mean total[b] / (K L) -- with its
// DC bin the mean of its neighbours, then / N / samplerate, dB and baseline as always; third column: kept[b] / K as it
// is (the DC bin too).
void write_text_header_excised(std::ostream& out, const std::string& start_stamp, const std::string& end_stamp);
void write_spectrum_text_excised(std::ostream& out, const std::vector<double>& clean, const std::vector<double>& kept,
                                 const std::vector<double>& total, int N, int64_t K, int64_t L, int64_t tuned_freq,
                                 int samplerate, bool linear, const std::vector<double>* baseline);
// --quantile: the header, whose last line names one column per quantile ("quantile 0.5 [dB/Hz]"), and the block.
// planes[i N .. i N + N) = quantile q[i] of the integrations of L frames; every column is its plane / L with the DC bin
// the mean of its neighbours, then / N / samplerate, dB and baseline as the power column always.
void write_text_header_quantiles(std::ostream& out, const std::string& start_stamp, const std::string& end_stamp,
                                 const std::vector<double>& q);
void write_spectrum_text_quantiles(std::ostream& out, const std::vector<double>& planes, const std::vector<double>& q, int N,
                                   int64_t L, int64_t tuned_freq, int samplerate, bool linear,
                                   const std::vector<double>* baseline);
// --cross: the header, whose last line names the five columns, and the block.  planes[4 x N] = Saa, Sbb, Re Sab, Im Sab
// over `frames` frames (rpf_accumulate_cross); the DC bin of each of the four is the mean of its neighbours, then the
// two power columns go / frames / N / samplerate, dB and baseline as always, and coherence (dimensionless: never dB, no
// baseline, "nan" where undefined) and phase [rad] are derived from the four (datastore.h: coherence, cross_phase).
void write_text_header_cross(std::ostream& out, const std::string& start_stamp, const std::string& end_stamp);
// --correlate: the header, whose last line names the columns (frequency, the power of every stream m, then coherence
// i-j and phase i-j [rad] for i < j), and the block.  vis[M x M x 2 x N] = V_ij re, im over `frames` frames
// (rpf_correlate); the DC bin of every plane is the mean of its neighbours, then the powers are written by the usual
// rules and coherence and phase derived from the planes (datastore.h: coherence_pair, cross_phase).
void write_text_header_correlate(std::ostream& out, const std::string& start_stamp, const std::string& end_stamp, int M);
void write_spectrum_text_correlate(std::ostream& out, const std::vector<double>& vis, int M, int N, int64_t frames,
                                   int64_t tuned_freq, int samplerate, bool linear, const std::vector<double>* baseline);
void write_spectrum_text_cross(std::ostream& out, const std::vector<double>& planes, int N, int64_t frames, int64_t tuned_freq,
                               int samplerate, bool linear, const std::vector<double>* baseline);
// --dedisperse: one block per trial.  The header carries one more line, "# DM <dm> pc cm^-3, largest delay <n>
// integrations", and names the columns time [s] and power [median units]; the block is one line per time t < T:
// t L S / samplerate in nine digits, then trial[t] / nb (nb = the bins of non-zero weight) in six, in dB unless
// `linear`; a blank line ends it.
void write_text_header_dedisperse(std::ostream& out, const std::string& start_stamp, const std::string& end_stamp, double dm,
                                  int64_t largest_delay);
void write_text_dedisperse(std::ostream& out, const double* trial, int64_t T, int64_t nb, int64_t L, int64_t step, int samplerate,
                           bool linear);
// --dedisperse --fold, block 1, the search plane: the usual three header lines, "# fold: <D> DMs x <P> periods, <NB> phase
// bins, <T> times", "#", the column names, then one line per (DM, period), DM-major with a blank line after every DM: the
// DM in six digits, the period in nine, chi2[d P + p] in six; a blank line ends the block.
void write_text_fold_plane(std::ostream& out, const std::string& start_stamp, const std::string& end_stamp,
                           const std::vector<double>& dms, const std::vector<double>& periods, int NB, int64_t T,
                           const std::vector<double>& chi2);
// ... block 2, the profile of one cell: "# DM <dm> pc cm^-3, period <p> s, reduced chi2 <v>", "#", the column names, then
// one line per phase bin: (b + 0.5) / NB, prof[b] / (hits[b] nb) (nb = the bins of non-zero weight; in dB unless `linear`;
// nan where hits[b] = 0) and hits[b]; a blank line ends it.
void write_text_fold_profile(std::ostream& out, const std::string& start_stamp, const std::string& end_stamp, double dm,
                             double period, double chi2, const double* prof, const int32_t* hits, int NB, int64_t nb, bool linear);
void spectrum_matrix_row(std::vector<double>& pwr, int N, int64_t repeats_done, int samplerate, bool linear,
                         const std::vector<double>* baseline, std::vector<float>& row);
// Matrix mode: append one float32 row to options.bin_file and keep the row/column
// bookkeeping of the .met file (acquisition.cxx:385-388,400-409,421-426).
void append_matrix_row(const Options& options, ScanMetadata& meta, std::vector<double>& pwr, int64_t repeats_done,
                       int64_t tuned_freq, int samplerate, const std::vector<double>* baseline);

}  // namespace rpf_host
#endif
