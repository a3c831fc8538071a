#include "options.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <vector>

#include "units.h"

namespace rpf_host {

const char* const kVersion = "1.0-beta2-mi355x";

namespace {

enum class Kind { Flag, Int, Int64, Double, Text };

struct Spec {
    char short_name;           // 0 = none
    const char* long_name;
    Kind kind;
    const char* value_name;
    const char* help;          // nullptr: parsed, but not in the --help text, which stays the text
                               // tests/golden/cli_refusals.json pins (README.md documents such options)
};

// Same options, names and help texts as params.cxx:104-141 (alphabetical like the man page).
const Spec kSpecs[] = {
    {'B', "baseline", Kind::Text, "file|-", "Subtract baseline, read baseline data from file or stdin."},
    {'b', "bins", Kind::Int, "bins in FFT spectrum", "Number of bins in FFT spectrum (must be even number)"},
    {0, "buffers", Kind::Int, "buffers", "Number of read buffers (don't touch unless running out of memory)."},
    {'c', "continue", Kind::Flag, "", "Repeat the same measurement endlessly."},
    {'d', "device", Kind::Int, "device index", "RTL-SDR device index."},
    {'e', "elapsed", Kind::Text, "seconds", "Scan session duration."},
    {'f', "freq", Kind::Text, "Hz | Hz:Hz", "Center frequency of the receiver or frequency range to scan."},
    {'g', "gain", Kind::Int, "1/10th of dB", "Receiver gain."},
    {'l', "linear", Kind::Flag, "", "Calculate linear power values instead of logarithmic."},
    {'m', "matrix", Kind::Text, "filename (without extension)",
     "Will output data in binary matrix format plus separate metadata text file"},
    {'n', "repeats", Kind::Int64, "repeats", "Number of scans for averaging (incompatible with -t)."},
    {'o', "overlap", Kind::Double, "percent",
     "Define lower boundary for overlap when frequency hopping (otherwise meaningless)."},
    {'p', "ppm", Kind::Int, "ppm", "Set custom ppm error in RTL-SDR device."},
    {'q', "quiet", Kind::Flag, "", "Limit verbosity."},
    {'r', "rate", Kind::Int, "samples/s", "Sample rate of the receiver."},
    {'s', "buffer-size", Kind::Int, "bytes", "Size of read buffers (leave it unless you know what you are doing)."},
    {'T', "strict-time", Kind::Flag, "",
     "End measurement when the time set with --time option is up, regardless of gathered samples."},
    {'t', "time", Kind::Text, "seconds", "Integration time (incompatible with -n)."},
    {'w', "window", Kind::Text, "file|-", "Use window function, from file or stdin."},
    // additive (not in the reference)
    {0, "input", Kind::Text, "file|-", "Replay interleaved IQ samples (see --format) from a file or stdin."},
    {0, "format", Kind::Text, "cu8|cs8|cs16",
     "Sample format of --input: cu8 (unsigned 8-bit, the default), cs8 (signed 8-bit), cs16 (signed 16-bit little-endian); "
     "also cf32 (float32 little-endian I/Q, taken as stored: no scaling)."},
    {0, "synthetic", Kind::Int64, "seed", "Use the built-in synthetic receiver instead of a dongle."},
    {0, "gpu", Kind::Int, "ordinal", "HIP device to run on."},
    {0, "gpus", Kind::Text, "a,b,...", "HIP devices to spread a scan over (one engine per listed device)."},
    {0, "frame-overlap", Kind::Text, "percent",
     "Overlap of consecutive FFT frames inside one acquisition (Welch averaging), 0 <= percent < 100; "
     "not the hop overlap of -o. Default 0."},
    {0, "stats", Kind::Flag, "",
     "Per-bin statistics: two more output columns, peak hold and the spectral kurtosis estimator "
     "(not with -m, not with several --gpus)."},
    {0, "series", Kind::Int64, "frames",
     "Spectrogram of --input: one spectrum per <frames> consecutive FFT frames, written one after the other "
     "(not with a frequency range, -n, -t, -c, -e, -m, --stats or several --gpus)."},
    {0, "series-stats", Kind::Int64, "frames",
     "Time-resolved statistics of --input: one block with the --stats columns (peak hold, spectral kurtosis) per "
     "<frames> consecutive FFT frames (implies --stats; not with --series, a frequency range, -n, -t, -c, -e, -m or several --gpus)."},
    {0, "excise", Kind::Int64, "frames",
     "Average of --input without interference: integrations of <frames> consecutive FFT frames whose spectral kurtosis "
     "leaves 1 +- sigma standard deviations are left out, bin by bin; one block with a kept-fraction column (implies "
     "--stats' engine; not with --series, --series-stats, a frequency range, -n, -t, -c, -e, -m or several --gpus)."},
    {0, "excise-sigma", Kind::Double, "sigma", "Width of the --excise thresholds in standard deviations of the estimator. Default 3."},
    {0, "quantile", Kind::Int64, "frames",
     "Per-bin quantiles of --input over time: the replay is cut into integrations of <frames> consecutive FFT frames and "
     "every bin's quantiles over them are written as one block, one column per quantile (not with --series, "
     "--series-stats, --excise, --stats, --pfb, a frequency range, -n, -t, -c, -e, -m or several --gpus)."},
    {0, "quantiles", Kind::Text, "a,b,...",
     "The quantiles --quantile writes, each in [0, 1], at most 8; the first is the power column. Default 0.5 (the median)."},
    {0, "pfb", Kind::Int, "taps",
     "Polyphase filter bank front end: every frame is <taps> x bins samples weighted by a windowed-sinc prototype and "
     "folded to <bins> before the FFT, 1 <= taps <= 32 (not with -w, --frame-overlap, --stats, --series, --series-stats, "
     "--excise or several --gpus)."},
    {0, "cross", Kind::Text, "file",
     "Cross-spectrum of --input (stream a) and <file> (stream b, same format, sample rate and tuning): one block with the "
     "power of a, the power of b, the magnitude-squared coherence and the phase of the cross-spectrum [rad] over the whole "
     "frames of the shorter file (not with a frequency range, -n, -t, -c, -e, -m, --stats, --series, --series-stats, "
     "--excise, --quantile, --pfb or several --gpus)."},
    {0, "stft", Kind::Text, "file",
     "Short-time Fourier transform of --input: the complex spectrum of every FFT frame, bin N/2 = DC, written to <file> as "
     "raw little-endian float32 pairs (re, im), frame after frame; nothing goes to stdout (power-of-two bins only; "
     "combines with -w, --format, --frame-overlap and --pfb; not with a frequency range, -n, -t, -c, -e, -m, --stats, "
     "--series, --series-stats, --excise, --quantile, --cross or several --gpus)."},
    // Correlator of --input (stream 0) and the listed files (streams 1, 2, ..., at most 7; same format, sample rate and
    // tuning): one block with the power of every stream, then the magnitude-squared coherence and the phase [rad] of every
    // pair i < j, over the whole frames of the shortest file (power-of-two bins only; combines with -w, --format,
    // --frame-overlap and --pfb; not with a frequency range, -n, -t, -c, -e, -m, --stats, --series, --series-stats,
    // --excise, --quantile, --cross, --stft or several --gpus).
    {0, "correlate", Kind::Text, "b,c,...", nullptr},
    // Incoherent dedispersion of --input: the replay is cut into integrations of <frames> consecutive FFT frames, every bin
    // is divided by its median over them, and for every dispersion measure of --dm (one value, or lo:hi:step; at most 4096
    // trials; pc cm^-3) the bins are added along that DM's delay curve: one block of time and power per trial (combines
    // with -w, --format, --frame-overlap and -l; not with a frequency range, -n, -t, -c, -e, -m, -B, --stats, --series,
    // --series-stats, --excise, --quantile, --cross, --stft, --correlate, --pfb or several --gpus).
    {0, "dedisperse", Kind::Int64, "frames", nullptr},
    {0, "dm", Kind::Text, "lo:hi:step | value", nullptr},
    // With --dedisperse: fold every trial of the DM-time plane at the periods of --fold (seconds; one value, or lo:hi:step;
    // at most 4096) into --phase-bins phase bins (1 ... 128, default 16): one block of reduced chi-square per (DM, period)
    // and the profile of the strongest cell, in place of the blocks of time and power.
    {0, "fold", Kind::Text, "lo:hi:step | period", nullptr},
    {0, "phase-bins", Kind::Int64, "n", nullptr},
    {0, "reduce", Kind::Text, "rccl|host", "With --gpus: where a scan's per-device spectra are added (default: rccl if it loads, else host)."},
    {'h', "help", Kind::Flag, "", "Displays usage information and exits."},
    {0, "version", Kind::Flag, "", "Displays version information and exits."},
};

struct Parsed {
    std::map<std::string, std::string> value;   // long name -> text ("" for flags)
    bool has(const char* n) const { return value.count(n) != 0; }
    const std::string& get(const char* n) const { return value.at(n); }
};

[[noreturn]] void parse_error(const std::string& what, const std::string& arg)
{
    // TCLAP's ArgException text as rethrown at params.cxx:266-270
    throw RPFexception("Error: " + what + " for arg " + arg, ReturnValue::TCLAPerror);
}

const Spec* find_spec(const std::string& token)
{
    for (const Spec& s : kSpecs) {
        if (token.size() == 2 && token[0] == '-' && s.short_name && token[1] == s.short_name) return &s;
        if (token.size() > 2 && token.compare(0, 2, "--") == 0 && token.substr(2) == s.long_name) return &s;
    }
    return nullptr;
}

template <typename T>
T to_number(const Spec& s, const std::string& text)
{
    std::istringstream in(text);
    T v{};
    if (!(in >> v) || !(in >> std::ws).eof())
        parse_error("Couldn't read argument value from string '" + text + "'",
                    std::string("--") + s.long_name);
    return v;
}

Parsed tokenize(int argc, const char* const* argv)
{
    Parsed out;
    for (int i = 1; i < argc; ++i) {
        std::string token = argv[i];
        if (token == "--" || token == "--ignore_rest") break;
        std::string attached;
        bool has_attached = false;
        // --name=value
        const size_t eq = token.find('=');
        if (token.compare(0, 2, "--") == 0 && eq != std::string::npos) {
            attached = token.substr(eq + 1);
            token = token.substr(0, eq);
            has_attached = true;
        }
        const Spec* spec = find_spec(token);
        if (!spec) parse_error("Couldn't find match for argument", token);
        const std::string key = spec->long_name;
        if (out.has(key.c_str())) parse_error("Argument already set!", "--" + key);
        if (spec->kind == Kind::Flag) {
            out.value[key] = "";
            continue;
        }
        if (!has_attached) {
            if (i + 1 >= argc) parse_error("Missing a value for this argument!", "--" + key);
            attached = argv[++i];
        }
        out.value[key] = attached;
    }
    return out;
}

void require_non_negative(const Parsed& p, const char* name)
{
    if (!p.has(name)) return;
    std::istringstream in(p.get(name));
    double v = 0;
    in >> v;
    if (v < 0)
        throw RPFexception(std::string("Argument to '") + name + "' must be a positive number.",
                           ReturnValue::InvalidArgument);
}

// A replay mode is an option that reads --input once, to its end, outside the acquisition loop.  One row each, in the
// order their refusals speak; replay_mode() below walks a row.
struct Refused { const char* option; const char* why; };
constexpr int kMaxRefused = 9;      // the most options one row refuses; the entry after them stays null (rows_end below)
struct ReplayMode {
    const char* name;
    int64_t Options::*frames;       // where its <frames> goes, checked against min_frames; null: the argument is a file
    int min_frames;
    const char* min_why;            // (what follows "at least <min_frames>")
    const char* input_why;          // "needs --input: <input_why>."
    const char* repeat_why;         // "does not combine with --repeats (-n): <repeat_why>."; so -t, -c, -e
    const char* matrix_why;         // "does not combine with -m (matrix mode): <matrix_why>."
    bool bin_stats;                 // turns Options::bin_stats on
    Refused refused[kMaxRefused + 1];   // "does not combine with --<option>: <why>.", in this order; ends at the first null
};

const char kOwnLength[] = "the integration length is its own argument and the replay is read once";
const char kAverage[] = "that writes every integration, this one their average";
const char kOneProduct[] = "one product of the integrations per run";
const char kSums[] = "those end in sums of |X|^2, this writes X itself";
const char kNoCross[] = "cross-spectra of those are not built";
const char kNoCorrelate[] = "visibilities of those are not built";
const char kPlainRows[] = "it reads the row store, which holds the plain series of one stream";

constexpr ReplayMode kReplayModes[] = {
    {"series", &Options::series_frames, 1, "", "it cuts a replayed stream into consecutive integrations", kOwnLength,
     "the spectra are text blocks", false, {{"stats", "time-resolved statistics are not built"}}},
    {"series-stats", &Options::series_frames, 1, "", "it cuts a replayed stream into consecutive integrations", kOwnLength,
     "the spectra are text blocks", true, {}},
    {"excise", &Options::excise_frames, 2, " (the spectral kurtosis of one frame is undefined)",
     "it averages a replayed stream", kOwnLength, "the average is one text block", true,
     {{"series", kAverage}, {"series-stats", kAverage}}},
    {"quantile", &Options::quantile_frames, 1, "", "it ranks the integrations of a replayed stream", kOwnLength,
     "the quantiles are columns of one text block", false,
     {{"series", kOneProduct}, {"series-stats", kOneProduct}, {"excise", kOneProduct},
      {"stats", "the row store holds the plain series"}, {"pfb", "quantiles of PFB spectra are not built"}}},
    {"stft", nullptr, 0, "", "it transforms the frames of a replayed stream",
     "the replay is read once, to its end, and every frame leaves a row", "the rows go to the file given to --stft", false,
     {{"stats", kSums}, {"series", kSums}, {"series-stats", kSums}, {"excise", kSums}, {"quantile", kSums}, {"cross", kSums}}},
    {"cross", nullptr, 0, "", "that is stream a, and the file given here stream b",
     "the two replays are read once, to the end of the shorter", "the cross-spectrum is one text block", false,
     {{"stats", kNoCross}, {"series", kNoCross}, {"series-stats", kNoCross}, {"excise", kNoCross}, {"quantile", kNoCross},
      {"pfb", kNoCross}}},
    {"correlate", nullptr, 0, "", "that is stream 0, and the files listed here streams 1, 2, ...",
     "the replays are read once, to the end of the shortest", "the visibilities are one text block", false,
     {{"stats", kNoCorrelate}, {"series", kNoCorrelate}, {"series-stats", kNoCorrelate}, {"excise", kNoCorrelate},
      {"quantile", kNoCorrelate}, {"cross", "--cross is the correlator's two-stream special case"},
      {"stft", "that writes the frames' spectra themselves"}}},
    {"dedisperse", &Options::dedisperse_frames, 1, "", "it adds the integrations of a replayed stream along delay curves",
     kOwnLength, "the DM-time plane is one text block per trial", false,
     {{"stats", kPlainRows}, {"series", kOneProduct}, {"series-stats", kOneProduct}, {"excise", kOneProduct},
      {"quantile", kOneProduct}, {"cross", kPlainRows}, {"stft", kPlainRows}, {"correlate", kPlainRows},
      {"pfb", kPlainRows}}},
};

// replay_mode() walks a row's refusals to the first null: every row keeps its last entry for it.
constexpr int kReplayModeCount = sizeof(kReplayModes) / sizeof(kReplayModes[0]);
constexpr bool rows_end(int row)
{
    return row == kReplayModeCount || (kReplayModes[row].refused[kMaxRefused].option == nullptr && rows_end(row + 1));
}
static_assert(rows_end(0), "a row of kReplayModes refuses more than kMaxRefused options: its list has no terminating null");

[[noreturn]] void refuse(const std::string& mode, const std::string& what)
{
    throw RPFexception("Option --" + mode + " " + what + " Exiting.", ReturnValue::InvalidArgument);
}

// <value> or <lo:hi:step> of --dm and --fold: the trials lo + i step for i = 0 ... floor((hi - lo) / step + 1e-9), at most
// 4096 of them, none negative.  `option` and `expecting` go into the refusal.
std::vector<double> parse_trial_list(const std::string& text, const char* option, const char* expecting)
{
    std::vector<double> part;
    size_t pos = 0;
    bool good = true;
    while (pos <= text.size()) {
        const size_t colon = std::min(text.find(':', pos), text.size());
        const std::string item = text.substr(pos, colon - pos);
        char* end = nullptr;
        const double v = std::strtod(item.c_str(), &end);
        // (digits, a point and an exponent only: strtod alone would also take blanks, hexadecimal and "inf")
        good = good && !item.empty() && item.find_first_not_of("0123456789.eE+-") == std::string::npos && *end == '\0' &&
               std::isfinite(v) && v >= 0.0;
        part.push_back(v);
        pos = colon + 1;
    }
    good = good && (part.size() == 1 || (part.size() == 3 && part[1] >= part[0] && part[2] > 0.0));
    if (!good)
        refuse("dedisperse", std::string("could not use the value given to --") + option + ": " + text + ". Expecting " + expecting +
                                 " or lo:hi:step, none negative, hi >= lo and step > 0.");
    if (part.size() == 1) return part;
    const double count = std::floor((part[1] - part[0]) / part[2] + 1e-9) + 1.0;
    if (count > 4096.0)
        refuse("dedisperse", std::string("takes at most 4096 trials in --") + option + ", got " +
                                 std::to_string(static_cast<long long>(std::min(count, 1e18))) + ".");
    std::vector<double> trials;
    for (int i = 0; i < static_cast<int>(count); ++i) trials.push_back(part[0] + i * part[2]);
    return trials;
}

// False when the command line does not name the mode; else takes its frame count, throws the first of the row's
// refusals that applies, and returns true.  `o` holds what parse_command_line has made of the other options by then.
bool replay_mode(const std::string& name, const Parsed& p, Options& o)
{
    if (!p.has(name.c_str())) return false;
    const ReplayMode* m = kReplayModes;
    while (name != m->name) ++m;
    if (m->frames) {
        o.*m->frames = to_number<int64_t>(*find_spec("--" + name), p.get(name.c_str()));
        if (o.*m->frames < m->min_frames)
            refuse(name, "needs a number of frames of at least " + std::to_string(m->min_frames) + m->min_why + ", got " +
                             p.get(name.c_str()) + ".");
    }
    if (!p.has("input")) refuse(name, std::string("needs --input: ") + m->input_why + ".");
    for (const Refused* r = m->refused; r->option; ++r)
        if (p.has(r->option)) refuse(name, std::string("does not combine with --") + r->option + ": " + r->why + ".");
    if (o.freq_hopping_isSet) refuse(name, "does not combine with a frequency range in -f: a replay is one stream.");
    for (const char* other : {"repeats", "time", "continue", "elapsed"})
        if (p.has(other))
            refuse(name, std::string("does not combine with --") + other + " (-" + find_spec(std::string("--") + other)->short_name +
                             "): " + m->repeat_why + ".");
    if (o.matrixMode) refuse(name, std::string("does not combine with -m (matrix mode): ") + m->matrix_why + ".");
    if (o.devices.size() > 1) refuse(name, "does not combine with several devices in --gpus.");
    if (m->bin_stats) o.bin_stats = true;
    return true;
}

}  // namespace

std::string usage_text()
{
    std::ostringstream o;
    o << "USAGE:\n   rpf_power [OPTION ...]\n\nObtain power spectrum from RTL device using FFTW library"
         " (MI355X engine build).\n\nWhere:\n";
    for (const Spec& s : kSpecs) {
        if (!s.help) continue;
        o << "   ";
        if (s.short_name) o << "-" << s.short_name << ",  ";
        o << "--" << s.long_name;
        if (s.kind != Kind::Flag) o << " <" << s.value_name << ">";
        o << "\n     " << s.help << "\n\n";
    }
    return o.str();
}

Options parse_command_line(int argc, const char* const* argv)
{
    const Parsed p = tokenize(argc, argv);
    Options o;
    if (p.has("help")) { o.show_help = true; return o; }
    if (p.has("version")) { o.show_version = true; return o; }

    // validate the types first (TCLAP does this while parsing)
    for (const Spec& s : kSpecs) {
        if (!p.has(s.long_name)) continue;
        if (s.kind == Kind::Int) (void)to_number<int>(s, p.get(s.long_name));
        if (s.kind == Kind::Int64) (void)to_number<int64_t>(s, p.get(s.long_name));
        if (s.kind == Kind::Double) (void)to_number<double>(s, p.get(s.long_name));
    }
    // params.cxx:146-147
    for (const char* name : {"bins", "rate", "gain", "device", "buffers", "buffer-size", "repeats"})
        require_non_negative(p, name);

    auto int_of = [&](const char* n, int fallback) {
        return p.has(n) ? to_number<int>(*find_spec(std::string("--") + n), p.get(n)) : fallback;
    };
    o.dev_index = int_of("device", o.dev_index);
    o.N = int_of("bins", o.N);
    if (o.N % 2 != 0) {                                              // params.cxx:150-155
        o.N++;
        std::cerr << "Number of bins should be even, changing to " << o.N << "." << std::endl;
    }
    o.linear = p.has("linear");
    o.gain = int_of("gain", o.gain);
    o.sample_rate = int_of("rate", o.sample_rate);
    o.buffers = int_of("buffers", o.buffers);
    o.buf_length = int_of("buffer-size", o.buf_length);
    o.endless = p.has("continue");
    o.talkless = p.has("quiet");
    o.strict_time = p.has("strict-time");
    if (p.has("overlap")) o.min_overlap = to_number<double>(*find_spec("--overlap"), p.get("overlap"));
    o.device = int_of("gpu", 0);
    if (p.has("gpus")) {
        if (p.has("gpu"))
            throw RPFexception("Options --gpu and --gpus are mutually exclusive. Exiting.", ReturnValue::InvalidArgument);
        const std::string list = p.get("gpus");
        size_t pos = 0;
        while (pos <= list.size()) {
            const size_t comma = std::min(list.find(',', pos), list.size());
            const std::string item = list.substr(pos, comma - pos);
            char* end = nullptr;
            const long v = std::strtol(item.c_str(), &end, 10);
            if (item.empty() || *end != '\0' || v < 0 || v > 4095)
                throw RPFexception("Could not parse the device list given to --gpus: " + list + ".\n"
                                   "Expecting comma-separated HIP device ordinals. Exiting.",
                                   ReturnValue::InvalidArgument);
            o.devices.push_back(static_cast<int>(v));
            pos = comma + 1;
        }
        o.device = o.devices.front();
    } else {
        o.devices.push_back(o.device);
    }
    if (p.has("reduce")) {
        o.reduce = p.get("reduce");
        if (o.reduce != "rccl" && o.reduce != "host")
            throw RPFexception("Argument to --reduce must be rccl or host. Exiting.", ReturnValue::InvalidArgument);
    }

    if (o.buf_length % base_buf != 0) {                              // params.cxx:171-175
        o.buf_length = static_cast<int>(std::floor(static_cast<double>(o.buf_length) / base_buf + 0.5) * base_buf);
        std::cerr << "Buffer length should be multiple of " << base_buf << ", changing to "
                  << o.buf_length << "." << std::endl;
    }
    o.ppm_error = int_of("ppm", o.ppm_error);

    if (p.has("freq")) {                                             // params.cxx:177-212
        const std::string text = p.get("freq");
        const size_t colon = text.find(':');
        if (colon != std::string::npos) {
            const std::string lo = text.substr(0, colon), hi = text.substr(colon + 1);
            if (lo.empty() || hi.empty())
                throw RPFexception("Could not parse frequency range given to --freq: " + text + ".\n"
                                   "Expecting form startfreq:stopfreq. Exiting.", ReturnValue::InvalidArgument);
            o.startfreq = parse_frequency(lo);
            o.stopfreq = parse_frequency(hi);
            if (o.startfreq < 0 || o.stopfreq < 0 || o.stopfreq < o.startfreq)
                throw RPFexception("Invalid frequency range given to --freq: " + text + ".\n"
                                   "Expecting positive numbers in ascending order, allowing the k,M,G "
                                   "multipliers. Exiting.", ReturnValue::InvalidArgument);
            o.freq_hopping_isSet = true;
            o.cfreq = (o.startfreq + o.stopfreq) / 2;
        } else {
            o.cfreq = parse_frequency(text);
            if (o.cfreq < 0)
                throw RPFexception("Invalid frequency given to --freq: " + std::to_string(o.cfreq) + ".\n"
                                   "Expecting a positive number, allowing the k,M,G multipliers. Exiting.",
                                   ReturnValue::InvalidArgument);
        }
    }

    if (p.has("frame-overlap")) {
        // (parsed here, not by the type check above: a non-number is an invalid argument, exit 3, like a value
        // out of range)
        const std::string text = p.get("frame-overlap");
        char* end = nullptr;
        o.frame_overlap = std::strtod(text.c_str(), &end);
        if (text.empty() || *end != '\0' || !(o.frame_overlap >= 0 && o.frame_overlap < 100))
            throw RPFexception("Invalid frame overlap given to --frame-overlap: " + text + ".\n"
                               "Expecting a percentage in [0, 100). Exiting.", ReturnValue::InvalidArgument);
        const int64_t cut = static_cast<int64_t>(std::floor(static_cast<double>(o.N) * o.frame_overlap / 100));
        o.frame_step = static_cast<int>(std::max<int64_t>(1, o.N - cut));
    }
    if (p.has("format")) {
        const std::string text = p.get("format");
        if (text == "cu8") o.sample_format = RPF_FORMAT_CU8;
        else if (text == "cs8") o.sample_format = RPF_FORMAT_CS8;
        else if (text == "cs16") o.sample_format = RPF_FORMAT_CS16;
        else if (text == "cf32") o.sample_format = RPF_FORMAT_CF32;
        else
            throw RPFexception("Unknown sample format given to --format: " + text + ".\n"
                               "Expecting one of cu8, cs8, cs16, cf32. Exiting.", ReturnValue::InvalidArgument);
        // the format describes a replayed file; a dongle and the synthetic receiver deliver cu8
        if (o.sample_format != RPF_FORMAT_CU8 && !p.has("input"))
            throw RPFexception("Option --format " + text + " needs --input: a dongle and --synthetic deliver cu8 "
                               "(one of cu8, cs8, cs16, cf32). Exiting.", ReturnValue::InvalidArgument);
    }
    if (p.has("pfb")) {
        // (before the repeats: the default and -t are sample budgets, which the span of a PFB frame turns into frames)
        o.pfb_taps = to_number<int>(*find_spec("--pfb"), p.get("pfb"));
        if (o.pfb_taps < 1 || o.pfb_taps > 32)
            throw RPFexception("Invalid number of taps given to --pfb: " + p.get("pfb") + ".\n"
                               "Expecting a number between 1 and 32. Exiting.", ReturnValue::InvalidArgument);
        // (all follow-ups: coefficients from a file; overlapped PFB frames; PFB in front of the statistics kernels;
        // a span carried across the shards of several devices)
        const struct { const char* name; const char* shown; const char* why; } refused[] = {
            {"window", "-w", "the PFB coefficients are the window"},
            {"frame-overlap", "--frame-overlap", "PFB frames advance by the number of bins"},
            {"stats", "--stats", "PFB with statistics is not built"},
            {"series", "--series", "PFB with a series is not built"},
            {"series-stats", "--series-stats", "PFB with a series is not built"},
            {"excise", "--excise", "PFB with excision is not built"},
        };
        for (const auto& r : refused)
            if (p.has(r.name))
                throw RPFexception(std::string("Option --pfb does not combine with ") + r.shown + ": " + r.why + ". Exiting.",
                                   ReturnValue::InvalidArgument);
        if (o.devices.size() > 1)
            throw RPFexception("Option --pfb does not combine with several devices in --gpus. Exiting.",
                               ReturnValue::InvalidArgument);
    }
    if (p.has("repeats")) o.repeats = to_number<int64_t>(*find_spec("--repeats"), p.get("repeats"));
    else o.repeats = o.frames_for_budget(o.buf_length / (o.sample_bytes() * o.N));  // params.cxx:214-217, as a sample budget
    if (p.has("time")) {
        o.integration_time = parse_time(p.get("time"));
        if (o.integration_time <= 0)
            throw RPFexception("Could not parse the value given to --time. Expecting format [WdXhYm]Z[s]. Exiting.",
                               ReturnValue::InvalidArgument);
        o.integration_time_isSet = true;
    }
    if (p.has("time") && p.has("repeats"))
        throw RPFexception("Options -n and -t are mutually exclusive. Exiting.", ReturnValue::InvalidArgument);
    if (o.strict_time && !p.has("time")) {
        std::cerr << "Warning: option --strict-time has no effect without --time." << std::endl;
        o.strict_time = false;
    }
    o.buf_length_isSet = p.has("buffer-size");
    o.baseline = p.has("baseline");
    if (o.baseline) o.baseline_file = p.get("baseline");
    o.window = p.has("window");
    if (o.window) o.window_file = p.get("window");
    o.matrixMode = p.has("matrix");
    if (o.matrixMode) {
        o.matrix_file = p.get("matrix");
        o.bin_file = o.matrix_file + ".bin";
        o.meta_file = o.matrix_file + ".met";
    }
    if (p.has("elapsed")) {
        o.session_duration = parse_time(p.get("elapsed"));
        if (o.session_duration <= 0)
            throw RPFexception("Could not parse the value given to --time. Expecting format [WdXhYm]Z[s]. Exiting.",
                               ReturnValue::InvalidArgument);
        o.session_duration_isSet = true;
    }
    o.bin_stats = p.has("stats");
    // (both are follow-ups: extra matrix files; a maximum beside the sum in the scan reducer)
    if (o.bin_stats && o.matrixMode)
        throw RPFexception("Option --stats does not combine with -m (matrix mode): the statistics are two more columns "
                           "of the text output. Exiting.", ReturnValue::InvalidArgument);
    if (o.bin_stats && o.devices.size() > 1)
        throw RPFexception("Option --stats does not combine with several devices in --gpus. Exiting.",
                           ReturnValue::InvalidArgument);
    // the replay modes (kReplayModes), in the table's order: with two of them given, the first one's refusals speak.
    // Beside each walk, what is that mode's own.
    if (p.has("series") && p.has("series-stats"))
        throw RPFexception("Option --series-stats does not combine with --series: it is the series with the statistics "
                           "columns. Exiting.", ReturnValue::InvalidArgument);
    replay_mode("series", p, o);
    o.series_stats = replay_mode("series-stats", p, o);       // (--stats beside it changes nothing)
    if (p.has("excise-sigma") && !p.has("excise"))
        throw RPFexception("Option --excise-sigma needs --excise: it sets the width of its thresholds. Exiting.",
                           ReturnValue::InvalidArgument);
    if (replay_mode("excise", p, o) && p.has("excise-sigma")) {
        o.excise_sigma = to_number<double>(*find_spec("--excise-sigma"), p.get("excise-sigma"));
        if (!(o.excise_sigma >= 0) || std::isinf(o.excise_sigma))
            refuse("excise", "needs a finite, non-negative --excise-sigma, got " + p.get("excise-sigma") + ".");
    }
    if (p.has("quantiles") && !p.has("quantile"))
        throw RPFexception("Option --quantiles needs --quantile: it lists the quantiles that one writes. Exiting.",
                           ReturnValue::InvalidArgument);
    if (replay_mode("quantile", p, o)) {
        o.quantiles.assign(1, 0.5);
        if (p.has("quantiles")) {
            const std::string list = p.get("quantiles");
            o.quantiles.clear();
            size_t pos = 0;
            while (pos <= list.size()) {
                const size_t comma = std::min(list.find(',', pos), list.size());
                const std::string item = list.substr(pos, comma - pos);
                char* end = nullptr;
                const double v = std::strtod(item.c_str(), &end);
                if (item.empty() || *end != '\0' || !(v >= 0.0 && v <= 1.0))
                    refuse("quantile", "could not use the list given to --quantiles: " + list +
                                       ". Expecting comma-separated numbers in [0, 1].");
                o.quantiles.push_back(v);
                pos = comma + 1;
            }
            if (o.quantiles.size() > 8)
                refuse("quantile", "takes at most 8 values in --quantiles, got " + std::to_string(o.quantiles.size()) + ".");
        }
    }
    if (replay_mode("stft", p, o)) {
        o.stft_file = p.get("stft");
        if (o.N & (o.N - 1)) refuse("stft", "needs a power-of-two number of bins (-b); got " + std::to_string(o.N) + ".");
    }
    if (replay_mode("cross", p, o)) {
        o.cross_file = p.get("cross");
        if (o.cross_file == "-" && p.get("input") == "-") refuse("cross", "cannot read both streams from stdin.");
    }
    if (replay_mode("correlate", p, o)) {
        const std::string list = p.get("correlate");
        size_t pos = 0;
        while (pos <= list.size()) {
            const size_t comma = std::min(list.find(',', pos), list.size());
            const std::string item = list.substr(pos, comma - pos);
            if (item.empty()) refuse("correlate", "could not use the list given to --correlate: " + list + ". Expecting comma-separated files.");
            o.correlate_files.push_back(item);
            pos = comma + 1;
        }
        if (o.correlate_files.size() > 7)
            refuse("correlate", "takes at most 7 files beside --input, got " + std::to_string(o.correlate_files.size()) + ".");
        if (o.N & (o.N - 1)) refuse("correlate", "needs a power-of-two number of bins (-b); got " + std::to_string(o.N) + ".");
        int from_stdin = p.get("input") == "-";
        for (const std::string& f : o.correlate_files) from_stdin += f == "-";
        if (from_stdin > 1) refuse("correlate", "cannot read more than one stream from stdin.");
    }
    if (p.has("dm") && !p.has("dedisperse"))
        throw RPFexception("Option --dm needs --dedisperse: it lists the dispersion measures that one tries. Exiting.",
                           ReturnValue::InvalidArgument);
    for (const char* name : {"fold", "phase-bins"})
        if (p.has(name) && !p.has("dedisperse"))
            throw RPFexception(std::string("Option --") + name + " needs --dedisperse: it folds the DM-time plane that one builds. Exiting.",
                               ReturnValue::InvalidArgument);
    if (replay_mode("dedisperse", p, o)) {
        if (o.baseline) refuse("dedisperse", "does not combine with --baseline (-B): the power is in units of every bin's median.");
        if (!p.has("dm")) refuse("dedisperse", "needs --dm: the dispersion measures to try, one value or lo:hi:step.");
        o.dms = parse_trial_list(p.get("dm"), "dm", "one dispersion measure");
        if (p.has("fold")) {
            o.fold_periods = parse_trial_list(p.get("fold"), "fold", "one period in seconds");
            o.phase_bins = p.has("phase-bins") ? to_number<int64_t>(*find_spec("--phase-bins"), p.get("phase-bins")) : 16;
            if (o.phase_bins < 1 || o.phase_bins > 128)
                refuse("dedisperse", "takes 1 to 128 phase bins in --phase-bins, got " + std::to_string(o.phase_bins) + ".");
            const long long cells = static_cast<long long>(o.dms.size()) * static_cast<long long>(o.fold_periods.size()) * o.phase_bins;
            if (cells > (1LL << 24))
                refuse("dedisperse", "folds at most 16777216 cells (DMs x periods x phase bins) in one run, got " + std::to_string(cells) + ".");
        } else if (p.has("phase-bins")) {
            throw RPFexception("Option --phase-bins needs --fold: it is the number of phase bins of the folded profiles. Exiting.",
                               ReturnValue::InvalidArgument);
        }
    }
    if (p.has("input")) o.input_file = p.get("input");
    o.synthetic = p.has("synthetic");
    if (p.has("synthetic")) o.synthetic_seed = static_cast<uint64_t>(to_number<int64_t>(*find_spec("--synthetic"), p.get("synthetic")));
    return o;
}

}  // namespace rpf_host
