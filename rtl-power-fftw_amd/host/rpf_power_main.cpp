// rpf_power -- the rtl_power_fftw program (/root/reference/src/rtl_power_fftw.cxx:50-233)
// on top of the MI355X engine: same command line, same stderr chatter, same
// gnuplot-compatible stdout / binary-matrix output, same exit codes.  The dongle
// is replaced by a replayed or synthetic byte stream (sample_source.h).
//
// One device (--gpu k, the default): the reference's loop, one acquisition after
// the other (rtl_power_fftw.cxx:132-205).
// Several devices (--gpus a,b,...): single process, one engine, one
// sample source and one producer thread per device.  The hops of a pass are dealt
// hop-major to the devices in contiguous frame-aligned ranges (frame k of the pass
// -> device floor(k G / (hops R)): whole hops when G divides the hop count, frame
// ranges of a hop otherwise); the main thread adds a hop's per-device accumulators
// in device order (fixed order: reproducible) and writes the spectra in hop order,
// so stdout is what one device would have printed.
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <memory>
#include <mutex>
#include <sstream>
#include <thread>

#include "acquisition.h"
#include "aux_data.h"
#include "datastore.h"
#include "interrupts.h"
#include "options.h"
#include "piece_reader.h"
#include "sample_source.h"
#include "scan_plan.h"

using namespace rpf_host;

namespace {

bool chatty(const Options& o) { return !o.talkless || o.outcnt == 0; }

void write_metadata(const Options& o, const ScanMetadata& m, int64_t repeats_done, int samplerate)
{
    // rtl_power_fftw.cxx:207-220; example in doc/rtl_power_fftw.1.md:186-194
    std::ofstream meta(o.meta_file, std::ios::out | std::ios::trunc);
    meta << m.metaCols << " # frequency bins (columns)" << std::endl;
    meta << (m.metaRows - 1) << " # scans (rows)" << std::endl;
    meta << m.startFreq << " # startFreq (Hz)" << std::endl;
    meta << m.endFreq << " # endFreq (Hz)" << std::endl;
    meta << m.stepFreq << " # stepFreq (Hz)" << std::endl;
    meta << static_cast<double>(o.N) * repeats_done / samplerate << " # effective integration time secs" << std::endl;
    meta << m.avgScanDur << " # avgScanDur (sec)" << std::endl;
    meta << m.firstAcqTimestamp << " # firstAcqTimestamp UTC" << std::endl;
    meta << m.lastAcqTimestamp << " # lastAcqTimestamp UTC" << std::endl;
}

void note_scan_extent(const Options& options, const Plan& plan, int actual_samplerate, ScanMetadata& meta)
{
    meta.tunfreq = static_cast<int>(plan.freqs_to_tune.front());
    meta.startFreq = static_cast<int>(meta.tunfreq + (0 - options.N / 2.0) * actual_samplerate / options.N);
    meta.tunfreq = static_cast<int>(plan.freqs_to_tune.back());
    meta.endFreq = static_cast<int>(meta.tunfreq + ((options.N - 1) - options.N / 2.0) * actual_samplerate / options.N);
    meta.stepFreq = actual_samplerate / options.N;
}

// ---- several devices --------------------------------------------------------------------
struct DeviceJob {
    int hop = 0;        // index into the pass's hop list
    int part = 0;       // index into that hop's parts
    Shard shard;
};

struct HopPart {
    std::vector<double> pwr;
    int64_t repeats_done = 0, device_readouts = 0, successful_readouts = 0, tuned_freq = 0;
    std::string start_stamp, end_stamp;
    int device_slot = 0;
    bool done = false;
};

// Frame ranges of one pass (hops x repeats frames) for device slot d of G -- the same
// partition as rtl-power-fftw_amd/sharding.py: shard_hops().
std::vector<DeviceJob> device_jobs(int hops, int64_t repeats, int G, int d, std::vector<int>& parts_per_hop)
{
    const int64_t total = static_cast<int64_t>(hops) * repeats;
    int64_t pos = (total * d + G - 1) / G;
    const int64_t end = (total * (d + 1) + G - 1) / G;
    std::vector<DeviceJob> jobs;
    while (pos < end) {
        DeviceJob job;
        job.hop = static_cast<int>(pos / repeats);
        job.shard.first_frame = pos - job.hop * repeats;
        job.shard.repeats = std::min(repeats - job.shard.first_frame, end - pos);
        job.part = parts_per_hop[job.hop]++;
        jobs.push_back(job);
        pos += job.shard.repeats;
    }
    return jobs;
}

// Bytes one hop takes out of a sequential replay (the producer's reads are rounded up to
// whole 16384-byte transfers, acquisition.cxx:288-300).
uint64_t replay_bytes_per_hop(const Options& options)
{
    const int64_t total = options.frame_span(options.repeats);
    int64_t read = 0;
    while (read < total) read += next_read_size(total, read, options.buf_length);
    return static_cast<uint64_t>(read);
}

class MultiDeviceScan {
public:
    MultiDeviceScan(Options& options, AuxData& aux, SampleSource& source, int actual_samplerate)
        : options_(options), aux_(aux), rate_(actual_samplerate)
    {
        for (size_t d = 0; d < options.devices.size(); ++d) {
            std::unique_ptr<SampleSource> s = source.clone();
            if (!s)
                throw RPFexception("--gpus with several devices needs a source every device can read on its own: "
                                   "--synthetic <seed> or a seekable --input <file> (not stdin, not a dongle).",
                                   ReturnValue::InvalidArgument);
            sources_.push_back(std::move(s));
            stores_.emplace_back(new Datastore(options, aux.window_values, options.devices[d]));
        }
        bytes_per_hop_ = replay_bytes_per_hop(options);
    }
    ~MultiDeviceScan() { rpf_scan_reducer_destroy(reducer_); }

    // north_star / SURVEY.md 8e: the per-device accumulators of a pass meet in ONE RCCL reduce onto the
    // first device (rpf_scan_reducer_*: ncclCommInitAll over the listed devices, librccl loaded with
    // dlopen).  Without RCCL, or with a device list it refuses (the same device twice), the main thread
    // adds them itself in device order -- the same sums up to the order of the additions.
    void prepare_reduce(int max_hops)
    {
        if (options_.reduce == "host" || reducer_ || reducer_tried_) return;
        reducer_tried_ = true;
        int rc = rpf_scan_reducer_create(options_.devices.data(), static_cast<int>(options_.devices.size()), options_.N,
                                         max_hops, &reducer_);
        if (rc != RPF_OK) {
            reducer_ = nullptr;
            if (options_.reduce == "rccl")
                throw RPFexception(std::string("--reduce rccl: ") + rpf_scan_reducer_last_error(nullptr), (ReturnValue)rc);
            if (chatty(options_))
                std::cerr << "RCCL reduce not available (" << rpf_scan_reducer_last_error(nullptr)
                          << "); adding the per-device spectra on the host." << std::endl;
        } else if (chatty(options_)) {
            std::cerr << "Per-device spectra are reduced over RCCL onto gpu " << options_.devices.front() << "." << std::endl;
        }
        reducer_hops_ = max_hops;
    }

    // One pass over `freqs`; spectra to stdout / the matrix file in hop order.  Returns
    // false when the pass was cut short (interrupt, exhausted replay).
    bool run_pass(const std::vector<int64_t>& freqs, ScanMetadata& meta, bool& meta_pending, const Plan& plan,
                  int64_t& last_repeats_done)
    {
        const int H = static_cast<int>(freqs.size()), G = static_cast<int>(stores_.size());
        std::vector<int> parts_per_hop(H, 0);
        std::vector<std::vector<DeviceJob>> jobs(G);
        for (int d = 0; d < G; ++d) jobs[d] = device_jobs(H, options_.repeats, G, d, parts_per_hop);
        std::vector<std::vector<HopPart>> parts(H);
        for (int h = 0; h < H; ++h) parts[h].resize(parts_per_hop[h]);
        for (int d = 0; d < G; ++d)
            for (DeviceJob& j : jobs[d]) {
                j.shard.hop_base = pass_base_ + static_cast<uint64_t>(j.hop) * bytes_per_hop_;
                parts[j.hop][j.part].device_slot = d;
            }

        prepare_reduce(H);
        const bool rccl = reducer_ && H <= reducer_hops_;
        if (rccl && rpf_scan_reducer_begin(reducer_) != RPF_OK)
            throw RPFexception(rpf_scan_reducer_last_error(reducer_), ReturnValue::HardwareError);
        std::vector<double> reduced;                 // rccl: hops x N, filled once every worker has finished

        std::mutex mutex;
        std::condition_variable progress;
        std::string error;
        ReturnValue error_code = ReturnValue::Success;
        std::vector<std::thread> workers;
        std::atomic<bool> cancel(false);       // a worker failed or the pass was cut short: start no further job
        // whatever leaves this scope -- the return at the end or an exception in between -- joins the workers first
        struct JoinAll {
            std::vector<std::thread>& threads;
            std::atomic<bool>& cancel;
            ~JoinAll()
            {
                cancel.store(true);
                for (std::thread& w : threads)
                    if (w.joinable()) w.join();
            }
        } join_all{workers, cancel};
        finished_workers_ = 0;
        for (int d = 0; d < G; ++d)
            workers.emplace_back([&, d]() {
                ScanMetadata unused;
                try {
                    for (const DeviceJob& j : jobs[d]) {
                        if (cancel.load()) break;
                        Acquisition acq(options_, aux_, *sources_[d], *stores_[d], unused, rate_, freqs[j.hop], j.shard);
                        acq.run();
                        if (rccl && stores_[d]->repeats_done > 0 &&
                            rpf_scan_reducer_deposit(reducer_, d, j.hop, stores_[d]->engine()) != RPF_OK)
                            throw RPFexception(rpf_scan_reducer_last_error(reducer_), ReturnValue::HardwareError);
                        std::lock_guard<std::mutex> lock(mutex);
                        HopPart& p = parts[j.hop][j.part];
                        if (!rccl) p.pwr = stores_[d]->pwr;
                        p.repeats_done = stores_[d]->repeats_done;
                        p.device_readouts = acq.device_readouts();
                        p.successful_readouts = acq.successful_readouts();
                        p.tuned_freq = acq.tuned_freq();
                        p.start_stamp = acq.start_stamp();
                        p.end_stamp = acq.end_stamp();
                        p.done = true;
                        progress.notify_all();
                        if (interrupts.load() >= static_cast<int>(InterruptState::FinishNow)) break;
                    }
                } catch (const std::exception& e) {
                    std::lock_guard<std::mutex> lock(mutex);
                    if (error.empty()) {
                        error = e.what();
                        const RPFexception* r = dynamic_cast<const RPFexception*>(&e);
                        error_code = r ? r->returnValue() : ReturnValue::AcquisitionError;
                    }
                    cancel.store(true);
                    progress.notify_all();
                }
                std::lock_guard<std::mutex> lock(mutex);
                finished_workers_++;
                progress.notify_all();
            });

        bool complete = true;
        const std::vector<double>* baseline = options_.baseline ? &aux_.baseline_values : nullptr;
        time_t hop_begin = std::time(nullptr);
        if (meta.cntTimeStamps == 0) {
            meta.firstAcqTimestamp = Acquisition::utc_now();
            meta.cntTimeStamps++;
        }
        if (rccl) {
            // the reduce needs every device's block: wait for the workers, then ONE ncclReduce + one D2H
            {
                std::unique_lock<std::mutex> lock(mutex);
                progress.wait(lock, [&]() { return finished_workers_ == G; });
            }
            // a failed worker: nothing was reduced, so nothing may be written (the loop below would
            // otherwise copy hop rows out of the empty `reduced`); JoinAll joins the workers
            if (!error.empty()) throw RPFexception(error, error_code);
            reduced.assign(static_cast<size_t>(H) * options_.N, 0.0);
            if (rpf_scan_reducer_reduce(reducer_, H, reduced.data()) != RPF_OK)
                throw RPFexception(rpf_scan_reducer_last_error(reducer_), ReturnValue::HardwareError);
        }
        for (int h = 0; h < H && complete; ++h) {
            {
                std::unique_lock<std::mutex> lock(mutex);
                auto ready = [&]() {
                    for (const HopPart& p : parts[h])
                        if (!p.done) return false;
                    return true;
                };
                progress.wait(lock, [&]() { return ready() || !error.empty() || finished_workers_ == G; });
                if (!ready()) {
                    complete = false;
                    break;
                }
            }
            // the hop's accumulator: per-device partial sums added in device order
            std::vector<double> pwr(options_.N, 0.0);
            int64_t repeats_done = 0, readouts = 0, successful = 0;
            if (rccl) std::copy(reduced.begin() + static_cast<size_t>(h) * options_.N,
                                reduced.begin() + static_cast<size_t>(h + 1) * options_.N, pwr.begin());
            for (const HopPart& p : parts[h]) {
                if (!rccl)
                    for (int i = 0; i < options_.N; ++i) pwr[i] += p.pwr[i];
                repeats_done += p.repeats_done;
                readouts += p.device_readouts;
                successful += p.successful_readouts;
            }
            const HopPart& first = parts[h].front();
            const HopPart& last = parts[h].back();
            if (chatty(options_)) {
                std::cerr << "Tuning to " << freqs[h] << " Hz (" << parts[h].size() << " device"
                          << (parts[h].size() == 1 ? "" : "s") << ", first: gpu "
                          << options_.devices[first.device_slot] << ")" << std::endl;
                std::cerr << "Device tuned to: " << first.tuned_freq << " Hz" << std::endl;
                std::cerr << "Acquisition started at " << first.start_stamp << std::endl;
                std::cerr << "Acquisition done at " << last.end_stamp << std::endl;
                print_acquisition_summary(options_.N, repeats_done, readouts, successful, rate_);
            }
            time_t now = std::time(nullptr);
            meta.scanBeg = hop_begin;
            meta.scanEnd = now;
            meta.lastAcqTimestamp = Acquisition::utc_now();
            meta.sumScanDur += static_cast<float>(std::difftime(now, hop_begin));
            meta.avgScanDur = meta.sumScanDur / meta.metaRows;
            hop_begin = now;
            last_repeats_done = repeats_done;
            if (repeats_done == 0) {
                std::cerr << "No complete spectrum at " << freqs[h] << " Hz (input exhausted); nothing written."
                          << std::endl;
                complete = false;
                break;
            }
            if (options_.matrixMode && meta_pending) {
                note_scan_extent(options_, plan, rate_, meta);
                meta_pending = false;
            }
            if (!options_.matrixMode) {
                write_text_header(std::cout, first.start_stamp, last.end_stamp);
                write_spectrum_text(std::cout, pwr, options_.N, repeats_done, first.tuned_freq, rate_,
                                    options_.linear, baseline);
            } else {
                append_matrix_row(options_, meta, pwr, repeats_done, first.tuned_freq, rate_, baseline);
            }
            hops_written_++;
            if (chatty(options_))
                for (const HopPart& p : parts[h]) {
                    std::cerr << "gpu " << options_.devices[p.device_slot] << ": ";
                    stores_[p.device_slot]->printQueueHistogram();
                }
            if (checkInterrupt(InterruptState::FinishNow)) complete = false;
        }
        if (!complete) cancel.store(true);
        for (std::thread& w : workers) w.join();
        if (!error.empty()) throw RPFexception(error, error_code);
        pass_base_ += static_cast<uint64_t>(H) * bytes_per_hop_;
        for (const auto& s : sources_)
            if (s->exhausted()) exhausted_ = true;
        return complete;
    }

    bool exhausted() const { return exhausted_; }
    int64_t hops_written() const { return hops_written_; }

private:
    Options& options_;
    AuxData& aux_;
    int rate_;
    std::vector<std::unique_ptr<SampleSource>> sources_;
    std::vector<std::unique_ptr<Datastore>> stores_;
    uint64_t bytes_per_hop_ = 0, pass_base_ = 0;
    int finished_workers_ = 0;
    rpf_scan_reducer* reducer_ = nullptr;
    bool reducer_tried_ = false;
    int reducer_hops_ = 0;
    bool exhausted_ = false;
    int64_t hops_written_ = 0;
};

// ---- the replay modes -------------------------------------------------------------------
struct NoSpectrum : RPFexception {
    NoSpectrum() : RPFexception("No complete spectrum could be acquired (input too short?).", ReturnValue::AcquisitionError) {}
};

// The loop of every replay mode over the pieces of its input (piece_reader.h; two readers: a piece of each at a time):
// fill, step(the bytes the shorter holds) -> the integrations it credits, consume them on every reader; until a step
// credits nothing, a reader has less than one integration left or Ctrl-C.  Returns the integrations credited in all and
// throws NoSpectrum if that is none.  held (if given): what each reader held when last filled -- once more after the
// last piece, so what is left of each input once the last common integration is taken.
template <class Step>
int64_t replay_pieces(const std::vector<PieceReader*>& in, Step step, size_t* held = nullptr)
{
    auto fill = [&]() {
        size_t have = SIZE_MAX;
        for (size_t r = 0; r < in.size(); ++r) {
            const size_t got = in[r]->fill();
            if (held) held[r] = got;
            have = std::min(have, got);
        }
        return have;
    };
    int64_t total = 0;
    set_CtrlC_handler(true);
    while (!checkInterrupt(InterruptState::FinishNow)) {
        const int64_t done = step(fill());
        if (done == 0) break;
        total += done;
        bool more = true;
        for (PieceReader* reader : in) more = reader->consume(done) && more;
        if (!more) {
            fill();
            break;
        }
    }
    if (total == 0) throw NoSpectrum();
    return total;
}

// --series <frames>: the replay cut into consecutive integrations of <frames> frames (rpf_accumulate_series), one text
// block per integration -- what `-c -n <frames> --input` writes, block for block, without an acquisition per block.
// The file is read in pieces of whole spectra (64 MB, or one spectrum if that is larger) with the bytes two pieces share
// carried over: piece_reader.h.
// --series-stats <frames> (options.series_stats): the same through rpf_accumulate_series_stats, every block with the
// --stats columns for M = <frames> -- what `--stats -c -n <frames> --input` writes.
int run_series(const Options& options, AuxData& aux, int actual_samplerate, int64_t tuned_freq)
{
    Datastore data(options, aux.window_values);
    const int64_t L = options.series_frames;
    PieceReader in(options.input_file, options.sample_bytes() * options.N, options.sample_bytes() * options.step(), L);
    const std::vector<double>* baseline = options.baseline ? &aux.baseline_values : nullptr;
    std::vector<double> rows, pwr(options.N), sum_sq, peak;
    const bool stats = options.series_stats;
    const size_t row = static_cast<size_t>(stats ? 3 : 1) * options.N;
    if (stats) {
        sum_sq.resize(options.N);
        peak.resize(options.N);
    }
    int64_t written = 0;
    auto report = [&]() {
        if (!chatty(options)) return;
        std::cerr << "Spectra written: " << written << ", " << L << " frames each ("
                  << (data.series_launches() == 1 ? "one launch per piece" : "one launch per spectrum") << ")" << std::endl;
        print_acquisition_summary(options.N, written * L, 0, 0, actual_samplerate);
    };
    std::string start_stamp = Acquisition::utc_now();      // (of every piece: from before it is read)
    try {
        written = replay_pieces({&in}, [&](size_t have) {
            const int64_t done = stats ? data.accumulate_series_stats(in.data(), have, L, in.per_piece(), rows)
                                       : data.accumulate_series(in.data(), have, L, in.per_piece(), rows);
            const std::string end_stamp = Acquisition::utc_now();
            for (int64_t k = 0; k < done; ++k) {
                const auto at = rows.begin() + static_cast<size_t>(k) * row;
                std::copy(at, at + options.N, pwr.begin());
                write_text_header(std::cout, start_stamp, end_stamp, stats);
                if (stats) {
                    std::copy(at + options.N, at + 2 * options.N, sum_sq.begin());
                    std::copy(at + 2 * options.N, at + 3 * options.N, peak.begin());
                    write_spectrum_text_stats(std::cout, pwr, sum_sq, peak, options.N, L, tuned_freq, actual_samplerate,
                                              options.linear, baseline);
                } else {
                    write_spectrum_text(std::cout, pwr, options.N, L, tuned_freq, actual_samplerate, options.linear, baseline);
                }
                std::cout << std::endl;          // (the blank line that closes a pass of -c)
            }
            start_stamp = Acquisition::utc_now();
            return done;
        });
    } catch (NoSpectrum&) {
        report();                                // (said of an input too short as well, before the refusal)
        throw;
    }
    report();
    return 0;
}

// --excise <frames>: the replay's average with the integrations that carried interference left out, bin by bin
// (rpf_accumulate_excised; thresholds sk_limits(<frames>, --excise-sigma)), ONE block for the file.  The file is read in
// pieces of whole integrations as run_series reads it; every piece leaves clean, kept and total of its integrations,
// and the pieces' results are added here in file order.
int run_excise(const Options& options, AuxData& aux, int actual_samplerate, int64_t tuned_freq)
{
    Datastore data(options, aux.window_values);
    const int64_t L = options.excise_frames;
    PieceReader in(options.input_file, options.sample_bytes() * options.N, options.sample_bytes() * options.step(), L);
    double sk_lo = 0, sk_hi = 0;
    sk_limits(L, options.excise_sigma, sk_lo, sk_hi);
    const size_t N = static_cast<size_t>(options.N);
    std::vector<double> piece, clean(N, 0.0), kept(N, 0.0), total(N, 0.0);
    const std::string start_stamp = Acquisition::utc_now();
    const int64_t K = replay_pieces({&in}, [&](size_t have) {
        const int64_t done = data.accumulate_excised(in.data(), have, L, in.per_piece(), sk_lo, sk_hi, piece);
        for (size_t i = 0; done > 0 && i < N; ++i) {
            clean[i] += piece[i];
            kept[i] += piece[N + i];
            total[i] += piece[2 * N + i];
        }
        return done;
    });
    const std::string end_stamp = Acquisition::utc_now();
    write_text_header_excised(std::cout, start_stamp, end_stamp);
    write_spectrum_text_excised(std::cout, clean, kept, total, options.N, K, L, tuned_freq, actual_samplerate, options.linear,
                                options.baseline ? &aux.baseline_values : nullptr);
    std::cout << std::endl;          // (the blank line that closes a pass)
    double flagged = 0;
    for (size_t i = 0; i < N; ++i) flagged += static_cast<double>(K) - kept[i];
    const double pairs = static_cast<double>(K) * static_cast<double>(N);
    std::cerr << "Excised: " << static_cast<int64_t>(flagged) << " of " << static_cast<int64_t>(pairs)
              << " (integration, bin) pairs flagged (" << 100.0 * flagged / pairs << " %), " << K << " integrations of " << L
              << " frames, spectral kurtosis kept in [" << sk_lo << ", " << sk_hi << "]" << std::endl;
    if (chatty(options)) print_acquisition_summary(options.N, K * L, 0, 0, actual_samplerate);
    return 0;
}

// What --quantile and --dedisperse say when the replay holds more integrations than the engine's row store keeps.
[[noreturn]] static void refuse_more_rows(int64_t max_rows, int64_t L, int N)
{
    throw RPFexception("Option --quantile: the input holds more than " + std::to_string(max_rows) + " integrations of " +
                       std::to_string(L) + " frames, which is what the device keeps of " + std::to_string(N) +
                       " bins (1 GiB of rows): raise <frames>. Exiting.", ReturnValue::InvalidArgument);
}

// --quantile <frames> [--quantiles a,b,...]: every bin's quantiles over the replay's integrations of <frames> frames
// (rpf_quantile_append per piece, ONE rpf_quantile_select at the end), one block for the file.  The file is read in
// pieces of whole integrations as run_series reads it; the rows stay in the engine's store on the device.
int run_quantile(const Options& options, AuxData& aux, int actual_samplerate, int64_t tuned_freq)
{
    Datastore data(options, aux.window_values);
    const int64_t L = options.quantile_frames;
    PieceReader in(options.input_file, options.sample_bytes() * options.N, options.sample_bytes() * options.step(), L);
    int64_t kept = 0;
    bool one_launch = true;
    const std::string start_stamp = Acquisition::utc_now();
    data.quantile_reset();
    const int64_t K = replay_pieces({&in}, [&](size_t have) {
        const int64_t coming = std::min(in.per_piece(), options.frames_in(static_cast<int64_t>(have)) / L);
        if (kept + coming > data.quantile_max_rows())
            refuse_more_rows(data.quantile_max_rows(), L, options.N);
        const int64_t done = data.quantile_append(in.data(), have, L, in.per_piece());
        one_launch = one_launch && (done == 0 || data.series_launches() == 1);
        kept += done;
        return done;
    });
    std::vector<double> planes;
    data.quantile_select(options.quantiles, planes);
    const std::string end_stamp = Acquisition::utc_now();
    write_text_header_quantiles(std::cout, start_stamp, end_stamp, options.quantiles);
    write_spectrum_text_quantiles(std::cout, planes, options.quantiles, options.N, L, tuned_freq, actual_samplerate,
                                  options.linear, options.baseline ? &aux.baseline_values : nullptr);
    std::cout << std::endl;          // (the blank line that closes a pass)
    std::cerr << "Quantiles: " << options.quantiles.size() << " of " << K << " integrations of " << L << " frames ("
              << (one_launch ? "one launch per piece" : "one launch per spectrum") << ")" << std::endl;
    if (chatty(options)) print_acquisition_summary(options.N, K * L, 0, 0, actual_samplerate);
    return 0;
}

// The median of v (the mean of the two middle values for an even count); v is reordered.
static double median_of(std::vector<double>& v)
{
    const size_t n = v.size(), h = n / 2;
    std::nth_element(v.begin(), v.begin() + h, v.end());
    const double hi = v[h];
    return n % 2 ? hi : (*std::max_element(v.begin(), v.begin() + h) + hi) / 2;
}

// --dedisperse <frames> --dm <lo:hi:step | value>: the DM-time plane of the replay's integrations of <frames> frames.  The
// file is appended to the engine's row store piece by piece as run_quantile does; then ONE rpf_quantile_select(0.5) gives
// every bin's median, the weights are w[b] = 1 / median[b] (0 for the DC bin and for a bin whose median is 0), and ONE
// rpf_dedisperse adds the bins along every trial's delay curve (dm_delays).  One block per trial: time and the mean of the
// summed bins in units of their medians.
// With --fold <period | lo:hi:step> [--phase-bins <n>], ONE rpf_dedisperse_fold takes the place of that rpf_dedisperse: the
// plane stays on the device and is folded there at every trial period (period_steps); fold_chi2 then gives the search
// plane, block 1, and the strongest cell's profile is block 2.
int run_dedisperse(const Options& options, AuxData& aux, int actual_samplerate, int64_t tuned_freq)
{
    const int64_t L = options.dedisperse_frames;
    const bool folding = !options.fold_periods.empty();
    std::vector<uint64_t> steps;
    if (folding) {
        const double t_row = (static_cast<double>(L) * static_cast<double>(options.step())) / static_cast<double>(actual_samplerate);
        for (double period : options.fold_periods)
            if (!(period / t_row >= 2.0)) {
                std::ostringstream why;
                why << std::setprecision(9) << "Option --dedisperse: the period " << period << " s of --fold is under two integrations of "
                    << L << " frames (" << t_row << " s each): the shortest period that works is " << 2.0 * t_row << " s. Exiting.";
                throw RPFexception(why.str(), ReturnValue::InvalidArgument);
            }
        steps = period_steps(options.fold_periods, static_cast<double>(actual_samplerate), options.N, L, options.step());
    }
    Datastore data(options, aux.window_values);
    const size_t N = static_cast<size_t>(options.N), D = options.dms.size();
    const std::vector<int32_t> delays = dm_delays(options.dms, static_cast<double>(tuned_freq), static_cast<double>(actual_samplerate),
                                                  options.N, L, options.step());
    PieceReader in(options.input_file, options.sample_bytes() * options.N, options.sample_bytes() * options.step(), L);
    int64_t kept = 0;
    const std::string start_stamp = Acquisition::utc_now();
    data.quantile_reset();
    const int64_t K = replay_pieces({&in}, [&](size_t have) {
        const int64_t coming = std::min(in.per_piece(), options.frames_in(static_cast<int64_t>(have)) / L);
        if (kept + coming > data.quantile_max_rows())
            refuse_more_rows(data.quantile_max_rows(), L, options.N);
        const int64_t done = data.quantile_append(in.data(), have, L, in.per_piece());
        kept += done;
        return done;
    });
    std::vector<double> median, weights(N, 0.0), plane;
    data.quantile_select(std::vector<double>(1, 0.5), median);
    int64_t nb = 0;
    for (size_t b = 0; b < N; ++b) {
        if (b != N / 2 && median[b] != 0.0) weights[b] = 1.0 / median[b];
        nb += weights[b] != 0.0;
    }
    if (nb == 0)
        throw RPFexception("Option --dedisperse: every bin but DC has a median of 0, so no bin is left to add. Exiting.",
                           ReturnValue::InvalidInput);
    if (folding) {
        const size_t P = steps.size(), NB = static_cast<size_t>(options.phase_bins);
        std::vector<double> prof, mom;
        std::vector<int32_t> hits;
        const int64_t T = data.dedisperse_fold(delays, weights, steps, options.phase_bins, prof, hits, mom);
        const std::string end_stamp = Acquisition::utc_now();
        const std::vector<double> chi2 = fold_chi2(prof, hits, mom, D, P, NB, T);
        size_t best = chi2.size();          // the strongest cell: the first of the largest values that are not NaN
        for (size_t i = 0; i < chi2.size(); ++i)
            if (!std::isnan(chi2[i]) && (best == chi2.size() || chi2[i] > chi2[best])) best = i;
        write_text_fold_plane(std::cout, start_stamp, end_stamp, options.dms, options.fold_periods, options.phase_bins, T, chi2);
        std::cerr << "Folded: " << K << " integrations of " << L << " frames, " << T << " times of " << D << " trials at " << P
                  << " periods";
        if (best < chi2.size()) {
            const size_t d = best / P, p = best % P;
            write_text_fold_profile(std::cout, start_stamp, end_stamp, options.dms[d], options.fold_periods[p], chi2[best],
                                    prof.data() + best * NB, hits.data() + p * NB, options.phase_bins, nb, options.linear);
            std::cerr << "; strongest cell: DM " << options.dms[d] << " (trial " << d << "), period " << std::setprecision(9)
                      << options.fold_periods[p] << std::setprecision(6) << " s (trial " << p << "), reduced chi2 " << chi2[best];
        }
        std::cout << std::endl;          // (the blank line that closes a pass)
        std::cerr << std::endl;
        if (chatty(options)) print_acquisition_summary(options.N, K * L, 0, 0, actual_samplerate);
        return 0;
    }
    const int64_t T = data.dedisperse(delays, weights, plane);
    const std::string end_stamp = Acquisition::utc_now();
    // the strongest sample in robust sigmas of its own trial: (x - median) / (1.4826 MAD), dedisperse.py's snr
    double best = -1;
    size_t best_d = 0;
    int64_t best_t = 0;
    for (size_t d = 0; d < D; ++d) {
        const double* trial = plane.data() + d * static_cast<size_t>(T);
        write_text_header_dedisperse(std::cout, start_stamp, end_stamp, options.dms[d],
                                     *std::max_element(delays.begin() + d * N, delays.begin() + (d + 1) * N));
        write_text_dedisperse(std::cout, trial, T, nb, L, options.step(), actual_samplerate, options.linear);
        if (T < 1) continue;
        std::vector<double> v(trial, trial + T);
        const double med = median_of(v);
        for (double& x : v) x = std::fabs(x - med);
        const double scale = 1.4826 * median_of(v);
        for (int64_t t = 0; t < T; ++t) {
            const double s = (trial[t] - med) / scale;
            if (s > best) {
                best = s;
                best_d = d;
                best_t = t;
            }
        }
    }
    std::cout << std::endl;          // (the blank line that closes a pass)
    std::cerr << "Dedispersed: " << K << " integrations of " << L << " frames, " << T << " times of " << D << " trials";
    if (T > 0 && best >= 0)
        std::cerr << "; strongest sample: DM " << options.dms[best_d] << " (trial " << best_d << ") at "
                  << static_cast<double>(best_t * L * options.step()) / actual_samplerate << " s, snr " << best;
    std::cerr << std::endl;
    if (chatty(options)) print_acquisition_summary(options.N, K * L, 0, 0, actual_samplerate);
    return 0;
}

// --input a --cross b: the cross-spectrum of the two replays (rpf_accumulate_cross) over the whole frames of the shorter,
// ONE block for the pair: power of a, power of b, coherence, phase.  Both files are read in pieces of whole frames
// (piece_reader.h with one frame per integration), a piece of each at a time; every pair of pieces leaves its four
// planes -- sums over its frames, so the pieces' planes are added here in file order.
int run_cross(const Options& options, AuxData& aux, int actual_samplerate, int64_t tuned_freq)
{
    Datastore data(options, aux.window_values);
    const size_t b = static_cast<size_t>(options.sample_bytes());
    PieceReader in_a(options.input_file, b * options.N, b * options.step(), 1);
    PieceReader in_b(options.cross_file, b * options.N, b * options.step(), 1);
    const size_t N = static_cast<size_t>(options.N);
    std::vector<double> piece, planes(4 * N, 0.0);
    size_t left[2] = {0, 0};
    const std::string start_stamp = Acquisition::utc_now();
    const int64_t frames = replay_pieces({&in_a, &in_b}, [&](size_t have) {
        const int64_t done = data.accumulate_cross(in_a.data(), in_b.data(), have / b * b, in_a.per_piece(), piece);
        for (size_t i = 0; done > 0 && i < 4 * N; ++i) planes[i] += piece[i];
        return done;
    }, left);
    const std::string end_stamp = Acquisition::utc_now();
    write_text_header_cross(std::cout, start_stamp, end_stamp);
    write_spectrum_text_cross(std::cout, planes, options.N, frames, tuned_freq, actual_samplerate, options.linear,
                              options.baseline ? &aux.baseline_values : nullptr);
    std::cout << std::endl;          // (the blank line that closes a pass)
    // what is left of each file once the last common frame is taken: the same unless the lengths differ
    std::cerr << "Cross-spectrum: " << frames << " frames of " << options.N << " bins from each stream"
              << (left[0] != left[1] ? " (the files differ in length: the whole frames of the shorter are used)" : "") << std::endl;
    if (chatty(options)) print_acquisition_summary(options.N, frames, 0, 0, actual_samplerate);
    return 0;
}

// --input a --correlate b,c,...: the visibilities of the M replays (rpf_correlate) over the whole frames of the shortest,
// ONE block: the power of every stream, then coherence and phase of every pair i < j.  Every file is read in pieces of
// whole frames (piece_reader.h with one frame per integration), a piece of each at a time; every set of pieces leaves
// its visibilities -- sums over its frames, so the pieces' are added here in file order.
int run_correlate(const Options& options, AuxData& aux, int actual_samplerate, int64_t tuned_freq)
{
    Datastore data(options, aux.window_values);
    const size_t b = static_cast<size_t>(options.sample_bytes());
    std::vector<std::unique_ptr<PieceReader>> readers;
    readers.emplace_back(new PieceReader(options.input_file, b * options.span_samples(), b * options.step(), 1));
    for (const std::string& f : options.correlate_files)
        readers.emplace_back(new PieceReader(f, b * options.span_samples(), b * options.step(), 1));
    const size_t M = readers.size(), N = static_cast<size_t>(options.N);
    std::vector<PieceReader*> in;
    std::vector<const uint8_t*> streams;
    for (auto& r : readers) {
        in.push_back(r.get());
        streams.push_back(r->data());
    }
    std::vector<double> piece, vis(2 * M * M * N, 0.0);
    std::vector<size_t> left(M, 0);
    const std::string start_stamp = Acquisition::utc_now();
    const int64_t frames = replay_pieces(in, [&](size_t have) {
        const int64_t done = data.correlate(streams, have / b * b, in[0]->per_piece(), piece);
        for (size_t i = 0; done > 0 && i < vis.size(); ++i) vis[i] += piece[i];
        return done;
    }, left.data());
    const std::string end_stamp = Acquisition::utc_now();
    write_text_header_correlate(std::cout, start_stamp, end_stamp, static_cast<int>(M));
    write_spectrum_text_correlate(std::cout, vis, static_cast<int>(M), options.N, frames, tuned_freq, actual_samplerate,
                                  options.linear, options.baseline ? &aux.baseline_values : nullptr);
    std::cout << std::endl;          // (the blank line that closes a pass)
    // what is left of each file once the last common frame is taken: the same unless the lengths differ
    bool differ = false;
    for (size_t m = 1; m < M; ++m) differ = differ || left[m] != left[0];
    std::cerr << "Correlator: " << frames << " frames of " << options.N << " bins from each of " << M << " streams"
              << (differ ? " (the files differ in length: the whole frames of the shortest are used)" : "") << std::endl;
    if (chatty(options)) print_acquisition_summary(options.N, frames, 0, 0, actual_samplerate);
    return 0;
}

// --input a --stft out: the complex spectrum of every frame of the replay (rpf_stft), raw little-endian float32 pairs,
// frame after frame, into `out`; nothing on stdout.  The file is read in pieces of whole frames that keep the input AND the
// rows a piece leaves within the budget (piece_reader.h with one frame per integration and the row cap of stft_pieces),
// the bytes neighbouring pieces share carried over.
int run_stft(const Options& options, AuxData& aux, int actual_samplerate)
{
    Datastore data(options, aux.window_values);
    const size_t b = static_cast<size_t>(options.sample_bytes());
    // (the frames of a piece by the engine's own rule: csrc/series_pieces.h, stft_pieces)
    const int64_t row_cap = rpf::stft_pieces(options.frame_bytes(), 8 * static_cast<size_t>(options.N)).per_piece;
    PieceReader in(options.input_file, b * options.span_samples(), b * options.step(), 1,
                   static_cast<int64_t>(rpf::kSeriesPieceBytes), row_cap);
    std::ofstream out(options.stft_file, std::ios::out | std::ios::trunc | std::ios::binary);
    if (!out) throw RPFexception("Could not open " + options.stft_file + " for writing.", ReturnValue::InvalidInput);
    std::vector<float> rows;
    const int64_t frames = replay_pieces({&in}, [&](size_t have) {
        const int64_t done = data.stft(in.data(), have / b * b, in.per_piece(), rows);
        if (done == 0) return done;
        out.write(reinterpret_cast<const char*>(rows.data()), static_cast<std::streamsize>(sizeof(float) * 2 * options.N * done));
        if (!out) throw RPFexception("Could not write to " + options.stft_file + ".", ReturnValue::InvalidInput);
        return done;
    });
    int lds = 0;
    (void)rpf_last_launch_info(data.engine(), nullptr, nullptr, nullptr, &lds);
    std::cerr << "STFT: " << frames << " frames of " << options.N << " bins, route: "
              << (options.pfb_taps ? "PFB fold, then " : "") << (lds > 0 ? "K1 store kernels" : "catch-all transform") << std::endl;
    if (chatty(options)) print_acquisition_summary(options.N, frames, 0, 0, actual_samplerate);
    return 0;
}

int run(int argc, char** argv)
{
    Options options = parse_command_line(argc, argv);
    if (options.show_help) {
        std::cout << usage_text();
        return 0;
    }
    if (options.show_version) {
        std::cout << argv[0] << "  version: " << kVersion << std::endl;
        return 0;
    }
    AuxData aux(options);

    std::unique_ptr<SampleSource> source;
    RtlSdrSource* dongle = nullptr;
    if (!options.input_file.empty()) source.reset(new FileSource(options.input_file, static_cast<size_t>(options.sample_bytes())));
    else if (options.synthetic) source.reset(new SyntheticSource(options.synthetic_seed));
    else source.reset(dongle = new RtlSdrSource(options.dev_index));   // rtl_power_fftw.cxx:65

    if (options.endless) options.session_duration_isSet = false;
    time_t exit_time = 0;
    if (options.session_duration_isSet) {
        exit_time = static_cast<int>(options.session_duration);
        std::cerr << "Scan session duration: " << exit_time << " seconds" << std::endl;
    }
    if (dongle) {
        // rtl_power_fftw.cxx:77-97: nearest available gain, provisional tuning, ppm
        dongle->print_gains();
        const int gain = dongle->nearest_gain(options.gain);
        std::cerr << "Selected nearest available gain: " << gain << " (" << 0.1 * gain << " dB)" << std::endl;
        dongle->set_gain(gain);
        try {
            dongle->set_frequency(options.cfreq);
        } catch (RPFexception&) {
        }
        if (options.ppm_error != 0) {
            dongle->set_freq_correction(options.ppm_error);
            std::cerr << "PPM error set to: " << options.ppm_error << std::endl;
        }
    } else {
        source->set_frequency(options.cfreq);
    }
    source->set_sample_rate(static_cast<uint32_t>(options.sample_rate));
    const int actual_samplerate = source->sample_rate();
    std::cerr << "Actual sample rate: " << actual_samplerate << " Hz" << std::endl;

    Plan plan(options, actual_samplerate);
    plan.print();

    if (!options.stft_file.empty()) return run_stft(options, aux, actual_samplerate);
    if (!options.correlate_files.empty()) return run_correlate(options, aux, actual_samplerate, source->frequency());
    if (!options.cross_file.empty()) return run_cross(options, aux, actual_samplerate, source->frequency());
    if (options.dedisperse_frames > 0) return run_dedisperse(options, aux, actual_samplerate, source->frequency());
    if (options.quantile_frames > 0) return run_quantile(options, aux, actual_samplerate, source->frequency());
    if (options.excise_frames > 0) return run_excise(options, aux, actual_samplerate, source->frequency());
    if (options.series_frames > 0) return run_series(options, aux, actual_samplerate, source->frequency());

    const bool multi = options.devices.size() > 1;
    std::unique_ptr<Datastore> data;                 // after Plan fixed N / repeats / buf_length
    std::unique_ptr<MultiDeviceScan> scan;
    if (multi) {
        scan.reset(new MultiDeviceScan(options, aux, *source, actual_samplerate));
        std::cerr << "Scan spread over " << options.devices.size() << " engines (gpus";
        for (int d : options.devices) std::cerr << " " << d;
        std::cerr << ")" << std::endl;
    } else {
        data.reset(new Datastore(options, aux.window_values));
    }
    set_CtrlC_handler(true);
    if (options.session_duration_isSet) exit_time += std::time(nullptr);
    if (options.matrixMode) std::ofstream(options.bin_file, std::ios::out | std::ios::trunc | std::ios::binary);

    ScanMetadata meta;
    bool meta_pending = true;
    options.finalfreq = static_cast<int>(plan.freqs_to_tune.back());
    int64_t last_repeats_done = 0;
    bool wrote_anything = false;
    bool stop = false;
    do {
        bool input_ended = false;
        if (multi) {
            const std::vector<int64_t> freqs(plan.freqs_to_tune.begin(), plan.freqs_to_tune.end());
            const bool complete = scan->run_pass(freqs, meta, meta_pending, plan, last_repeats_done);
            wrote_anything = scan->hops_written() > 0;
            input_ended = scan->exhausted();
            if (!complete && input_ended) stop = true;
        } else {
            for (auto hop = plan.freqs_to_tune.begin(); hop != plan.freqs_to_tune.end();) {
                Acquisition acquisition(options, aux, *source, *data, meta, actual_samplerate, *hop);
                try {
                    acquisition.run();
                    ++hop;
                } catch (TuneError& e) {
                    std::cerr << "Unable to tune to " << e.frequency() << ". Dropping from frequency list." << std::endl;
                    hop = plan.freqs_to_tune.erase(hop);
                    continue;
                }
                if (chatty(options)) acquisition.print_summary();
                last_repeats_done = data->repeats_done;
                if (data->repeats_done == 0) {
                    // the reference would divide by zero here and print a spectrum of NaNs (acquisition.cxx:393)
                    std::cerr << "No complete spectrum at " << acquisition.tuned_freq()
                              << " Hz; nothing written." << std::endl;
                    // (a second Ctrl-C must end the scan here too, not retune once per remaining hop)
                    if (source->exhausted() || checkInterrupt(InterruptState::FinishNow)) break;
                    continue;
                }
                if (options.matrixMode && meta_pending) {
                    note_scan_extent(options, plan, actual_samplerate, meta);
                    meta_pending = false;
                }
                acquisition.write_data(std::cout);
                wrote_anything = true;
                if (chatty(options)) data->printQueueHistogram();
                if (source->exhausted()) break;
                if (checkInterrupt(InterruptState::FinishNow)) break;
            }
            input_ended = source->exhausted();
        }
        if (options.talkless && options.outcnt == 0) options.outcnt++;

        // a second blank line closes a full pass over the hops (man page, FREQUENCY SCANNING)
        if (options.session_duration_isSet) {
            if (std::time(nullptr) >= exit_time) {
                stop = true;
                std::cerr << "Session duration elapsed." << std::endl;
                std::cout << std::endl;
            }
        } else {
            std::cout << std::endl;
        }
        if (options.endless) stop = false;
        if (!options.session_duration_isSet && !options.endless) stop = true;
        if (checkInterrupt(InterruptState::FinishPass)) stop = true;
        if (plan.freqs_to_tune.empty()) stop = true;
        if (input_ended) {
            // a finite replay has nothing more to give: --continue / -e would spin on empty reads
            if (!stop) std::cerr << "Input exhausted, ending the session." << std::endl;
            stop = true;
        }
    } while (!stop);

    if (options.matrixMode) write_metadata(options, meta, last_repeats_done, actual_samplerate);
    if (plan.freqs_to_tune.empty())
        throw RPFexception("No valid frequencies left.", ReturnValue::AcquisitionError);
    if (!wrote_anything) throw NoSpectrum();
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    try {
        return run(argc, argv);
    } catch (RPFexception& e) {
        std::cerr << e.what() << std::endl;
        return static_cast<int>(e.returnValue());
    }
}
