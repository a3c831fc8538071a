// rpf_engine.cpp -- implementation of include/rpf_engine.h: the buffer pool and
// consumer thread of Datastore (/root/reference/src/datastore.cxx:23-103)
// re-designed around a HIP device.
//
//   producer (caller's thread)                consumer (engine thread)                  recycler (engine thread)
//   --------------------------                ------------------------                  ------------------------
//   rpf_buffer_acquire  <-- empty_  <-------------------------------------------------  each buffer as soon as ITS
//   fill pinned buffer                                                                   H2D copy has landed
//   rpf_buffer_submit   --> occupied_ ------->  pop everything queued; per buffer one
//                                               hipMemcpyAsync H2D, at once, on
//                                               alternating copy streams, into the
//                                               device staging slot being filled; when
//                                               the slot is full (or at the end): carry
//                                               the previous slot's unfinished frame in
//                                               front, fused kernel + reduce (compute stream)
//   rpf_finish          --> finished_ ------->  launch the last slot, sync, pwr -> host, exit
//
// Pinned host buffers let the H2D copies overlap the kernels (copy streams + compute stream + events); a frame that
// straddles two slots (datastore.cxx:52,68,81) is completed by copying the tail of the previous staging slot in front
// of the new bytes, device to device.
#include "../../include/rpf_engine.h"
#include "rpf_engine_testing.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "bluestein_tables.h"
#include "cross_core.h"
#include "correlate_core.h"
#include "dedisperse_core.h"
#include "fold_core.h"
#include "engine_family.h"
#include "rpf_kernels.h"
#include "series_pieces.h"

namespace {

thread_local std::string g_last_error;

struct HostBuffer {
    uint8_t* data = nullptr;
    size_t size = 0;   // bytes valid after submit (Buffer::size())
    hipEvent_t copied = nullptr;    // its H2D copy has finished: the producer may refill it
    bool external = false;          // a piece of a caller's registered stream (rpf_accumulate's direct path): never recycled
};

constexpr int kStagingSlots = 3;    // device staging ring: one slot filling, one waiting for its kernel, one running
constexpr int kCopyStreams = 2;     // H2D copies alternate between two streams (two SDMA queues): no gap between copies

struct StagingSlot {
    uint8_t* base = nullptr;        // device memory: [head_room | coalesce x buffer_capacity]
    hipEvent_t copy_done[kCopyStreams] = {};   // everything copied into the slot on that stream has landed
    hipEvent_t kernel_done = nullptr;
    bool in_flight = false;
    // the last transform launched over the slot (still valid until the slot is reopened): what a fused launch that
    // gave up is re-run on
    const uint8_t* launch_ptr = nullptr;
    int64_t launch_frames = 0;
    bool launched_fused = false;
    unsigned* verdict = nullptr;    // pinned host word the launch's verdict kernel sets to 1 if it gave up
};

// A pinned host block and its twin on the device, for a table the host writes anew for every call and uploads on the
// call's stream.  The pair serves one call at a time: reserve() waits until the call before has passed `done`, which
// record() puts behind the launches that read the table.
struct UploadTable {
    uint8_t* host = nullptr;
    uint8_t* device = nullptr;
    size_t bytes = 0;             // ... each holds
    hipEvent_t done = nullptr;

    int reserve(rpf_engine* e, size_t need);
    int record(rpf_engine* e, hipStream_t s);
    void release_blocks();        // the two blocks
    void release();               // ... and the event
};

}  // namespace

struct rpf_engine {
    // configuration (Params fields Datastore reads)
    int N = 0;
    int step = 0;                 // frame step S in complex samples (rpf_config::frame_step; N = frames side by side)
    int format = RPF_FORMAT_CU8;  // sample format (RPF_FLAG_SAMPLE_FORMAT)
    size_t sample_bytes = 2;      // bytes per complex sample, b: every byte count below is b x samples
    bool has_window = false;
    int n_buffers = 0;
    size_t buffer_capacity = 0;
    int device = 0;
    bool use_dma = true;
    int variant = 0;
    bool stats = false;           // RPF_FLAG_BIN_STATS: S2 and PK kept beside the power on every path

    // Datastore public state
    int64_t repeats = 0;        // params.repeats of the running acquisition
    int64_t repeats_done = 0;   // datastore.h:38
    std::mutex status_mutex;    // datastore.h:40
    std::deque<HostBuffer*> empty_buffers;      // :43
    std::deque<HostBuffer*> occupied_buffers;   // :44
    bool acquisition_finished = false;          // :45
    std::condition_variable status_change;      // :46
    std::vector<int> queue_histogram;           // :47
    std::vector<double> pwr;                    // :53
    std::vector<double> sum_sq, peak;           // stats engines: S2[N], PK[N] of the last acquisition

    std::vector<HostBuffer> pool;
    uint8_t* pool_base = nullptr;        // the pool as ONE pinned allocation: neighbouring buffers can travel in one copy
    std::vector<std::pair<const uint8_t*, size_t>> registered;     // rpf_stream_register: caller memory pinned for direct replay
    size_t bytes_landed = 0;             // H2D bytes whose copy has finished (recycler; under recycle_mutex)
    std::thread worker;
    bool worker_running = false;
    int worker_rc = RPF_OK;
    std::string worker_error;

    // device side
    hipStream_t copy_streams[kCopyStreams] = {}, compute_stream = nullptr;
    // buffers whose copies are in flight, in issue order; the recycler thread waits for each copy and hands the buffer back
    std::mutex recycle_mutex;
    std::condition_variable recycle_cv;
    std::deque<std::pair<hipEvent_t, HostBuffer*>> recycle_queue;
    bool recycle_stop = false;
    std::string recycler_error;
    rpf::cf* d_twiddles = nullptr;
    rpf::Family family = rpf::Family::K1; // the kernel family that serves N (engine_family.h), chosen once at creation
    bool fused = false;                   // four-step: by the fused persistent kernel (Y stays in the XCDs' L2) -- until retire_fused
    void* d_fused_ctl = nullptr;          // its team counters / abort flag
    rpf::cf* d_fused_scratch = nullptr;   // its Y (two rounds per XCD); kept apart from d_scratch, the two-kernel path's
    // What became of the fused launches, written by their verdict kernels into pinned host memory:
    // [0 .. 2] one word per staging slot (queue path), [3] launches of the device-resident entries that gave up
    // (cumulative), [4] all launches that gave up (cumulative).
    unsigned* h_fused_words = nullptr;
    unsigned* d_fused_words = nullptr;    // the same words as the device addresses them
    bool last_was_fused = false;          // the last transform launched was the fused kernel
    unsigned fused_aborts_seen = 0;       // h_fused_words[3] when the host last looked
    int64_t fused_recovered = 0;          // launches re-run on K2a/K2b after giving up (queue path)
    int fused_fault_mode = 0, fused_fault_skip = 0, fused_fault_count = 0;   // rpf_debug_fused_fault
    int gen_h = 0;                        // catch-all path: its two-level twiddle split (d_tw_sub = T0, d_tw_sub2 = T1)
    rpf::cf* d_chirp = nullptr;           // Bluestein families: g[n], N entries
    rpf::cf* d_bhat = nullptr;            // frequency-domain chirp, M entries
    rpf::cf* d_tw_sub = nullptr;          // four-step: twiddles of the N1-point column transforms
    rpf::cf* d_tw_sub2 = nullptr;         // four-step: twiddles of the N2-point row transforms
    rpf::cf* d_scratch = nullptr;         // four-step: intermediate Y
    size_t scratch_bytes = 0;             // its size now; grown on demand (two-kernel four-step and large Bluestein paths)
    size_t scratch_per_frame = 0, scratch_max = 0;
    rpf::cf* d_step2 = nullptr;           // large Bluestein: second transform's inter-step twiddles
    uint8_t* d_gather = nullptr;          // overlapped frames on the non-K1 families: one chunk, side by side
    int64_t gather_frames = 0;            // ... frames it holds (kGatherBytes / 2N, at least one)
    float* d_window = nullptr;
    double* d_partial = nullptr;
    size_t partial_stride = 0;            // elements from one partial spectrum to the next (0: N; large Bluestein: its M)
    double* d_pwr = nullptr;              // N doubles; a stats engine's: 3 N, the planes S1 (= pwr), S2, PK
    size_t head_room = 0;                 // >= 2N, multiple of 256
    size_t coalesce = 1;                  // host buffers one staging slot holds (= one transform launch)
    std::vector<StagingSlot> staging;
    rpf::LaunchInfo plan;                 // resident grid for this N
    rpf::LaunchInfo last;                 // last launch
    int last_slots = 0;                   // partial spectra left by the last transform
    rpf::SlotRanges last_ranges;          // ... and which of them belong to which hop (K1 hop launches)
    int last_hops = 0;                    // hops of the last rpf_device_fused_hops (0: a single-acquisition transform)
    // series entries (rpf_accumulate_device_series[_stats], rpf_accumulate_series[_stats]; a stats engine's rows and
    // slots are three planes); all allocated at the first call that needs them
    bool series_planned = false;
    rpf::LaunchInfo series_plan;          // the series kernel's resident grid
    double* d_series_partial = nullptr;   // its scratch: 2 x grid x N doubles (a stats engine's: x 3), whatever K is
    int series_launches = 0;              // transform-kernel launches of the last series call
    uint8_t* d_series_in = nullptr;       // rpf_accumulate_series: one piece of the host stream ...
    size_t series_in_bytes = 0;
    size_t series_in_stride = 0;          // ... bytes from one stream's piece to the next (the entries of several streams)
    double* d_series_out = nullptr;       // ... and its rows (N doubles each; a stats engine's 3 N)
    size_t series_out_rows = 0;
    // excised average (rpf_accumulate[_device]_excised): a piece's rows go to d_series_out, and
    double* d_excise_state = nullptr;     // the (row group, bin) accumulators, then 3 N doubles: the host entry's result
    uint8_t* d_excise_mask = nullptr;     // the host entry's mask bytes of one piece
    size_t excise_mask_bytes = 0;
    // per-bin quantiles (rpf_quantile_*): the row store, grown by doubling up to quantile_max_rows(), and what a
    // selection works in; all allocated at the first call that needs them
    double* d_quantile_rows = nullptr;    // quantile_cap rows of N doubles, the first quantile_rows of them stored
    int64_t quantile_rows = 0, quantile_cap = 0;
    void* d_quantile_work = nullptr;      // rpf::quantile_work_bytes(N): the selection state of one call at a time
    double* d_quantile_out = nullptr;     // rpf_quantile_select: the result on the device, quantile_out_planes x N doubles
    size_t quantile_out_planes = 0;
    // polyphase filter bank front end (rpf_engine_create_pfb): this engine owns the queues and the fold, `inner` the transform
    int taps = 0;                         // T; 0 = an engine without PFB
    float* d_pfb_coeffs = nullptr;        // h[T x N]
    rpf_engine* inner = nullptr;          // a rectangular cf32 engine of the same N, device and staging flag
    float* d_pfb_z = nullptr;             // one chunk of folded frames, float32 I/Q side by side; allocated at the first launch
    int64_t pfb_chunk_frames = 0;         // ... frames it holds (kGatherBytes / 8N, at least one)
    // cross-spectrum of two streams (rpf_accumulate[_device]_cross); everything below `window` is made at the first call
    uint32_t flags = 0;                   // rpf_config::flags as given, and
    std::vector<float> window;            // ... the window as given (host): what the cf32 engine below is created from
    rpf_engine* cross_inner = nullptr;    // the cf32 engine of the same N, window, frame step, device and flags; a cf32 engine: itself
    float* d_cross_uv = nullptr;          // u = a + b, then v = a + i b: one chunk of whole frames each, cf32
    size_t cross_v_offset = 0;            // ... floats from u to v
    int64_t cross_chunk_frames = 0;       // ... frames a chunk holds (as many as span at most kGatherBytes, at least one)
    double* d_cross_planes = nullptr;     // Paa, Pbb, Puu, Pvv, then the host entry's four output planes: 8 N doubles
    bool last_was_cross = false;          // the last transform launched was a cross call's: rpf_last_launch_info reports cross_inner's
    // the frames' spectra themselves (rpf_stft_device, rpf_stft); everything made at the first call that needs it
    bool stft_planned = false;
    rpf::LaunchInfo stft_plan;            // K1: the store kernels' resident grid
    rpf_engine* stft_inner = nullptr;     // a family other than K1 and the catch-all: the catch-all engine of the same
                                          // N, window, frame step, format, device and staging flag
    float* d_stft_rows = nullptr;         // rpf_stft: the rows of one piece
    size_t stft_rows = 0;                 // ... rows (of 2 N floats) it holds
    bool last_was_stft = false;           // the last transform launched was an STFT call's on stft_inner
    // the correlator of up to eight streams (rpf_correlate_device, rpf_correlate); made at the first call, grown for a
    // call with more streams than any before it
    float* d_corr_rows = nullptr;         // M blocks of correlate_chunk_frames(N) rows of 2 N floats
    size_t corr_rows = 0;                 // ... rows it holds
    double* d_corr_partial = nullptr;     // the X-engine's partial planes: G M^2 N doubles where G > 1
    size_t corr_partial = 0;              // ... doubles it holds
    double* d_corr_planes = nullptr;      // the M^2 running planes, then the host entry's result: 3 M^2 N doubles
    size_t corr_planes = 0;               // ... doubles it holds
    // incoherent dedispersion of the stored integrations (rpf_dedisperse_device, rpf_dedisperse); made at the first call
    UploadTable dd_tables;                // the weights, the spans and the delay table of one call, as uploaded
    double* d_dd_out = nullptr;           // rpf_dedisperse: the D x T result on the device
    size_t dd_out = 0;                    // ... doubles it holds
    // fold of a plane at trial periods (rpf_fold_device, rpf_dedisperse_fold); made at the first call
    UploadTable fold_steps;               // the steps of one call, as uploaded; its `done` also guards the scratch
    uint8_t* d_fold_scratch = nullptr;    // the partials of one group of series (fold_core.h), at most 256 MB
    size_t fold_scratch_bytes = 0;        // ... bytes it holds
    uint8_t* d_fold_out = nullptr;        // rpf_dedisperse_fold: prof, mom and hits on the device
    size_t fold_out_bytes = 0;            // ... bytes it holds

    mutable std::string last_error;
};

namespace {

// Waits on `cv` until `pred` holds, after first polling for it for up to ~100 us with the lock dropped between looks.
// The three hand-offs of a buffer's round trip (copy landed -> recycler -> producer -> consumer) are each a thread
// wake-up; a condition-variable wake-up costs 10 - 50 us and a 1.6 MB buffer is 30 us of PCIe time, so with the
// reference's five buffers sleeping threads left the link idle a quarter of the time (41 of the 53.7 GB/s two copy
// streams reach, tools/h2d_rate.cpp).  A waiter that has just been busy looks again before it sleeps.
template <class Pred>
void wait_briefly_then_block(std::unique_lock<std::mutex>& lock, std::condition_variable& cv, Pred pred)
{
    if (pred()) return;
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(100);
    do {
        lock.unlock();
        std::this_thread::yield();
        lock.lock();
        if (pred()) return;
    } while (std::chrono::steady_clock::now() < deadline);
    cv.wait(lock, pred);
}

int fail(rpf_engine* e, int rc, const std::string& msg)
{
    if (e) e->last_error = msg;
    g_last_error = msg;
    return rc;
}

// ---- the refusals the entries share, each worded once.  All but refuse() test their condition first and return RPF_OK
// where it does not hold: the text is built only for a call that is refused. ----

int refuse(rpf_engine* e, const char* who, const std::string& text)
{
    return fail(e, RPF_ERR_INVALID_ARGUMENT, std::string(who) + ": " + text);
}

int refuse_if_running(rpf_engine* e, const char* who)
{
    return e->worker_running ? refuse(e, who, "acquisition running") : RPF_OK;
}

int refuse_negative_repeats(rpf_engine* e, int64_t repeats)
{
    return repeats < 0 ? fail(e, RPF_ERR_INVALID_ARGUMENT, "Argument to 'repeats' must be a positive number.") : RPF_OK;
}

// subject: "d_stream", "d_a and d_b", "every stream", "streams" -- as the entry's own message has always had it
int refuse_unaligned_stream(rpf_engine* e, const char* who, const char* subject, const void* ptr)
{
    if (!(reinterpret_cast<uintptr_t>(ptr) & (e->sample_bytes - 1))) return RPF_OK;
    return refuse(e, who, std::string(subject) + " must be at least 2-byte aligned (4-byte for 16-bit samples, 8-byte for cf32)");
}

int refuse_unaligned_out(rpf_engine* e, const char* who, const char* name, const void* ptr)
{
    return (reinterpret_cast<uintptr_t>(ptr) & 15) ? refuse(e, who, std::string(name) + " must be 16-byte aligned") : RPF_OK;
}

int refuse_ragged_bytes(rpf_engine* e, const char* who, size_t nbytes)
{
    if (nbytes % e->sample_bytes == 0) return RPF_OK;
    return refuse(e, who, "nbytes must be a multiple of the sample size (" + std::to_string(e->sample_bytes) + " bytes)");
}

int refuse_not_power_of_two(rpf_engine* e, const char* who)
{
    if (!(e->N & (e->N - 1))) return RPF_OK;
    return refuse(e, who, "the number of bins must be a power of two (Bluestein's spectrum lacks its final chirp); got " +
                              std::to_string(e->N));
}

// the cross, STFT and correlator entries: built on the plain power path and the cf32 / catch-all engines
int refuse_stats_engine(rpf_engine* e, const char* who)
{
    return e->stats ? refuse(e, who, "not on an engine created with RPF_FLAG_BIN_STATS") : RPF_OK;
}

int refuse_variant(rpf_engine* e, const char* who)
{
    return e->variant != 0 ? refuse(e, who, "not with a kernel variant other than 0") : RPF_OK;
}

// Frame f of a stream is bytes [bfS, bfS + b span), b bytes per sample; span: N samples, or T N on a PFB engine (whose
// frames advance by N).  series_pieces.h has the two formulas.
rpf::FrameBytes frame_bytes(const rpf_engine* e)
{
    const size_t span = static_cast<size_t>(e->N) * static_cast<size_t>(std::max(e->taps, 1));
    return {e->sample_bytes * span, e->sample_bytes * static_cast<size_t>(e->step)};
}

// frames(B) of a stream of B bytes at frame step S, and the bytes `frames` frames span: b span + bS (frames - 1)
int64_t frames_in(const rpf_engine* e, size_t nbytes) { return frame_bytes(e).frames_in(nbytes); }
size_t frame_span(const rpf_engine* e, int64_t frames) { return frame_bytes(e).span(frames); }

bool overlapped(const rpf_engine* e) { return e->step != e->N; }

bool is_k1(const rpf_engine* e) { return e->family == rpf::Family::K1; }

// Makes the engine's device current for the scope of an entry point and puts the
// caller's back afterwards: in a multi-GPU process (one engine per device, or a
// caller that has another device selected) a launch against engine-owned memory
// must not depend on -- nor disturb -- the calling thread's current device.
class DeviceScope {
public:
    explicit DeviceScope(int device)
    {
        if (hipGetDevice(&prev_) != hipSuccess) prev_ = -1;
        status_ = (prev_ == device) ? hipSuccess : hipSetDevice(device);
        changed_ = (status_ == hipSuccess && prev_ != device);
    }
    ~DeviceScope()
    {
        if (changed_ && prev_ >= 0) (void)hipSetDevice(prev_);
    }
    hipError_t status() const { return status_; }
private:
    int prev_ = -1;
    bool changed_ = false;
    hipError_t status_ = hipSuccess;
};

#define HIP_TRY(e, call)                                                                 \
    do {                                                                                 \
        hipError_t err__ = (call);                                                       \
        if (err__ != hipSuccess)                                                         \
            return fail(e, RPF_ERR_HARDWARE,                                             \
                        std::string(#call) + ": " + hipGetErrorString(err__));           \
    } while (0)

// Engine-owned device scratch of *have units of `unit` bytes holds `need` of them.  Grows, never shrinks: a call that
// needs more than any before it synchronises `s` and the engine's stream once, frees and allocates.
template <class T>
int grow_scratch(rpf_engine* e, T** d_ptr, size_t* have, size_t need, size_t unit, hipStream_t s)
{
    if (need <= *have) return RPF_OK;
    HIP_TRY(e, hipStreamSynchronize(s));
    if (s != e->compute_stream) HIP_TRY(e, hipStreamSynchronize(e->compute_stream));
    if (*d_ptr) (void)hipFree(*d_ptr);
    *d_ptr = nullptr;
    *have = 0;
    HIP_TRY(e, hipMalloc(d_ptr, need * unit));
    *have = need;
    return RPF_OK;
}

int UploadTable::reserve(rpf_engine* e, size_t need)
{
    if (done)
        HIP_TRY(e, hipEventSynchronize(done));
    else
        HIP_TRY(e, hipEventCreateWithFlags(&done, hipEventDisableTiming));
    if (need <= bytes) return RPF_OK;
    release_blocks();
    HIP_TRY(e, hipHostMalloc(reinterpret_cast<void**>(&host), need, hipHostMallocDefault));
    HIP_TRY(e, hipMalloc(&device, need));
    bytes = need;
    return RPF_OK;
}

int UploadTable::record(rpf_engine* e, hipStream_t s)
{
    HIP_TRY(e, hipEventRecord(done, s));
    return RPF_OK;
}

void UploadTable::release_blocks()
{
    if (host) (void)hipHostFree(host);
    (void)hipFree(device);
    host = device = nullptr;
    bytes = 0;
}

void UploadTable::release()
{
    release_blocks();
    if (done) (void)hipEventDestroy(done);
    done = nullptr;
}

// The last lines of a host entry: the result to the caller's memory, then the one synchronise the caller waits for.
int copy_back(rpf_engine* e, void* dst, const void* d_src, size_t bytes, hipStream_t s)
{
    HIP_TRY(e, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    return RPF_OK;
}

// The host loop of the entries that take their streams from host memory: the K integrations (of L frames) of each of
// the M `streams` in the pieces of series_pieces.h through d_series_in, stream m's piece at d_series_in + m stride.
// The stride (e->series_in_stride, for the body) is the piece's bytes, rounded up to 256 where M > 1.
// prepare(per_piece) makes room for what a piece leaves; body(k0, kc, s) enqueues integrations [k0, k0 + kc) and at most
// one copy back.  A piece is ONE copy in per stream from the caller's pointer (a registered stream from where it lies),
// stream by stream, then the body and ONE synchronise; a failed body's rc is looked at first, then the stream is
// synchronised and the rc returns.
// *landed: the integrations whose synchronise succeeded, which comes after the body, so a body cannot count them.
template <class Prepare, class Body>
int series_host_pieces(rpf_engine* e, const uint8_t* const* streams, int M, int64_t L, int64_t K, int64_t row_cap,
                       Prepare prepare, Body body, int64_t* landed = nullptr)
{
    hipStream_t s = e->compute_stream;
    const rpf::SeriesPieces p = rpf::series_pieces(frame_bytes(e), L, K, rpf::kSeriesPieceBytes, row_cap);
    const size_t stride = M > 1 ? (p.bytes + 255) / 256 * 256 : p.bytes;
    e->series_in_stride = stride;
    int rc = grow_scratch(e, &e->d_series_in, &e->series_in_bytes, static_cast<size_t>(M) * stride, 1, s);
    if (rc != RPF_OK || (rc = prepare(p.per_piece)) != RPF_OK) return rc;
    for (int64_t k0 = 0; k0 < K; k0 += p.per_piece) {
        const int64_t kc = std::min(p.per_piece, K - k0);
        for (int m = 0; m < M; ++m)
            HIP_TRY(e, hipMemcpyAsync(e->d_series_in + static_cast<size_t>(m) * stride, streams[m] + static_cast<size_t>(k0) * p.hop,
                                      frame_span(e, kc * L), hipMemcpyHostToDevice, s));
        if ((rc = body(k0, kc, s)) != RPF_OK) {
            (void)hipStreamSynchronize(s);
            return rc;
        }
        HIP_TRY(e, hipStreamSynchronize(s));
        if (landed) *landed = k0 + kc;
    }
    return RPF_OK;
}

// K1 over up to rpf::kMaxHops acquisitions in ONE launch (hop_partition.h): leaves the partial
// spectra of hop h in the slots [slots->begin[h], slots->begin[h+1]) of e->d_partial.
int launch_fused_hops(rpf_engine* e, const uint8_t* const* d_frames, const int64_t* nframes, int H,
                      hipStream_t stream, rpf::SlotRanges* slots, int* nslots)
{
    if (H == 1
#ifdef RPF_TUNING
        && !std::getenv("RPF_TUNE_SCAN_KERNEL")
#endif
    ) {
        // a scan of one hop is a single acquisition: the plain kernel (1.8 us per launch less)
        for (int h = 0; h <= rpf::kMaxHops; ++h) slots->begin[h] = 0;
        *nslots = 0;
        if (nframes[0] < 1) return RPF_OK;
        const int64_t wanted = (nframes[0] + e->plan.fpw - 1) / e->plan.fpw;
        const int grid = static_cast<int>(std::min<int64_t>(e->plan.grid, wanted));
        // overlapped frames: the strided instantiation, LDS-DMA where every frame start is 16-byte aligned
        const long pitch = static_cast<long>(e->sample_bytes) * e->step;
        const bool dma1 = e->use_dma && (reinterpret_cast<uintptr_t>(d_frames[0]) % 16) == 0 && pitch % 16 == 0;
        HIP_TRY(e, rpf::launch_fft_accum(e->N, e->variant, e->has_window, dma1, d_frames[0], nframes[0], e->d_twiddles,
                                         e->d_window, e->d_partial, grid, stream, &e->last, pitch, e->format, e->stats));
        for (int h = 1; h <= rpf::kMaxHops; ++h) slots->begin[h] = grid;
        *nslots = grid;
        return RPF_OK;
    }
    if (e->stats) return fail(e, RPF_ERR_INVALID_ARGUMENT, "the one-launch scan does not keep per-bin statistics");
    rpf::HopArgs args;
    bool interleave_single = false;
#ifdef RPF_TUNING
    interleave_single = H == 1 && std::getenv("RPF_TUNE_INTERLEAVE") != nullptr;     // A/B of the two iteration orders
#endif
    const int grid = rpf::partition_hops(nframes, H, e->plan.fpw, e->plan.grid, &args, slots, interleave_single);
    if (grid < 0) return fail(e, RPF_ERR_INVALID_ARGUMENT, "too many frames for one launch");
    bool dma = e->use_dma;
    for (int h = 0; h < rpf::kMaxHops; ++h) {
        args.stream[h] = h < H ? d_frames[h] : nullptr;
        if (h < H && nframes[h] > 0 && (reinterpret_cast<uintptr_t>(d_frames[h]) % 16) != 0) dma = false;
    }
    *nslots = slots->begin[H];
    if (grid == 0) return RPF_OK;           // no whole frame anywhere: every slot range is empty
    HIP_TRY(e, rpf::launch_fft_accum_hops(e->N, e->variant, e->has_window, dma, args, e->d_twiddles, e->d_window,
                                          e->d_partial, grid, stream, &e->last, e->format));
    return RPF_OK;
}

// The intermediate of the two-kernel four-step and large Bluestein paths: sized to what the launches need, not to the
// 2 GB (4 GB) a whole device-resident acquisition can use -- a queue-fed engine never launches more than a 32 MB slot
// of input.  Grows (never shrinks) when a larger launch arrives: one stream synchronisation, then free + allocate; if
// the device cannot give more the launch runs in smaller batches on what there is.
int ensure_scratch(rpf_engine* e, int64_t nframes, hipStream_t stream)
{
    if (!e->scratch_per_frame) return RPF_OK;
    const size_t want = std::min<size_t>(e->scratch_max, static_cast<size_t>(nframes) * e->scratch_per_frame);
    if (want <= e->scratch_bytes) return RPF_OK;
    HIP_TRY(e, hipStreamSynchronize(stream));
    HIP_TRY(e, hipStreamSynchronize(e->compute_stream));
    const size_t had = e->scratch_bytes;
    (void)hipFree(e->d_scratch);
    e->d_scratch = nullptr;
    e->scratch_bytes = 0;
    void* p = nullptr;
    if (hipMalloc(&p, want) == hipSuccess) {
        e->scratch_bytes = want;
    } else {
        (void)hipGetLastError();
        // what there was before, or (nothing yet: an engine that has just left the fused kernel) one frame's worth
        const size_t least = std::max(had, e->scratch_per_frame);
        HIP_TRY(e, hipMalloc(&p, least));
        e->scratch_bytes = least;
    }
    e->d_scratch = static_cast<rpf::cf*>(p);
    return RPF_OK;
}

// This engine keeps to K2a/K2b from here on (a fused launch gave up).  Nothing is freed -- launches in flight may
// still be using the fused kernel's scratch --; the two-kernel path's intermediate is allocated by ensure_scratch at
// its first launch (one stream synchronisation).
void retire_fused(rpf_engine* e)
{
    if (!e->fused) return;
    e->fused = false;
    e->scratch_per_frame = rpf::fourstep_scratch_bytes_per_frame(e->N);
    e->scratch_max = rpf::fourstep_scratch_bytes(e->N);
}

// The device-resident entries return without synchronising, so a launch of theirs that gave up is found out later:
// its verdict kernel has counted it in pinned host memory by the time the caller's stream has passed it.  Every
// later entry looks (no synchronisation) and retires the fused kernel once it sees a count it has not seen.
void note_device_path_aborts(rpf_engine* e)
{
    if (!e->h_fused_words) return;
    const unsigned now = __atomic_load_n(&e->h_fused_words[3], __ATOMIC_ACQUIRE);
    if (now != e->fused_aborts_seen) {
        e->fused_aborts_seen = now;
        retire_fused(e);
    }
}

// ---- one transform launch per family: `nframes` frames side by side from d_frames -> *nslots partial spectra in
// e->d_partial (launch_transform) ----

// The fused persistent kernel while the engine has it, else the pair K2a/K2b.
int transform_fourstep(rpf_engine* e, const uint8_t* d_frames, int64_t nframes, hipStream_t stream, int* nslots)
{
    const bool dma = e->use_dma && (reinterpret_cast<uintptr_t>(d_frames) % 4) == 0;
    if (!e->fused) {
        if (int rc = ensure_scratch(e, nframes, stream)) return rc;
        HIP_TRY(e, rpf::launch_fourstep(e->N, e->has_window, dma, d_frames, nframes, e->d_tw_sub,
                                        e->d_tw_sub2, e->d_twiddles, e->d_window, e->d_scratch, e->scratch_bytes,
                                        e->d_partial, e->plan.grid, stream));
        e->last = e->plan;
        *nslots = rpf::fourstep_partial_slots(e->N);
        return RPF_OK;
    }
    int fault = 0;                       // rpf_debug_fused_fault: `count` launches after `skip` untouched ones
    if (e->fused_fault_count != 0) {
        if (e->fused_fault_skip > 0) {
            --e->fused_fault_skip;
        } else {
            fault = e->fused_fault_mode;
            if (e->fused_fault_count > 0) --e->fused_fault_count;
        }
    }
    HIP_TRY(e, rpf::launch_fourstep_fused(e->N, e->has_window, dma, d_frames, nframes, e->d_tw_sub, e->d_tw_sub2,
                                          e->d_twiddles, e->d_window, e->d_fused_scratch, e->d_partial,
                                          e->d_fused_ctl, stream, fault));
    e->last = e->plan;
    e->last_was_fused = true;
    *nslots = rpf::fourstep_fused_slots(e->N);
    return RPF_OK;
}

int transform_generic(rpf_engine* e, const uint8_t* d_frames, int64_t nframes, hipStream_t stream, int* nslots)
{
    HIP_TRY(e, rpf::launch_generic(e->N, d_frames, nframes, e->d_window, e->d_chirp, e->d_bhat, e->d_tw_sub,
                                   e->d_tw_sub2, e->gen_h, e->d_scratch, e->d_partial, /*accumulate=*/false, stream,
                                   e->format, e->stats));
    e->last = e->plan;
    *nslots = 1;
    return RPF_OK;
}

int transform_bigblu(rpf_engine* e, const uint8_t* d_frames, int64_t nframes, hipStream_t stream, int* nslots)
{
    const bool dma = e->use_dma && (reinterpret_cast<uintptr_t>(d_frames) % 4) == 0;
    if (int rc = ensure_scratch(e, nframes, stream)) return rc;
    HIP_TRY(e, rpf::launch_bigblu(e->N, dma, d_frames, nframes, e->d_tw_sub, e->d_tw_sub2, e->d_twiddles,
                                  e->d_step2, e->d_chirp, e->d_bhat, e->d_scratch, e->scratch_bytes, e->d_partial,
                                  e->plan.grid, stream));
    e->last = e->plan;
    *nslots = rpf::bigblu_partial_slots(e->N);
    return RPF_OK;
}

// (trims the grid to the frames itself: the split form needs a multiple of its factor)
int transform_mixed(rpf_engine* e, const uint8_t* d_frames, int64_t nframes, hipStream_t stream, int* nslots)
{
    HIP_TRY(e, rpf::launch_mixed(e->N, e->variant, d_frames, nframes, e->d_twiddles, e->d_window, e->d_partial,
                                 e->plan.grid, stream, &e->last));
    *nslots = e->last.slots ? e->last.slots : e->last.grid;
    return RPF_OK;
}

int transform_bluestein(rpf_engine* e, const uint8_t* d_frames, int64_t nframes, hipStream_t stream, int* nslots)
{
    const int64_t wanted = (nframes + e->plan.fpw - 1) / e->plan.fpw;
    const int grid = static_cast<int>(std::min<int64_t>(e->plan.grid, wanted));
    HIP_TRY(e, rpf::launch_bluestein(e->N, d_frames, nframes, e->d_twiddles, e->d_chirp, e->d_bhat,
                                     e->d_partial, grid, stream, &e->last));
    *nslots = grid;
    return RPF_OK;
}

// Enqueue the engine's transform for `nframes` frames starting at
// d_frames; leaves *nslots partial spectra in e->d_partial.  K1 reads the frames at the engine's frame step; every
// other family reads them side by side (launch_frames gathers overlapped frames for them first).
int launch_transform(rpf_engine* e, const uint8_t* d_frames, int64_t nframes, hipStream_t stream,
                     int* nslots)
{
    e->last_was_fused = false;
    switch (e->family) {
    case rpf::Family::K1: {     // one acquisition per launch (RPF_TUNE_SCAN_KERNEL, tuning build: the scan kernel on one hop, A/B)
        rpf::SlotRanges slots;
        return launch_fused_hops(e, &d_frames, &nframes, 1, stream, &slots, nslots);
    }
    case rpf::Family::Mixed: return transform_mixed(e, d_frames, nframes, stream, nslots);
    case rpf::Family::FourStep: return transform_fourstep(e, d_frames, nframes, stream, nslots);
    case rpf::Family::Bluestein: return transform_bluestein(e, d_frames, nframes, stream, nslots);
    case rpf::Family::BigBluestein: return transform_bigblu(e, d_frames, nframes, stream, nslots);
    case rpf::Family::Generic: return transform_generic(e, d_frames, nframes, stream, nslots);
    case rpf::Family::None: break;        // (a PFB engine: launch_pfb runs the inner engine's)
    }
    return fail(e, RPF_ERR_INVALID_ARGUMENT, "a PFB engine has no transform of its own");
}

// K3 over the e->last_slots partial spectra the last transform left (not a hop launch's, not a stats engine's).
// slot_verdict: launch_frames' -- null: a fused launch that gave up leaves d_out NaN-filled and is counted in
// h_fused_words[3]; else K3 leaves d_out alone and the word becomes 1.
int reduce_last(rpf_engine* e, double* d_out, bool accumulate, hipStream_t stream, unsigned* slot_verdict)
{
    const bool fused = e->last_was_fused;
    HIP_TRY(e, rpf::launch_reduce(e->d_partial, e->last_slots, e->N, d_out, accumulate, stream, e->partial_stride,
                                  fused && slot_verdict ? rpf::fourstep_fused_abort_word(e->d_fused_ctl) : nullptr));
    // a fused launch whose teams did not assemble must not leave something that looks like a spectrum
    if (fused)
        HIP_TRY(e, rpf::launch_fused_verdict(e->d_fused_ctl, slot_verdict ? nullptr : d_out, e->N,
                                             slot_verdict ? slot_verdict : e->d_fused_words + 3, e->d_fused_words + 4, stream));
    return RPF_OK;
}

// launch_frames for frames the transform reads where they lie (K1 at any frame step; the other families at step N)
int launch_side_by_side(rpf_engine* e, const uint8_t* d_frames, int64_t nframes, double* d_out, bool accumulate,
                        hipStream_t stream, unsigned* slot_verdict, bool want_stats)
{
    if (e->fused && !slot_verdict) note_device_path_aborts(e);
    e->last_was_cross = false;
    e->last_was_stft = false;
    int nslots = 0;
    int rc = launch_transform(e, d_frames, nframes, stream, &nslots);
    if (rc != RPF_OK) return rc;
    e->last_slots = nslots;
    e->last_hops = 0;
    if (e->stats) {
        // three planes per slot (K1: one slot per workgroup; the catch-all path: one slot)
        if (want_stats)
            HIP_TRY(e, rpf::launch_reduce_stats(e->d_partial, nslots, e->N, d_out, accumulate, stream));
        else
            HIP_TRY(e, rpf::launch_reduce(e->d_partial, nslots, e->N, d_out, accumulate, stream,
                                          static_cast<size_t>(rpf::kStatsPlanes) * e->N));
        return RPF_OK;
    }
    return reduce_last(e, d_out, accumulate, stream, slot_verdict);
}

// Overlapped frames on a family that reads frames side by side: chunks of at most kGatherBytes of frames are gathered
// into e->d_gather (rpf_frames.hip) and the size's unchanged transform + reduce runs over each, the chunks after the
// first adding into d_out.  (Four-step sizes are on the two-kernel path here: rpf_engine_create.)
int launch_gathered(rpf_engine* e, const uint8_t* d_frames, int64_t nframes, double* d_out, bool accumulate,
                    hipStream_t stream, bool want_stats)
{
    const size_t frame = e->sample_bytes * static_cast<size_t>(e->N);
    if (!e->d_gather) {
        e->gather_frames = std::max<int64_t>(1, static_cast<int64_t>(rpf::kGatherBytes / frame));
        HIP_TRY(e, hipMalloc(&e->d_gather, static_cast<size_t>(e->gather_frames) * frame));
    }
    const long pitch = static_cast<long>(e->sample_bytes) * e->step;
    for (int64_t f0 = 0; f0 < nframes; f0 += e->gather_frames) {
        const int64_t n = std::min(e->gather_frames, nframes - f0);
        HIP_TRY(e, rpf::launch_gather_frames(d_frames + f0 * pitch, n, pitch, static_cast<long>(frame), e->d_gather, stream));
        const int rc = launch_side_by_side(e, e->d_gather, n, d_out, accumulate || f0 > 0, stream, nullptr, want_stats);
        if (rc != RPF_OK) return rc;
    }
    return RPF_OK;
}

// A PFB engine: chunks of at most kGatherBytes of folded frames are produced in e->d_pfb_z (rpf_pfb.hip: one fold launch
// over the chunk's n + T - 1 input frames) and the inner cf32 engine's unchanged transform + reduce runs over each, the
// chunks after the first adding into d_out -- what launch_gathered does for overlapped frames.  The scratch comes from
// hipMalloc, so the inner launch sees a 16-byte aligned stream and stages it through LDS-DMA unless told not to.
int launch_pfb(rpf_engine* e, const uint8_t* d_frames, int64_t nframes, double* d_out, bool accumulate, hipStream_t stream)
{
    const size_t zframe = sizeof(float) * 2 * static_cast<size_t>(e->N);
    if (!e->d_pfb_z) {
        e->pfb_chunk_frames = std::max<int64_t>(1, static_cast<int64_t>(rpf::kGatherBytes / zframe));
        HIP_TRY(e, hipMalloc(&e->d_pfb_z, static_cast<size_t>(e->pfb_chunk_frames) * zframe));
    }
    const size_t row = e->sample_bytes * static_cast<size_t>(e->N);
    for (int64_t f0 = 0; f0 < nframes; f0 += e->pfb_chunk_frames) {
        const int64_t n = std::min(e->pfb_chunk_frames, nframes - f0);
        HIP_TRY(e, rpf::launch_pfb_fold(d_frames + static_cast<size_t>(f0) * row, n, e->N, e->taps, e->format, e->d_pfb_coeffs,
                                        e->d_pfb_z, stream));
        const int rc = launch_side_by_side(e->inner, reinterpret_cast<const uint8_t*>(e->d_pfb_z), n, d_out, accumulate || f0 > 0,
                                           stream, nullptr, false);
        if (rc != RPF_OK) return fail(e, rc, e->inner->last_error);
    }
    return RPF_OK;
}

// Transform + reduce for `nframes` frames starting at d_frames.
// slot_verdict: the queue path's pinned word for this launch -- if a fused launch gives up, K3 leaves d_out as it
// is, the word becomes 1 and the worker re-runs the bytes on K2a/K2b (recover_fused); null (the device-resident
// entries): d_out is NaN-filled and the launch counted in h_fused_words[3].
// want_stats (stats engines only): d_out is three planes of N, S1, S2, PK, combined with what it holds by +, +, max
// when `accumulate`; without it a stats engine's launch leaves S1 alone in d_out[N] (the same kernels, K3 over plane 0).
int launch_frames(rpf_engine* e, const uint8_t* d_frames, int64_t nframes, double* d_out,
                  bool accumulate, hipStream_t stream, unsigned* slot_verdict = nullptr, bool want_stats = false)
{
    if (nframes <= 0) return RPF_OK;
    if (e->taps) return launch_pfb(e, d_frames, nframes, d_out, accumulate, stream);
    if (overlapped(e) && !is_k1(e)) return launch_gathered(e, d_frames, nframes, d_out, accumulate, stream, want_stats);
    return launch_side_by_side(e, d_frames, nframes, d_out, accumulate, stream, slot_verdict, want_stats);
}

// Hands the pool's buffers back to the producer, each as soon as ITS copy has landed (datastore.cxx:91-94 returns a
// buffer when the worker is done with it; here "done" is the end of the H2D copy, not of the transform).  A thread of
// its own so that the consumer thread never blocks on a copy while new buffers are waiting to be issued: with five
// 1.6 MB buffers a blocking consumer alternated 4-buffer and 1-buffer groups and left the link idle between them
// (37 GB/s of the 54.5 GB/s large buffers reach).
void recycler_main(rpf_engine* e)
{
    (void)hipSetDevice(e->device);
    std::unique_lock<std::mutex> lk(e->recycle_mutex);
    for (;;) {
        wait_briefly_then_block(lk, e->recycle_cv, [&]() { return !e->recycle_queue.empty() || e->recycle_stop; });
        if (e->recycle_queue.empty()) break;                     // stop requested and everything handed back
        const std::pair<hipEvent_t, HostBuffer*> item = e->recycle_queue.front();
        e->recycle_queue.pop_front();
        lk.unlock();
        if (item.first) {
            const hipError_t err = hipEventSynchronize(item.first);
            if (err != hipSuccess && e->recycler_error.empty())
                e->recycler_error = std::string("hipEventSynchronize(copied): ") + hipGetErrorString(err);
        }
        const size_t landed = item.first ? item.second->size : 0;
        {
            std::lock_guard<std::mutex> status(e->status_mutex);
            e->empty_buffers.push_back(item.second);             // datastore.cxx:91-94
            e->status_change.notify_all();
        }
        lk.lock();
        e->bytes_landed += landed;
    }
}

// Consumer thread: the GPU counterpart of Datastore::fftThread.
void worker_main(rpf_engine* e)
{
    // First failure wins; after it the worker issues no further HIP work and only
    // keeps the hand-off protocol alive (buffers go straight back to the producer)
    // until rpf_finish reports the error.
    auto bail = [&](hipError_t err, const char* what) {
        if (e->worker_rc != RPF_OK) return;
        e->worker_rc = RPF_ERR_HARDWARE;
        e->worker_error = std::string(what) + ": " + hipGetErrorString(err);
    };
    auto ok = [&]() { return e->worker_rc == RPF_OK; };
#define WORKER_TRY(call, what)                          \
    do {                                                \
        if (ok()) {                                     \
            hipError_t err__ = (call);                  \
            if (err__ != hipSuccess) bail(err__, what); \
        }                                               \
    } while (0)
    WORKER_TRY(hipSetDevice(e->device), "hipSetDevice");
    {
        std::lock_guard<std::mutex> lk(e->recycle_mutex);
        e->recycle_stop = false;
        e->recycler_error.clear();
        e->bytes_landed = 0;
    }
    std::thread recycler;
    try {
        recycler = std::thread(recycler_main, e);
    } catch (const std::exception& ex) {
        // no second thread to be had: the acquisition fails (rpf_finish says why) and this thread keeps the hand-off
        // protocol alive by returning every buffer itself
        if (ok()) {
            e->worker_rc = RPF_ERR_HARDWARE;
            e->worker_error = std::string("cannot start the buffer recycler thread: ") + ex.what();
        }
    }
    auto hand_back = [&](HostBuffer* b, hipEvent_t copied) {
        if (!recycler.joinable()) {
            if (copied) (void)hipEventSynchronize(copied);
            std::lock_guard<std::mutex> status(e->status_mutex);
            e->empty_buffers.push_back(b);
            e->status_change.notify_all();
            return;
        }
        std::lock_guard<std::mutex> lk(e->recycle_mutex);
        e->recycle_queue.emplace_back(copied, b);
        e->recycle_cv.notify_one();
    };

    const size_t step_bytes = e->sample_bytes * static_cast<size_t>(e->step);    // frame f starts at byte f * step_bytes
    const size_t slot_bytes = e->coalesce * e->buffer_capacity;
    size_t carry = 0;             // bytes of an unfinished frame at the end of the previous slot
    const uint8_t* carry_src = nullptr;
    size_t slot_idx = 0;
    int64_t frames_issued = 0;    // == repeats_done once everything has drained
    // The staging slot being filled: buffers are copied into it one by one as the producer submits them -- each copy
    // issued at once, on alternating copy streams -- and ONE transform is launched over the slot when it is full or the
    // acquisition ends; the stream the kernels see is the concatenation of the buffers in FIFO order either way.
    StagingSlot* cur = nullptr;
    size_t off = 0;               // bytes copied into `cur`
    bool used[kCopyStreams] = {};
    unsigned next_stream = 0;
    size_t bytes_issued = 0;      // H2D bytes whose copy has been issued (against rpf_engine::bytes_landed)

    // A fused four-step launch gave up (its teams did not assemble: rpf_fourstep.hip): K3 has left d_pwr alone and the
    // slot still holds the launch's bytes.  Everything in flight is waited for, the engine leaves the fused kernel for
    // good, and every slot whose launch gave up is run again on K2a/K2b, oldest first -- the order of the additions
    // into d_pwr is the launch order whenever all fused launches in flight gave up (a device that has become busy),
    // and differs from it by the place of the re-run terms otherwise (double addition: ~1e-16 relative).
    // The reference's worker has no failure path (datastore.cxx:48-96); neither has this one for this cause.
    auto recover_fused = [&](size_t oldest) {
        WORKER_TRY(hipStreamSynchronize(e->compute_stream), "hipStreamSynchronize(recover)");
        retire_fused(e);
        for (size_t k = 0; k < e->staging.size(); ++k) {
            StagingSlot& s = e->staging[(oldest + k) % e->staging.size()];
            if (!s.launched_fused || !s.verdict || __atomic_load_n(s.verdict, __ATOMIC_ACQUIRE) == 0) continue;
            *s.verdict = 0;
            s.launched_fused = false;
            if (!ok()) continue;
            int rc = launch_frames(e, s.launch_ptr, s.launch_frames, e->d_pwr, /*accumulate=*/true, e->compute_stream);
            if (rc != RPF_OK) {
                e->worker_rc = rc;
                e->worker_error = e->last_error;
            }
            ++e->fused_recovered;
        }
        // (the re-runs read the slots: nothing may be copied into one before they are done)
        WORKER_TRY(hipStreamSynchronize(e->compute_stream), "hipStreamSynchronize(recover)");
        for (auto& s : e->staging) s.in_flight = false;
    };
    auto gave_up = [&](const StagingSlot& s) {
        return s.launched_fused && s.verdict && __atomic_load_n(s.verdict, __ATOMIC_ACQUIRE) != 0;
    };
    auto open_slot = [&]() {
        const size_t idx = slot_idx;
        cur = &e->staging[slot_idx];
        slot_idx = (slot_idx + 1) % e->staging.size();
        // The slot is free once its own kernel AND the following slot's carry copy (which read its tail) are done;
        // the latter precedes that slot's kernel_done in stream order.
        StagingSlot& after = e->staging[slot_idx];
        for (StagingSlot* s : {cur, &after}) {
            if (!s->in_flight) continue;
            WORKER_TRY(hipEventSynchronize(s->kernel_done), "hipEventSynchronize(kernel_done)");
            s->in_flight = false;
            if (gave_up(*s)) recover_fused(idx);        // (`cur` is the oldest slot in flight)
        }
        cur->launched_fused = false;
        off = 0;
        for (bool& u : used) u = false;
    };
    auto launch_slot = [&]() {
        if (!cur) return;
        // new bytes sit right after the head room; the carried partial frame goes immediately in front of them
        uint8_t* const dst = cur->base + e->head_room;
        for (int c = 0; c < kCopyStreams; ++c) {
            if (!used[c]) continue;
            WORKER_TRY(hipEventRecord(cur->copy_done[c], e->copy_streams[c]), "hipEventRecord(copy_done)");
            WORKER_TRY(hipStreamWaitEvent(e->compute_stream, cur->copy_done[c], 0), "hipStreamWaitEvent");
        }
        if (carry)
            WORKER_TRY(hipMemcpyAsync(dst - carry, carry_src, carry, hipMemcpyDeviceToDevice, e->compute_stream),
                       "hipMemcpyAsync(carry)");
        const size_t avail = carry + off;
        int64_t nframes = frames_in(e, avail);
        nframes = std::min<int64_t>(nframes, e->repeats - frames_issued);    // datastore.cxx:67
        if (ok() && nframes > 0) {
            if (cur->verdict) *cur->verdict = 0;
            int rc = launch_frames(e, dst - carry, nframes, e->d_pwr, /*accumulate=*/true, e->compute_stream, cur->verdict, e->stats);
            if (rc != RPF_OK) {
                e->worker_rc = rc;
                e->worker_error = e->last_error;
            }
            cur->launch_ptr = dst - carry;
            cur->launch_frames = nframes;
            cur->launched_fused = rc == RPF_OK && e->last_was_fused;
            frames_issued += nframes;
        }
        WORKER_TRY(hipEventRecord(cur->kernel_done, e->compute_stream), "hipEventRecord(kernel_done)");
        cur->in_flight = ok();
        // the unfinished frame (if any) stays in this slot until the next one is launched: what follows the last
        // frame's start + bS, less than a frame's span -- bN bytes, b T N on a PFB engine -- (everything, before the
        // first frame is complete)
        const size_t consumed = static_cast<size_t>(std::max<int64_t>(nframes, 0)) * step_bytes;
        carry = (frames_issued < e->repeats) ? avail - consumed : 0;
        carry_src = dst + off - carry;
        cur = nullptr;
        off = 0;
    };

    std::vector<HostBuffer*> batch;
    std::unique_lock<std::mutex> status_lock(e->status_mutex, std::defer_lock);
    while (true) {
        // Wait until we have a bufferful of data (datastore.cxx:54-64)
        status_lock.lock();
        wait_briefly_then_block(status_lock, e->status_change,
                                [&]() { return !e->occupied_buffers.empty() || e->acquisition_finished; });
        if (e->occupied_buffers.empty()) {
            status_lock.unlock();
            break;   // acquisition finished
        }
        batch.assign(e->occupied_buffers.begin(), e->occupied_buffers.end());
        e->occupied_buffers.clear();
        status_lock.unlock();

        // A lone buffer while the link is busy anyway: look a few microseconds longer for its neighbour -- two buffers that
        // lie next to each other in the pool travel in ONE copy (below), and a 1.6 MB copy pays ~4 us of set-up per 29 us of
        // transfer (tools/h2d_rate.cpp: 50 GB/s in 1.6 MB copies, 57 GB/s in 6.5 MB ones).  Costs nothing: at least two
        // buffers' worth of bytes are still on their way.
        if (batch.size() == 1 && ok() && !batch[0]->external) {
            size_t landed;
            {
                std::lock_guard<std::mutex> lk(e->recycle_mutex);
                landed = e->bytes_landed;
            }
            const size_t in_flight = bytes_issued - landed;
            if (in_flight >= 2 * e->buffer_capacity) {
                // (the more is on its way, the longer the look may take: a buffer's worth is ~30 us of link time)
                const auto deadline = std::chrono::steady_clock::now() +
                                      std::chrono::microseconds(in_flight >= 3 * e->buffer_capacity ? 20 : 8);
                do {
                    std::this_thread::yield();
                    status_lock.lock();
                    if (!e->occupied_buffers.empty()) {
                        batch.insert(batch.end(), e->occupied_buffers.begin(), e->occupied_buffers.end());
                        e->occupied_buffers.clear();
                    }
                    status_lock.unlock();
                } while (batch.size() == 1 && std::chrono::steady_clock::now() < deadline);
            }
        }

        for (size_t i = 0; i < batch.size();) {
            HostBuffer* const b = batch[i];
            // datastore.cxx:67: once the quota is met (by what is staged already) the rest of the stream is ignored
            const int64_t staged = frames_issued + frames_in(e, carry + off);
            if (!ok() || b->size == 0 || staged >= e->repeats) {
                if (!b->external) hand_back(b, nullptr);
                ++i;
                continue;
            }
            if (cur && off + b->size > slot_bytes) launch_slot();
            if (!cur) open_slot();
            // the run of buffers that follow b in the queue AND in memory (the pool is one allocation; the pieces of a
            // registered stream are consecutive anyway), as far as the slot and the quota take them: one copy
            size_t run = 1, bytes = b->size;
            while (i + run < batch.size()) {
                const HostBuffer* const nb = batch[i + run];
                if (nb->data != b->data + bytes || nb->size == 0 || nb->external != b->external || off + bytes + nb->size > slot_bytes) break;
                if (frames_issued + frames_in(e, carry + off + bytes) >= e->repeats) break;
                bytes += nb->size;
                ++run;
            }
            const unsigned c = next_stream;
            next_stream = (next_stream + 1) % kCopyStreams;
            WORKER_TRY(hipMemcpyAsync(cur->base + e->head_room + off, b->data, bytes, hipMemcpyHostToDevice, e->copy_streams[c]),
                       "hipMemcpyAsync(H2D)");
            HostBuffer* const last = batch[i + run - 1];
            if (!b->external) WORKER_TRY(hipEventRecord(last->copied, e->copy_streams[c]), "hipEventRecord(copied)");
            used[c] = true;
            off += bytes;
            bytes_issued += bytes;
            if (!b->external)
                for (size_t k = 0; k < run; ++k) hand_back(batch[i + k], ok() ? last->copied : nullptr);
            i += run;
        }
    }
    launch_slot();   // what the last, partly filled slot holds

    {
        std::lock_guard<std::mutex> lk(e->recycle_mutex);
        e->recycle_stop = true;
        e->recycle_cv.notify_one();
    }
    if (recycler.joinable()) recycler.join();             // every buffer is back in empty_buffers
    if (ok() && !e->recycler_error.empty()) {
        e->worker_rc = RPF_ERR_HARDWARE;
        e->worker_error = e->recycler_error;
    }

    WORKER_TRY(hipStreamSynchronize(e->compute_stream), "hipStreamSynchronize");
    // the launches still in flight at the end: any fused one that gave up is re-run now (slot_idx = the oldest slot)
    for (const auto& s : e->staging)
        if (ok() && gave_up(s)) {
            recover_fused(slot_idx);
            break;
        }
    for (auto& s : e->staging) {
        s.in_flight = false;
        s.launched_fused = false;
    }
    WORKER_TRY(hipMemcpy(e->pwr.data(), e->d_pwr, sizeof(double) * e->N, hipMemcpyDeviceToHost), "hipMemcpy(pwr)");
    if (e->stats) {
        WORKER_TRY(hipMemcpy(e->sum_sq.data(), e->d_pwr + e->N, sizeof(double) * e->N, hipMemcpyDeviceToHost), "hipMemcpy(sum_sq)");
        WORKER_TRY(hipMemcpy(e->peak.data(), e->d_pwr + 2 * static_cast<size_t>(e->N), sizeof(double) * e->N, hipMemcpyDeviceToHost),
                   "hipMemcpy(peak)");
    }
    e->repeats_done = frames_issued;
#undef WORKER_TRY
}

void release_device(rpf_engine* e);

// An engine this one made for itself (create_inner); `self`: the cross entries of a cf32 engine use the engine itself.
void destroy_inner(rpf_engine** slot, const rpf_engine* self)
{
    if (*slot && *slot != self) {
        release_device(*slot);
        delete *slot;
    }
    *slot = nullptr;
}

void release_device(rpf_engine* e)
{
    // every device block the engine owns (hipFree of a null pointer does nothing; d_fused_words is h_fused_words as the
    // device addresses it)
    void* const blocks[] = {e->d_twiddles, e->d_tw_sub, e->d_tw_sub2, e->d_scratch, e->d_fused_ctl, e->d_fused_scratch,
                            e->d_step2, e->d_gather, e->d_chirp, e->d_bhat, e->d_window, e->d_partial,
                            e->d_series_partial, e->d_series_in, e->d_series_out, e->d_excise_state, e->d_excise_mask,
                            e->d_quantile_rows, e->d_quantile_work, e->d_quantile_out, e->d_pfb_coeffs, e->d_pfb_z,
                            e->d_cross_uv, e->d_cross_planes, e->d_stft_rows, e->d_corr_rows, e->d_corr_partial,
                            e->d_corr_planes, e->d_dd_out, e->d_fold_scratch, e->d_fold_out, e->d_pwr};
    for (void* p : blocks) (void)hipFree(p);
    if (e->h_fused_words) (void)hipHostFree(e->h_fused_words);
    e->dd_tables.release();
    e->fold_steps.release();
    destroy_inner(&e->inner, e);
    destroy_inner(&e->cross_inner, e);
    destroy_inner(&e->stft_inner, e);
    for (auto& s : e->staging) {
        if (s.base) (void)hipFree(s.base);
        if (s.kernel_done) (void)hipEventDestroy(s.kernel_done);
        for (hipEvent_t ev : s.copy_done)
            if (ev) (void)hipEventDestroy(ev);
    }
    for (hipStream_t cs : e->copy_streams)
        if (cs) (void)hipStreamDestroy(cs);
    if (e->compute_stream) (void)hipStreamDestroy(e->compute_stream);
    for (auto& b : e->pool) {
        if (b.data && !e->pool_base) (void)hipHostFree(b.data);
        if (b.copied) (void)hipEventDestroy(b.copied);
    }
    if (e->pool_base) (void)hipHostFree(e->pool_base);
    for (const auto& r : e->registered) (void)hipHostUnregister(const_cast<uint8_t*>(r.first));
}

}  // namespace

extern "C" {

int rpf_abi_version(void) { return RPF_ABI_VERSION; }

int rpf_supported_n(int N)
{
    return (rpf::kernel_supported(N) || rpf::fourstep_supported(N) || rpf::mixed_supported(N) || rpf::bluestein_supported(N) ||
            rpf::bigblu_supported(N) || rpf::generic_supported(N)) ? 1 : 0;
}

const char* rpf_last_global_error(void) { return g_last_error.c_str(); }

}  // extern "C"

namespace {

struct PfbSpec {
    int taps;
    const float* coeffs;      // taps x N
};

// What check_config reads out of a configuration it accepts.
struct Checked {
    int step, format, variant;
    size_t sample_bytes;
    bool stats;
    rpf::Family family;
};

// Every argument check of rpf_engine_create (pfb null) and rpf_engine_create_pfb, all of them before any device is
// touched (include/rpf_engine.h) and in the order callers see them answered.
int check_config(const rpf_config* cfg, const PfbSpec* pfb, rpf_engine** out, Checked* c)
{
    auto bad = [](const std::string& msg) { return fail(nullptr, RPF_ERR_INVALID_ARGUMENT, msg); };
    if (!out) return bad("rpf_engine_create: out is NULL");
    *out = nullptr;
    // (the config of ABI 2's first form ends at `flags`: frame step N)
    if (!cfg || (cfg->struct_size != sizeof(rpf_config) && cfg->struct_size != offsetof(rpf_config, frame_step)))
        return bad("rpf_engine_create: bad rpf_config size");
    if (cfg->N < 2 || (cfg->N % 2) != 0) return bad("Number of bins must be a positive even number.");
    const std::string bins = std::to_string(cfg->N);
    const int32_t frame_step = cfg->struct_size == sizeof(rpf_config) ? cfg->frame_step : 0;
    if (frame_step < 0 || frame_step > cfg->N)
        return bad("Frame step must be between 1 and the number of bins (" + bins + "), or 0 for " + bins + "; got " +
                   std::to_string(frame_step) + ".");
    c->step = frame_step == 0 ? cfg->N : frame_step;
    c->format = static_cast<int>((cfg->flags >> 16) & 0xfu);
    if (c->format != RPF_FORMAT_CU8 && c->format != RPF_FORMAT_CS8 && c->format != RPF_FORMAT_CS16 && c->format != RPF_FORMAT_CF32)
        return bad("Sample format must be 0 (cu8), 1 (cs8), 2 (cs16) or 4 (cf32); got " + std::to_string(c->format) + ".");
    c->sample_bytes = static_cast<size_t>(rpf::sample_bytes_of(c->format));
    c->stats = (cfg->flags & RPF_FLAG_BIN_STATS) != 0;
    c->variant = static_cast<int>((cfg->flags >> 8) & 0xffu);
    const bool ask_fused = (cfg->flags & RPF_FLAG_FOURSTEP_FUSED) != 0;
    if (c->stats && ask_fused)
        return bad("RPF_FLAG_BIN_STATS does not combine with RPF_FLAG_FOURSTEP_FUSED: the statistics run on K1 or on the catch-all path.");
    if (c->stats && c->variant != 0) return bad("RPF_FLAG_BIN_STATS does not combine with a kernel variant other than 0.");
    if (pfb) {
        if (pfb->taps < 1 || pfb->taps > rpf::kPfbMaxTaps)
            return bad("Number of PFB taps must be between 1 and " + std::to_string(rpf::kPfbMaxTaps) + "; got " +
                       std::to_string(pfb->taps) + ".");
        if (static_cast<int64_t>(pfb->taps) * cfg->N > (static_cast<int64_t>(1) << 26))
            return bad("PFB taps x bins must not exceed 67108864; got " + std::to_string(pfb->taps) + " x " + bins + ".");
        if (!pfb->coeffs) return bad("rpf_engine_create_pfb: coeffs is NULL");
        if (cfg->window) return bad("A PFB engine takes no window: the PFB coefficients are the window.");
        if (c->step != cfg->N)
            return bad("PFB frames advance by the number of bins: frame_step must be 0 or " + bins + "; got " +
                       std::to_string(frame_step) + ".");
        if (c->stats) return bad("PFB does not combine with RPF_FLAG_BIN_STATS.");
        if (ask_fused)
            return bad("PFB does not combine with RPF_FLAG_FOURSTEP_FUSED: the folded frames run on K1 or on the catch-all path.");
        if (c->variant != 0) return bad("PFB does not combine with a kernel variant other than 0.");
    }
    // the kernel family (engine_family.h has the rule), from what this build has at N
    const int N = cfg->N, v = c->variant;
    const rpf::FamilyQuery q{N, v, c->format == RPF_FORMAT_CU8, c->stats, cfg->window != nullptr,
                             (cfg->flags & RPF_FLAG_CATCH_ALL) != 0, (cfg->flags & RPF_FLAG_NO_MIXED_RADIX) != 0, ask_fused,
                             rpf::kernel_supported(N, 0), rpf::kernel_supported(N, v), rpf::mixed_supported(N, v),
                             rpf::fourstep_supported(N), rpf::bluestein_supported(N), rpf::bigblu_supported(N),
                             rpf::generic_supported(N)};
    c->family = pfb ? rpf::Family::None : rpf::select_family(q);
    // (a PFB engine transforms nothing itself: what counts is that its inner cf32 engine has a kernel)
    if (pfb ? !(q.k1_v0 || q.generic) : c->family == rpf::Family::None)
        return bad("No gfx950 kernel for " + bins +
                   " bins in this build (supported: every even N up to 8388608 and the powers of two up to 67108864).");
    if (cfg->n_buffers < 1) return bad("Argument to 'buffers' must be a positive number.");
    if (cfg->buffer_capacity < 2 || (cfg->buffer_capacity % 2) != 0)
        return bad("Buffer size must be a positive even number of bytes.");
    if (static_cast<size_t>(cfg->buffer_capacity) % c->sample_bytes != 0)
        return bad("Buffer size must be a multiple of the sample size (" + std::to_string(c->sample_bytes) + " bytes).");
    return RPF_OK;
}

rpf_engine* new_engine(const rpf_config* cfg, const Checked& c, const PfbSpec* pfb)
{
    rpf_engine* e = new rpf_engine();
    e->N = cfg->N;
    e->step = c.step;
    e->format = c.format;
    e->sample_bytes = c.sample_bytes;
    e->has_window = cfg->window != nullptr;
    e->flags = cfg->flags;
    if (cfg->window) e->window.assign(cfg->window, cfg->window + cfg->N);
    e->n_buffers = cfg->n_buffers;
    e->buffer_capacity = static_cast<size_t>(cfg->buffer_capacity);
    e->device = cfg->device;
    e->use_dma = !(cfg->flags & RPF_FLAG_NO_LDS_DMA);
    e->variant = c.variant;
    e->stats = c.stats;
    if (c.stats) {
        e->sum_sq.assign(e->N, 0.0);
        e->peak.assign(e->N, 0.0);
    }
    e->family = c.family;
    e->taps = pfb ? pfb->taps : 0;
    e->queue_histogram.assign(e->n_buffers + 1, 0);
    e->pwr.assign(e->N, 0.0);
    return e;
}

// ---- the steps of a creation: each returns its code, create_engine frees everything once on any but RPF_OK ----

// *d_ptr = a device block holding the `count` values at `host`
template <class T, class U>
int upload(rpf_engine* e, T** d_ptr, const U* host, size_t count)
{
    HIP_TRY(e, hipMalloc(d_ptr, sizeof(U) * count));
    HIP_TRY(e, hipMemcpy(*d_ptr, host, sizeof(U) * count, hipMemcpyHostToDevice));
    return RPF_OK;
}

// master twiddles W_n^k ("plan": where fftwf_plan_dft_1d stands, datastore.cxx:32)
int upload_twiddles(rpf_engine* e, rpf::cf** d_ptr, int n)
{
    std::vector<rpf::cf> tw;
    rpf::make_twiddles(n, tw);
    return upload(e, d_ptr, tw.data(), tw.size());
}

// room for `slots` partial spectra of `len` doubles
int alloc_partial(rpf_engine* e, size_t slots, size_t len)
{
    HIP_TRY(e, hipMalloc(&e->d_partial, sizeof(double) * len * slots));
    return RPF_OK;
}

// ---- one prepare per family: its tables on the device, e->plan, the partial spectra, the scratch policy ----

// master twiddles of the transform length and the window as it is given: what K1 and the mixed-radix kernels read
int upload_twiddles_and_window(rpf_engine* e, const rpf_config* cfg)
{
    if (int rc = upload_twiddles(e, &e->d_twiddles, e->N)) return rc;
    return cfg->window ? upload(e, &e->d_window, cfg->window, static_cast<size_t>(e->N)) : RPF_OK;
}

int prepare_k1(rpf_engine* e, const rpf_config* cfg)
{
    if (int rc = upload_twiddles_and_window(e, cfg)) return rc;
    HIP_TRY(e, rpf::plan_launch(e->N, e->variant, e->has_window, true, e->device, &e->plan, e->format, e->stats));
    rpf::LaunchInfo tmp;
    HIP_TRY(e, rpf::plan_launch(e->N, e->variant, e->has_window, false, e->device, &tmp, e->format, e->stats));
    e->plan.grid = std::min(e->plan.grid, tmp.grid);
    // a workgroup leaves one partial per hop it touches; a stats engine's: three planes per workgroup, no scans
    const size_t grid = e->plan.grid;
    return alloc_partial(e, e->stats ? grid * rpf::kStatsPlanes : grid + rpf::kMaxHops, e->N);
}

int prepare_mixed(rpf_engine* e, const rpf_config* cfg)
{
    if (int rc = upload_twiddles_and_window(e, cfg)) return rc;
    HIP_TRY(e, rpf::plan_mixed(e->N, e->variant, e->has_window, e->device, &e->plan));
    return alloc_partial(e, e->plan.grid, e->N);
}

// bluestein_tables.h's g and bhat (the window is in g: the Bluestein families have no window table)
int upload_chirp(rpf_engine* e, const rpf_config* cfg)
{
    std::vector<float> g, bhat;
    rpf::make_bluestein_tables(e->N, cfg->window, g, bhat);
    if (int rc = upload(e, &e->d_chirp, g.data(), g.size())) return rc;
    return upload(e, &e->d_bhat, bhat.data(), bhat.size());
}

int prepare_bluestein(rpf_engine* e, const rpf_config* cfg)
{
    if (int rc = upload_twiddles(e, &e->d_twiddles, rpf::bluestein_length(e->N))) return rc;
    if (int rc = upload_chirp(e, cfg)) return rc;
    HIP_TRY(e, rpf::plan_bluestein(e->N, e->device, &e->plan));
    return alloc_partial(e, e->plan.grid, e->N);
}

int prepare_bigblu(rpf_engine* e, const rpf_config* cfg)
{
    int M = 0, m1 = 0, m2 = 0;
    rpf::bigblu_lengths(e->N, &M, &m1, &m2);
    HIP_TRY(e, rpf::bigblu_prepare(e->N, e->device, &e->plan));
    // the kernels read chirp, kernel spectrum and inter-step twiddles in their own lane order
    std::vector<float> g, bhat;
    rpf::make_bluestein_tables(e->N, cfg->window, g, bhat);
    std::vector<rpf::cf> g_t, bhat_t, step_tw, step_tw2;
    rpf::bigblu_tables(e->N, reinterpret_cast<const rpf::cf*>(g.data()), reinterpret_cast<const rpf::cf*>(bhat.data()), g_t,
                       bhat_t, step_tw, step_tw2);
    int rc = upload_twiddles(e, &e->d_tw_sub, m1);
    if (rc == RPF_OK) rc = upload_twiddles(e, &e->d_tw_sub2, m2);
    if (rc == RPF_OK) rc = upload(e, &e->d_chirp, g_t.data(), g_t.size());
    if (rc == RPF_OK) rc = upload(e, &e->d_bhat, bhat_t.data(), bhat_t.size());
    if (rc == RPF_OK) rc = upload(e, &e->d_twiddles, step_tw.data(), step_tw.size());
    if (rc == RPF_OK) rc = upload(e, &e->d_step2, step_tw2.data(), step_tw2.size());
    if (rc != RPF_OK) return rc;
    // (the intermediate starts at 256 MB and grows with the launches: ensure_scratch)
    e->scratch_per_frame = rpf::bigblu_scratch_bytes_per_frame(e->N);
    e->scratch_max = rpf::bigblu_scratch_bytes(e->N);
    e->scratch_bytes = std::min<size_t>(e->scratch_max, std::max<size_t>(e->scratch_per_frame, static_cast<size_t>(256) << 20));
    HIP_TRY(e, hipMalloc(&e->d_scratch, e->scratch_bytes));
    e->partial_stride = static_cast<size_t>(M);          // partial spectra of M (not N) doubles each
    return alloc_partial(e, rpf::bigblu_partial_slots(e->N), M);
}

int prepare_fourstep(rpf_engine* e, const rpf_config* cfg)
{
    HIP_TRY(e, rpf::fourstep_prepare(e->N, e->device, &e->plan));
    int n1 = 0, n2 = 0;
    rpf::fourstep_sub_lengths(e->N, &n1, &n2);
    // K2a reads the inter-step twiddles and the window in its own lane order
    std::vector<rpf::cf> step_tw;
    std::vector<float> window_t;
    rpf::fourstep_tables(e->N, cfg->window, step_tw, window_t);
    int rc = upload_twiddles(e, &e->d_tw_sub, n1);
    if (rc == RPF_OK) rc = upload_twiddles(e, &e->d_tw_sub2, n2);
    if (rc == RPF_OK) rc = upload(e, &e->d_twiddles, step_tw.data(), step_tw.size());
    if (rc == RPF_OK && cfg->window) rc = upload(e, &e->d_window, window_t.data(), window_t.size());
    if (rc != RPF_OK) return rc;
    // The fused kernel (one persistent launch, the intermediate stays in each XCD's L2) where
    // the device is the 8 x 32-CU part it is written for and its teams assemble; else K2a/K2b.
    int fused_grid = 0;
    // (overlapped frames: the two-kernel path -- the fused kernel's give-up verdict is one word per staging slot,
    // which the gather path's several launches per slot would share)
    if (!(cfg->flags & RPF_FLAG_NO_FOURSTEP_FUSED) && e->step == e->N &&
        rpf::fourstep_fused_prepare(e->N, e->device, &fused_grid) == hipSuccess) {
        HIP_TRY(e, hipMalloc(&e->d_fused_scratch, rpf::fourstep_fused_scratch_bytes(e->N)));
        HIP_TRY(e, hipMalloc(&e->d_fused_ctl, rpf::fourstep_fused_ctl_bytes()));
        HIP_TRY(e, hipHostMalloc(reinterpret_cast<void**>(&e->h_fused_words), 64, hipHostMallocMapped));
        std::memset(e->h_fused_words, 0, 64);
        HIP_TRY(e, hipHostGetDevicePointer(reinterpret_cast<void**>(&e->d_fused_words), e->h_fused_words, 0));
        e->fused = true;
        // (room for either path's partial spectra: a fused launch that gives up is re-run on K2a/K2b)
        return alloc_partial(e, std::max<size_t>(rpf::fourstep_fused_slots(e->N), rpf::fourstep_partial_slots(e->N)), e->N);
    }
    (void)hipGetLastError();
    e->scratch_per_frame = rpf::fourstep_scratch_bytes_per_frame(e->N);
    e->scratch_max = rpf::fourstep_scratch_bytes(e->N);
    e->scratch_bytes = std::min<size_t>(e->scratch_max, static_cast<size_t>(256) << 20);
    HIP_TRY(e, hipMalloc(&e->d_scratch, e->scratch_bytes));
    return alloc_partial(e, rpf::fourstep_partial_slots(e->N), e->N);
}

int prepare_generic(rpf_engine* e, const rpf_config* cfg)
{
    std::vector<rpf::cf> t0, t1;
    rpf::generic_twiddle_tables(e->N, t0, t1, &e->gen_h);
    int rc = upload(e, &e->d_tw_sub, t0.data(), t0.size());
    if (rc == RPF_OK) rc = upload(e, &e->d_tw_sub2, t1.data(), t1.size());
    if (rc == RPF_OK && cfg->window) rc = upload(e, &e->d_window, cfg->window, static_cast<size_t>(e->N));
    if (rc == RPF_OK && rpf::generic_length(e->N) != e->N) rc = upload_chirp(e, cfg);      // its Bluestein form
    if (rc != RPF_OK) return rc;
    HIP_TRY(e, hipMalloc(&e->d_scratch, rpf::generic_scratch_bytes(e->N)));
    hipDeviceProp_t prop;
    HIP_TRY(e, hipGetDeviceProperties(&prop, e->device));
    e->plan.grid = prop.multiProcessorCount;
    e->plan.block = 256;
    e->plan.fpw = rpf::generic_batch(e->N);
    e->plan.lds_bytes = 0;
    return alloc_partial(e, e->stats ? rpf::kStatsPlanes : 1, e->N);
}

int prepare_family(rpf_engine* e, const rpf_config* cfg)
{
    switch (e->family) {
    case rpf::Family::K1: return prepare_k1(e, cfg);
    case rpf::Family::Mixed: return prepare_mixed(e, cfg);
    case rpf::Family::FourStep: return prepare_fourstep(e, cfg);
    case rpf::Family::Bluestein: return prepare_bluestein(e, cfg);
    case rpf::Family::BigBluestein: return prepare_bigblu(e, cfg);
    case rpf::Family::Generic: return prepare_generic(e, cfg);
    case rpf::Family::None: break;        // (a PFB engine: create_pfb makes the inner engine, which has the tables)
    }
    return RPF_OK;
}

// Prove once that the eight teams assemble on this device (one round per team on a dummy
// stream); if they do not, this engine uses the two-kernel path.
int prove_fused(rpf_engine* e)
{
    const size_t round_bytes = 2u * 262144u * 8u;         // FR frames of N samples for each of 8 teams
    void* d_dummy = nullptr;
    struct FreeOnExit {                                   // (every exit of this function)
        void*& p;
        ~FreeOnExit() { (void)hipFree(p); }
    } free_dummy{d_dummy};
    HIP_TRY(e, hipMalloc(&d_dummy, round_bytes));
    HIP_TRY(e, hipMemset(d_dummy, 0x80, round_bytes));
    bool aborted = true;
    hipError_t lerr = rpf::launch_fourstep_fused(e->N, e->has_window, true, static_cast<const uint8_t*>(d_dummy),
                                                 static_cast<long>(round_bytes / (2u * static_cast<size_t>(e->N))),
                                                 e->d_tw_sub, e->d_tw_sub2, e->d_twiddles, e->d_window, e->d_fused_scratch,
                                                 e->d_partial, e->d_fused_ctl, e->compute_stream);
    if (lerr == hipSuccess) lerr = rpf::fourstep_fused_aborted(e->d_fused_ctl, e->compute_stream, &aborted);
    if (lerr != hipSuccess || aborted) {
        (void)hipGetLastError();
        retire_fused(e);
        (void)hipFree(e->d_fused_scratch);          // (nothing is in flight here)
        e->d_fused_scratch = nullptr;
        e->scratch_bytes = std::min<size_t>(e->scratch_max, static_cast<size_t>(256) << 20);
        HIP_TRY(e, hipMalloc(&e->d_scratch, e->scratch_bytes));
    }
    return RPF_OK;
}

// The buffer pool, the device staging ring and the verdict words of its slots.  inner_of_pfb: the transform engine a
// PFB engine owns -- it is never fed through its queues, so its staging slots hold one (minimal) buffer each.
int create_queues(rpf_engine* e, bool inner_of_pfb)
{
    // buffer pool: pinned host memory (datastore.cxx:27-28)
    // ONE allocation, the buffers side by side: what the producer fills in order the consumer can send in one copy.
    // (If that much pinned memory is not to be had in one piece: buffer by buffer, as before.)
    e->pool.resize(e->n_buffers);
    {
        void* p = nullptr;
        if (hipHostMalloc(&p, e->buffer_capacity * static_cast<size_t>(e->n_buffers), hipHostMallocDefault) == hipSuccess)
            e->pool_base = static_cast<uint8_t*>(p);
        else
            (void)hipGetLastError();
    }
    for (size_t k = 0; k < e->pool.size(); ++k) {
        HostBuffer& b = e->pool[k];
        if (e->pool_base) {
            b.data = e->pool_base + k * e->buffer_capacity;
        } else {
            void* p = nullptr;
            HIP_TRY(e, hipHostMalloc(&p, e->buffer_capacity, hipHostMallocDefault));
            b.data = static_cast<uint8_t*>(p);
        }
        b.size = e->buffer_capacity;
        HIP_TRY(e, hipEventCreateWithFlags(&b.copied, hipEventDisableTiming));
        e->empty_buffers.push_back(&b);
    }
    // device staging ring: head room for a carried partial frame + one buffer
    // (a PFB engine carries up to a whole span, b T N bytes, less one sample)
    e->head_room = (frame_bytes(e).frame + 255) / 256 * 256;
    // a slot (= one transform launch) holds as many buffers as fit 32 MB, at least one -- more than the pool has where the
    // buffers are small: they return to the producer when their copy lands, not when the slot is launched
    e->coalesce = inner_of_pfb ? 1 : std::max<size_t>(1, (32u << 20) / e->buffer_capacity);
    e->staging.resize(kStagingSlots);
    for (auto& s : e->staging) {
        HIP_TRY(e, hipMalloc(&s.base, e->head_room + e->coalesce * e->buffer_capacity));
        HIP_TRY(e, hipEventCreateWithFlags(&s.kernel_done, hipEventDisableTiming));
        for (hipEvent_t& ev : s.copy_done) HIP_TRY(e, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    static_assert(kStagingSlots <= 3, "h_fused_words[0 .. 2]: one verdict word per staging slot");
    if (e->h_fused_words)
        for (size_t k = 0; k < e->staging.size(); ++k) e->staging[k].verdict = e->h_fused_words + k;
    return RPF_OK;
}

int create_engine(const rpf_config* cfg, const PfbSpec* pfb, bool inner_of_pfb, rpf_engine** out);

// An engine of this one's N and device that serves it from the inside (a PFB engine's transform, the cross entries'
// cf32 engine, the STFT's catch-all engine): never fed through its queues, so it has one minimal buffer.  A creation
// that fails has said why in g_last_error; that becomes this engine's message too.
int create_inner(rpf_engine* e, uint32_t flags, const float* window, int frame_step, rpf_engine** slot)
{
    rpf_config icfg;
    icfg.struct_size = sizeof(icfg);
    icfg.N = e->N;
    icfg.window = window;
    icfg.n_buffers = 1;
    icfg.buffer_capacity = 8;
    icfg.device = e->device;
    icfg.flags = flags;
    icfg.frame_step = frame_step;
    const int rc = create_engine(&icfg, nullptr, /*inner_of_pfb=*/true, slot);
    return rc == RPF_OK ? rc : fail(e, rc, g_last_error);
}

// The window an inner engine is created from: this engine's, as it was given.
const float* window_as_given(const rpf_engine* e) { return e->window.empty() ? nullptr : e->window.data(); }

// A PFB engine's coefficients and its transform: a rectangular cf32 engine of the same N, device and staging flag.
int create_pfb(rpf_engine* e, const rpf_config* cfg, const PfbSpec* pfb)
{
    if (int rc = upload(e, &e->d_pfb_coeffs, pfb->coeffs, static_cast<size_t>(e->taps) * static_cast<size_t>(e->N))) return rc;
    return create_inner(e, (cfg->flags & (RPF_FLAG_NO_LDS_DMA | RPF_FLAG_CATCH_ALL)) | RPF_FLAG_SAMPLE_FORMAT(RPF_FORMAT_CF32),
                        nullptr, 0, &e->inner);
}

// Everything a new engine owns on its device, step by step; the first step that fails has said why and ends it.
int build_engine(rpf_engine* e, const rpf_config* cfg, const PfbSpec* pfb, bool inner_of_pfb)
{
    DeviceScope on_device(e->device);       // the caller's current device is restored on return
    HIP_TRY(e, on_device.status());
    for (hipStream_t& cs : e->copy_streams) HIP_TRY(e, hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    HIP_TRY(e, hipStreamCreateWithFlags(&e->compute_stream, hipStreamNonBlocking));
    if (int rc = prepare_family(e, cfg)) return rc;
    const size_t pwr_bytes = sizeof(double) * e->N * (e->stats ? rpf::kStatsPlanes : 1);
    HIP_TRY(e, hipMalloc(&e->d_pwr, pwr_bytes));
    HIP_TRY(e, hipMemset(e->d_pwr, 0, pwr_bytes));
    if (int rc = e->fused ? prove_fused(e) : RPF_OK) return rc;
    if (int rc = create_queues(e, inner_of_pfb)) return rc;
    return pfb ? create_pfb(e, cfg, pfb) : RPF_OK;
}

// rpf_engine_create (pfb null) and rpf_engine_create_pfb: check, new engine, build.  A failed build frees everything and
// clears the sticky HIP error (it is not the caller's next HIP call's problem); rpf_last_global_error says what failed.
int create_engine(const rpf_config* cfg, const PfbSpec* pfb, bool inner_of_pfb, rpf_engine** out)
{
    Checked c;
    if (int rc = check_config(cfg, pfb, out, &c)) return rc;
    int ndev = 0;
    hipError_t err = hipGetDeviceCount(&ndev);
    if (err != hipSuccess || ndev < 1)
        return fail(nullptr, RPF_ERR_HARDWARE,
                    std::string("No HIP device available (") + (err != hipSuccess ? hipGetErrorString(err) : "device count 0") +
                        "); this engine has no CPU path.");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, RPF_ERR_INVALID_ARGUMENT, "Invalid HIP device ordinal.");
    rpf_engine* e = new_engine(cfg, c, pfb);
    const int rc = build_engine(e, cfg, pfb, inner_of_pfb);
    if (rc != RPF_OK) {
        (void)hipGetLastError();
        DeviceScope on_device(e->device);
        release_device(e);
        delete e;
        return rc;
    }
    *out = e;
    return RPF_OK;
}

}  // namespace

extern "C" {

int rpf_engine_create(const rpf_config* cfg, rpf_engine** out) { return create_engine(cfg, nullptr, false, out); }

int rpf_engine_create_pfb(const rpf_config* cfg, int taps, const float* coeffs, rpf_engine** out)
{
    const PfbSpec pfb{taps, coeffs};
    return create_engine(cfg, &pfb, false, out);
}

int rpf_pfb_taps(const rpf_engine* e) { return e ? e->taps : -1; }

void rpf_engine_destroy(rpf_engine* e)
{
    if (!e) return;
    if (e->worker_running) {
        int64_t dummy;
        (void)rpf_finish(e, &dummy);
    }
    {
        DeviceScope on_device(e->device);
        release_device(e);
    }
    delete e;
}

const char* rpf_last_error(const rpf_engine* e) { return e ? e->last_error.c_str() : g_last_error.c_str(); }

int rpf_begin(rpf_engine* e, int64_t repeats)
{
    if (!e) return fail(nullptr, RPF_ERR_INVALID_ARGUMENT, "rpf_begin: NULL engine");
    if (e->worker_running) return fail(e, RPF_ERR_INVALID_ARGUMENT, "rpf_begin: acquisition already running");
    if (repeats < 0) return fail(e, RPF_ERR_INVALID_ARGUMENT, "Argument to 'repeats' must be a positive number.");
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    // acquisition.cxx:252-254
    std::fill(e->pwr.begin(), e->pwr.end(), 0.0);
    if (e->stats) {
        std::fill(e->sum_sq.begin(), e->sum_sq.end(), 0.0);
        std::fill(e->peak.begin(), e->peak.end(), 0.0);
    }
    HIP_TRY(e, hipMemsetAsync(e->d_pwr, 0, sizeof(double) * e->N * (e->stats ? rpf::kStatsPlanes : 1), e->compute_stream));
    {
        std::lock_guard<std::mutex> lock(e->status_mutex);
        e->acquisition_finished = false;
    }
    e->repeats_done = 0;
    e->repeats = repeats;
    e->worker_rc = RPF_OK;
    e->worker_error.clear();
    // acquisition.cxx:256
    try {
        e->worker = std::thread(worker_main, e);
    } catch (const std::exception& ex) {      // (no exception crosses the C boundary)
        return fail(e, RPF_ERR_HARDWARE, std::string("rpf_begin: cannot start the consumer thread: ") + ex.what());
    }
    e->worker_running = true;
    return RPF_OK;
}

int rpf_buffer_acquire(rpf_engine* e, uint8_t** buf, size_t* capacity)
{
    if (!e || !buf) return fail(e, RPF_ERR_INVALID_ARGUMENT, "rpf_buffer_acquire: NULL argument");
    // acquisition.cxx:278-285
    std::unique_lock<std::mutex> lock(e->status_mutex);
    e->queue_histogram[e->empty_buffers.size()]++;
    wait_briefly_then_block(lock, e->status_change, [&]() { return !e->empty_buffers.empty(); });
    HostBuffer* b = e->empty_buffers.front();
    e->empty_buffers.pop_front();
    lock.unlock();
    *buf = b->data;
    if (capacity) *capacity = e->buffer_capacity;
    return RPF_OK;
}

static HostBuffer* find_buffer(rpf_engine* e, const uint8_t* p)
{
    for (auto& b : e->pool)
        if (b.data == p) return &b;
    return nullptr;
}

int rpf_buffer_submit(rpf_engine* e, uint8_t* buf, size_t nbytes)
{
    if (!e) return fail(nullptr, RPF_ERR_INVALID_ARGUMENT, "rpf_buffer_submit: NULL engine");
    HostBuffer* b = find_buffer(e, buf);
    if (!b) return fail(e, RPF_ERR_INVALID_ARGUMENT, "rpf_buffer_submit: not an engine buffer");
    if (nbytes > e->buffer_capacity || (nbytes % 2) != 0)
        return fail(e, RPF_ERR_INVALID_ARGUMENT, "rpf_buffer_submit: size must be even and <= capacity");
    if (nbytes % e->sample_bytes != 0)     // a sample never straddles two buffers (frames may)
        return fail(e, RPF_ERR_INVALID_ARGUMENT, "rpf_buffer_submit: size must be a multiple of the sample size (" +
                                                     std::to_string(e->sample_bytes) + " bytes)");
    if (!e->worker_running) return fail(e, RPF_ERR_INVALID_ARGUMENT, "rpf_buffer_submit: no acquisition running");
    b->size = nbytes;   // buffer.resize(dataNeeded), acquisition.cxx:302
    // acquisition.cxx:320-323
    std::lock_guard<std::mutex> lock(e->status_mutex);
    e->occupied_buffers.push_back(b);
    e->status_change.notify_all();
    return RPF_OK;
}

int rpf_buffer_unget(rpf_engine* e, uint8_t* buf)
{
    if (!e) return fail(nullptr, RPF_ERR_INVALID_ARGUMENT, "rpf_buffer_unget: NULL engine");
    HostBuffer* b = find_buffer(e, buf);
    if (!b) return fail(e, RPF_ERR_INVALID_ARGUMENT, "rpf_buffer_unget: not an engine buffer");
    // acquisition.cxx:310-314 (no notify needed)
    std::lock_guard<std::mutex> lock(e->status_mutex);
    e->empty_buffers.push_front(b);
    return RPF_OK;
}

int rpf_finish(rpf_engine* e, int64_t* repeats_done)
{
    if (!e) return fail(nullptr, RPF_ERR_INVALID_ARGUMENT, "rpf_finish: NULL engine");
    if (!e->worker_running) return fail(e, RPF_ERR_INVALID_ARGUMENT, "rpf_finish: no acquisition running");
    // acquisition.cxx:343-347
    {
        std::lock_guard<std::mutex> lock(e->status_mutex);
        e->acquisition_finished = true;
        e->status_change.notify_all();
    }
    e->worker.join();
    e->worker_running = false;
    if (repeats_done) *repeats_done = e->repeats_done;
    if (e->worker_rc != RPF_OK) return fail(e, e->worker_rc, e->worker_error);
    return RPF_OK;
}

int rpf_get_power(const rpf_engine* e, double* out)
{
    if (!e || !out) return RPF_ERR_INVALID_ARGUMENT;
    // datastore.h:40-47: results are read only after the worker has been joined
    if (e->worker_running)
        return fail(const_cast<rpf_engine*>(e), RPF_ERR_INVALID_ARGUMENT,
                    "rpf_get_power: acquisition still running (call rpf_finish first)");
    std::memcpy(out, e->pwr.data(), sizeof(double) * e->N);
    return RPF_OK;
}

int rpf_has_bin_stats(const rpf_engine* e) { return e && e->stats ? 1 : 0; }

int rpf_get_bin_stats(const rpf_engine* e, double* sum_sq, double* peak)
{
    if (!e) return RPF_ERR_INVALID_ARGUMENT;
    rpf_engine* me = const_cast<rpf_engine*>(e);
    if (!e->stats) return fail(me, RPF_ERR_INVALID_ARGUMENT, "rpf_get_bin_stats: the engine was created without RPF_FLAG_BIN_STATS");
    if (e->worker_running)
        return fail(me, RPF_ERR_INVALID_ARGUMENT, "rpf_get_bin_stats: acquisition still running (call rpf_finish first)");
    if (sum_sq) std::memcpy(sum_sq, e->sum_sq.data(), sizeof(double) * e->N);
    if (peak) std::memcpy(peak, e->peak.data(), sizeof(double) * e->N);
    return RPF_OK;
}

int rpf_copy_power_device(const rpf_engine* e, double* d_dst, void* hip_stream, int dst_device)
{
    if (!e || !d_dst) return RPF_ERR_INVALID_ARGUMENT;
    rpf_engine* me = const_cast<rpf_engine*>(e);
    if (e->worker_running)
        return fail(me, RPF_ERR_INVALID_ARGUMENT, "rpf_copy_power_device: acquisition still running (call rpf_finish first)");
    DeviceScope on_device(e->device);
    HIP_TRY(me, on_device.status());
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (dst_device == e->device)
        HIP_TRY(me, hipMemcpyAsync(d_dst, e->d_pwr, sizeof(double) * e->N, hipMemcpyDeviceToDevice, s));
    else
        HIP_TRY(me, hipMemcpyPeerAsync(d_dst, dst_device, e->d_pwr, e->device, sizeof(double) * e->N, s));
    HIP_TRY(me, hipStreamSynchronize(s));
    return RPF_OK;
}

int64_t rpf_get_repeats_done(const rpf_engine* e) { return e ? e->repeats_done : 0; }

int rpf_get_histogram(const rpf_engine* e, int* out)
{
    if (!e || !out) return RPF_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(const_cast<rpf_engine*>(e)->status_mutex);
    std::memcpy(out, e->queue_histogram.data(), sizeof(int) * e->queue_histogram.size());
    return RPF_OK;
}

// The producer side of rpf_accumulate: pageable stream -> pinned hand-off buffer.  One thread copies
// ~10 GB/s, a fifth of what the H2D link behind it takes, so a large buffer is filled by several threads
// (measured with 5 x 105 MB buffers: 8.0 -> see bench.py's end_to_end; small buffers are not worth a fork).
static void fill_buffer(uint8_t* dst, const uint8_t* src, size_t n)
{
    constexpr size_t kPiece = 4u << 20;
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t want = std::min<size_t>(std::min<size_t>(hw ? hw : 1, 8), n / kPiece);
    if (want < 2) {
        std::memcpy(dst, src, n);
        return;
    }
    std::vector<std::thread> helpers;
    const size_t share = (n / want + 63) & ~static_cast<size_t>(63);
    size_t forked_from = n;          // [0, forked_from) is copied by this thread: its own share, plus what no helper took
    try {
        helpers.reserve(want - 1);
        for (size_t t = want - 1; t >= 1; --t) {      // from the far end, so that what is left over is one run
            const size_t lo = t * share, hi = std::min(n, lo + share);
            if (lo < hi) {
                helpers.emplace_back([=]() { std::memcpy(dst + lo, src + lo, hi - lo); });
                forked_from = lo;
            }
        }
    } catch (...) {
        // std::thread could not start (thread limit, out of memory): nothing may leave rpf_accumulate's
        // extern "C" frame as an exception -- this thread copies the rest itself
    }
    std::memcpy(dst, src, std::min(n, forked_from));
    for (std::thread& h : helpers) h.join();
}

int rpf_accumulate(rpf_engine* e, const uint8_t* stream, size_t nbytes, int64_t repeats,
                   double* pwr_out, int64_t* repeats_done)
{
    if (!e || (!stream && nbytes)) return fail(e, RPF_ERR_INVALID_ARGUMENT, "rpf_accumulate: NULL argument");
    int rc = rpf_begin(e, repeats);
    if (rc != RPF_OK) return rc;
    size_t pos = 0;
    const size_t cap = e->buffer_capacity;
    // A stream the caller has pinned (rpf_stream_register): no copy into the pool -- its pieces go to the consumer as they
    // lie, and the consumer sends neighbours in one copy, a staging slot at a time.
    std::vector<HostBuffer> pieces;
    for (const auto& r : e->registered) {
        if (stream >= r.first && stream + nbytes <= r.first + r.second) {
            const size_t whole = ~(e->sample_bytes - 1);       // (2, 4 or 8: whole samples)
            const size_t piece = std::min<size_t>(e->coalesce * e->buffer_capacity, static_cast<size_t>(8) << 20) & whole;
            const size_t even = nbytes & whole;
            pieces.reserve(even / piece + 1);
            for (size_t at = 0; at < even; at += piece) {
                HostBuffer hb;
                hb.data = const_cast<uint8_t*>(stream) + at;
                hb.size = std::min(piece, even - at);
                hb.external = true;
                pieces.push_back(hb);
            }
            {
                std::lock_guard<std::mutex> lock(e->status_mutex);
                for (HostBuffer& hb : pieces) e->occupied_buffers.push_back(&hb);
                e->status_change.notify_all();
            }
            pos = nbytes;
            break;
        }
    }
    while (pos < nbytes) {
        uint8_t* buf = nullptr;
        rc = rpf_buffer_acquire(e, &buf, nullptr);
        if (rc != RPF_OK) break;
        const size_t n = std::min(cap, (nbytes - pos) & ~(e->sample_bytes - 1));
        if (n == 0) {
            rpf_buffer_unget(e, buf);
            break;
        }
        fill_buffer(buf, stream + pos, n);
        rc = rpf_buffer_submit(e, buf, n);
        if (rc != RPF_OK) break;
        pos += n;
    }
    int64_t done = 0;
    int rc2 = rpf_finish(e, &done);
    if (rc == RPF_OK) rc = rc2;
    if (repeats_done) *repeats_done = done;
    if (rc == RPF_OK && pwr_out) std::memcpy(pwr_out, e->pwr.data(), sizeof(double) * e->N);
    return rc;
}

// rpf_accumulate_device and rpf_accumulate_device_stats (want_stats: needs a stats engine, d_out is its three planes)
static int accumulate_device(rpf_engine* e, const char* who, bool want_stats, const void* d_stream, size_t nbytes,
                             int64_t repeats, double* d_out, void* hip_stream, int64_t* repeats_done)
{
    if (!e || !d_out || (!d_stream && nbytes)) return refuse(e, who, "NULL argument");
    if (want_stats && !e->stats) return refuse(e, who, "the engine was created without RPF_FLAG_BIN_STATS");
    int rc = refuse_if_running(e, who);
    if (rc == RPF_OK) rc = refuse_negative_repeats(e, repeats);
    if (rc == RPF_OK) rc = refuse_unaligned_stream(e, who, "d_stream", d_stream);
    if (rc == RPF_OK) rc = refuse_unaligned_out(e, who, want_stats ? "d_out" : "d_pwr_out", d_out);
    if (rc != RPF_OK) return rc;
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    hipStream_t s = static_cast<hipStream_t>(hip_stream);   // NULL = the HIP null stream
    int64_t nframes = frames_in(e, nbytes);
    nframes = std::min(nframes, repeats);
    if (repeats_done) *repeats_done = nframes;
    if (nframes == 0) {
        HIP_TRY(e, hipMemsetAsync(d_out, 0, sizeof(double) * e->N * (want_stats ? rpf::kStatsPlanes : 1), s));
        return RPF_OK;
    }
    return launch_frames(e, static_cast<const uint8_t*>(d_stream), nframes, d_out, /*accumulate=*/false, s, nullptr, want_stats);
}

int rpf_accumulate_device(rpf_engine* e, const void* d_stream, size_t nbytes, int64_t repeats,
                          double* d_pwr_out, void* hip_stream, int64_t* repeats_done)
{
    return accumulate_device(e, "rpf_accumulate_device", false, d_stream, nbytes, repeats, d_pwr_out, hip_stream, repeats_done);
}

int rpf_accumulate_device_stats(rpf_engine* e, const void* d_stream, size_t nbytes, int64_t repeats,
                                double* d_out, void* hip_stream, int64_t* repeats_done)
{
    return accumulate_device(e, "rpf_accumulate_device_stats", true, d_stream, nbytes, repeats, d_out, hip_stream, repeats_done);
}

// ---- cross-spectrum of two streams: four power spectra and the polarisation identity (include/rpf_engine.h) ----------

// Everything both cross entries refuse, before any launch.
static int cross_check(rpf_engine* e, const char* who, const void* a, const void* b, size_t nbytes, int64_t repeats,
                       const void* out)
{
    if (!e || !out || ((!a || !b) && nbytes)) return refuse(e, who, "NULL argument");
    int rc = refuse_stats_engine(e, who);
    if (rc == RPF_OK && e->taps) rc = refuse(e, who, "not on a PFB engine");
    if (rc == RPF_OK) rc = refuse_variant(e, who);
    if (rc == RPF_OK) rc = refuse_if_running(e, who);
    if (rc == RPF_OK) rc = refuse_negative_repeats(e, repeats);
    if (rc == RPF_OK) rc = refuse_ragged_bytes(e, who, nbytes);
    return rc;
}

// The cf32 engine (a cf32 engine: itself) and the scratch of the cross entries, made at the first call.
static int ensure_cross(rpf_engine* e)
{
    if (!e->cross_inner) {
        if (e->format == RPF_FORMAT_CF32) {
            e->cross_inner = e;
        } else {
            const uint32_t flags = (e->flags & ~RPF_FLAG_SAMPLE_FORMAT(0xf)) | RPF_FLAG_SAMPLE_FORMAT(RPF_FORMAT_CF32);
            if (int rc = create_inner(e, flags, window_as_given(e), e->step, &e->cross_inner)) return rc;
        }
    }
    const size_t N = static_cast<size_t>(e->N), S = static_cast<size_t>(e->step);
    if (!e->d_cross_uv) {
        const rpf::FrameBytes fb{sizeof(float) * 2 * N, sizeof(float) * 2 * S};
        const int64_t chunk = std::max<int64_t>(1, fb.frames_in(rpf::kGatherBytes));
        const size_t floats = fb.span(chunk) / sizeof(float);              // of one stream
        const size_t v_offset = (floats + 63) / 64 * 64;                   // v starts 256-byte aligned
        HIP_TRY(e, hipMalloc(&e->d_cross_uv, sizeof(float) * (v_offset + floats)));
        e->cross_chunk_frames = chunk;
        e->cross_v_offset = v_offset;
    }
    if (!e->d_cross_planes) HIP_TRY(e, hipMalloc(&e->d_cross_planes, sizeof(double) * 2 * rpf::kCrossPlanes * N));
    return RPF_OK;
}

// Paa, Pbb, Puu, Pvv of `nframes` frames of d_a and d_b into (accumulate: added to) e->d_cross_planes, on `s`: the two
// streams through this engine's own path, then per chunk of whole frames one combine launch over the chunk's span of
// samples and the cf32 engine's path over u and over v, the chunks after the first adding.
static int cross_enqueue(rpf_engine* e, const uint8_t* d_a, const uint8_t* d_b, int64_t nframes, bool accumulate, hipStream_t s)
{
    const size_t N = static_cast<size_t>(e->N);
    double* const planes = e->d_cross_planes;
    rpf_engine* const in = e->cross_inner;
    int rc = launch_frames(e, d_a, nframes, planes, accumulate, s);
    if (rc == RPF_OK) rc = launch_frames(e, d_b, nframes, planes + N, accumulate, s);
    if (rc != RPF_OK) return rc;
    float* const u = e->d_cross_uv;
    float* const v = u + e->cross_v_offset;
    const size_t pitch = e->sample_bytes * static_cast<size_t>(e->step);
    for (int64_t f0 = 0; f0 < nframes; f0 += e->cross_chunk_frames) {
        const int64_t n = std::min(e->cross_chunk_frames, nframes - f0);
        const long samples = static_cast<long>(e->N) + static_cast<long>(e->step) * static_cast<long>(n - 1);
        HIP_TRY(e, rpf::launch_cross_combine(d_a + static_cast<size_t>(f0) * pitch, d_b + static_cast<size_t>(f0) * pitch, samples,
                                             e->format, u, v, s));
        rc = launch_frames(in, reinterpret_cast<const uint8_t*>(u), n, planes + 2 * N, accumulate || f0 > 0, s);
        if (rc == RPF_OK) rc = launch_frames(in, reinterpret_cast<const uint8_t*>(v), n, planes + 3 * N, accumulate || f0 > 0, s);
        if (rc != RPF_OK) return in == e ? rc : fail(e, rc, in->last_error);
    }
    e->last_was_cross = true;
    return RPF_OK;
}

int rpf_accumulate_device_cross(rpf_engine* e, const void* d_a, const void* d_b, size_t nbytes, int64_t repeats, double* d_out,
                                void* hip_stream, int64_t* repeats_done)
{
    const char* who = "rpf_accumulate_device_cross";
    int rc = cross_check(e, who, d_a, d_b, nbytes, repeats, d_out);
    if (rc == RPF_OK) rc = refuse_unaligned_stream(e, who, "d_a and d_b",
                                                     reinterpret_cast<const void*>(reinterpret_cast<uintptr_t>(d_a) | reinterpret_cast<uintptr_t>(d_b)));
    if (rc == RPF_OK) rc = refuse_unaligned_out(e, who, "d_out", d_out);
    if (rc != RPF_OK) return rc;
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const int64_t nframes = std::min(frames_in(e, nbytes), repeats);
    if (repeats_done) *repeats_done = nframes;
    if (nframes == 0) {
        HIP_TRY(e, hipMemsetAsync(d_out, 0, sizeof(double) * rpf::kCrossPlanes * e->N, s));
        return RPF_OK;
    }
    if ((rc = ensure_cross(e)) != RPF_OK) return rc;
    rc = cross_enqueue(e, static_cast<const uint8_t*>(d_a), static_cast<const uint8_t*>(d_b), nframes, /*accumulate=*/false, s);
    if (rc != RPF_OK) return rc;
    HIP_TRY(e, rpf::launch_cross_finish(e->d_cross_planes, e->N, d_out, s));
    return RPF_OK;
}

int rpf_accumulate_cross(rpf_engine* e, const uint8_t* a, const uint8_t* b, size_t nbytes, int64_t repeats, double* out,
                         int64_t* repeats_done)
{
    int rc = cross_check(e, "rpf_accumulate_cross", a, b, nbytes, repeats, out);
    if (rc != RPF_OK) return rc;
    const int64_t nframes = std::min(frames_in(e, nbytes), repeats);
    if (repeats_done) *repeats_done = nframes;
    const size_t out_doubles = rpf::kCrossPlanes * static_cast<size_t>(e->N);
    if (nframes == 0) {
        std::fill(out, out + out_doubles, 0.0);
        return RPF_OK;
    }
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    hipStream_t s = e->compute_stream;
    if ((rc = ensure_cross(e)) != RPF_OK) return rc;
    // pieces of whole frames (L = 1), one piece of each stream at a time, side by side
    const uint8_t* const streams[2] = {a, b};
    rc = series_host_pieces(
        e, streams, 2, 1, nframes, INT64_MAX, [](int64_t) { return static_cast<int>(RPF_OK); },
        [&](int64_t k0, int64_t kc, hipStream_t ps) {
            return cross_enqueue(e, e->d_series_in, e->d_series_in + e->series_in_stride, kc, /*accumulate=*/k0 > 0, ps);
        });
    if (rc != RPF_OK) return rc;
    double* const d_result = e->d_cross_planes + out_doubles;
    HIP_TRY(e, rpf::launch_cross_finish(e->d_cross_planes, e->N, d_result, s));
    return copy_back(e, out, d_result, sizeof(double) * out_doubles, s);
}

// ---- the frames' spectra themselves: rpf_stft_device, rpf_stft (include/rpf_engine.h has the definition) -------------

// Everything both entries refuse, before any launch.
static int stft_check(rpf_engine* e, const char* who, const void* stream, size_t nbytes, int64_t max_frames, const void* out)
{
    if (!e || !out || !stream) return refuse(e, who, "NULL argument");
    int rc = refuse_not_power_of_two(e, who);
    if (rc == RPF_OK) rc = refuse_stats_engine(e, who);
    if (rc == RPF_OK) rc = refuse_variant(e, who);
    if (rc == RPF_OK) rc = refuse_if_running(e, who);
    if (rc == RPF_OK && max_frames < 0) rc = refuse(e, who, "max_frames must not be negative");
    if (rc == RPF_OK) rc = refuse_ragged_bytes(e, who, nbytes);
    return rc;
}

// K1's store kernels serve every K1 engine the checks let through.
static bool stft_native(const rpf_engine* e) { return is_k1(e) && rpf::stft_supported(e->N, e->format); }

// What the engine's route needs, made at the first call: the store kernels' grid, or the catch-all engine of a family
// that is neither K1 nor the catch-all, or (PFB) the fold's scratch and what the inner engine's route needs.
static int ensure_stft(rpf_engine* e)
{
    if (e->taps) {
        if (!e->d_pfb_z) {
            const size_t zframe = sizeof(float) * 2 * static_cast<size_t>(e->N);
            e->pfb_chunk_frames = std::max<int64_t>(1, static_cast<int64_t>(rpf::kGatherBytes / zframe));
            HIP_TRY(e, hipMalloc(&e->d_pfb_z, static_cast<size_t>(e->pfb_chunk_frames) * zframe));
        }
        const int rc = ensure_stft(e->inner);
        return rc == RPF_OK ? rc : fail(e, rc, e->inner->last_error);
    }
    if (stft_native(e)) {
        if (!e->stft_planned) {
            HIP_TRY(e, rpf::plan_stft(e->N, e->has_window, e->device, &e->stft_plan, e->format));
            e->stft_planned = true;
        }
        return RPF_OK;
    }
    if (e->family == rpf::Family::Generic || e->stft_inner) return RPF_OK;
    return create_inner(e, (e->flags & (RPF_FLAG_NO_LDS_DMA | RPF_FLAG_SAMPLE_FORMAT(0xf))) | RPF_FLAG_CATCH_ALL, window_as_given(e),
                        e->step, &e->stft_inner);
}

// One launch of the plain or (frame step != N) the strided store kernel: rows [0, nframes) of d_out.
static int transform_stft_k1(rpf_engine* e, const uint8_t* d_frames, int64_t nframes, rpf::cf* d_out, hipStream_t s)
{
    const int64_t wanted = (nframes + e->stft_plan.fpw - 1) / e->stft_plan.fpw;
    const int grid = static_cast<int>(std::min<int64_t>(e->stft_plan.grid, wanted));
    const long pitch = static_cast<long>(e->sample_bytes) * e->step;
    const bool dma = e->use_dma && (reinterpret_cast<uintptr_t>(d_frames) % 16) == 0 && pitch % 16 == 0;
    HIP_TRY(e, rpf::launch_fft_stft(e->N, e->has_window, dma, d_frames, nframes, e->d_twiddles, e->d_window, d_out, grid, s,
                                    &e->last, pitch, e->format));
    return RPF_OK;
}

// The catch-all engine's Stockham transform with the rows as its last pass's destination (rpf_generic.hip), in batches
// of generic_batch(N) frames; overlapped frames go through the frame gather first, a chunk of scratch at a time.
static int transform_stft_generic(rpf_engine* e, const uint8_t* d_frames, int64_t nframes, rpf::cf* d_out, hipStream_t s)
{
    const size_t frame = e->sample_bytes * static_cast<size_t>(e->N);
    auto rows = [&](const uint8_t* side_by_side, int64_t n, rpf::cf* d_rows) {
        HIP_TRY(e, rpf::launch_generic(e->N, side_by_side, n, e->d_window, e->d_chirp, e->d_bhat, e->d_tw_sub, e->d_tw_sub2,
                                       e->gen_h, e->d_scratch, nullptr, false, s, e->format, false, d_rows));
        e->last = e->plan;
        return RPF_OK;
    };
    if (!overlapped(e)) return rows(d_frames, nframes, d_out);
    if (!e->d_gather) {
        e->gather_frames = std::max<int64_t>(1, static_cast<int64_t>(rpf::kGatherBytes / frame));
        HIP_TRY(e, hipMalloc(&e->d_gather, static_cast<size_t>(e->gather_frames) * frame));
    }
    const long pitch = static_cast<long>(e->sample_bytes) * e->step;
    for (int64_t f0 = 0; f0 < nframes; f0 += e->gather_frames) {
        const int64_t n = std::min(e->gather_frames, nframes - f0);
        HIP_TRY(e, rpf::launch_gather_frames(d_frames + f0 * pitch, n, pitch, static_cast<long>(frame), e->d_gather, s));
        if (int rc = rows(e->d_gather, n, d_out + static_cast<size_t>(f0) * e->N)) return rc;
    }
    return RPF_OK;
}

static int stft_enqueue(rpf_engine* e, const uint8_t* d_frames, int64_t nframes, rpf::cf* d_out, hipStream_t s);

// A PFB engine, the channelizer: the existing fold per chunk of scratch, then the inner cf32 engine's STFT of the folded
// frames into the chunk's rows.
static int transform_stft_pfb(rpf_engine* e, const uint8_t* d_frames, int64_t nframes, rpf::cf* d_out, hipStream_t s)
{
    const size_t row = e->sample_bytes * static_cast<size_t>(e->N);
    for (int64_t f0 = 0; f0 < nframes; f0 += e->pfb_chunk_frames) {
        const int64_t n = std::min(e->pfb_chunk_frames, nframes - f0);
        HIP_TRY(e, rpf::launch_pfb_fold(d_frames + static_cast<size_t>(f0) * row, n, e->N, e->taps, e->format, e->d_pfb_coeffs,
                                        e->d_pfb_z, s));
        const int rc = stft_enqueue(e->inner, reinterpret_cast<const uint8_t*>(e->d_pfb_z), n, d_out + static_cast<size_t>(f0) * e->N, s);
        if (rc != RPF_OK) return fail(e, rc, e->inner->last_error);
    }
    return RPF_OK;
}

// Rows [0, nframes) of d_out on `s` by the engine's route (ensure_stft has run).
static int stft_enqueue(rpf_engine* e, const uint8_t* d_frames, int64_t nframes, rpf::cf* d_out, hipStream_t s)
{
    e->last_was_cross = false;
    e->last_was_stft = false;
    if (e->taps) return transform_stft_pfb(e, d_frames, nframes, d_out, s);
    if (stft_native(e)) return transform_stft_k1(e, d_frames, nframes, d_out, s);
    if (e->family == rpf::Family::Generic) return transform_stft_generic(e, d_frames, nframes, d_out, s);
    const int rc = transform_stft_generic(e->stft_inner, d_frames, nframes, d_out, s);
    if (rc != RPF_OK) return fail(e, rc, e->stft_inner->last_error);
    e->last_was_stft = true;
    return RPF_OK;
}

int rpf_stft_device(rpf_engine* e, const void* d_stream, size_t nbytes, int64_t max_frames, void* d_out, int64_t* frames_done,
                    void* hip_stream)
{
    const char* who = "rpf_stft_device";
    int rc = stft_check(e, who, d_stream, nbytes, max_frames, d_out);
    if (rc == RPF_OK) rc = refuse_unaligned_stream(e, who, "d_stream", d_stream);
    if (rc == RPF_OK) rc = refuse_unaligned_out(e, who, "d_out", d_out);
    if (rc != RPF_OK) return rc;
    const int64_t nframes = std::min(frames_in(e, nbytes), max_frames);
    if (frames_done) *frames_done = 0;
    if (nframes == 0) return RPF_OK;
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    if ((rc = ensure_stft(e)) != RPF_OK) return rc;
    rc = stft_enqueue(e, static_cast<const uint8_t*>(d_stream), nframes, static_cast<rpf::cf*>(d_out),
                      static_cast<hipStream_t>(hip_stream));
    if (rc == RPF_OK && frames_done) *frames_done = nframes;         // (rows that were enqueued, never rows that were not)
    return rc;
}

int rpf_stft(rpf_engine* e, const uint8_t* stream, size_t nbytes, int64_t max_frames, void* out, int64_t* frames_done)
{
    int rc = stft_check(e, "rpf_stft", stream, nbytes, max_frames, out);
    if (rc != RPF_OK) return rc;
    const int64_t nframes = std::min(frames_in(e, nbytes), max_frames);
    if (frames_done) *frames_done = 0;
    if (nframes == 0) return RPF_OK;
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    hipStream_t s = e->compute_stream;
    if ((rc = ensure_stft(e)) != RPF_OK) return rc;
    // The series family's piece loop with one frame per integration and the rows as the second bound (series_pieces.h,
    // stft_pieces: the cap is budget / row bytes): a piece's rows go to d_stft_rows and come back in ONE copy.
    const size_t row_floats = 2 * static_cast<size_t>(e->N);
    const int64_t row_cap = rpf::stft_pieces(frame_bytes(e), sizeof(float) * row_floats).per_piece;
    float* const host_rows = static_cast<float*>(out);
    return series_host_pieces(
        e, &stream, 1, 1, nframes, row_cap,
        [&](int64_t per_piece) {
            return grow_scratch(e, &e->d_stft_rows, &e->stft_rows, static_cast<size_t>(per_piece), sizeof(float) * row_floats, s);
        },
        [&](int64_t k0, int64_t kc, hipStream_t ps) {
            if (int prc = stft_enqueue(e, e->d_series_in, kc, reinterpret_cast<rpf::cf*>(e->d_stft_rows), ps)) return prc;
            HIP_TRY(e, hipMemcpyAsync(host_rows + static_cast<size_t>(k0) * row_floats, e->d_stft_rows,
                                      sizeof(float) * row_floats * static_cast<size_t>(kc), hipMemcpyDeviceToHost, ps));
            return static_cast<int>(RPF_OK);
        },
        frames_done);
}

// ---- the correlator of up to eight streams: rpf_correlate_device, rpf_correlate (include/rpf_engine.h) ---------------

// Everything both entries refuse, before any launch.
static int correlate_check(rpf_engine* e, const char* who, const void* const* streams, int n_streams, size_t nbytes,
                           int64_t repeats, const void* out)
{
    bool null = !e || !streams || !out;
    for (int m = 0; !null && m < n_streams && m < rpf::kCorrelateMaxStreams; ++m) null = !streams[m];
    if (null) return refuse(e, who, "NULL argument");
    if (n_streams < rpf::kCorrelateMinStreams || n_streams > rpf::kCorrelateMaxStreams)
        return refuse(e, who, "n_streams must be 2 to 8; got " + std::to_string(n_streams));
    int rc = refuse_not_power_of_two(e, who);
    if (rc == RPF_OK) rc = refuse_stats_engine(e, who);
    if (rc == RPF_OK) rc = refuse_variant(e, who);
    if (rc == RPF_OK) rc = refuse_if_running(e, who);
    if (rc == RPF_OK) rc = refuse_negative_repeats(e, repeats);
    if (rc == RPF_OK) rc = refuse_ragged_bytes(e, who, nbytes);
    return rc;
}

// What the STFT route needs, the rows scratch of M streams, the X-engine's partial planes and the running planes (the
// host entry: and its result), made at the first call and grown for a call with more streams.
static int ensure_correlate(rpf_engine* e, int M, bool host, hipStream_t s)
{
    int rc = ensure_stft(e);
    if (rc != RPF_OK) return rc;
    const size_t N = static_cast<size_t>(e->N), MM = static_cast<size_t>(M) * static_cast<size_t>(M);
    const int64_t C = rpf::correlate_chunk_frames(e->N);
    if ((rc = grow_scratch(e, &e->d_corr_rows, &e->corr_rows, static_cast<size_t>(M) * static_cast<size_t>(C),
                           sizeof(float) * 2 * N, s)) != RPF_OK)
        return rc;
    const int64_t G = rpf::correlate_groups(e->N, M, C);
    if (G > 1 && (rc = grow_scratch(e, &e->d_corr_partial, &e->corr_partial, static_cast<size_t>(G) * MM * N, sizeof(double), s)) != RPF_OK)
        return rc;
    return grow_scratch(e, &e->d_corr_planes, &e->corr_planes, (host ? 3 : 1) * MM * N, sizeof(double), s);
}

// The M^2 running planes of `nframes` frames of the M device streams into (accumulate: added to) e->d_corr_planes, on
// `s`: per chunk of correlate_chunk_frames(N) frames the M streams' rows by the STFT route (stream m from frame f0 at
// byte f0 b S) into rows block m, then the X-engine over the chunk, the chunks after the first adding.
static int correlate_enqueue(rpf_engine* e, const uint8_t* const* d_streams, int M, int64_t nframes, bool accumulate, hipStream_t s)
{
    const int64_t C = rpf::correlate_chunk_frames(e->N);
    const size_t block = static_cast<size_t>(C) * static_cast<size_t>(e->N);          // complex values per rows block
    const size_t pitch = frame_bytes(e).pitch;
    rpf::cf* const rows = reinterpret_cast<rpf::cf*>(e->d_corr_rows);
    for (int64_t f0 = 0; f0 < nframes; f0 += C) {
        const int64_t n = std::min(C, nframes - f0);
        for (int m = 0; m < M; ++m)
            if (int rc = stft_enqueue(e, d_streams[m] + static_cast<size_t>(f0) * pitch, n, rows + m * block, s)) return rc;
        HIP_TRY(e, rpf::launch_correlate_xengine(e->d_corr_rows, static_cast<long>(block), M, e->N, n,
                                                 rpf::correlate_groups(e->N, M, n), e->d_corr_partial, e->d_corr_planes,
                                                 accumulate || f0 > 0, s));
    }
    return RPF_OK;
}

int rpf_correlate_device(rpf_engine* e, const void* const* d_streams, int n_streams, size_t nbytes, int64_t repeats, double* d_out,
                         void* hip_stream, int64_t* frames_done)
{
    const char* who = "rpf_correlate_device";
    if (frames_done) *frames_done = 0;
    int rc = correlate_check(e, who, d_streams, n_streams, nbytes, repeats, d_out);
    for (int m = 0; rc == RPF_OK && m < n_streams; ++m) rc = refuse_unaligned_stream(e, who, "every stream", d_streams[m]);
    if (rc == RPF_OK) rc = refuse_unaligned_out(e, who, "d_out", d_out);
    if (rc != RPF_OK) return rc;
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const int64_t nframes = std::min(frames_in(e, nbytes), repeats);
    const size_t out_doubles = 2 * static_cast<size_t>(n_streams) * static_cast<size_t>(n_streams) * static_cast<size_t>(e->N);
    if (nframes == 0) {
        HIP_TRY(e, hipMemsetAsync(d_out, 0, sizeof(double) * out_doubles, s));
        return RPF_OK;
    }
    if ((rc = ensure_correlate(e, n_streams, /*host=*/false, s)) != RPF_OK) return rc;
    const uint8_t* ptrs[rpf::kCorrelateMaxStreams];
    for (int m = 0; m < n_streams; ++m) ptrs[m] = static_cast<const uint8_t*>(d_streams[m]);
    if ((rc = correlate_enqueue(e, ptrs, n_streams, nframes, /*accumulate=*/false, s)) != RPF_OK) return rc;
    HIP_TRY(e, rpf::launch_correlate_finish(e->d_corr_planes, n_streams, e->N, d_out, s));
    if (frames_done) *frames_done = nframes;                          // (frames that were enqueued, never frames that were not)
    return RPF_OK;
}

int rpf_correlate(rpf_engine* e, const uint8_t* const* streams, int n_streams, size_t nbytes, int64_t repeats, double* out,
                  int64_t* frames_done)
{
    if (frames_done) *frames_done = 0;
    int rc = correlate_check(e, "rpf_correlate", reinterpret_cast<const void* const*>(streams), n_streams, nbytes, repeats, out);
    if (rc != RPF_OK) return rc;
    const int64_t nframes = std::min(frames_in(e, nbytes), repeats);
    const size_t MM = static_cast<size_t>(n_streams) * static_cast<size_t>(n_streams), N = static_cast<size_t>(e->N);
    if (nframes == 0) {
        std::fill(out, out + 2 * MM * N, 0.0);
        return RPF_OK;
    }
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    hipStream_t s = e->compute_stream;
    if ((rc = ensure_correlate(e, n_streams, /*host=*/true, s)) != RPF_OK) return rc;
    // pieces of whole frames (L = 1), one piece of each stream at a time, side by side
    rc = series_host_pieces(
        e, streams, n_streams, 1, nframes, INT64_MAX, [](int64_t) { return static_cast<int>(RPF_OK); },
        [&](int64_t k0, int64_t kc, hipStream_t ps) {
            const uint8_t* ptrs[rpf::kCorrelateMaxStreams];
            for (int m = 0; m < n_streams; ++m) ptrs[m] = e->d_series_in + static_cast<size_t>(m) * e->series_in_stride;
            return correlate_enqueue(e, ptrs, n_streams, kc, /*accumulate=*/k0 > 0, ps);
        });
    if (rc != RPF_OK) return rc;
    double* const d_result = e->d_corr_planes + MM * N;
    HIP_TRY(e, rpf::launch_correlate_finish(e->d_corr_planes, n_streams, e->N, d_result, s));
    if ((rc = copy_back(e, out, d_result, sizeof(double) * 2 * MM * N, s)) != RPF_OK) return rc;
    if (frames_done) *frames_done = nframes;                          // (only with the visibilities of all of them in `out`)
    return RPF_OK;
}

int rpf_device_fused(rpf_engine* e, const void* d_stream, size_t nbytes, int64_t repeats,
                     void* hip_stream, int64_t* repeats_done)
{
    const char* who = "rpf_device_fused";
    if (!e || !d_stream) return refuse(e, who, "NULL argument");
    if (e->taps) return refuse(e, who, "not on a PFB engine (the fold and the transform are several launches: use rpf_accumulate_device)");
    if (e->stats) return refuse(e, who, "not on an engine with RPF_FLAG_BIN_STATS (use rpf_accumulate_device_stats)");
    if (int rc = refuse_if_running(e, who)) return rc;
    if (int rc = refuse_unaligned_stream(e, who, "d_stream", d_stream)) return rc;
    if (overlapped(e) && !is_k1(e)) return refuse(e, who, "overlapped frames (frame step < N) on this size need rpf_accumulate_device");
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    int64_t nframes = frames_in(e, nbytes);
    nframes = std::min(nframes, repeats);
    if (nframes < 1) return refuse(e, who, "no whole frame");
    if (repeats_done) *repeats_done = nframes;
    if (e->fused) note_device_path_aborts(e);
    int nslots = 0;
    int rc = launch_transform(e, static_cast<const uint8_t*>(d_stream), nframes,
                              static_cast<hipStream_t>(hip_stream), &nslots);
    if (rc == RPF_OK) {
        e->last_slots = nslots;
        e->last_hops = 0;
    }
    return rc;
}

int rpf_device_reduce(rpf_engine* e, double* d_pwr_out, void* hip_stream)
{
    const char* who = "rpf_device_reduce";
    if (!e || !d_pwr_out) return refuse(e, who, "NULL argument");
    if (int rc = refuse_unaligned_out(e, who, "d_pwr_out", d_pwr_out)) return rc;
    if (e->stats) return refuse(e, who, "not on an engine with RPF_FLAG_BIN_STATS (use rpf_accumulate_device_stats)");
    if (e->taps) return refuse(e, who, "not on a PFB engine (use rpf_accumulate_device)");
    if (e->last_slots < 1 && e->last_hops < 1) return refuse(e, who, "nothing to reduce");
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    if (e->last_hops > 0) {
        HIP_TRY(e, rpf::launch_reduce_hops(e->d_partial, e->last_ranges, e->last_hops, e->N, d_pwr_out,
                                           /*accumulate=*/false, static_cast<hipStream_t>(hip_stream)));
        return RPF_OK;
    }
    return reduce_last(e, d_pwr_out, /*accumulate=*/false, static_cast<hipStream_t>(hip_stream), nullptr);
}

// Shared argument checks of the hop entries; fills frames[h] = min(repeats[h], frames(nbytes[h])).
static int check_hops(rpf_engine* e, const char* who, const void* const* d_streams, const size_t* nbytes,
                      const int64_t* repeats, int H, std::vector<int64_t>* frames)
{
    if (!e || !d_streams || !nbytes || !repeats || H < 1) return refuse(e, who, "NULL argument or no hop");
    if (int rc = refuse_if_running(e, who)) return rc;
    frames->resize(H);
    for (int h = 0; h < H; ++h) {
        if (int rc = refuse_negative_repeats(e, repeats[h])) return rc;
        if (!d_streams[h] && nbytes[h]) return refuse(e, who, "NULL stream");
        if (int rc = refuse_unaligned_stream(e, who, "streams", d_streams[h])) return rc;
        (*frames)[h] = std::min<int64_t>(frames_in(e, nbytes[h]), repeats[h]);
    }
    return RPF_OK;
}

int rpf_max_hops_per_launch(void) { return rpf::kMaxHops; }

int64_t rpf_frames_in(const rpf_engine* e, size_t nbytes) { return e ? frames_in(e, nbytes) : 0; }

int rpf_sample_bytes(const rpf_engine* e) { return e ? static_cast<int>(e->sample_bytes) : 0; }

int rpf_sample_format(const rpf_engine* e) { return e ? e->format : -1; }

size_t rpf_frame_span(const rpf_engine* e, int64_t frames) { return e ? frame_span(e, frames) : 0; }

int rpf_accumulate_device_hops(rpf_engine* e, const void* const* d_streams, const size_t* nbytes,
                               const int64_t* repeats, int n_hops, double* d_pwr_out, void* hip_stream,
                               int64_t* repeats_done)
{
    const char* who = "rpf_accumulate_device_hops";
    std::vector<int64_t> frames;
    int rc = check_hops(e, who, d_streams, nbytes, repeats, n_hops, &frames);
    if (rc != RPF_OK) return rc;
    if (!d_pwr_out) return refuse(e, who, "NULL argument");
    if ((rc = refuse_unaligned_out(e, who, "d_pwr_out", d_pwr_out)) != RPF_OK) return rc;
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (repeats_done)
        for (int h = 0; h < n_hops; ++h) repeats_done[h] = frames[h];
    const size_t N = static_cast<size_t>(e->N);
    if (e->taps || !is_k1(e) || overlapped(e) || e->stats) {
        // the other kernel families -- and overlapped frames (the scan kernel reads frames side by side), stats
        // engines (the scan kernel keeps no statistics; what comes back here is the power alone) and PFB engines (a
        // fold in front of every transform) -- run one acquisition per launch set
        for (int h = 0; h < n_hops; ++h) {
            if (frames[h] == 0) {
                HIP_TRY(e, hipMemsetAsync(d_pwr_out + h * N, 0, sizeof(double) * N, s));
                continue;
            }
            rc = launch_frames(e, static_cast<const uint8_t*>(d_streams[h]), frames[h], d_pwr_out + h * N,
                               /*accumulate=*/false, s);
            if (rc != RPF_OK) return rc;
        }
        return RPF_OK;
    }
    // K1: ONE persistent launch + ONE reduce per rpf::kMaxHops hops
    for (int h0 = 0; h0 < n_hops; h0 += rpf::kMaxHops) {
        const int hc = std::min(rpf::kMaxHops, n_hops - h0);
        const uint8_t* ptrs[rpf::kMaxHops];
        for (int h = 0; h < hc; ++h) ptrs[h] = static_cast<const uint8_t*>(d_streams[h0 + h]);
        rpf::SlotRanges slots;
        int nslots = 0;
        rc = launch_fused_hops(e, ptrs, frames.data() + h0, hc, s, &slots, &nslots);
        if (rc != RPF_OK) return rc;
        // (a hop without a whole frame has an empty slot range: the reduce writes zeros)
        HIP_TRY(e, rpf::launch_reduce_hops(e->d_partial, slots, hc, e->N, d_pwr_out + h0 * N, /*accumulate=*/false, s));
        e->last_slots = nslots;
        e->last_ranges = slots;
        e->last_hops = hc;
    }
    return RPF_OK;
}

int rpf_device_fused_hops(rpf_engine* e, const void* const* d_streams, const size_t* nbytes,
                          const int64_t* repeats, int n_hops, void* hip_stream, int64_t* repeats_done)
{
    const char* who = "rpf_device_fused_hops";
    std::vector<int64_t> frames;
    int rc = check_hops(e, who, d_streams, nbytes, repeats, n_hops, &frames);
    if (rc != RPF_OK) return rc;
    if (e->stats) return refuse(e, who, "not on an engine with RPF_FLAG_BIN_STATS");
    if (e->taps) return refuse(e, who, "not on a PFB engine (use rpf_accumulate_device_hops)");
    if (!is_k1(e) || n_hops > rpf::kMaxHops || overlapped(e))
        return refuse(e, who, "needs a size the LDS-resident kernel serves, frames side by side (frame step N) and at most "
                              "rpf_max_hops_per_launch() hops");
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    if (repeats_done)
        for (int h = 0; h < n_hops; ++h) repeats_done[h] = frames[h];
    const uint8_t* ptrs[rpf::kMaxHops];
    for (int h = 0; h < n_hops; ++h) ptrs[h] = static_cast<const uint8_t*>(d_streams[h]);
    int nslots = 0;
    rc = launch_fused_hops(e, ptrs, frames.data(), n_hops, static_cast<hipStream_t>(hip_stream), &e->last_ranges, &nslots);
    if (rc != RPF_OK) return rc;
    e->last_slots = nslots;
    e->last_hops = n_hops;
    return RPF_OK;
}

// ---- spectrogram: consecutive L-frame spectra of one stream ----------------------------------------------------

// The series kernel serves this engine: K1 (variant 0), frames side by side, and L small enough for its int frame index.
// (A stats engine asks for the kernels with statistics; only the _series_stats entries get here on one.)
static bool series_native(const rpf_engine* e, int64_t L)
{
    return is_k1(e) && !overlapped(e) && e->variant == 0 && L <= INT32_MAX - 64 &&
           (e->stats ? rpf::series_stats_supported(e->N, e->format) : rpf::series_supported(e->N, e->format));
}

// want_stats: the _series_stats entries, which need the flag as the plain ones need its absence.  *K = the spectra of
// the call.
static int series_check(rpf_engine* e, const char* who, const void* stream, size_t nbytes, int64_t L, int64_t max_spectra,
                        const void* out, bool want_stats, int64_t* K)
{
    if (!e || !out || (!stream && nbytes)) return refuse(e, who, "NULL argument");
    if (e->taps) return refuse(e, who, "not on a PFB engine (PFB with series, statistics or excision is not built)");
    if (want_stats && !e->stats) return refuse(e, who, "the engine was created without RPF_FLAG_BIN_STATS");
    if (!want_stats && e->stats) return refuse(e, who, "not on an engine with RPF_FLAG_BIN_STATS (time-resolved statistics are not built)");
    if (int rc = refuse_if_running(e, who)) return rc;
    if (L < 1) return refuse(e, who, "frames_per_spectrum must be at least 1");
    if (max_spectra < 0) return refuse(e, who, "max_spectra must not be negative");
    *K = std::min(max_spectra, frames_in(e, nbytes) / L);
    return RPF_OK;
}

// What all six entries of the family do after their own checks, before any device work: a device entry's pointers
// (null in a host entry) are refused if misaligned, the launch count starts over and the caller learns K.
static int series_begin(rpf_engine* e, const char* who, const void* d_stream, const void* d_out, int64_t K, int64_t* done)
{
    if (int rc = refuse_unaligned_stream(e, who, "d_stream", d_stream)) return rc;
    if (int rc = refuse_unaligned_out(e, who, "d_out", d_out)) return rc;
    e->series_launches = 0;
    if (done) *done = K;
    return RPF_OK;
}

// K spectra of L frames from d_stream into d_out on `s`; counts the transform launches into e->series_launches.
// On a stats engine a row is three planes, S1, S2, PK (rpf_accumulate_device_series_stats).
static int series_enqueue(rpf_engine* e, const uint8_t* d_stream, int64_t L, int64_t K, double* d_out, hipStream_t s)
{
    const size_t row = static_cast<size_t>(e->N) * (e->stats ? rpf::kStatsPlanes : 1);       // doubles per row
    if (!series_native(e, L)) {
        // spectrum by spectrum through the engine's own single-acquisition path (any size, any frame step): spectrum k
        // starts at frame k L = byte k L bS
        const size_t hop = static_cast<size_t>(L) * e->sample_bytes * static_cast<size_t>(e->step);
        for (int64_t k = 0; k < K; ++k) {
            const int rc = launch_frames(e, d_stream + static_cast<size_t>(k) * hop, L, d_out + static_cast<size_t>(k) * row,
                                         /*accumulate=*/false, s, nullptr, /*want_stats=*/e->stats);
            if (rc != RPF_OK) return rc;
            ++e->series_launches;
        }
        return RPF_OK;
    }
    if (!e->series_planned) {
        HIP_TRY(e, e->stats ? rpf::plan_series_stats(e->N, e->has_window, e->device, &e->series_plan, e->format)
                            : rpf::plan_series(e->N, e->has_window, e->device, &e->series_plan, e->format));
        HIP_TRY(e, hipMalloc(&e->d_series_partial, sizeof(double) * 2 * row * static_cast<size_t>(e->series_plan.grid)));
        e->series_planned = true;
    }
    const long frame_bytes = static_cast<long>(e->sample_bytes) * e->N;
    const bool dma = e->use_dma && (reinterpret_cast<uintptr_t>(d_stream) % 16) == 0;     // (bN is a multiple of 16)
    const int64_t per_launch = rpf::series_max_spectra(L, e->series_plan.fpw);          // K ips fits an int
    const int64_t launches = (K + per_launch - 1) / per_launch;
    const int64_t share = (K + launches - 1) / launches;
    for (int64_t k0 = 0; k0 < K; k0 += share) {
        const int64_t kc = std::min(share, K - k0);
        rpf::SeriesArgs args;
        const int grid = rpf::partition_series(kc, L, e->series_plan.fpw, e->series_plan.grid, frame_bytes, &args);
        if (grid < 1) return fail(e, RPF_ERR_INVALID_ARGUMENT, "series: too many frames for one launch");
        args.stream = d_stream + static_cast<size_t>(k0) * static_cast<size_t>(args.spectrum_bytes);
        args.out = d_out + static_cast<size_t>(k0) * row;
        HIP_TRY(e, (e->stats ? rpf::launch_fft_accum_series_stats : rpf::launch_fft_accum_series)(
                       e->N, e->has_window, dma, args, e->d_twiddles, e->d_window, e->d_series_partial, grid, s, &e->last,
                       e->format));
        ++e->series_launches;
    }
    return RPF_OK;
}

static int series_device(rpf_engine* e, const char* who, bool want_stats, const void* d_stream, size_t nbytes,
                         int64_t frames_per_spectrum, int64_t max_spectra, double* d_out, void* hip_stream,
                         int64_t* spectra_done)
{
    int64_t K = 0;
    int rc = series_check(e, who, d_stream, nbytes, frames_per_spectrum, max_spectra, d_out, want_stats, &K);
    if (rc != RPF_OK || (rc = series_begin(e, who, d_stream, d_out, K, spectra_done)) != RPF_OK) return rc;
    if (K == 0) return RPF_OK;
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    return series_enqueue(e, static_cast<const uint8_t*>(d_stream), frames_per_spectrum, K, d_out,
                          static_cast<hipStream_t>(hip_stream));
}

int rpf_accumulate_device_series(rpf_engine* e, const void* d_stream, size_t nbytes, int64_t frames_per_spectrum,
                                 int64_t max_spectra, double* d_out, void* hip_stream, int64_t* spectra_done)
{
    return series_device(e, "rpf_accumulate_device_series", false, d_stream, nbytes, frames_per_spectrum, max_spectra, d_out,
                         hip_stream, spectra_done);
}

int rpf_accumulate_device_series_stats(rpf_engine* e, const void* d_stream, size_t nbytes, int64_t frames_per_spectrum,
                                       int64_t max_spectra, double* d_out, void* hip_stream, int64_t* spectra_done)
{
    return series_device(e, "rpf_accumulate_device_series_stats", true, d_stream, nbytes, frames_per_spectrum, max_spectra,
                         d_out, hip_stream, spectra_done);
}

// The engine's row scratch holds `rows` rows (N doubles each; a stats engine's 3 N).
static int ensure_series_rows(rpf_engine* e, int64_t rows, hipStream_t s)
{
    const size_t row_bytes = sizeof(double) * e->N * (e->stats ? rpf::kStatsPlanes : 1);
    return grow_scratch(e, &e->d_series_out, &e->series_out_rows, static_cast<size_t>(rows), row_bytes, s);
}

static int series_host(rpf_engine* e, const char* who, bool want_stats, const uint8_t* stream, size_t nbytes, int64_t L,
                       int64_t max_spectra, double* out, int64_t* spectra_done)
{
    int64_t K = 0;
    int rc = series_check(e, who, stream, nbytes, L, max_spectra, out, want_stats, &K);
    if (rc != RPF_OK || (rc = series_begin(e, who, nullptr, nullptr, K, spectra_done)) != RPF_OK) return rc;
    if (K == 0) return RPF_OK;
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    const size_t row = static_cast<size_t>(e->N) * (e->stats ? rpf::kStatsPlanes : 1);       // doubles per row
    return series_host_pieces(
        e, &stream, 1, L, K, INT64_MAX, [&](int64_t per_piece) { return ensure_series_rows(e, per_piece, e->compute_stream); },
        [&](int64_t k0, int64_t kc, hipStream_t s) -> int {
            const int rc = series_enqueue(e, e->d_series_in, L, kc, e->d_series_out, s);
            if (rc != RPF_OK) return rc;
            HIP_TRY(e, hipMemcpyAsync(out + static_cast<size_t>(k0) * row, e->d_series_out, sizeof(double) * row * static_cast<size_t>(kc),
                                      hipMemcpyDeviceToHost, s));
            return RPF_OK;
        });
}

int rpf_accumulate_series(rpf_engine* e, const uint8_t* stream, size_t nbytes, int64_t frames_per_spectrum,
                          int64_t max_spectra, double* out, int64_t* spectra_done)
{
    return series_host(e, "rpf_accumulate_series", false, stream, nbytes, frames_per_spectrum, max_spectra, out, spectra_done);
}

int rpf_accumulate_series_stats(rpf_engine* e, const uint8_t* stream, size_t nbytes, int64_t frames_per_spectrum,
                                int64_t max_spectra, double* out, int64_t* spectra_done)
{
    return series_host(e, "rpf_accumulate_series_stats", true, stream, nbytes, frames_per_spectrum, max_spectra, out,
                       spectra_done);
}

// ---- excised average: the series of statistics, judged by SK and summed where it passes ------------------------

constexpr size_t kExciseRowBytes = static_cast<size_t>(64) << 20;      // a piece of rows: as many as fit, at least one

// Everything series_check refuses for a stats entry, and what only the excised entries refuse.
static int excise_check(rpf_engine* e, const char* who, const void* stream, size_t nbytes, int64_t L, int64_t max_spectra,
                        double sk_lo, double sk_hi, const void* out, int64_t* K)
{
    const int rc = series_check(e, who, stream, nbytes, L, max_spectra, out, /*want_stats=*/true, K);
    if (rc != RPF_OK) return rc;
    if (L < 2) return refuse(e, who, "frames_per_spectrum must be at least 2 (the spectral kurtosis of one frame is undefined)");
    if (sk_lo != sk_lo || sk_hi != sk_hi) return refuse(e, who, "a threshold is NaN");
    if (sk_lo > sk_hi) return refuse(e, who, "sk_lo is above sk_hi");
    return RPF_OK;
}

static int64_t excise_row_cap(const rpf_engine* e)
{
    return std::max<int64_t>(1, static_cast<int64_t>(kExciseRowBytes / (sizeof(double) * rpf::kStatsPlanes * e->N)));
}

static int ensure_excise_state(rpf_engine* e)
{
    if (e->d_excise_state) return RPF_OK;
    HIP_TRY(e, hipMalloc(&e->d_excise_state,
                         sizeof(double) * (rpf::excise_state_doubles(e->N) + rpf::kExcisePlanes * static_cast<size_t>(e->N))));
    return RPF_OK;
}

// Rows [k0, k0 + kc) of the call from d_stream (its first byte is row k0's) into the row scratch, then into the
// accumulators, on `s`; d_mask: this piece's bytes or null.
static int excise_piece(rpf_engine* e, const uint8_t* d_stream, int64_t L, int64_t k0, int64_t kc, double sk_lo,
                        double sk_hi, uint8_t* d_mask, hipStream_t s)
{
    const int rc = series_enqueue(e, d_stream, L, kc, e->d_series_out, s);
    if (rc != RPF_OK) return rc;
    HIP_TRY(e, rpf::launch_excise_rows(e->d_series_out, kc, k0, e->N, L, sk_lo, sk_hi, e->d_excise_state, d_mask, k0 == 0, s));
    return RPF_OK;
}

int rpf_accumulate_device_excised(rpf_engine* e, const void* d_stream, size_t nbytes, int64_t frames_per_spectrum,
                                  int64_t max_spectra, double sk_lo, double sk_hi, double* d_out, uint8_t* d_mask,
                                  void* hip_stream, int64_t* spectra_done)
{
    const char* who = "rpf_accumulate_device_excised";
    const int64_t L = frames_per_spectrum;
    int64_t K = 0;
    int rc = excise_check(e, who, d_stream, nbytes, L, max_spectra, sk_lo, sk_hi, d_out, &K);
    if (rc != RPF_OK || (rc = series_begin(e, who, d_stream, d_out, K, spectra_done)) != RPF_OK) return rc;
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (K == 0) {
        HIP_TRY(e, hipMemsetAsync(d_out, 0, sizeof(double) * rpf::kExcisePlanes * e->N, s));
        return RPF_OK;
    }
    const int64_t per_piece = std::min(K, excise_row_cap(e));
    if ((rc = ensure_series_rows(e, per_piece, s)) != RPF_OK || (rc = ensure_excise_state(e)) != RPF_OK) return rc;
    const size_t hop = static_cast<size_t>(L) * frame_bytes(e).pitch;
    for (int64_t k0 = 0; k0 < K; k0 += per_piece) {
        const int64_t kc = std::min(per_piece, K - k0);
        rc = excise_piece(e, static_cast<const uint8_t*>(d_stream) + static_cast<size_t>(k0) * hop, L, k0, kc, sk_lo, sk_hi,
                          d_mask ? d_mask + static_cast<size_t>(k0) * e->N : nullptr, s);
        if (rc != RPF_OK) return rc;
    }
    HIP_TRY(e, rpf::launch_excise_combine(e->d_excise_state, e->N, d_out, s));
    return RPF_OK;
}

int rpf_accumulate_excised(rpf_engine* e, const uint8_t* stream, size_t nbytes, int64_t frames_per_spectrum,
                           int64_t max_spectra, double sk_lo, double sk_hi, double* out, uint8_t* mask,
                           int64_t* spectra_done)
{
    const char* who = "rpf_accumulate_excised";
    const int64_t L = frames_per_spectrum;
    int64_t K = 0;
    int rc = excise_check(e, who, stream, nbytes, L, max_spectra, sk_lo, sk_hi, out, &K);
    if (rc != RPF_OK || (rc = series_begin(e, who, nullptr, nullptr, K, spectra_done)) != RPF_OK) return rc;
    const size_t out_doubles = rpf::kExcisePlanes * static_cast<size_t>(e->N);
    if (K == 0) {
        std::fill(out, out + out_doubles, 0.0);
        return RPF_OK;
    }
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    hipStream_t s = e->compute_stream;
    // (a piece's rows are capped as the device entry's are, on top of its input's 64 MB)
    rc = series_host_pieces(
        e, &stream, 1, L, K, excise_row_cap(e),
        [&](int64_t per_piece) -> int {
            int rc = grow_scratch(e, &e->d_excise_mask, &e->excise_mask_bytes, mask ? static_cast<size_t>(per_piece) * e->N : 0, 1, s);
            if (rc == RPF_OK) rc = ensure_series_rows(e, per_piece, s);
            return rc != RPF_OK ? rc : ensure_excise_state(e);
        },
        [&](int64_t k0, int64_t kc, hipStream_t s) -> int {
            const int rc = excise_piece(e, e->d_series_in, L, k0, kc, sk_lo, sk_hi, mask ? e->d_excise_mask : nullptr, s);
            if (rc != RPF_OK) return rc;
            if (mask)
                HIP_TRY(e, hipMemcpyAsync(mask + static_cast<size_t>(k0) * e->N, e->d_excise_mask, static_cast<size_t>(kc) * e->N,
                                          hipMemcpyDeviceToHost, s));
            return RPF_OK;
        });
    if (rc != RPF_OK) return rc;
    double* d_result = e->d_excise_state + rpf::excise_state_doubles(e->N);
    HIP_TRY(e, rpf::launch_excise_combine(e->d_excise_state, e->N, d_result, s));
    return copy_back(e, out, d_result, sizeof(double) * out_doubles, s);
}

// ---- per-bin quantiles: rows of the series kept in HBM, order statistics by radix select -----------------------------

constexpr int64_t kQuantileStoreDoubles = static_cast<int64_t>(1) << 27;      // 1 GiB of rows

static int64_t quantile_max_rows(const rpf_engine* e) { return std::max<int64_t>(1, kQuantileStoreDoubles / e->N); }

// What every quantile entry refuses, before anything else: the store holds the rows of the plain series.
static int quantile_check(rpf_engine* e, const char* who)
{
    if (!e) return refuse(e, who, "NULL argument");
    if (e->taps) return refuse(e, who, "not on a PFB engine (quantiles of PFB spectra are not built)");
    if (e->stats)
        return refuse(e, who, "not on an engine with RPF_FLAG_BIN_STATS (the row store holds the rows of rpf_accumulate_device_series)");
    return refuse_if_running(e, who);
}

// The append entries' checks; *K = the rows the call appends.  Nothing on the device is touched.
static int quantile_append_check(rpf_engine* e, const char* who, const void* stream, size_t nbytes, int64_t L,
                                 int64_t max_spectra, int64_t* K)
{
    int rc = quantile_check(e, who);
    if (rc != RPF_OK) return rc;
    if ((rc = series_check(e, who, stream, nbytes, L, max_spectra, /*out=*/e, /*want_stats=*/false, K)) != RPF_OK) return rc;
    if (e->quantile_rows + *K > quantile_max_rows(e))
        return refuse(e, who, std::to_string(e->quantile_rows) + " rows stored and " + std::to_string(*K) +
                                  " to append, the store holds at most " + std::to_string(quantile_max_rows(e)) + " rows of " +
                                  std::to_string(e->N) + " bins (1 GiB): raise the frames per integration or cap max_spectra");
    return RPF_OK;
}

// Room for `rows` rows (<= quantile_max_rows): the capacity doubles until they fit.  A growth synchronises `s` and the
// engine's stream once, moves the stored rows and frees the old block.
static int ensure_quantile_rows(rpf_engine* e, int64_t rows, hipStream_t s)
{
    if (rows <= e->quantile_cap) return RPF_OK;
    int64_t cap = std::max<int64_t>(e->quantile_cap, 1);
    while (cap < rows) cap *= 2;
    cap = std::min(cap, quantile_max_rows(e));
    const size_t row_bytes = sizeof(double) * static_cast<size_t>(e->N);
    double* grown = nullptr;
    HIP_TRY(e, hipStreamSynchronize(s));
    if (s != e->compute_stream) HIP_TRY(e, hipStreamSynchronize(e->compute_stream));
    HIP_TRY(e, hipMalloc(&grown, row_bytes * static_cast<size_t>(cap)));
    if (e->quantile_rows > 0) {
        const hipError_t err = hipMemcpy(grown, e->d_quantile_rows, row_bytes * static_cast<size_t>(e->quantile_rows), hipMemcpyDeviceToDevice);
        if (err != hipSuccess) {
            (void)hipFree(grown);
            HIP_TRY(e, err);
        }
    }
    if (e->d_quantile_rows) (void)hipFree(e->d_quantile_rows);
    e->d_quantile_rows = grown;
    e->quantile_cap = cap;
    return RPF_OK;
}

int rpf_quantile_reset(rpf_engine* e)
{
    if (!e) return refuse(e, "rpf_quantile_reset", "NULL argument");
    e->quantile_rows = 0;
    return RPF_OK;
}

int64_t rpf_quantile_rows(const rpf_engine* e) { return e ? e->quantile_rows : -1; }

int64_t rpf_quantile_max_rows(const rpf_engine* e) { return e ? quantile_max_rows(e) : -1; }

int rpf_quantile_append_device(rpf_engine* e, const void* d_stream, size_t nbytes, int64_t frames_per_spectrum,
                               int64_t max_spectra, void* hip_stream, int64_t* appended)
{
    const char* who = "rpf_quantile_append_device";
    int64_t K = 0;
    int rc = quantile_append_check(e, who, d_stream, nbytes, frames_per_spectrum, max_spectra, &K);
    if (rc != RPF_OK || (rc = series_begin(e, who, d_stream, nullptr, K, appended)) != RPF_OK) return rc;
    if (K == 0) return RPF_OK;
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if ((rc = ensure_quantile_rows(e, e->quantile_rows + K, s)) != RPF_OK) return rc;
    // (N is even: every row of the store is 16-byte aligned, as the series wants its output)
    rc = series_enqueue(e, static_cast<const uint8_t*>(d_stream), frames_per_spectrum, K,
                        e->d_quantile_rows + static_cast<size_t>(e->quantile_rows) * e->N, s);
    if (rc != RPF_OK) return rc;
    e->quantile_rows += K;
    return RPF_OK;
}

int rpf_quantile_append(rpf_engine* e, const uint8_t* stream, size_t nbytes, int64_t frames_per_spectrum,
                        int64_t max_spectra, int64_t* appended)
{
    const char* who = "rpf_quantile_append";
    const int64_t L = frames_per_spectrum;
    int64_t K = 0;
    int rc = quantile_append_check(e, who, stream, nbytes, L, max_spectra, &K);
    if (rc != RPF_OK || (rc = series_begin(e, who, nullptr, nullptr, K, appended)) != RPF_OK) return rc;
    if (K == 0) return RPF_OK;
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    // the pieces of rpf_accumulate_series (the same launches, so the same rows) to the store's tail, counted once landed
    const int64_t stored = e->quantile_rows;
    int64_t landed = 0;
    rc = series_host_pieces(
        e, &stream, 1, L, K, INT64_MAX, [&](int64_t) { return ensure_quantile_rows(e, stored + K, e->compute_stream); },
        [&](int64_t k0, int64_t kc, hipStream_t s) {
            return series_enqueue(e, e->d_series_in, L, kc, e->d_quantile_rows + static_cast<size_t>(stored + k0) * e->N, s);
        },
        &landed);
    e->quantile_rows = stored + landed;
    return rc;
}

// The select entries' checks and the ranks of the call (the same in every bin).
static int quantile_select_check(rpf_engine* e, const char* who, const double* q, int nq, const void* out,
                                 rpf::QuantileRanks* ranks)
{
    const int rc = quantile_check(e, who);
    if (rc != RPF_OK) return rc;
    if (nq < 1 || nq > rpf::kQuantileMaxQ)
        return refuse(e, who, "nq must be in 1 .. " + std::to_string(rpf::kQuantileMaxQ) + ", got " + std::to_string(nq));
    if (!q || !out) return refuse(e, who, "NULL argument");
    ranks->nq = nq;
    for (int i = 0; i < rpf::kQuantileMaxQ; ++i) {
        ranks->j[i] = 0;
        ranks->g[i] = 0.0;
    }
    for (int i = 0; i < nq; ++i) {
        if (!(q[i] >= 0.0 && q[i] <= 1.0))
            return refuse(e, who, "q[" + std::to_string(i) + "] = " + std::to_string(q[i]) + " is not in [0, 1]");
        if (e->quantile_rows > 0) {
            int64_t j = 0;
            rpf::quantile_rank(q[i], e->quantile_rows, j, ranks->g[i]);
            ranks->j[i] = static_cast<uint32_t>(j);
        }
    }
    return RPF_OK;
}

static int quantile_select_enqueue(rpf_engine* e, const rpf::QuantileRanks& ranks, double* d_out, hipStream_t s)
{
    if (!e->d_quantile_work && e->quantile_rows > 0) HIP_TRY(e, hipMalloc(&e->d_quantile_work, rpf::quantile_work_bytes(e->N)));
    HIP_TRY(e, rpf::launch_quantile_select(e->d_quantile_rows, e->quantile_rows, e->N, ranks, e->d_quantile_work, d_out, s));
    return RPF_OK;
}

int rpf_quantile_select_device(rpf_engine* e, const double* q, int nq, double* d_out, void* hip_stream)
{
    const char* who = "rpf_quantile_select_device";
    rpf::QuantileRanks ranks;
    int rc = quantile_select_check(e, who, q, nq, d_out, &ranks);
    if (rc == RPF_OK) rc = refuse_unaligned_out(e, who, "d_out", d_out);
    if (rc != RPF_OK) return rc;
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    return quantile_select_enqueue(e, ranks, d_out, static_cast<hipStream_t>(hip_stream));
}

int rpf_quantile_select(rpf_engine* e, const double* q, int nq, double* out)
{
    rpf::QuantileRanks ranks;
    int rc = quantile_select_check(e, "rpf_quantile_select", q, nq, out, &ranks);
    if (rc != RPF_OK) return rc;
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    hipStream_t s = e->compute_stream;
    rc = grow_scratch(e, &e->d_quantile_out, &e->quantile_out_planes, static_cast<size_t>(nq), sizeof(double) * e->N, s);
    if (rc != RPF_OK) return rc;
    if ((rc = quantile_select_enqueue(e, ranks, e->d_quantile_out, s)) != RPF_OK) return rc;
    return copy_back(e, out, e->d_quantile_out, sizeof(double) * static_cast<size_t>(nq) * e->N, s);
}

// ---- incoherent dedispersion of the stored integrations: rpf_dedisperse_device, rpf_dedisperse (include/rpf_engine.h) --

// The largest entry of the D x N table, or -1 where one is negative (*at = its index).
static int64_t dedisperse_dmax(const int32_t* delays, size_t cells, size_t* at)
{
    int32_t dmax = 0;
    for (size_t i = 0; i < cells; ++i) {
        if (delays[i] < 0) {
            if (at) *at = i;
            return -1;
        }
        dmax = std::max(dmax, delays[i]);
    }
    return dmax;
}

// Everything both entries refuse, before any device work; *T = the times of the call.
static int dedisperse_check(rpf_engine* e, const char* who, const int32_t* delays, const double* weights, int n_trials,
                            const void* out, int64_t capacity, int64_t* times, int64_t* T)
{
    if (times) *times = 0;
    const int rc = quantile_check(e, who);
    if (rc != RPF_OK) return rc;
    if (!delays || !out || !times) return refuse(e, who, "NULL argument");
    if (n_trials < 1 || n_trials > rpf::kDedispMaxTrials)
        return refuse(e, who, "n_trials must be in 1 .. " + std::to_string(rpf::kDedispMaxTrials) + ", got " + std::to_string(n_trials));
    const size_t N = static_cast<size_t>(e->N);
    size_t at = 0;
    const int64_t dmax = dedisperse_dmax(delays, static_cast<size_t>(n_trials) * N, &at);
    if (dmax < 0)
        return refuse(e, who, "negative delay " + std::to_string(delays[at]) + " at trial " + std::to_string(at / N) + ", bin " +
                                  std::to_string(at % N));
    for (size_t b = 0; weights && b < N; ++b)
        if (!std::isfinite(weights[b])) return refuse(e, who, "weights[" + std::to_string(b) + "] is not finite");
    *T = rpf::dedisperse_times(e->quantile_rows, dmax);
    if (static_cast<int64_t>(n_trials) * *T > capacity)
        return refuse(e, who, std::to_string(n_trials) + " trials of " + std::to_string(*T) + " times need " +
                                  std::to_string(static_cast<int64_t>(n_trials) * *T) + " doubles, the capacity is " +
                                  std::to_string(capacity));
    return RPF_OK;
}

// Uploads the weights (NULL: ones), the spans of dedisperse_core.h and the table into the engine's tables, then the
// launch, all on `s`.  The tables serve one call at a time (UploadTable).
static int dedisperse_enqueue(rpf_engine* e, const int32_t* delays, const double* weights, int D, int64_t T, double* d_out,
                              hipStream_t s)
{
    const size_t N = static_cast<size_t>(e->N);
    const int tiles = rpf::dedisperse_trial_tiles(D), nblocks = rpf::dedisperse_bin_blocks(e->N);
    const size_t spans_at = sizeof(double) * N, delays_at = spans_at + sizeof(rpf::DedispSpan) * tiles * nblocks;
    const size_t bytes = delays_at + sizeof(int32_t) * static_cast<size_t>(D) * N;
    UploadTable& t = e->dd_tables;
    if (int rc = t.reserve(e, bytes)) return rc;
    double* const w = reinterpret_cast<double*>(t.host);
    if (weights)
        std::copy(weights, weights + N, w);
    else
        std::fill(w, w + N, 1.0);
    rpf::DedispSpan* const spans = reinterpret_cast<rpf::DedispSpan*>(t.host + spans_at);
    for (int tile = 0; tile < tiles; ++tile)
        for (int blk = 0; blk < nblocks; ++blk) spans[tile * nblocks + blk] = rpf::dedisperse_span(delays, w, e->N, D, tile, blk);
    std::memcpy(t.host + delays_at, delays, bytes - delays_at);
    HIP_TRY(e, hipMemcpyAsync(t.device, t.host, bytes, hipMemcpyHostToDevice, s));
    const hipError_t launched = rpf::launch_dedisperse(e->d_quantile_rows, e->quantile_rows, e->N,
                                                       reinterpret_cast<const int32_t*>(t.device + delays_at),
                                                       reinterpret_cast<const double*>(t.device), t.device + spans_at, D, T,
                                                       d_out, s);
    // (recorded whether or not the launch went out: the copy above reads the pinned block until then)
    if (int rc = t.record(e, s)) return rc;
    HIP_TRY(e, launched);
    return RPF_OK;
}

int64_t rpf_dedisperse_times(const rpf_engine* e, const int32_t* delays, int n_trials)
{
    if (!e || !delays || n_trials < 1) return -1;
    const int64_t dmax = dedisperse_dmax(delays, static_cast<size_t>(n_trials) * static_cast<size_t>(e->N), nullptr);
    return dmax < 0 ? -1 : rpf::dedisperse_times(e->quantile_rows, dmax);
}

int rpf_dedisperse_device(rpf_engine* e, const int32_t* delays, const double* weights, int n_trials, double* d_out,
                          int64_t capacity, void* hip_stream, int64_t* times)
{
    const char* who = "rpf_dedisperse_device";
    int64_t T = 0;
    int rc = dedisperse_check(e, who, delays, weights, n_trials, d_out, capacity, times, &T);
    if (rc == RPF_OK) rc = refuse_unaligned_out(e, who, "d_out", d_out);
    if (rc != RPF_OK) return rc;
    if (T == 0) return RPF_OK;
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    if (int err = dedisperse_enqueue(e, delays, weights, n_trials, T, d_out, static_cast<hipStream_t>(hip_stream))) return err;
    *times = T;
    return RPF_OK;
}

int rpf_dedisperse(rpf_engine* e, const int32_t* delays, const double* weights, int n_trials, double* out, int64_t capacity,
                   int64_t* times)
{
    int64_t T = 0;
    int rc = dedisperse_check(e, "rpf_dedisperse", delays, weights, n_trials, out, capacity, times, &T);
    if (rc != RPF_OK || T == 0) return rc;
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    hipStream_t s = e->compute_stream;
    const size_t cells = static_cast<size_t>(n_trials) * static_cast<size_t>(T);
    if ((rc = grow_scratch(e, &e->d_dd_out, &e->dd_out, cells, sizeof(double), s)) != RPF_OK) return rc;
    if ((rc = dedisperse_enqueue(e, delays, weights, n_trials, T, e->d_dd_out, s)) != RPF_OK) return rc;
    if ((rc = copy_back(e, out, e->d_dd_out, sizeof(double) * cells, s)) != RPF_OK) return rc;
    *times = T;
    return RPF_OK;
}

// ---- fold of a plane at trial periods: rpf_fold_device, rpf_dedisperse_fold (include/rpf_engine.h) ---------------------

// What both entries refuse of the fold's own arguments, before any device work (`e` is not NULL here).
static int fold_check(rpf_engine* e, const char* who, int D, int64_t T, const uint64_t* steps, int P, int NB, const void* prof,
                      int64_t capacity)
{
    auto range = [&](const char* name, int hi, int got) {
        return refuse(e, who, std::string(name) + " must be in 1 .. " + std::to_string(hi) + ", got " + std::to_string(got));
    };
    if (!steps || !prof) return refuse(e, who, "NULL argument");
    if (D < 1 || D > rpf::kFoldMaxSeries) return range("n_series", rpf::kFoldMaxSeries, D);
    if (P < 1 || P > rpf::kFoldMaxPeriods) return range("n_periods", rpf::kFoldMaxPeriods, P);
    if (NB < 1 || NB > rpf::kFoldMaxBins) return range("phase_bins", rpf::kFoldMaxBins, NB);
    if (T < 0 || T >= (static_cast<int64_t>(1) << 31)) return refuse(e, who, "T must be in 0 .. 2^31 - 1, got " + std::to_string(T));
    const int64_t cells = static_cast<int64_t>(D) * P * NB;
    if (cells > capacity || cells > rpf::kFoldMaxCells)
        return refuse(e, who, std::to_string(D) + " series x " + std::to_string(P) + " periods x " + std::to_string(NB) +
                                  " phase bins are " + std::to_string(cells) + " cells, the capacity is " + std::to_string(capacity) +
                                  " and a call folds at most " + std::to_string(rpf::kFoldMaxCells));
    return RPF_OK;
}

// Uploads the steps into the engine's table and enqueues the launches of every group of series, all on `s`.  The table
// and the scratch serve one call at a time (UploadTable).
static int fold_enqueue(rpf_engine* e, const double* d_x, int D, int64_t T, const uint64_t* steps, int P, int NB, double* d_prof,
                        int32_t* d_hits, double* d_mom, hipStream_t s)
{
    UploadTable& t = e->fold_steps;
    if (int rc = t.reserve(e, sizeof(uint64_t) * P)) return rc;
    uint64_t* const d_steps = reinterpret_cast<uint64_t*>(t.device);
    const int per_group = rpf::fold_group_series(D, P, NB);
    const size_t need = rpf::fold_scratch(per_group, P, NB).bytes;
    if (need > e->fold_scratch_bytes) {          // (nothing of this engine reads the scratch now: the table's `done` has passed)
        (void)hipFree(e->d_fold_scratch);
        e->d_fold_scratch = nullptr;
        e->fold_scratch_bytes = 0;
        HIP_TRY(e, hipMalloc(&e->d_fold_scratch, need));
        e->fold_scratch_bytes = need;
    }
    std::copy(steps, steps + P, reinterpret_cast<uint64_t*>(t.host));
    HIP_TRY(e, hipMemcpyAsync(d_steps, t.host, sizeof(uint64_t) * P, hipMemcpyHostToDevice, s));
    hipError_t launched = hipSuccess;
    const size_t cells = static_cast<size_t>(P) * NB;
    for (int s0 = 0; s0 < D && launched == hipSuccess; s0 += per_group)
        launched = rpf::launch_fold(d_x + static_cast<size_t>(s0) * T, std::min(per_group, D - s0), T, d_steps, P, NB,
                                    e->d_fold_scratch, d_prof + s0 * cells, s0 == 0 ? d_hits : nullptr,
                                    d_mom ? d_mom + 2 * static_cast<size_t>(s0) : nullptr, s);
    // (recorded whether or not the launches went out: the copy above reads the pinned block until then)
    if (int rc = t.record(e, s)) return rc;
    HIP_TRY(e, launched);
    return RPF_OK;
}

int rpf_fold_device(rpf_engine* e, const double* d_series, int n_series, int64_t T, const uint64_t* steps, int n_periods,
                    int phase_bins, double* d_prof, int64_t capacity, int32_t* d_hits, double* d_mom, void* hip_stream)
{
    const char* who = "rpf_fold_device";
    if (!e || !d_series) return refuse(e, who, "NULL argument");
    int rc = refuse_if_running(e, who);
    if (rc == RPF_OK) rc = fold_check(e, who, n_series, T, steps, n_periods, phase_bins, d_prof, capacity);
    if (rc != RPF_OK) return rc;
    if (reinterpret_cast<uintptr_t>(d_series) & 7) return refuse(e, who, "d_series must be 8-byte aligned");
    if ((reinterpret_cast<uintptr_t>(d_prof) & 15) || (reinterpret_cast<uintptr_t>(d_mom) & 15))
        return refuse(e, who, "d_prof and d_mom must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_hits) & 3) return refuse(e, who, "d_hits must be 4-byte aligned");
    if (T == 0) return RPF_OK;
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    return fold_enqueue(e, d_series, n_series, T, steps, n_periods, phase_bins, d_prof, d_hits, d_mom,
                        static_cast<hipStream_t>(hip_stream));
}

int rpf_dedisperse_fold(rpf_engine* e, const int32_t* delays, const double* weights, int n_trials, const uint64_t* steps,
                        int n_periods, int phase_bins, double* prof, int64_t capacity, int32_t* hits, double* mom, int64_t* times)
{
    const char* who = "rpf_dedisperse_fold";
    int64_t T = 0;
    // (the plane goes to engine scratch, grown to fit: its capacity is no refusal of this entry)
    int rc = dedisperse_check(e, who, delays, weights, n_trials, prof, INT64_MAX, times, &T);
    if (rc != RPF_OK) return rc;
    if ((rc = fold_check(e, who, n_trials, T, steps, n_periods, phase_bins, prof, capacity)) != RPF_OK || T == 0) return rc;
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    hipStream_t s = e->compute_stream;
    const size_t D = static_cast<size_t>(n_trials), cells = static_cast<size_t>(n_periods) * phase_bins;
    // prof, then mom, then hits: every offset a multiple of 16 bytes
    const size_t mom_at = sizeof(double) * D * cells, hits_at = mom_at + sizeof(double) * 2 * D;
    if ((rc = grow_scratch(e, &e->d_dd_out, &e->dd_out, D * static_cast<size_t>(T), sizeof(double), s)) != RPF_OK) return rc;
    if ((rc = grow_scratch(e, &e->d_fold_out, &e->fold_out_bytes, hits_at + sizeof(int32_t) * cells, 1, s)) != RPF_OK) return rc;
    if ((rc = dedisperse_enqueue(e, delays, weights, n_trials, T, e->d_dd_out, s)) != RPF_OK) return rc;
    double* const d_prof = reinterpret_cast<double*>(e->d_fold_out);
    double* const d_mom = reinterpret_cast<double*>(e->d_fold_out + mom_at);
    int32_t* const d_hits = reinterpret_cast<int32_t*>(e->d_fold_out + hits_at);
    if ((rc = fold_enqueue(e, e->d_dd_out, n_trials, T, steps, n_periods, phase_bins, d_prof, hits ? d_hits : nullptr,
                           mom ? d_mom : nullptr, s)) != RPF_OK)
        return rc;
    HIP_TRY(e, hipMemcpyAsync(prof, d_prof, mom_at, hipMemcpyDeviceToHost, s));
    if (mom) HIP_TRY(e, hipMemcpyAsync(mom, d_mom, sizeof(double) * 2 * D, hipMemcpyDeviceToHost, s));
    if (hits) HIP_TRY(e, hipMemcpyAsync(hits, d_hits, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    *times = T;
    return RPF_OK;
}

int rpf_series_launches(const rpf_engine* e) { return e ? e->series_launches : 0; }

int rpf_stream_register(rpf_engine* e, const void* stream, size_t nbytes)
{
    if (!e || !stream || nbytes == 0) return refuse(e, "rpf_stream_register", "NULL or empty stream");
    if (int rc = refuse_if_running(e, "rpf_stream_register")) return rc;
    DeviceScope on_device(e->device);
    HIP_TRY(e, on_device.status());
    const hipError_t err = hipHostRegister(const_cast<void*>(stream), nbytes, hipHostRegisterDefault);
    if (err != hipSuccess) {
        (void)hipGetLastError();
        return fail(e, RPF_ERR_HARDWARE, std::string("hipHostRegister: ") + hipGetErrorString(err));
    }
    e->registered.emplace_back(static_cast<const uint8_t*>(stream), nbytes);
    return RPF_OK;
}

int rpf_stream_unregister(rpf_engine* e, const void* stream)
{
    if (!e || !stream) return refuse(e, "rpf_stream_unregister", "NULL argument");
    if (int rc = refuse_if_running(e, "rpf_stream_unregister")) return rc;
    for (size_t k = 0; k < e->registered.size(); ++k) {
        if (e->registered[k].first != stream) continue;
        DeviceScope on_device(e->device);
        HIP_TRY(e, on_device.status());
        HIP_TRY(e, hipHostUnregister(const_cast<void*>(stream)));
        e->registered.erase(e->registered.begin() + static_cast<long>(k));
        return RPF_OK;
    }
    return refuse(e, "rpf_stream_unregister", "not a registered stream");
}

int rpf_fused_status(rpf_engine* e, int* active, int64_t* launches_gave_up, int64_t* launches_recovered)
{
    if (!e) return RPF_ERR_INVALID_ARGUMENT;
    if (e->fused && !e->worker_running) note_device_path_aborts(e);
    if (active) *active = (e->family == rpf::Family::FourStep && e->fused) ? 1 : 0;
    if (launches_gave_up) *launches_gave_up = e->h_fused_words ? __atomic_load_n(&e->h_fused_words[4], __ATOMIC_ACQUIRE) : 0;
    if (launches_recovered) *launches_recovered = e->fused_recovered;
    return RPF_OK;
}

int rpf_debug_fused_fault(rpf_engine* e, int mode, int skip, int count)
{
    if (!e || mode < 0 || mode > 2 || skip < 0) return refuse(e, "rpf_debug_fused_fault", "bad argument");
    if (int rc = refuse_if_running(e, "rpf_debug_fused_fault")) return rc;
    e->fused_fault_mode = mode;
    e->fused_fault_skip = skip;
    e->fused_fault_count = mode ? count : 0;
    return RPF_OK;
}

int rpf_last_launch_info(const rpf_engine* e, int* grid, int* block, int* frames_per_wg,
                         int* lds_bytes)
{
    if (!e) return RPF_ERR_INVALID_ARGUMENT;
    if (e->inner) e = e->inner;           // a PFB engine reports its transform launch
    if (e->last_was_cross && e->cross_inner) e = e->cross_inner;      // ... and a cross call the cf32 engine's
    if (e->last_was_stft && e->stft_inner) e = e->stft_inner;         // ... and an STFT call on another family the catch-all engine's
    if (grid) *grid = e->last.grid ? e->last.grid : e->plan.grid;
    if (block) *block = e->plan.block;
    if (frames_per_wg) *frames_per_wg = e->plan.fpw;
    if (lds_bytes) *lds_bytes = e->plan.lds_bytes;
    return RPF_OK;
}

}  // extern "C"
