"""Overlapped FFT frames (rpf_config::frame_step S): frame rate of the device-resident path against S = N.
One JSON line per case: frames/s, frame-samples/s (N x frames/s) and input-samples/s (the stream's samples consumed
per second).  Back-to-back rpf_accumulate_device calls (transform + reduce), HIP events around the batch.
  N = 4096, rectangular and Hann: S in {N, 3N/4, N/2, N/4, N/2 + 1}, 10 000 frames -- K1's strided instantiation
  N = 5000, 65536, 262144: S in {N, N/2} -- the frame gather + the size's kernel; the four-step sizes also at S = N on
  the two-kernel path ("two_kernel"), which is what they run with S != N
Usage: python tools/gpu_frame_overlap.py > profiles/frame_overlap.json"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import rtl_power_fftw_amd as rpf  # noqa: E402

dev = torch.device("cuda:0")
stream = torch.cuda.current_stream().cuda_stream


def timed(fn, K, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(K):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / K * 1e-3            # seconds per call


def case(N, step, frames, window=False, flags=0, label=None, K=20):
    nbytes = 2 * N + 2 * step * (frames - 1)
    d_in = rpf.synth.noise_tones_iq_torch(3, nbytes // 2, dev)
    out = torch.empty(N, dtype=torch.float64, device=dev)
    w = rpf.synth.hann_window(N) if window else None
    with rpf.Datastore(rpf.Params(N=N, window=window, frame_step=step), w, flags=flags) as ds:
        assert ds.frames_in(nbytes) == frames
        sec = timed(lambda: ds.accumulate_device(d_in.data_ptr(), nbytes, frames, out.data_ptr(), stream), K)
    row = {"N": N, "step": step, "window": "hann" if window else "rect", "frames": frames,
           "path": label or ("k1" if N <= 8192 and (N & (N - 1)) == 0 else "gather" if step != N else "default"),
           "us_per_call": round(sec * 1e6, 2), "frames_per_s": frames / sec, "frame_samples_per_s": N * frames / sec,
           "input_samples_per_s": (nbytes // 2) / sec}
    print(json.dumps(row), flush=True)
    return row


def main():
    N = 4096
    for window in (False, True):
        for step in (N, 3 * N // 4, N // 2, N // 4, N // 2 + 1):
            case(N, step, 10000, window, K=50)
    for N, frames in ((5000, 20000), (65536, 2000), (262144, 500)):
        if N >= 65536:
            case(N, N, frames, flags=rpf._lib.FLAG_NO_FOURSTEP_FUSED, label="two_kernel")
        case(N, N, frames)
        case(N, N // 2, frames)


if __name__ == "__main__":
    main()
