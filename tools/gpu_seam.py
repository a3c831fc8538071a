"""The per-acquisition seam of the flagship step: K1 -> K3 -> next K1.

Replays bench.py's C2 step shape (N = 4096, 10 000 frames, rectangular window, 9 rotating 81.92 MB
buffers, `device_fused` then `device_reduce`) or its C5 scan (8 hops x 5000 frames in one
`device_fused_hops` launch, then `device_reduce`), and has three modes:

  python tools/gpu_seam.py [--workload C2|C5] [--steps K]
      the step loop alone; run it under
      rocprofv3 --kernel-trace --stats -d OUT -o seam -- python tools/gpu_seam.py
  python tools/gpu_seam.py --report OUT
      medians over the timed steps of that trace: K1 duration, K1 end -> K3 start, K3 duration,
      K3 end -> next K1 start, and the step (K1 start -> next K1 start)
  RPF_ENGINE_LIB=rtl-power-fftw_amd/librpf_engine_timing.so python tools/gpu_seam.py --phases
      (make -C rtl-power-fftw_amd/csrc kvariant: the -DRPF_PHASE_TIMING build) K1's fixed cost from the
      seam marks of each workgroup (RPF_SEAM_MARK): kernel start -> first frame unpacked, end of the frame
      loop -> partial spectrum drained, and how long the workgroups with one round less wait for the last one
"""
import argparse
import csv
import ctypes
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, R_C2, R_C5, HOPS = 4096, 10000, 5000, 8


def workload(args):
    import torch
    import rtl_power_fftw_amd as rpf

    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    ds = rpf.Datastore(rpf.Params(N=N, repeats=R_C2), device=0)
    if args.workload == "C2":
        base = rpf.synth.noise_tones_iq_torch(2, N * R_C2, dev)
        nb = -(-(640 << 20) // base.numel())                       # bench.py's replay-buffer count: 9
        bufs = [base] + [torch.roll(base, shifts=2 * N * 37 * i) for i in range(1, nb)]
        out = torch.empty(N, dtype=torch.float64, device=dev)

        def step(i):
            ds.device_fused(bufs[i % nb].data_ptr(), 2 * N * R_C2, R_C2, s)
            ds.device_reduce(out.data_ptr(), s)
    else:
        hops = [rpf.synth.noise_tones_iq_torch(50 + h, N * R_C5, dev) for h in range(HOPS)]
        out = torch.empty(HOPS, N, dtype=torch.float64, device=dev)
        ptrs = [h.data_ptr() for h in hops]

        def step(i):
            ds.device_fused_hops(ptrs, [2 * N * R_C5] * HOPS, [R_C5] * HOPS, s)
            ds.device_reduce(out.data_ptr(), s)
    for i in range(args.warmup):
        step(i)
    torch.cuda.synchronize()
    if args.phases:
        return phases(ds, step, args)
    for i in range(args.steps):
        step(i)
    torch.cuda.synchronize()
    ds.close()


def phases(ds, step, args):
    import torch
    import rtl_power_fftw_amd as rpf

    lib = rpf.load()
    fn = lib.rpf_debug_seam_marks
    fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    info = ds.launch_info()
    grid, fpw = info["grid"], info["frames_per_wg"]
    slots = -(-R_C2 // fpw)                                       # frame pairs of the acquisition
    marks = (ctypes.c_ulonglong * (2048 * 4))()
    nw = ctypes.c_int()
    pro, loop, flush, tail, span = [], [], [], [], []
    for i in range(args.steps):
        fn(marks, ctypes.byref(nw), 1)                            # reset
        step(i)
        torch.cuda.synchronize()
        fn(marks, ctypes.byref(nw), 0)
        m = [marks[4 * w: 4 * w + 4] for w in range(grid)]
        t0, t_end = min(x[0] for x in m), max(x[3] for x in m)
        its = [len(range(w, slots, grid)) for w in range(grid)]
        full = max(its)
        us = 0.01                                                 # 100 MHz realtime clock
        pro.append(statistics.median((x[1] - x[0]) * us for x in m))
        loop.append(statistics.median((x[2] - x[1]) * us for x, n in zip(m, its) if n == full))
        flush.append(statistics.median((x[3] - x[2]) * us for x in m))
        short = [(t_end - x[3]) * us for x, n in zip(m, its) if n < full]
        tail.append(statistics.median(short) if short else 0.0)
        span.append((t_end - t0) * us)
    med = statistics.median
    print("K1 seam marks (%s, grid %d x %d frames per workgroup, %d steps, medians; 100 MHz clock = 0.01 us)"
          % (args.workload, grid, fpw, args.steps))
    print("  first workgroup start -> last workgroup drained   %7.2f us" % med(span))
    print("  kernel start -> first frame unpacked (prologue)   %7.2f us" % med(pro))
    print("  first unpack -> loop end, %2d-round workgroups     %7.2f us" % (full, med(loop)))
    print("  loop end -> partial spectrum drained (flush)      %7.2f us" % med(flush))
    print("  %2d-round workgroups idle until the last one ends  %7.2f us  (%d of %d workgroups)"
          % (full - 1, med(tail), sum(1 for w in range(grid) if len(range(w, slots, grid)) < full), grid))
    ds.close()


def report(path):
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit("no *kernel_trace.csv under %s" % path)
    rows = []
    for f in files:
        with open(f) as fh:
            for r in csv.DictReader(fh):
                name = r["Kernel_Name"]
                kind = "K1" if "fft_accum" in name else "K3" if "reduce_kernel" in name else None
                if kind:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind))
    rows.sort()
    k1, gap13, k3, gap31, stepd = [], [], [], [], []
    for i in range(len(rows) - 2):
        (a0, a1, ka), (b0, b1, kb), (c0, _, kc) = rows[i], rows[i + 1], rows[i + 2]
        if (ka, kb, kc) == ("K1", "K3", "K1"):
            k1.append(a1 - a0)
            gap13.append(b0 - a1)
            k3.append(b1 - b0)
            gap31.append(c0 - b1)
            stepd.append(c0 - a0)
    n = len(k1)
    k1, gap13, k3, gap31, stepd = (x[n // 10:] for x in (k1, gap13, k3, gap31, stepd))   # the first tenth: warm-up
    med = lambda x: statistics.median(x) / 1000.0
    print("seam from %s: %d K1 -> K3 -> K1 triples (medians, us; first tenth dropped)" % (path, len(k1)))
    for label, x in (("K1 duration", k1), ("K1 end -> K3 start", gap13), ("K3 duration", k3),
                     ("K3 end -> next K1 start", gap31), ("step (K1 start -> next K1 start)", stepd)):
        print("  %-34s %8.2f" % (label, med(x)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workload", choices=["C2", "C5"], default="C2")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--phases", action="store_true", help="seam marks of the timing build")
    ap.add_argument("--report", metavar="DIR", help="summarise a rocprofv3 kernel trace under DIR")
    args = ap.parse_args()
    if args.report:
        report(args.report)
    else:
        workload(args)


if __name__ == "__main__":
    main()
