"""Cases, streams, bars and record of the STFT phase census (tests/test_stft_forms.py without a GPU,
tests/test_gpu_stft_forms.py on one): the rows of rpf_stft_device against the numpy complex128 transform of the same
prepared frames, at every K1 size x window x format and on the catch-all route from 2 to 2^22 bins.  The figure is
stft_bars.err; prepared_frames, cpu_f32_rows and f64_rows are stft_bars' own.

Fine bar.  BAR = 2 x CPU_F32, the project's standing margin for two float32 implementations of one calculation:
CPU_F32[case] is err of the CPU float32 path (rpf_oracle_fft_f32) on the judged rows' prepared frames, computed by
`tools/gpu_stft_forms.py --cpu-only` before any device run; tests/test_stft_forms.py recomputes every figure and fails if
the record drifts by more than 2 %.  No number here was picked for the GPU.

Exact cases.  At N = 2 and 4 with cu8 the CPU figure is 0: every intermediate is an integer below 2^24 and no twiddle
but 1 and -i occurs, so float32 makes no rounding.  BAR is 0 there and the device must give err == 0.

Coarse bar.  COARSE = 1e-3, asserted for every case without exception.  Each phase-only symmetry error (conjugate, re
and im swapped, negated, im negated, times i, the linear phase of a one-sample shift) leaves every bin's power where it
was (within 1e-15) and gives err >= 1.4 at every size measured (N = 2 ... 2^23, cu8 / cs16 / cf32, rectangular and
Hann); the largest float32 rounding figure measured on the CPU over the candidate sizes is 5.0e-5 (cf32, 2^22 bins, 3
frames).  1e-3 sits 20 x above the one and over 1000 x below the other, so it separates them whatever the fine bar
does.

RECORDED_NOT_ASSERTED (the precedent: the Bluestein lengths of tests/test_gpu_seams.py) may name at most two cases, on
the catch-all route only, whose err exceeded the fine bar on the MI355X for a cause read out of the code and stated
beside the entry; COARSE and the power identity stay asserted for them.  It has one entry.

K1 cases judge 16 rows of F = (RAWD + 1) grid fpw + fpw + 1 frames (k1_rows): the first iteration, the second, the
first one fed from a ring slot refilled inside the loop, the ragged tail.  Which rows those are depends on the store
kernels' resident grid, so GEOMETRY records (grid, frames per workgroup) of every case on the MI355X (256 CUs) and the
GPU test checks that the device plans that grid before it judges."""
import functools

import numpy as np

from rtl_power_fftw_amd import _lib, synth
import stft_bars

K1_SIZES = [64, 128, 256, 512, 1024, 2048, 4096, 8192]
FORMATS = ("cu8", "cs8", "cs16", "cf32")
FORMS = ("rect", "hann")
K1_CASES = [(fmt, N, form) for N in K1_SIZES for form in FORMS for fmt in FORMATS]
JUDGED_ROWS = 16
COARSE = 1e-3
K1_SEED = {"cu8": 2100, "cs8": 2100, "cs16": 2200, "cf32": 2300}


def window_of(N, form):
    return synth.hann_window(N) if form == "hann" else None


# ---- K1: frame count, judged rows, streams ------------------------------------------------------------------------------

def ring_depth(fmt, N):
    """RAWD of k1_size(): kRingSmall by format up to 256 bins, 2 beyond, 1 where cf32's two-deep ring does not fit."""
    if fmt == "cf32":
        return 2 if N in (512, 1024) else 1
    if N <= 256:
        return 2 if fmt == "cs16" else 4
    return 2


def k1_frames(fmt, N, grid, fpw):
    """The smallest count that reaches a frame fed from a ring slot refilled inside the loop and leaves a ragged tail."""
    return (ring_depth(fmt, N) + 1) * grid * fpw + fpw + 1


def k1_rows(fmt, N, grid, fpw):
    """The JUDGED_ROWS rows of a K1 case, ascending: frames 0, 1, fpw - 1; the first, a middle and the last frame of
    iteration 1; the first three of iteration RAWD; F - 2, F - 1; the rest spread evenly."""
    rawd, per, F = ring_depth(fmt, N), grid * fpw, k1_frames(fmt, N, grid, fpw)
    rows = {0, 1, fpw - 1, per, per + per // 2, 2 * per - 1, rawd * per, rawd * per + 1, rawd * per + 2, F - 2, F - 1}
    for k in range(1, 2 * JUDGED_ROWS):
        if len(rows) == JUDGED_ROWS:
            break
        rows.add(k * F // (2 * JUDGED_ROWS))
    assert len(rows) == JUDGED_ROWS and min(rows) == 0 and max(rows) == F - 1
    return sorted(rows)


def k1_samples(fmt):
    """Samples of the longest K1 case of a format: one stream per format serves every size (a case takes its prefix)."""
    both = ("cu8", "cs8") if fmt in ("cu8", "cs8") else (fmt,)
    return max(k1_frames(f, N, *GEOMETRY[(f, N, form)]) * N for f, N, form in K1_CASES if f in both)


def _cu8(seed, nsamples, first=0):
    return np.minimum(synth.noise_tones_iq(seed, nsamples, first=first), 254)        # 255 has no cs8 counterpart


@functools.lru_cache(maxsize=None)
def k1_stream(fmt, nsamples=None):
    """The bytes of a format's K1 stream: cu8 noise_tones_iq (clamped to 254) and cs8 its to_cs8, cs16 the full-range
    noise_tones_cs16, cf32 gaussian_cf32."""
    n = k1_samples(fmt) if nsamples is None else nsamples
    if fmt == "cu8":
        return _cu8(K1_SEED[fmt], n)
    if fmt == "cs8":
        return synth.to_cs8(k1_stream("cu8", nsamples))
    if fmt == "cs16":
        return synth.noise_tones_cs16(K1_SEED[fmt], n)
    return synth.gaussian_cf32(K1_SEED[fmt], n).view(np.uint8)


def frames_of(stream, fmt, N, rows):
    """Frames `rows` of a stream of back-to-back frames, side by side."""
    b = _lib.SAMPLE_BYTES[fmt] * N
    raw = np.ascontiguousarray(stream).reshape(-1).view(np.uint8)
    return np.concatenate([raw[f * b: (f + 1) * b] for f in rows])


def k1_judged_frames(case, grid=None, fpw=None):
    """The judged frames' bytes, side by side, without the stream between them where the generator can seek."""
    fmt, N, form = case
    grid, fpw = GEOMETRY[case] if grid is None else (grid, fpw)
    rows = k1_rows(fmt, N, grid, fpw)
    if fmt in ("cu8", "cs8"):
        raw = np.concatenate([_cu8(K1_SEED[fmt], N, first=f * N) for f in rows])
        return raw if fmt == "cu8" else synth.to_cs8(raw)
    return frames_of(k1_stream(fmt), fmt, N, rows)


# ---- the catch-all route ------------------------------------------------------------------------------------------------

def generic_batch(N):
    return max(1, min(64, (1 << 22) // N))


# (format, N, form); what each size adds: tests/test_gpu_stft_forms.py, section (c)
CATCH_ALL_CASES = ([(fmt, N, "rect") for N in (2, 4, 8, 16, 32) for fmt in ("cu8", "cf32")] +
                   [("cu8", 32, "hann"), ("cf32", 32, "hann"),
                    ("cu8", 32768, "rect"), ("cu8", 32768, "hann"), ("cf32", 32768, "rect"),
                    ("cu8", 131072, "rect"), ("cf32", 131072, "hann"), ("cu8", 262144, "rect"),
                    ("cf32", 524288, "rect"), ("cu8", 1048576, "rect"), ("cu8", 4194304, "rect")])
EXACT_CASES = [("cu8", 2, "rect"), ("cu8", 4, "rect")]


def catch_all_frames(N):
    return 3 if N == 1 << 22 else 2 * generic_batch(N) + 5       # three batches, the last ragged


def catch_all_rows(N):
    B, F = generic_batch(N), catch_all_frames(N)
    return [F - 1] if N == 1 << 22 else [0, B - 1, B, 2 * B, F - 1]


def catch_all_seed(case):
    fmt, N, form = case
    return 2400 + 4 * N.bit_length() + 2 * (form == "hann") + (fmt == "cf32")


def catch_all_stream(case):
    fmt, N, form = case
    n = catch_all_frames(N) * N
    if fmt == "cu8":
        return synth.noise_tones_iq(catch_all_seed(case), n)
    return synth.gaussian_cf32(catch_all_seed(case), n).view(np.uint8)


def catch_all_judged_frames(case):
    fmt, N, form = case
    if fmt == "cu8":
        return np.concatenate([synth.noise_tones_iq(catch_all_seed(case), N, first=f * N) for f in catch_all_rows(N)])
    return frames_of(catch_all_stream(case), fmt, N, catch_all_rows(N))


# ---- figures ------------------------------------------------------------------------------------------------------------

def judged_frames(case):
    return k1_judged_frames(case) if case in GEOMETRY else catch_all_judged_frames(case)


def references(judged, case):
    """(prepared frames, their complex128 rows) of judged frames' bytes: the reference of those rows alone."""
    fmt, N, form = case
    frames = stft_bars.prepared_frames(judged, fmt, N, window=window_of(N, form))
    return frames, stft_bars.f64_rows(frames)


def cpu_figure(case):
    frames, want = references(judged_frames(case), case)
    return stft_bars.err(stft_bars.cpu_f32_rows(frames), want)


def worst(got, want):
    """(err, row, bin) of stft_bars.err's largest term."""
    mag = np.abs(want)
    q = np.abs(np.asarray(got, dtype=np.complex128) - want) / np.maximum(mag, np.median(mag, axis=1, keepdims=True))
    r, k = np.unravel_index(int(np.argmax(q)), q.shape)
    return float(q[r, k]), int(r), int(k)


# (format, N, form) -> (grid, frames per workgroup) of the store kernels' resident grid on the MI355X
GEOMETRY = {('cu8', 64, 'rect'): (1024, 32), ('cs8', 64, 'rect'): (1024, 32), ('cs16', 64, 'rect'): (1024, 32),
    ('cf32', 64, 'rect'): (1024, 32), ('cu8', 64, 'hann'): (1024, 32), ('cs8', 64, 'hann'): (1024, 32),
    ('cs16', 64, 'hann'): (1024, 32), ('cf32', 64, 'hann'): (1024, 32), ('cu8', 128, 'rect'): (512, 32),
    ('cs8', 128, 'rect'): (512, 32), ('cs16', 128, 'rect'): (512, 32), ('cf32', 128, 'rect'): (512, 32),
    ('cu8', 128, 'hann'): (512, 32), ('cs8', 128, 'hann'): (512, 32), ('cs16', 128, 'hann'): (512, 32),
    ('cf32', 128, 'hann'): (512, 32), ('cu8', 256, 'rect'): (512, 16), ('cs8', 256, 'rect'): (512, 16),
    ('cs16', 256, 'rect'): (512, 16), ('cf32', 256, 'rect'): (512, 16), ('cu8', 256, 'hann'): (512, 16),
    ('cs8', 256, 'hann'): (512, 16), ('cs16', 256, 'hann'): (512, 16), ('cf32', 256, 'hann'): (512, 16),
    ('cu8', 512, 'rect'): (1280, 4), ('cs8', 512, 'rect'): (1280, 4), ('cs16', 512, 'rect'): (1024, 4),
    ('cf32', 512, 'rect'): (768, 4), ('cu8', 512, 'hann'): (1024, 4), ('cs8', 512, 'hann'): (1024, 4),
    ('cs16', 512, 'hann'): (1024, 4), ('cf32', 512, 'hann'): (768, 4), ('cu8', 1024, 'rect'): (768, 4),
    ('cs8', 1024, 'rect'): (768, 4), ('cs16', 1024, 'rect'): (512, 4), ('cf32', 1024, 'rect'): (256, 4),
    ('cu8', 1024, 'hann'): (512, 4), ('cs8', 1024, 'hann'): (512, 4), ('cs16', 1024, 'hann'): (512, 4),
    ('cf32', 1024, 'hann'): (256, 4), ('cu8', 2048, 'rect'): (256, 4), ('cs8', 2048, 'rect'): (256, 4),
    ('cs16', 2048, 'rect'): (256, 4), ('cf32', 2048, 'rect'): (256, 4), ('cu8', 2048, 'hann'): (256, 4),
    ('cs8', 2048, 'hann'): (256, 4), ('cs16', 2048, 'hann'): (256, 4), ('cf32', 2048, 'hann'): (256, 4),
    ('cu8', 4096, 'rect'): (256, 2), ('cs8', 4096, 'rect'): (256, 2), ('cs16', 4096, 'rect'): (256, 2),
    ('cf32', 4096, 'rect'): (256, 2), ('cu8', 4096, 'hann'): (256, 2), ('cs8', 4096, 'hann'): (256, 2),
    ('cs16', 4096, 'hann'): (256, 2), ('cf32', 4096, 'hann'): (256, 2), ('cu8', 8192, 'rect'): (256, 1),
    ('cs8', 8192, 'rect'): (256, 1), ('cs16', 8192, 'rect'): (256, 1), ('cf32', 8192, 'rect'): (256, 1),
    ('cu8', 8192, 'hann'): (256, 1), ('cs8', 8192, 'hann'): (256, 1), ('cs16', 8192, 'hann'): (256, 1),
    ('cf32', 8192, 'hann'): (256, 1)}

# (format, N, form) -> err of the CPU float32 path against complex128 on the judged rows
CPU_F32 = {('cu8', 64, 'rect'): 2.115e-07, ('cs8', 64, 'rect'): 2.115e-07, ('cs16', 64, 'rect'): 2.256e-07,
    ('cf32', 64, 'rect'): 2.807e-07, ('cu8', 64, 'hann'): 3.127e-07, ('cs8', 64, 'hann'): 3.127e-07,
    ('cs16', 64, 'hann'): 2.254e-07, ('cf32', 64, 'hann'): 2.467e-07, ('cu8', 128, 'rect'): 2.859e-07,
    ('cs8', 128, 'rect'): 2.859e-07, ('cs16', 128, 'rect'): 2.882e-07, ('cf32', 128, 'rect'): 3.502e-07,
    ('cu8', 128, 'hann'): 3.279e-07, ('cs8', 128, 'hann'): 3.279e-07, ('cs16', 128, 'hann'): 3.122e-07,
    ('cf32', 128, 'hann'): 3.100e-07, ('cu8', 256, 'rect'): 3.315e-07, ('cs8', 256, 'rect'): 3.315e-07,
    ('cs16', 256, 'rect'): 3.927e-07, ('cf32', 256, 'rect'): 4.204e-07, ('cu8', 256, 'hann'): 3.464e-07,
    ('cs8', 256, 'hann'): 3.464e-07, ('cs16', 256, 'hann'): 3.553e-07, ('cf32', 256, 'hann'): 3.411e-07,
    ('cu8', 512, 'rect'): 3.623e-07, ('cs8', 512, 'rect'): 3.623e-07, ('cs16', 512, 'rect'): 3.356e-07,
    ('cf32', 512, 'rect'): 4.536e-07, ('cu8', 512, 'hann'): 6.136e-07, ('cs8', 512, 'hann'): 6.136e-07,
    ('cs16', 512, 'hann'): 4.304e-07, ('cf32', 512, 'hann'): 5.727e-07, ('cu8', 1024, 'rect'): 7.175e-07,
    ('cs8', 1024, 'rect'): 7.175e-07, ('cs16', 1024, 'rect'): 5.199e-07, ('cf32', 1024, 'rect'): 7.015e-07,
    ('cu8', 1024, 'hann'): 6.697e-07, ('cs8', 1024, 'hann'): 6.697e-07, ('cs16', 1024, 'hann'): 5.626e-07,
    ('cf32', 1024, 'hann'): 8.765e-07, ('cu8', 2048, 'rect'): 9.909e-07, ('cs8', 2048, 'rect'): 9.909e-07,
    ('cs16', 2048, 'rect'): 7.042e-07, ('cf32', 2048, 'rect'): 1.211e-06, ('cu8', 2048, 'hann'): 1.149e-06,
    ('cs8', 2048, 'hann'): 1.149e-06, ('cs16', 2048, 'hann'): 7.024e-07, ('cf32', 2048, 'hann'): 1.220e-06,
    ('cu8', 4096, 'rect'): 9.801e-07, ('cs8', 4096, 'rect'): 9.801e-07, ('cs16', 4096, 'rect'): 8.213e-07,
    ('cf32', 4096, 'rect'): 1.854e-06, ('cu8', 4096, 'hann'): 1.931e-06, ('cs8', 4096, 'hann'): 1.931e-06,
    ('cs16', 4096, 'hann'): 1.331e-06, ('cf32', 4096, 'hann'): 1.547e-06, ('cu8', 8192, 'rect'): 1.605e-06,
    ('cs8', 8192, 'rect'): 1.605e-06, ('cs16', 8192, 'rect'): 1.247e-06, ('cf32', 8192, 'rect'): 2.816e-06,
    ('cu8', 8192, 'hann'): 3.021e-06, ('cs8', 8192, 'hann'): 3.021e-06, ('cs16', 8192, 'hann'): 1.953e-06,
    ('cf32', 8192, 'hann'): 1.318e-06, ('cu8', 2, 'rect'): 0.0, ('cf32', 2, 'rect'): 3.985e-08,
    ('cu8', 4, 'rect'): 0.0, ('cf32', 4, 'rect'): 9.327e-08, ('cu8', 8, 'rect'): 4.396e-08,
    ('cf32', 8, 'rect'): 9.180e-08, ('cu8', 16, 'rect'): 1.765e-07, ('cf32', 16, 'rect'): 1.561e-07,
    ('cu8', 32, 'rect'): 1.817e-07, ('cf32', 32, 'rect'): 2.155e-07, ('cu8', 32, 'hann'): 1.708e-07,
    ('cf32', 32, 'hann'): 1.792e-07, ('cu8', 32768, 'rect'): 1.941e-06, ('cu8', 32768, 'hann'): 2.801e-06,
    ('cf32', 32768, 'rect'): 6.880e-06, ('cu8', 131072, 'rect'): 6.632e-06, ('cf32', 131072, 'hann'): 7.422e-06,
    ('cu8', 262144, 'rect'): 4.241e-06, ('cf32', 524288, 'rect'): 2.708e-05, ('cu8', 1048576, 'rect'): 1.195e-05,
    ('cu8', 4194304, 'rect'): 1.466e-05}

BAR = {case: 2.0 * e for case, e in CPU_F32.items()}

# case -> the cause, read out of the code (see the module docstring for what may stand here)
RECORDED_NOT_ASSERTED = {
    ("cu8", 32768, "rect"):
        "err 3.916e-06 = 2.02 x the CPU path's, at frame 64, bin N/8 = 4096.  Not a twiddle: a float32 emulation of "
        "run_fft on the CPU gives this figure to the last digit with the two-level twiddle product and with once-rounded "
        "twiddles alike.  The stream's period-8 tone stands at bin 5N/8 with |X| = 3.2e5, where float32 values are 0.031 "
        "apart; the transform's error there is 0.0168, half a spacing.  The last radix-4 pass of run_fft forms bin N/8 "
        "and bin 5N/8 from the same four inputs (outputs 4p and 4p + 2 of one butterfly, apc + bpd and apc - bpd), so "
        "the same 0.0168 lands on bin N/8, which holds only a weak harmonic (|X| = 4.0e3, below the row's median 4.3e3): "
        "0.0168 / 4295 = 3.9e-6.  rpf_oracle_fft_f32 runs its radix-2 pass last and pairs bin N/8 otherwise (0.0023 "
        "there, 0.0146 on the tone).  Off the multiples of N/16, where the tones' harmonics lie, the device's err is "
        "5.4e-7 and the CPU path's 5.9e-7.  One float32 spacing of the tone over the median is 7.3e-6: either path's "
        "worst is a matter of which way one rounding at the tone's magnitude went."}

# (format, N, form) -> err of rpf_stft_device against complex128 measured by tests/test_gpu_stft_forms.py
MEASURED = {('cu8', 64, 'rect'): 1.914e-07, ('cs8', 64, 'rect'): 1.914e-07, ('cs16', 64, 'rect'): 1.843e-07,
    ('cf32', 64, 'rect'): 2.767e-07, ('cu8', 64, 'hann'): 2.597e-07, ('cs8', 64, 'hann'): 2.597e-07,
    ('cs16', 64, 'hann'): 2.285e-07, ('cf32', 64, 'hann'): 2.455e-07, ('cu8', 128, 'rect'): 2.568e-07,
    ('cs8', 128, 'rect'): 2.568e-07, ('cs16', 128, 'rect'): 2.369e-07, ('cf32', 128, 'rect'): 3.502e-07,
    ('cu8', 128, 'hann'): 2.939e-07, ('cs8', 128, 'hann'): 2.939e-07, ('cs16', 128, 'hann'): 3.364e-07,
    ('cf32', 128, 'hann'): 3.073e-07, ('cu8', 256, 'rect'): 2.607e-07, ('cs8', 256, 'rect'): 2.607e-07,
    ('cs16', 256, 'rect'): 4.046e-07, ('cf32', 256, 'rect'): 3.533e-07, ('cu8', 256, 'hann'): 4.870e-07,
    ('cs8', 256, 'hann'): 4.870e-07, ('cs16', 256, 'hann'): 5.261e-07, ('cf32', 256, 'hann'): 3.326e-07,
    ('cu8', 512, 'rect'): 3.695e-07, ('cs8', 512, 'rect'): 3.695e-07, ('cs16', 512, 'rect'): 3.170e-07,
    ('cf32', 512, 'rect'): 6.329e-07, ('cu8', 512, 'hann'): 4.023e-07, ('cs8', 512, 'hann'): 4.023e-07,
    ('cs16', 512, 'hann'): 4.603e-07, ('cf32', 512, 'hann'): 3.837e-07, ('cu8', 1024, 'rect'): 5.921e-07,
    ('cs8', 1024, 'rect'): 5.921e-07, ('cs16', 1024, 'rect'): 5.199e-07, ('cf32', 1024, 'rect'): 7.001e-07,
    ('cu8', 1024, 'hann'): 6.847e-07, ('cs8', 1024, 'hann'): 6.847e-07, ('cs16', 1024, 'hann'): 5.659e-07,
    ('cf32', 1024, 'hann'): 8.252e-07, ('cu8', 2048, 'rect'): 6.479e-07, ('cs8', 2048, 'rect'): 6.479e-07,
    ('cs16', 2048, 'rect'): 3.827e-07, ('cf32', 2048, 'rect'): 1.384e-06, ('cu8', 2048, 'hann'): 9.161e-07,
    ('cs8', 2048, 'hann'): 9.161e-07, ('cs16', 2048, 'hann'): 7.072e-07, ('cf32', 2048, 'hann'): 8.859e-07,
    ('cu8', 4096, 'rect'): 9.577e-07, ('cs8', 4096, 'rect'): 9.577e-07, ('cs16', 4096, 'rect'): 7.093e-07,
    ('cf32', 4096, 'rect'): 1.318e-06, ('cu8', 4096, 'hann'): 1.459e-06, ('cs8', 4096, 'hann'): 1.459e-06,
    ('cs16', 4096, 'hann'): 1.301e-06, ('cf32', 4096, 'hann'): 8.349e-07, ('cu8', 8192, 'rect'): 1.538e-06,
    ('cs8', 8192, 'rect'): 1.538e-06, ('cs16', 8192, 'rect'): 1.232e-06, ('cf32', 8192, 'rect'): 2.824e-06,
    ('cu8', 8192, 'hann'): 2.414e-06, ('cs8', 8192, 'hann'): 2.414e-06, ('cs16', 8192, 'hann'): 1.548e-06,
    ('cf32', 8192, 'hann'): 1.517e-06, ('cu8', 2, 'rect'): 0.0, ('cf32', 2, 'rect'): 3.985e-08,
    ('cu8', 4, 'rect'): 0.0, ('cf32', 4, 'rect'): 9.327e-08, ('cu8', 8, 'rect'): 5.419e-08,
    ('cf32', 8, 'rect'): 9.273e-08, ('cu8', 16, 'rect'): 1.239e-07, ('cf32', 16, 'rect'): 1.561e-07,
    ('cu8', 32, 'rect'): 1.738e-07, ('cf32', 32, 'rect'): 1.796e-07, ('cu8', 32, 'hann'): 1.635e-07,
    ('cf32', 32, 'hann'): 2.144e-07, ('cu8', 32768, 'rect'): 3.916e-06, ('cu8', 32768, 'hann'): 2.183e-06,
    ('cf32', 32768, 'rect'): 6.924e-06, ('cu8', 131072, 'rect'): 6.720e-06, ('cf32', 131072, 'hann'): 5.933e-06,
    ('cu8', 262144, 'rect'): 4.167e-06, ('cf32', 524288, 'rect'): 9.892e-06, ('cu8', 1048576, 'rect'): 6.909e-06,
    ('cu8', 4194304, 'rect'): 1.464e-05}
