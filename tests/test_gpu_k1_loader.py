"""K1 at 4096 bins with the loader wave (csrc/k1_loader.h) on the MI355X: cu8, rectangular window, random bytes of a
fixed seed, against the engine's own VGPR-staging kernel, which has no loader and no LDS-DMA.  The same bytes at a
device pointer that is 2 mod 16 take that kernel (rpf_engine.cpp: LDS-DMA needs 16-byte alignment); frames go to the
same workgroups and meet the same accumulators in the same order in both, so the float64 spectra are required to be
the same bits, np.array_equal.  (On the commit before the loader the two kernels were already bit-identical at every
frame count below -- measured with this file; profiles/k1_loader.json has the run.)

Frame counts, with F = grid x frames_per_wg of launch_info(): 1, 2, 3 (fewer workgroups than CUs, an inactive second
frame slot), F/2, F-1, F, F+1 (exactly one iteration and the first step into a second), 2F, 2F+1, 3F+7, 4F-1 (two, three
and four iterations: the two-deep ring wraps at three; ragged last rounds).  Every count runs twice on ONE engine with
another count in between: a ring slot, a counter or a barrier left in a state by one launch would show in the next."""
import numpy as np
import pytest

import rtl_power_fftw_amd as rpf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda:0")
N = 4096


@pytest.fixture(scope="module")
def rig():
    """One engine, the random stream on the device at an aligned and at a 2-mod-16 pointer, and the cache of reference
    spectra (computed once per frame count, never written again)."""
    ds = rpf.Datastore(rpf.Params(N=N))
    li = ds.launch_info()
    F = li["grid"] * li["frames_per_wg"]
    nbytes = 2 * N * (4 * F - 1)
    rng = np.random.default_rng(20260)
    host = torch.from_numpy(rng.integers(0, 256, size=nbytes, dtype=np.uint8))
    aligned = torch.empty(nbytes + 64, dtype=torch.uint8, device=DEV)
    shifted = torch.empty(nbytes + 64, dtype=torch.uint8, device=DEV)
    a0 = (-aligned.data_ptr()) % 16
    s0 = (2 - shifted.data_ptr()) % 16
    aligned[a0:a0 + nbytes].copy_(host)
    shifted[s0:s0 + nbytes].copy_(host)
    torch.cuda.synchronize()
    box = {"ds": ds, "F": F, "aligned": aligned.data_ptr() + a0, "shifted": shifted.data_ptr() + s0,
           "keep": (aligned, shifted), "want": {}}
    assert box["aligned"] % 16 == 0 and box["shifted"] % 16 == 2
    yield box
    ds.close()


def run(box, ptr, R):
    out = torch.zeros(N, dtype=torch.float64, device=DEV)
    n = box["ds"].accumulate_device(ptr, 2 * N * R, R, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert n == R
    return out.cpu().numpy()


def reference(box, R):
    if R not in box["want"]:
        want = run(box, box["shifted"], R)
        want.setflags(write=False)
        box["want"][R] = want
    return box["want"][R]


def frame_counts(F):
    return {"1": 1, "2": 2, "3": 3, "F/2": F // 2, "F-1": F - 1, "F": F, "F+1": F + 1, "2F": 2 * F, "2F+1": 2 * F + 1,
            "3F+7": 3 * F + 7, "4F-1": 4 * F - 1}


CASES = ["1", "2", "3", "F/2", "F-1", "F", "F+1", "2F", "2F+1", "3F+7", "4F-1"]


@pytest.mark.parametrize("case", CASES)
def test_loader_kernel_is_bit_identical_to_the_vgpr_staging_kernel(rig, case):
    counts = frame_counts(rig["F"])
    R = counts[case]
    other = counts[CASES[(CASES.index(case) + 5) % len(CASES)]]      # another count in between, another iteration count
    assert other != R
    want = reference(rig, R)
    assert want.min() > 0.0                                           # random bytes: every bin has power
    first = run(rig, rig["aligned"], R)
    between = run(rig, rig["aligned"], other)
    second = run(rig, rig["aligned"], R)
    print("R=%d (%s, F=%d): first %s, second %s; in between R=%d %s" % (
        R, case, rig["F"], np.array_equal(first, want), np.array_equal(second, want), other,
        np.array_equal(between, reference(rig, other))))
    assert np.array_equal(first, want)
    assert np.array_equal(between, reference(rig, other))
    assert np.array_equal(second, want)
