"""The K1 -> K3 seam (the partial-spectrum flush of K1 and of the scan kernel, K3's loads) changes where bytes live,
never a bit of what is computed: the SHA-256 of the float64 spectra of a fixed set of seeded runs -- recorded with the
library before the flush was written through -- must come out again.

Recording (GPU, the library under test; writes the fixture):
    python tests/test_gpu_seam_bitexact.py --write tests/golden/seam_bitexact_sha256.json
"""
import hashlib
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import rtl_power_fftw_amd as rpf  # noqa: E402
from rtl_power_fftw_amd import synth  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "seam_bitexact_sha256.json")
RAGGED = 1531                      # frames: not a multiple of 512, nor of any K1 grid's frames per round

# name -> (N, frames, hann window, frame step or None, seed)
CASES = {
    "C2_rect_4096x10000": (4096, 10000, False, None, 2),
    "C3_hann_4096x10000": (4096, 10000, True, None, 3),
    **{"k1_%d_ragged" % n: (n, RAGGED, False, None, 70 + i) for i, n in enumerate((128, 256, 512, 1024, 2048, 4096, 8192))},
    "strided_hann_4096_half_overlap": (4096, 3001, True, 2048, 80),
}
C5 = dict(N=4096, R=5000, hops=8, seed=50)


def sha(t):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy(), dtype=np.float64).tobytes()).hexdigest()


def spectra():
    """name -> SHA-256 of the float64 spectrum (C5: of the [hops, N] block) on cuda:0."""
    import torch
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    out = {}
    for name, (N, R, hann, step, seed) in CASES.items():
        S = step or N
        nsamp = (R - 1) * S + N
        x = synth.noise_tones_iq_torch(seed, nsamp, dev)
        w = synth.hann_window(N) if hann else None
        pwr = torch.empty(N, dtype=torch.float64, device=dev)
        with rpf.Datastore(rpf.Params(N=N, window=hann, repeats=R, frame_step=step), w) as ds:
            n = ds.accumulate_device(x.data_ptr(), x.numel(), R, pwr.data_ptr(), s)
            torch.cuda.synchronize()
        assert n == R, (name, n)
        out[name] = sha(pwr)
    N, R, H = C5["N"], C5["R"], C5["hops"]
    hops = [synth.noise_tones_iq_torch(C5["seed"] + h, N * R, dev) for h in range(H)]
    pwr = torch.empty(H, N, dtype=torch.float64, device=dev)
    with rpf.Datastore(rpf.Params(N=N, repeats=R)) as ds:
        done = ds.device_fused_hops([h.data_ptr() for h in hops], [2 * N * R] * H, [R] * H, s)
        ds.device_reduce(pwr.data_ptr(), s)
        torch.cuda.synchronize()
    assert done == [R] * H, done
    out["C5_scan_8hops_4096x5000"] = sha(pwr)
    return out


def test_fixture_covers_every_case():
    with open(FIXTURE) as f:
        want = json.load(f)
    assert set(want) == set(CASES) | {"C5_scan_8hops_4096x5000"}
    assert all(len(v) == 64 for v in want.values())


@pytest.mark.gpu
def test_spectra_bit_identical():
    pytest.importorskip("torch")
    with open(FIXTURE) as f:
        want = json.load(f)
    got = spectra()
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not bad, bad


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--write":
        with open(sys.argv[2], "w") as f:
            json.dump(spectra(), f, indent=1, sort_keys=True)
            f.write("\n")
    else:
        print(json.dumps(spectra(), indent=1, sort_keys=True))
