"""Which kernel family an engine configuration gets, on the MI355X: one configuration per rule of csrc/engine_family.h's
select_family (and per form inside a family), at the smallest size that takes the rule.  A wrong choice still passes
parity -- it is a slower or slightly different spectrum -- so what is compared is what tells the families apart: the
launch geometry after one rpf_accumulate_device (grid, workgroup size, frames per workgroup, dynamic LDS), whether the
fused four-step kernel is active, and the SHA-256 of the N float64 output bytes for a seeded synth stream.
tests/golden/engine_families.json holds what the build before the family became one enumerator gave
(tests/golden/make_engine_families.py wrote it).  Exact equality throughout.

The frame count of a case is the fixture's: 2 x grid x frames_per_wg where that stream stays within 64 MB (K1, mixed
and Bluestein trim their grid to the frames: the launched grid is then the planned one), FEW frames otherwise.  The
recorder ran every case twice in fresh engines; where the two digests differed the fixture's digest is null and the
rest is compared -- which only a case whose fused kernel is active may do (the fused kernel's teams add their rounds in
the order they finish).  `grid` is compared on a device with the fixture's CU count only."""
import hashlib
import json
import os

import pytest

import rtl_power_fftw_amd as rpf
from rtl_power_fftw_amd import _lib, synth
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda:0")

FIXTURE = os.path.join(GOLDEN, "engine_families.json")
FIELDS = ("grid", "block", "frames_per_wg", "lds_bytes")
MAX_STREAM_BYTES = 64 << 20
FEW = 16
SEED = 20261019

# name: the rule under test -> what the engine is created with (N first; the rest default to a plain cu8 engine)
CASES = {
    "k1": dict(N=512),
    "catch_all_by_flag": dict(N=512, flags=_lib.FLAG_CATCH_ALL),
    "mixed_planned": dict(N=1000),
    "mixed_split": dict(N=20000),                               # 2 x 10000, mixed_plans_split.inc
    "mixed_stockham": dict(N=486),                              # 2 x 3^5: in neither plan table
    "no_mixed_to_bluestein": dict(N=1000, flags=_lib.FLAG_NO_MIXED_RADIX),
    "bluestein": dict(N=2046),
    "large_bluestein": dict(N=4098),
    "no_mixed_to_large_bluestein": dict(N=20000, flags=_lib.FLAG_NO_MIXED_RADIX),
    "no_mixed_to_fourstep": dict(N=16384, flags=_lib.FLAG_NO_MIXED_RADIX),
    "fused_flag_to_fourstep": dict(N=16384, flags=_lib.FLAG_FOURSTEP_FUSED),
    "mixed_32768": dict(N=32768),
    "fourstep_windowed_32768": dict(N=32768, window=True),
    "two_kernel_windowed_32768": dict(N=32768, window=True, flags=_lib.FLAG_NO_FOURSTEP_FUSED),
    "fourstep_fused": dict(N=65536),
    "fourstep_two_kernel": dict(N=65536, flags=_lib.FLAG_NO_FOURSTEP_FUSED),
    "fourstep_overlapped": dict(N=65536, step=32768),           # two-kernel, gathered
    "generic_power_of_two": dict(N=524288),
    "generic_bluestein_form": dict(N=131074),
    "signed_format_to_catch_all": dict(N=1000, fmt="cs8"),
    "stats_to_catch_all": dict(N=1000, stats=True),
    "cf32_to_catch_all": dict(N=65536, fmt="cf32"),
    "pfb_over_k1": dict(N=512, taps=4),
    "pfb_over_catch_all": dict(N=1000, taps=4),
}


def engine_for(case):
    c = CASES[case]
    N, window = c["N"], c.get("window", False)
    params = rpf.Params(N=N, window=window, frame_step=c.get("step"), sample_format=c.get("fmt", "cu8"),
                        bin_stats=c.get("stats", False), pfb_taps=c.get("taps", 0))
    return rpf.Datastore(params, synth.hann_window(N) if window else None, flags=c.get("flags", 0))


def max_frames(ds):
    """The frames a stream of MAX_STREAM_BYTES holds on this engine."""
    return ds.frames_in(MAX_STREAM_BYTES)


def stream_for(ds, case, frames):
    """The seeded stream of `frames` frames in the engine's format, on the device: synth's noise + tones bytes as they
    are (cu8), re-centred (cs8), or as the float32 values v - 127 (cf32)."""
    nbytes = ds.frame_span(frames)
    assert nbytes <= MAX_STREAM_BYTES
    fmt = CASES[case].get("fmt", "cu8")
    u = synth.noise_tones_iq_torch(SEED, nbytes // ds.sample_bytes, DEV)
    if fmt == "cs8":
        u = (u.to(torch.int16) - 127).to(torch.int8).view(torch.uint8)
    elif fmt == "cf32":
        u = (u.to(torch.float32) - 127.0).view(torch.uint8)
    else:
        assert fmt == "cu8"
    assert u.numel() == nbytes
    return u


def run(case, frames):
    """One rpf_accumulate_device over `frames` frames in a fresh engine: what the fixture holds for the case."""
    with engine_for(case) as ds:
        N = ds.params.N
        stream = stream_for(ds, case, frames)
        out = torch.empty(N, dtype=torch.float64, device=DEV)
        s = torch.cuda.current_stream().cuda_stream
        assert ds.accumulate_device(stream.data_ptr(), stream.numel(), frames, out.data_ptr(), s) == frames
        torch.cuda.synchronize()
        rec = dict(ds.launch_info())
        rec["frames"] = frames
        rec["fused_active"] = ds.fused_status()["active"]
        rec["sha256"] = hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()
    return rec


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_the_cases_and_only_fused_digests_are_open(recorded):
    assert sorted(recorded["records"]) == sorted(CASES)
    for case, want in recorded["records"].items():
        assert want["sha256"] is not None or want["fused_active"], case


@pytest.mark.parametrize("case", list(CASES))
def test_family_is_the_recorded_one(recorded, case):
    want = recorded["records"][case]
    same_cus = torch.cuda.get_device_properties(0).multi_processor_count == recorded["cu_count"]
    got = run(case, want["frames"])
    print("%s: %s%s" % (case, got, "" if same_cus else " (another CU count: grid not compared)"))
    compared = [f for f in (FIELDS if same_cus else FIELDS[1:])] + ["fused_active"]
    if want["sha256"] is not None:
        compared.append("sha256")
    assert {f: got[f] for f in compared} == {f: want[f] for f in compared}
