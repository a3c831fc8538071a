#!/usr/bin/env python3
"""Records tests/golden/engine_families.json: per configuration of tests/test_gpu_engine_families.py the frame count,
Datastore.launch_info() after one rpf_accumulate_device, whether the fused four-step kernel is active and the SHA-256
of the output, on the MI355X, from the library that is built in the tree (or RPF_ENGINE_LIB).  Run it on the build
whose choice of kernel family is to be the yardstick (the fixture in git is from the commit before the family became
one enumerator) from the repository root:

    python tests/golden/make_engine_families.py [OUTPUT.json]

The frame count: a first launch over as many frames as 64 MB hold says what grid and frames per workgroup the case
runs with; 2 x grid x frames_per_wg frames if that many fit (the grid was then not trimmed to the frames: it is the
planned one), else the test's FEW.  Every case then runs twice in fresh engines.  Two different digests are recorded
as null, which only a case with the fused kernel active may do: anything else stops the recorder.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

import test_gpu_engine_families as t  # noqa: E402


def main():
    prop = torch.cuda.get_device_properties(0)
    records = {}
    for case in t.CASES:
        with t.engine_for(case) as ds:
            most = t.max_frames(ds)
        probe = t.run(case, most)
        want = 2 * probe["grid"] * probe["frames_per_wg"]
        frames = want if want <= most else min(t.FEW, most)
        first, second = t.run(case, frames), t.run(case, frames)
        if first["sha256"] != second["sha256"]:
            assert first["fused_active"], "%s: two runs, two digests, and no fused kernel: %s %s" % (case, first, second)
            first["sha256"] = second["sha256"] = None
        assert first == second, (case, first, second)
        records[case] = first
        print(case, first, flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else t.FIXTURE
    with open(path, "w") as f:
        json.dump({"device": prop.name, "cu_count": prop.multi_processor_count, "records": records}, f, indent=0,
                  sort_keys=True)
        f.write("\n")
    print("wrote %s: %d records, %d CUs" % (path, len(records), prop.multi_processor_count))


if __name__ == "__main__":
    main()
