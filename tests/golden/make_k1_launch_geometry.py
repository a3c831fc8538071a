#!/usr/bin/env python3
"""Records tests/golden/k1_launch_geometry.json: what Datastore.launch_info() reports for every K1 size x sample
format x {plain, windowed} x entry kind of tests/test_gpu_k1_geometry.py, on the MI355X, from the library that is
built in the tree.  Run it on the build whose geometry is to be the yardstick (the fixture in git is from the commit
before K1's per-size tables were merged into one) from the repository root:

    python tests/golden/make_k1_launch_geometry.py [OUTPUT.json]

Each case is launched three times: on a handful of frames (block, frames per workgroup and LDS bytes do not depend on
the stream), on more frames than any resident grid could hold -- workgroups per CU are bounded by the CU's 160 KB of
LDS, its 2048 threads and 32 -- which gives the planned grid, and on the 2 x grid x frames_per_wg frames the test will
use, which has to give the same record.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

import test_gpu_k1_geometry as t  # noqa: E402

CU_LDS_BYTES, CU_THREADS, CU_WORKGROUPS = 160 << 10, 2048, 32


def main():
    prop = torch.cuda.get_device_properties(0)
    cus = prop.multi_processor_count
    records = {}
    for N in t.SIZES:
        for fmt in t.FORMATS:
            for window in (False, True):
                engines = {}
                for kind in t.KINDS:
                    if t.engine_key(kind) not in engines:
                        engines[t.engine_key(kind)] = t.engine_for(kind, N, fmt, window)
                    ds = engines[t.engine_key(kind)]
                    small = t.launch(ds, kind, 2 * t.SERIES_L)
                    per_cu = min(CU_LDS_BYTES // small["lds_bytes"], CU_THREADS // small["block"], CU_WORKGROUPS)
                    rec = t.launch(ds, kind, 2 * per_cu * cus * small["frames_per_wg"])
                    assert rec["grid"] <= per_cu * cus and rec["grid"] % cus == 0, rec
                    assert {f: rec[f] for f in t.FIELDS[1:]} == {f: small[f] for f in t.FIELDS[1:]}, (small, rec)
                    again = t.launch(ds, kind, 2 * rec["grid"] * rec["frames_per_wg"])
                    assert again == rec, (again, rec)
                    records[t.key(N, fmt, window, kind)] = rec
                    print(t.key(N, fmt, window, kind), rec, flush=True)
                for ds in engines.values():
                    ds.close()
    path = sys.argv[1] if len(sys.argv) > 1 else t.FIXTURE
    with open(path, "w") as f:
        json.dump({"device": prop.name, "cu_count": cus, "records": records}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d records, %d CUs" % (path, len(records), cus))


if __name__ == "__main__":
    main()
