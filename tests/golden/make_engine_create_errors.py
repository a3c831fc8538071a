#!/usr/bin/env python3
"""Records tests/golden/engine_create_errors.json: the return code and rpf_last_global_error() text of
rpf_engine_create / rpf_engine_create_pfb for every configuration of tests/test_engine_create.py, from the library that
is built in the tree (or RPF_ENGINE_LIB), on a machine WITHOUT a GPU -- there a configuration that passes every check
answers "No HIP device available", which is the point.  Run it on the build whose checks are to be the yardstick (the
fixture in git is from the commit before create_engine was taken apart) from the repository root:

    python tests/golden/make_engine_create_errors.py [OUTPUT.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import test_engine_create as t  # noqa: E402


def main():
    assert not t.have_gpu(), "record this on a machine without a GPU"
    records = {}
    for name, c in t.CASES.items():
        records[name] = list(t.create(c))
        print(name, records[name], flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else t.FIXTURE
    with open(path, "w") as f:
        json.dump(records, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d records" % (path, len(records)))


if __name__ == "__main__":
    main()
