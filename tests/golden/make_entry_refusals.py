#!/usr/bin/env python3
"""Records what the engine's entry points answer when they refuse a call, from the library that is built in the tree (or
RPF_ENGINE_LIB).  Run it on the build whose answers are to be the yardstick (the fixtures in git are from the commit
before the entries' refusals, inner engines and piece loops were stated once), from the repository root:

    python tests/golden/make_entry_refusals.py null [OUTPUT.json]     any machine: tests/golden/entry_refusals_null.json,
                                                                       the cases of tests/test_entry_refusals.py
    python tests/golden/make_entry_refusals.py gpu [OUTPUT.json]      on the MI355X: tests/golden/entry_refusals.json,
                                                                       the cases of tests/test_gpu_entry_refusals.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def write(path, records, count):
    with open(path, "w") as f:
        json.dump(records, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d records" % (path, count))


def record_null(path):
    import test_entry_refusals as t
    records = {}
    for name in t.CASES:
        records[name] = t.answer(name)
        print(name, records[name], flush=True)
    write(path or t.FIXTURE, records, len(records))


def record_gpu(path):
    import test_gpu_entry_refusals as t
    c = t.Context()
    records = {"refusals": {}, "out_parameters": {}}
    for name in t.CASES:
        records["refusals"][name] = t.answer(c, name)
        print(name, records["refusals"][name], flush=True)
    for name in t.OUT_CASES:
        records["out_parameters"][name] = t.out_answer(c, name)
        print(name, records["out_parameters"][name], flush=True)
    c.close()
    write(path or t.FIXTURE, records, len(records["refusals"]) + len(records["out_parameters"]))


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else ""
    path = sys.argv[2] if len(sys.argv) > 2 else None
    if which == "null":
        record_null(path)
    elif which == "gpu":
        record_gpu(path)
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    main()
