#!/usr/bin/env python3
"""Regenerate tests/golden/reference_headers.json: what the reference's Eigen-free headers yield, recorded so that
tests/test_reference_headers.py can check the project against them where the reference tree is absent.

PROVENANCE: tests/csrc/reference_headers_probe.cpp compiled against the reference's include/ directory (UniBwTAS/continuous_clustering,
general.hpp, point_types.hpp, utils/thread_pool.hpp) prints the colour enum values, the RawPoint / RawPoints layout, a digest of the
distance test and xy length over 2 M seeded pairs and whether ThreadPool(0) runs jobs inline; continuous_clustering.hpp:15-22 gives the
names of the ground labels. Only these results are stored, no program text of the reference.

    CC_REFERENCE_ROOT=<reference tree> python tests/golden/make_reference_headers.py
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import test_reference_headers as trh  # noqa: E402


def main():
    ref_root = os.environ.get("CC_REFERENCE_ROOT", "")
    inc = trh.reference_include(ref_root)
    if not inc:
        raise SystemExit("set CC_REFERENCE_ROOT to the reference tree (its include/continuous_clustering/clustering/general.hpp must exist)")
    with tempfile.TemporaryDirectory() as tmp:
        rc, out, parsed = trh.run_probe(tmp, inc)
    if rc != 0:
        raise SystemExit("the probe found differences:\n" + out[-2000:])
    rec = trh.record_from_probe(parsed)
    rec["ground_label_names"] = trh.ground_label_names(ref_root)
    rec = {"source": "UniBwTAS/continuous_clustering include/continuous_clustering (general.hpp, point_types.hpp, utils/thread_pool.hpp, "
                     "clustering/continuous_clustering.hpp), through tests/csrc/reference_headers_probe.cpp", **rec}
    with open(trh.RECORD, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, sort_keys=True))


if __name__ == "__main__":
    main()
