"""CPU: pin constants and the inline helpers of the hot path against the REFERENCE'S OWN HEADERS.

general.hpp, point_types.hpp and utils/thread_pool.hpp need no Eigen, so — unlike cc.cpp (tests/test_reference_build.py, which skips without
Eigen3) — they compile wherever the reference tree is. tests/csrc/reference_headers_probe.cpp static_asserts every CC_GP_* / CC_DBG_* value
(include/cc_hip.h:45-62) and the drop-in class's GP_* enum against the colour enum (general.hpp:208-357), RawPoint / RawPoints size and field
offsets (point_types.hpp:10-28) against the drop-in class's mirror, checks Point3D::operator- + lengthSquared (the association's distance test,
cc.cpp:638-641) against the oracle's close_enough and Point2D::length / lengthXY against the oracle's len2 on 2 M random pairs bit for bit,
and that ThreadPool::enqueue runs a job inline with num_threads == 0 (thread_pool.hpp:31-35,58-64: the single-threaded mode the oracle
restates). The names cc.hpp:15-22 gives the ground labels are checked as text.

What the headers yield (colour values, layouts, a digest of the 2 M pair results, the ground label names) is recorded in
tests/golden/reference_headers.json (tests/golden/make_reference_headers.py writes it from the reference tree). Without the reference tree
($CC_REFERENCE_ROOT) the probe is compiled with -DCC_RECORDED_REFERENCE and the project's side is compared with that record; with the tree the
probe compares both sides directly and the record must still be what the headers yield.
It does not lift "parity unpinned"  — the algorithm itself needs Eigen3 — it takes the constants out of the unpinned set."""
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("CC_REFERENCE_ROOT", "")
RECORD = os.path.join(ROOT, "tests", "golden", "reference_headers.json")
PROBE = os.path.join(ROOT, "tests", "csrc", "reference_headers_probe.cpp")
EXPECTED_GROUND_LABELS = {"GP_UNKNOWN": "WHITE", "GP_GROUND": "GREEN", "GP_OBSTACLE": "RED", "GP_EGO_VEHICLE": "MAGENTA", "GP_FOG": "LIGHTGRAY"}


def reference_include(ref_root=REF):
    """The reference's include/ directory, or None where the tree is not on this machine."""
    inc = os.path.join(ref_root, "include") if ref_root else ""
    return inc if inc and os.path.exists(os.path.join(inc, "continuous_clustering", "clustering", "general.hpp")) else None


def run_probe(out_dir, ref_include=None):
    """Compile and run the probe (against the reference headers, or in recorded mode). Returns (returncode, stdout, parsed lines)."""
    exe = os.path.join(str(out_dir), "reference_headers_probe" + ("" if ref_include else "_recorded"))
    flags = ["-I" + ref_include] if ref_include else ["-DCC_RECORDED_REFERENCE"]
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-Wno-subobject-linkage", *flags, "-o", exe, PROBE], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]  # (a static_assert that fails is a compile error naming the constant)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    parsed = {"pin": {}, "ours": {}, "oracle": {}, "ref": {}}
    for line in r.stdout.splitlines():
        parts = line.split()
        if parts and parts[0] == "pin" and len(parts) == 4:
            parsed["pin"][parts[1]] = (parts[2], int(parts[3]))
        elif parts and parts[0] in ("ours", "oracle", "ref") and len(parts) == 3:
            parsed[parts[0]][parts[1]] = parts[2] if parts[1].endswith("digest") else int(parts[2])
    return r.returncode, r.stdout, parsed


def record_from_probe(parsed):
    """The part of the reference-mode probe output that the record holds."""
    ref = parsed["ref"]
    return {"colours": {k.split(".", 1)[1]: v for k, v in ref.items() if k.startswith("colour.")},
            "layout": {k: v for k, v in ref.items() if k.startswith("RawPoint")},
            "pairs": {"digest": ref["pairs.digest"], "close": ref["pairs.close"]},
            "thread_pool_runs_inline": bool(ref["thread_pool.runs_inline"])}


def ground_label_names(ref_root):
    """cc.hpp:15-22 cannot be compiled without Eigen; the five enumerators are one line each: GP_X = COLOUR."""
    text = open(os.path.join(ref_root, "include", "continuous_clustering", "clustering", "continuous_clustering.hpp")).read()
    return dict(re.findall(r"\b(GP_[A-Z_]+)\s*=\s*([A-Z]+)\s*,", text))


def load_record():
    with open(RECORD) as f:
        return json.load(f)


def test_constants_layouts_and_inline_helpers_match_the_reference_headers(tmp_path):
    rec = load_record()
    # the project's side against the record of what the reference headers yield
    rc, out, got = run_probe(tmp_path)
    assert rc == 0, out[-2000:]
    assert set(got["pin"]) and all(rec["colours"][colour] == value for colour, value in got["pin"].values()), (got["pin"], rec["colours"])
    assert got["ours"] == rec["layout"], (got["ours"], rec["layout"])
    assert got["oracle"]["pairs.digest"] == rec["pairs"]["digest"] and got["oracle"]["pairs.close"] == rec["pairs"]["close"]
    assert rec["pairs"]["close"] > 100000  # both outcomes exercised
    assert rec["thread_pool_runs_inline"] is True
    # where the reference tree is present: both sides compiled together, and the record must be what the headers give today
    inc = reference_include()
    if inc:
        rc, out, got_ref = run_probe(tmp_path, inc)
        assert rc == 0, out[-2000:]
        assert re.search(r"close (\d+) ", out) and int(re.search(r"close (\d+) ", out).group(1)) > 100000, out
        assert " bad 0" in out
        assert record_from_probe(got_ref) == {k: rec[k] for k in ("colours", "layout", "pairs", "thread_pool_runs_inline")}


def test_ground_label_names_of_the_reference_class_header():
    rec = load_record()
    got = rec["ground_label_names"]
    if reference_include():
        got = ground_label_names(REF)
        assert got == rec["ground_label_names"]
    assert got == EXPECTED_GROUND_LABELS
    ours = open(os.path.join(ROOT, "include", "cc_hip.h")).read()
    for name, colour in got.items():
        assert re.search(r"CC_%s = \d+,\s*/\* %s \*/" % (name, colour), ours), (name, colour)
