"""CPU: the range a reader of held columns may look at (held_range / held_from, continuous_clustering_amd/csrc/cc_k_held.h) without HIP.

tests/csrc/held_range_probe.cpp includes only that header (g++, CC_HELD_RANGE_ONLY) and prints both functions for the tuples it is given.
The plan kernels of the takes and of the replay evaluator, the id backlog and the cursor queries on the host all call these two functions.
Expected values come from `rule` below, a restatement that shares no expression with the header, and — for the cases the contract names
("The range of held columns") — from the figures written out next to them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "csrc", "held_range_probe.cpp")
RING = 3600


def rule(first, cleared, upper, cursor, ring):
    """(from, to, lost): nothing below the cursor, the stream's first column or what was cleared; up to `upper`; at most a ring."""
    to = max(upper, cursor, first, cleared)
    lo = max(cursor, first, cleared, to - ring)
    return lo, to, lo - max(cursor, first)


B = 2 ** 31  # 64-bit columns: the same cases, this far up
# name: ((first_column, clear_done, upper, cursor, ring_cols), (from, to, lost) written out)
CASES = {
    "never started": ((-1, -1, -1, 0, RING), (0, 0, 0)),
    "never started, cursor sought": ((-1, -1, -1, 7, RING), (7, 7, 0)),
    "cursor below first_column": ((100, -1, 300, 0, RING), (100, 300, 0)),
    "cursor below first_column, some cleared below it too": ((100, 50, 300, 0, RING), (100, 300, 0)),
    "clear_done beyond the cursor": ((10, 500, 900, 200, RING), (500, 900, 300)),
    "clear_done beyond a cursor below first_column": ((250, 500, 900, 200, RING), (500, 900, 250)),
    "cursor at clear_done": ((10, 500, 900, 500, RING), (500, 900, 0)),
    "cursor sought past upper": ((10, 500, 900, 1000, RING), (1000, 1000, 0)),
    "cursor at upper": ((10, 500, 900, 900, RING), (900, 900, 0)),
    "more than a ring": ((0, 0, 5000, 100, RING), (1400, 5000, 1300)),
    "exactly a ring": ((0, 0, 3700, 100, RING), (100, 3700, 0)),
    "a ring and one": ((0, 0, 3701, 100, RING), (101, 3701, 1)),
    "more than a ring, cleared in between": ((0, 1000, 5000, 100, RING), (1400, 5000, 1300)),
    "past 2^31: plain": ((B + 5, B + 40, B + 2000, B + 100, RING), (B + 100, B + 2000, 0)),
    "past 2^31: cleared beyond the cursor": ((B + 5, B + 700, B + 2000, B + 100, RING), (B + 700, B + 2000, 600)),
    "past 2^31: more than a ring": ((5, 40, B + 9000, B + 100, RING), (B + 5400, B + 9000, 5300)),
    "past 2^31: cursor far below": ((5, 2 ** 40, 2 ** 40 + 2200, 17, RING), (2 ** 40, 2 ** 40 + 2200, 2 ** 40 - 17)),
    "past 2^31: cursor sought past upper": ((5, 40, B + 9000, 2 ** 40, RING), (2 ** 40, 2 ** 40, 0)),
}


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """name -> ((from, to, lost), held_from) as the probe prints them"""
    exe = os.path.join(str(tmp_path_factory.mktemp("held")), "held_range_probe")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-o", exe, PROBE], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-4000:]
    names = sorted(CASES)
    text = "".join("%d %d %d %d %d\n" % CASES[n][0] for n in names)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [line.split() for line in r.stdout.splitlines()]
    assert len(lines) == len(names) and all(p[0] == "range" and p[4] == "from" and len(p) == 6 for p in lines), r.stdout[-2000:]
    return {n: ((int(p[1]), int(p[2]), int(p[3])), int(p[5])) for n, p in zip(names, lines)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_held_range_and_held_from(answers, name):
    args, written_out = CASES[name]
    first, cleared, _, cursor, _ = args
    assert rule(*args) == written_out, "the test's own two statements of the rule disagree"
    got, got_from = answers[name]
    assert got == written_out, (args, got)
    lo, to, lost = got
    assert lo <= to and lost >= 0 and to - lo <= args[4]
    # the lower end alone (the cursor queries, the id backlog): the range's, before the ring clamp
    assert got_from == max(cursor, first, cleared), (args, got_from)
    assert lo == max(got_from, to - args[4])
