"""CPU: the range a reader needs that hands the columns a stream still holds over as whole rotations, rotation r into slot r % slots of a
ring of row-major images (image_range / image_rotation_share, continuous_clustering_amd/csrc/cc_k_held.h), without HIP.

tests/csrc/image_range_probe.cpp includes only that header (g++, CC_HELD_RANGE_ONLY) and prints both functions for the tuples it is given.
No kernel calls them yet. Expected values come from `rule` below, a restatement that shares no expression with the header, and from the
figures written out next to each case."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "csrc", "image_range_probe.cpp")
W, RING = 360, 3600


def rule(first, cleared, upper, cursor, ring, w, slots):
    """(from, to, readable_from, lost, skipped, rotation_from, rotation_to) and {rotation: (written, lost)}"""
    to = max(upper, cursor, first, cleared)
    lo = max(cursor, first, cleared, to - ring)                   # the held range [lo, to)
    lost = lo - max(cursor, first)
    begin = max(cursor, first - first % w if first >= 0 else 0)   # the whole first rotation is written
    if lo // w > begin // w:                                      # the rotation the cursor stands in is abandoned
        begin = lo - lo % w
    skipped = 0
    oldest = (to // w - (slots - 1)) * w                          # the image ring holds `slots` rotations
    if begin < oldest:
        skipped = max(0, oldest - max(begin, lo))
        begin = oldest
    shares = {}
    for col in range(begin, to) if to - begin <= slots * w else ():
        wr, ls = shares.get(col // w, (0, 0))
        shares[col // w] = (wr + 1, ls + (1 if first <= col < lo else 0))
    return (begin, to, max(begin, lo), lost, skipped, begin // w, max(begin // w, to // w)), shares


B = (2 ** 31 // W + 1) * W   # the first rotation boundary past 2^31
T = (2 ** 40 // W + 1) * W
# name: ((first_column, clear_done, upper, cursor, slots), (from, to, readable_from, lost, skipped, rotation_from, rotation_to), {rotation: (written, lost)})
CASES = {
    "never started": ((-1, -1, -1, 0, 3), (0, 0, 0, 0, 0, 0, 0), {}),
    "first take, first column mid-rotation": ((100, -1, 300, 0, 3), (0, 300, 100, 0, 0, 0, 0), {0: (300, 0)}),
    "first take, first column in the middle of rotation 2": ((800, -1, 1000, 0, 3), (720, 1000, 800, 0, 0, 2, 2), {2: (280, 0)}),
    "continuation mid-rotation": ((100, 50, 700, 500, 3), (500, 700, 500, 0, 0, 1, 1), {1: (200, 0)}),
    "nothing new": ((100, 50, 700, 700, 3), (700, 700, 700, 0, 0, 1, 1), {}),
    "ends exactly at a boundary": ((100, 50, 720, 500, 3), (500, 720, 500, 0, 0, 1, 2), {1: (220, 0)}),
    "crossing one boundary": ((100, -1, 400, 300, 3), (300, 400, 300, 0, 0, 0, 1), {0: (60, 0), 1: (40, 0)}),
    "crossing two boundaries": ((100, -1, 1000, 300, 3), (300, 1000, 300, 0, 0, 0, 2), {0: (60, 0), 1: (360, 0), 2: (280, 0)}),
    "clear_done beyond the cursor inside its rotation": ((10, 500, 900, 400, 3), (400, 900, 500, 100, 0, 1, 2), {1: (320, 100), 2: (180, 0)}),
    "clear_done beyond the cursor in a later rotation": ((10, 800, 1200, 400, 3), (720, 1200, 800, 400, 0, 2, 3), {2: (360, 80), 3: (120, 0)}),
    "clear_done beyond a cursor below first_column": ((100, 200, 300, 0, 3), (0, 300, 200, 100, 0, 0, 0), {0: (300, 100)}),
    "cursor sought past upper": ((10, 500, 900, 1000, 3), (1000, 1000, 1000, 0, 0, 2, 2), {}),
    "overrun, 2 slots": ((0, 0, 1500, 100, 2), (1080, 1500, 1080, 0, 980, 3, 4), {3: (360, 0), 4: (60, 0)}),
    "overrun, 3 slots": ((0, 0, 1500, 100, 3), (720, 1500, 720, 0, 620, 2, 4), {2: (360, 0), 3: (360, 0), 4: (60, 0)}),
    "no overrun, 5 slots": ((0, 0, 1500, 100, 5), (100, 1500, 100, 0, 0, 0, 4), {0: (260, 0), 1: (360, 0), 2: (360, 0), 3: (360, 0), 4: (60, 0)}),
    "overrun and loss, 2 slots": ((0, 500, 1500, 100, 2), (1080, 1500, 1080, 400, 580, 3, 4), {3: (360, 0), 4: (60, 0)}),
    "overrun up to a boundary, 2 slots": ((0, 0, 1440, 100, 2), (1080, 1440, 1080, 0, 980, 3, 4), {3: (360, 0)}),
    "past 2^31: continuation across a boundary": ((5, B + 40, B + 500, B + 100, 3), (B + 100, B + 500, B + 100, 0, 0, B // W, B // W + 1),
                                                  {B // W: (260, 0), B // W + 1: (140, 0)}),
    "past 2^31: cleared beyond the cursor": ((5, B + 200, B + 300, B + 100, 3), (B + 100, B + 300, B + 200, 100, 0, B // W, B // W), {B // W: (200, 100)}),
    "past 2^31: more than a ring, 3 slots": ((5, 40, B + 9000, B + 100, 3), (B + 8280, B + 9000, B + 8280, 5300, 2880, B // W + 23, B // W + 25),
                                             {B // W + 23: (360, 0), B // W + 24: (360, 0)}),
    "past 2^40: cursor far below": ((5, T + 10, T + 400, 17, 3), (T, T + 400, T + 10, T + 10 - 17, 0, T // W, T // W + 1), {T // W: (360, 10), T // W + 1: (40, 0)}),
}


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """name -> (the seven figures, {rotation: (written, lost)}) as the probe prints them"""
    exe = os.path.join(str(tmp_path_factory.mktemp("images")), "image_range_probe")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-o", exe, PROBE], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-4000:]
    names = sorted(CASES)
    text = "".join("%d %d %d %d %d %d %d\n" % (CASES[n][0][:4] + (RING, W, CASES[n][0][4])) for n in names)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [line.split() for line in r.stdout.splitlines()]
    assert len(lines) == len(names) and all(p[0] == "image" and p[8] == "shares" for p in lines), r.stdout[-2000:]
    out = {}
    for n, p in zip(names, lines):
        shares = {int(a): (int(b), int(c)) for a, b, c in (x.split(":") for x in p[9:])}
        out[n] = (tuple(int(x) for x in p[1:8]), shares)
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_image_range(answers, name):
    (first, cleared, upper, cursor, slots), written_out, shares_out = CASES[name]
    mine, my_shares = rule(first, cleared, upper, cursor, RING, W, slots)
    assert mine == written_out and my_shares == shares_out, ("the test's own two statements of the rule disagree", mine, my_shares)
    got, got_shares = answers[name]
    assert got == written_out, (CASES[name][0], got)
    assert got_shares == shares_out, (CASES[name][0], got_shares)
    frm, to, readable, lost, skipped, rf, rt = got
    assert frm <= readable <= to or frm == to
    assert lost >= 0 and skipped >= 0 and to - frm <= slots * W and len(got_shares) <= slots
    assert sum(w for w, _ in got_shares.values()) == to - frm
    # the rotations whose last column is written are exactly those whose end lies inside (from, to]
    assert list(range(rf, rt)) == [r for r in sorted(got_shares) if (r + 1) * W <= to]
