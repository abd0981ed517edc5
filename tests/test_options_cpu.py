"""CPU: the option table of cc_engine_set_option (continuous_clustering_amd/csrc/cc_options.h) without the engine.

tests/csrc/options_probe.cpp includes only that header (g++, no HIP), prints its rows and clamps the values it is given. Checked here:
  * the table's names are exactly the 36 the if / else-if chain it replaced accepted (written out below), exactly the names the option block of
    include/cc_hip.h documents, and hold every option tests/test_gpu_stress.py walks over;
  * every row's kind and bounds, and what it makes of INT32_MIN, -1, 0, 1, its upper bound, its upper bound + 1 and INT32_MAX, against what that
    chain stored (PARENT below restates the chain's expressions, narrowing casts included — nothing here is computed from the table under test);
  * INT64_MIN and INT64_MAX end up inside the row's range: a value beyond 32 bits saturates where the chain's `(int) value` wrapped."""
import ast
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "csrc", "options_probe.cpp")
I32_MIN, I32_MAX, I64_MIN, I64_MAX = -2 ** 31, 2 ** 31 - 1, -2 ** 63, 2 ** 63 - 1
TREE_SLOTS, SL_CAP = 256, 8192  # cc_device.h, cc_k_scan.h (the probe compiles the header with these defaults)


def i32(v):
    """(int) value of the chain: two's-complement narrowing."""
    return (v + 2 ** 31) % 2 ** 32 - 2 ** 31


def clamp(lo, hi):
    return lambda v: i32(lo if v < lo else (hi if v > hi else v))


def boolean(v):
    return int(v != 0)


def tri(v):
    return -1 if v < 0 else int(v != 0)


# name: (kind, lo, hi, what the chain stored for `value`). Three options write two fields: their tuple is compared through the clamped value.
PARENT = {
    "resident": ("bool", 0, 1, boolean),
    "mirror_views": ("bool", 0, 1, boolean),
    "resident_idle_ms": ("int", 1, 10000, clamp(1, 10000)),
    "lds_tree_limit": ("int", 1, TREE_SLOTS, clamp(1, TREE_SLOTS)),
    "pipeline": ("int", -1, 2, lambda v: (v != 0, 2 if v >= 2 else 1)),
    "graphs": ("bool", 0, 1, boolean),
    "sub_batch": ("int", 0, I64_MAX, lambda v: 0 if v < 0 else v),
    "assoc_sweep_blocks": ("int", 1, 1024, clamp(1, 1024)),
    "forget_inclination_table": ("action", 0, 1, boolean),
    "prewarm_small_graphs": ("action", 0, 1, boolean),
    "defer_tail_max_streams": ("int", 0, I32_MAX, lambda v: 0 if v < 0 else i32(v)),
    "assoc_cooldown": ("int", 0, 1000, clamp(0, 1000)),
    "timing_every": ("int", 1, I32_MAX, lambda v: 1 if v < 1 else i32(v)),
    "parallel_insert": ("int", -1, 2, lambda v: (v != 0, v == 1)),
    "input_on_engine_stream": ("bool", 0, 1, boolean),
    "assoc_waves": ("int", 0, 5, lambda v: (True, 3) if v <= 0 or v > 4 else (False, i32(v))),
    "insert_split_blocks": ("int", 0, 8, clamp(0, 8)),
    "insert_wide_max_streams": ("int", 0, 1 << 20, clamp(0, 1 << 20)),
    "skip_idle_fallbacks": ("bool", 0, 1, boolean),
    "fuse_front": ("bool", 0, 1, boolean),
    "small_front": ("bool", 0, 1, boolean),
    "small_all": ("bool", 0, 1, boolean),
    "small_direct": ("bool", 0, 1, boolean),
    "check_input_lifetime": ("int", 0, 2, clamp(0, 2)),
    "lazy_gate": ("int", 0, 4096, clamp(0, 4096)),
    "lazy_gate_from": ("int", 0, 1 << 20, clamp(0, 1 << 20)),
    "seg_small_max": ("int", 0, 63, clamp(0, 63)),
    "assoc_batch": ("bool", 0, 1, boolean),
    "assoc_rounds": ("int", 0, 8, clamp(0, 8)),
    "scan_store_fin": ("tri", -1, 1, tri),
    "scan_split": ("int", 0, 2, clamp(0, 2)),
    "scan_cap": ("int", 1, 1 << 20, clamp(1, 1 << 20)),
    "scan_long_records": ("int", 1, SL_CAP, clamp(1, SL_CAP)),
    "scan_packed": ("tri", -1, 1, tri),
    "mirror_fields": ("bool", 0, 1, boolean),
    "limit_columns": ("int", 1, I32_MAX, lambda v: i32(1 if v < 1 else v)),
}
TWO_FIELDS = {"pipeline", "parallel_insert", "assoc_waves"}


def probes(hi):
    return [v for v in (I32_MIN, -1, 0, 1, hi, hi + 1, I32_MAX) if v <= I64_MAX]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """(rows, clamped): the table as the probe prints it, and its answers for every (name, value) asked below plus one unknown name."""
    exe = os.path.join(str(tmp_path_factory.mktemp("options")), "options_probe")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-o", exe, PROBE], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-4000:]
    asked = [(name, v) for name, (_, _, hi, _) in PARENT.items() for v in probes(hi) + [I64_MIN, I64_MAX]]
    text = "".join("%s %d\n" % q for q in asked) + "no_such_option 1\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    rows, clamped, unknown = {}, {}, []
    for parts in (line.split() for line in r.stdout.splitlines()):
        if parts[0] == "row":
            assert parts[1] not in rows, "option listed twice: " + parts[1]
            rows[parts[1]] = (parts[2], int(parts[3]), int(parts[4]))
        elif parts[0] == "clamp":
            clamped[(parts[1], int(parts[2]))] = int(parts[3])
        else:
            unknown.append(parts[1])
    assert unknown == ["no_such_option"] and set(clamped) == set(asked)
    return rows, clamped


def test_the_table_names_are_the_accepted_the_documented_and_the_walked_ones(probe):
    rows, _ = probe
    assert len(PARENT) == 36 and set(rows) == set(PARENT)
    header = open(os.path.join(ROOT, "include", "cc_hip.h")).read()
    block = header[header.index("Engine tuning / test hooks"):header.index("int cc_engine_set_option(")]
    documented = re.findall(r'^ \*  "([a-z_]+)"', block, flags=re.M)
    assert len(documented) == len(set(documented)) and set(documented) == set(rows), sorted(set(documented) ^ set(rows))
    stress = ast.parse(open(os.path.join(ROOT, "tests", "test_gpu_stress.py")).read())
    walked = [k.value for node in ast.walk(stress) if isinstance(node, ast.Assign) and isinstance(node.value, ast.Dict) and
              any(isinstance(t, ast.Name) and t.id == "choices" for t in node.targets) for k in node.value.keys]
    assert len(walked) >= 10 and set(walked) <= set(rows), sorted(set(walked) - set(rows))


@pytest.mark.parametrize("name", sorted(PARENT))
def test_every_row_clamps_as_the_chain_it_replaced(probe, name):
    rows, clamped = probe
    kind, lo, hi, stored = PARENT[name]
    assert rows[name] == (kind, lo, hi)
    for v in probes(hi):
        got = clamped[(name, v)]
        assert lo <= got <= hi, (v, got)
        if I32_MIN <= v <= I32_MAX or hi == I64_MAX:
            # the 32-bit range (and all of sub_batch's, an int64_t field): exactly what the chain stored
            assert (stored(got) if name in TWO_FIELDS else got) == stored(v), (v, got, stored(v))
        else:
            assert got == hi, (v, got)  # beyond it (an upper bound of INT32_MAX, plus one): saturated, where `(int) value` wrapped
    for v in (I64_MIN, I64_MAX):
        assert lo <= clamped[(name, v)] <= hi, (v, clamped[(name, v)])
