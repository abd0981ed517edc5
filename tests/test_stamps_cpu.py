"""CPU: the host twins of the firing-stamp log (include/cc_stamps.h) against the plain-Python model of tests/stamp_cases.py,
which is written from the reference's lines (cc.cpp:1007-1010, 1025-1028, 1121; ros_utils.cpp:51-71, 251-266): resolution across a ring
wrap, across 2^32 and with nothing pushed; the cluster, column and sec / nsec rules at the edges of uint64; struct sizes; the C-ABI's
exports and refusals. Nothing here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import stamp_cases as sc
from continuous_clustering_amd import EngineError, capi, stamps, take

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = sc.M64


@pytest.fixture(scope="module")
def lib():
    from continuous_clustering_amd import build, load_library
    build.build()
    load_library()
    return stamps._lib()


@pytest.fixture(scope="module")
def logs(lib):
    return sc.fill_log(stamps.HostFiringStamps(sc.S, sc.CAPACITY)), sc.fill_log(sc.ModelLog(sc.S, sc.CAPACITY))


def _both(logs, stream, keys):
    twin, model = logs
    got, miss = twin.resolve(stream, keys)
    ref = [model.resolve(stream, k) for k in keys]
    assert [int(v) for v in got] == [v for v, _ in ref] and [bool(m) for m in miss] == [m for _, m in ref]
    return got, miss


def test_resolution_across_a_ring_wrap(logs):
    """capacity 1024, 3000 pushed: 1975 is gone although its slot holds firing 2999's stamp, 1976 is the oldest held, 3000 is not pushed yet"""
    twin, model = logs
    assert twin.capacity == 1024 and twin.counters(0) == (3000, 0)
    pushed = twin.rings[0][np.arange(1976, 3000) & 1023]
    got, miss = _both(logs, 0, sc.WRAP_KEYS)
    assert list(miss) == [True, False, False, True] and got[0] == 0 and got[3] == 0
    assert 1975 & 1023 == 2999 & 1023 and twin.rings[0][1975 & 1023] == got[2] != 0
    assert got[1] == pushed[0] and got[2] == pushed[-1]
    keys = np.arange(1900, 3010)
    got, miss = _both(logs, 0, keys)
    assert np.array_equal(miss, (keys < 1976) | (keys >= 3000)) and (got[~miss] != 0).all()
    assert not np.all(np.diff(got[~miss].astype(np.int64)) > 0)            # (the stamps are not monotonic in the firing index)


def test_resolution_across_two_to_the_32(logs):
    twin, _ = logs
    assert twin.counters(2)[0] == (1 << 32) + 500
    idx = np.arange(sc.SEEK_AT - 40, sc.SEEK_AT + 1020)
    got, miss = _both(logs, 2, idx & sc.M32)
    assert np.array_equal(miss, (idx < sc.SEEK_AT) | (idx >= sc.SEEK_AT + 1000))   # nothing from before the seek, nothing beyond the head
    assert np.array_equal(got[~miss], twin.rings[2][idx[~miss] & 1023])
    assert (idx[~miss] & sc.M32).min() == 0 and (idx[~miss] & sc.M32).max() == sc.M32  # keys from both sides of the boundary


def test_nothing_pushed_resolves_nothing(logs, lib):
    got, miss = _both(logs, 1, [0, 1, 1023, sc.M32])
    assert miss.all() and not got.any()
    fresh = stamps.HostFiringStamps(1, 8)
    fresh.seek(0, 5000)                                                          # head != 0 but nothing held
    got, miss = fresh.resolve(0, [4999, 5000, 4992])
    assert miss.all() and not got.any()
    fresh.push_host(0, [7])
    assert fresh.resolve(0, [5000])[0][0] == 7 and fresh.resolve(0, [4999])[1][0]


def test_capacity_is_rounded_up_to_a_power_of_two(lib):
    assert [stamps.round_capacity(c) for c in (1, 2, 3, 1000, 1024, 1025, 1 << 31)] == [1, 2, 4, 1024, 1024, 2048, 1 << 31]
    assert stamps.round_capacity(0) == 0 and stamps.round_capacity(-4) == 0 and stamps.round_capacity((1 << 31) + 1) == 0


def test_push_with_repeat_is_push_of_the_expanded_array(lib):
    rng = np.random.default_rng(5)
    for repeat in (3, 16):
        st = sc.jittered(rng, 2 * 20).reshape(2, 20)
        a, b = stamps.HostFiringStamps(2, 512), stamps.HostFiringStamps(2, 512)
        a.push(st, repeat)
        for s in range(2):
            b.push_host(s, np.repeat(st[s], repeat))
        assert sc.same(a.rings, b.rings) and sc.same(a.heads, b.heads) and a.counters(1)[0] == 20 * repeat
    with pytest.raises(EngineError) as e:
        a.push(np.zeros((2, 40), dtype=np.uint64), 16)                           # 640 > 512
    assert e.value.code == capi.CC_ERR_INVALID_ARGUMENT and "cc_stamps_host_push" in str(e.value)


def test_cluster_rule_at_the_edges_of_uint64(logs):
    """stamps above 2^63, differing only in the high or only in the low word, an odd max - min, and max = 2^64 - 1 where (min + max) / 2
    overflows; a zero among the members is not skipped"""
    twin, model = logs
    cl, rec = sc.cluster_case()
    for last in (True, False):
        mid, got_points = twin.of_clusters(cl, rec, last)
        ref, ref_points = sc.model_of_clusters(model, cl, rec, last)
        assert sc.same(mid, ref) and sc.same(got_points, ref_points), last
    sp = mid[len(sc.CLUSTER_SIZES):]
    assert (sp["min_stamp"][0], sp["max_stamp"][0], sp["stamp"][0]) == ((1 << 63) + 10, (1 << 63) + 13, (1 << 63) + 11)   # odd: rounds down
    assert (sp["min_stamp"][1], sp["max_stamp"][1], sp["stamp"][1]) == ((5 << 32) | 7, (9 << 32) | 7, (7 << 32) | 7)
    assert (sp["min_stamp"][2], sp["max_stamp"][2]) == ((5 << 32) | 7, (5 << 32) | 1000)
    assert (sp["min_stamp"][3], sp["max_stamp"][3], sp["stamp"][3]) == (1, M64, 1 << 63) and (1 + M64) // 2 != ((1 + M64) & M64) // 2
    assert sp["min_stamp"][4] == 0 and sp["max_stamp"][4] >= sc.EARLIEST and sp["n_missing"][4] == 0       # the firing STAMPED 0 is held
    assert (sp["min_stamp"][5], sp["max_stamp"][5], sp["stamp"][5]) == (M64, M64, M64)
    assert (mid["n_missing"][:5] > 0).any() and mid["n_missing"][0] == 0
    assert [twin.counters(s)[1] for s in range(sc.S)] == [model.counters(s)[1] for s in range(sc.S)]
    assert twin.counters(0)[1] > 0 and twin.counters(2)[1] > 0 and twin.counters(4)[1] == 0


def test_point_and_column_rules(logs):
    """a column with no record, with only zeros, with zeros mixed with stamps; streams with empty slices between the others"""
    twin, model = logs
    rec, table = sc.point_case()
    got, got_sn = twin.of_points(rec, table)
    ref, ref_sn = sc.model_of_points(model, rec, table)
    assert sc.same(got, ref) and sc.same(got_sn, ref_sn)
    cols, streams = twin.of_columns(rec, table)
    ref_cols, ref_streams = sc.model_of_columns(model, rec, table)
    assert sc.same(cols, ref_cols) and sc.same(streams, ref_streams)
    assert len(cols) == 26 and streams[1] == 0 and streams[3] == 0 and not cols[17:21].any()
    last = cols[21:]                                                             # stream 4
    assert last[0] >= sc.EARLIEST and last[1] == 0 and last[2] >= sc.EARLIEST and last[3] == 0 and last[4] == 1
    assert cols[3] == 0 and cols[4] != 0                                         # stream 0, the column without a record
    assert streams[4] == 1 and streams[0] == min(int(v) for v in got[:300] if v)
    assert [twin.counters(s)[1] for s in range(sc.S)] == [model.counters(s)[1] for s in range(sc.S)]


def test_sec_nsec_split(lib):
    values = [0, 1, 999_999_999, 10 ** 9, sc.BASE + 123_456_789, ((1 << 32) - 1) * 10 ** 9 + 999_999_999, (1 << 32) * 10 ** 9, M64]
    got = stamps.host_sec_nsec(values)
    assert [tuple(int(x) for x in row) for row in got] == [sc.sec_nsec(v) for v in values]
    assert tuple(got[4]) == (1_700_000_000, 123_456_789) and tuple(got[6]) == (0, 0) and got[7][0] == (M64 // 10 ** 9) & sc.M32


def test_struct_sizes_match_the_header(lib):
    txt = open(os.path.join(ROOT, "include", "cc_stamps.h")).read()
    assert ctypes.sizeof(stamps.ClusterStamp) == stamps.CLUSTER_STAMP_DTYPE.itemsize == 32 and "/* 32 bytes" in txt
    body = re.search(r"typedef struct cc_cluster_stamp \{(.*?)\} cc_cluster_stamp;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [f for f, _ in stamps.ClusterStamp._fields_] == list(stamps.CLUSTER_STAMP_DTYPE.names)
    assert [stamps.CLUSTER_STAMP_DTYPE.fields[n][1] for n in names] == [getattr(stamps.ClusterStamp, n).offset for n in names] == [0, 8, 16, 24, 28]
    assert ctypes.sizeof(stamps.HostLog) == 48


def test_header_symbols_are_exported_and_bad_arguments_are_refused_before_the_device_is_looked_for(lib):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cc_stamps.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(cc_[a-z_0-9]+)\s*\(", txt)))
    assert len(names) == 21 and "cc_firing_stamps_of_clusters" in names, names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/cc_stamps.h but not exported by libcc_hip.so"
    hip = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cc_hip.h")).read(), flags=re.S)
    assert "cc_firing_stamps" not in hip and "cc_stamps_" not in hip                # the side-car keeps out of the engine's header
    bad, h = capi.CC_ERR_INVALID_ARGUMENT, ctypes.c_void_p()
    assert lib.cc_firing_stamps_create(None, 0, 1, 64, None) == bad and b"cc_firing_stamps_create" in lib.cc_firing_stamps_last_error()
    for S, cap in ((0, 64), (65536, 64), (1, 0), (1, (1 << 31) + 1)):
        assert lib.cc_firing_stamps_create(ctypes.byref(h), 0, S, cap, None) == bad and b"cc_firing_stamps_create" in lib.cc_firing_stamps_last_error()
    for name, call in (("cc_firing_stamps_sync", lambda: lib.cc_firing_stamps_sync(None)),
                       ("cc_firing_stamps_push", lambda: lib.cc_firing_stamps_push(None, 1, None, 1)),
                       ("cc_firing_stamps_push_host", lambda: lib.cc_firing_stamps_push_host(None, 0, 1, None)),
                       ("cc_firing_stamps_seek", lambda: lib.cc_firing_stamps_seek(None, 0, 0)),
                       ("cc_firing_stamps_reset_streams", lambda: lib.cc_firing_stamps_reset_streams(None, 0, None)),
                       ("cc_firing_stamps_counters", lambda: lib.cc_firing_stamps_counters(None, 0, None, None)),
                       ("cc_firing_stamps_of_points", lambda: lib.cc_firing_stamps_of_points(None, 0, None, None, None, None)),
                       ("cc_firing_stamps_of_columns", lambda: lib.cc_firing_stamps_of_columns(None, 0, None, None, None, None, None)),
                       ("cc_firing_stamps_of_clusters", lambda: lib.cc_firing_stamps_of_clusters(None, 0, 0, None, 0, None, None, None))):
        assert call() == bad and name.encode() in lib.cc_firing_stamps_last_error(), name
    assert lib.cc_firing_stamps_hip_stream(None) is None and lib.cc_firing_stamps_capacity(None) == 0
    lib.cc_firing_stamps_destroy(None)
    import torch
    if not torch.cuda.is_available():
        assert lib.cc_firing_stamps_create(ctypes.byref(h), 0, 1, 64, None) == capi.CC_ERR_NO_DEVICE
        assert b"no gfx950 device" in lib.cc_firing_stamps_last_error()


def test_host_twins_refuse_what_the_device_calls_refuse(lib):
    twin = stamps.HostFiringStamps(2, 16)
    rec, cl = np.zeros(3, dtype=take.TAKE_POINT_DTYPE), np.zeros(1, dtype=take.TAKE_CLUSTER_DTYPE)
    log = ctypes.byref(twin._log)
    out = np.zeros(1, dtype=stamps.CLUSTER_STAMP_DTYPE)
    bad = capi.CC_ERR_INVALID_ARGUMENT
    assert lib.cc_stamps_host_of_clusters(log, 0, 1, cl.ctypes.data, 3, None, out.ctypes.data, None) == bad
    assert b"stamps need the records" in lib.cc_firing_stamps_last_error()
    assert lib.cc_stamps_host_of_points(log, 3, rec.ctypes.data, None, out.ctypes.data, None) == bad
    assert lib.cc_stamps_host_resolve(log, 2, 0, None, None, None) == bad and b"no such stream 2" in lib.cc_firing_stamps_last_error()
    with pytest.raises(EngineError):
        twin.push_host(0, np.zeros(17, dtype=np.uint64))
    assert lib.cc_stamps_host_of_clusters(log, 0, 0, None, 0, None, None, None) == 0   # zero clusters and zero records is legal
    table = np.zeros(2, dtype=take.TAKE_STREAM_DTYPE)
    assert lib.cc_stamps_host_of_points(log, 0, None, table.ctypes.data, None, None) == 0


def test_package_reexports_the_names():
    import continuous_clustering_amd as cca
    assert cca.stamps is stamps and cca.FiringStamps is stamps.FiringStamps and cca.CLUSTER_STAMP_DTYPE is stamps.CLUSTER_STAMP_DTYPE
    assert {"stamps", "FiringStamps", "CLUSTER_STAMP_DTYPE"} <= set(cca.__all__)
