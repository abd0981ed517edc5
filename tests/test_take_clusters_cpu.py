"""CPU: the cluster hand-over ABI (cc_engine_take_clusters / _take_clusters_cursor, include/cc_hip.h) as far as it can be checked without a
device: struct layouts in the header, in ctypes and in the numpy dtypes agree; both functions are exported and refuse a NULL engine; the
package re-exports the names."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_TYPES = {"float": (ctypes.c_float, "<f4"), "uint32_t": (ctypes.c_uint32, "<u4"), "uint16_t": (ctypes.c_uint16, "<u2"),
           "uint8_t": (ctypes.c_uint8, "|u1"), "int64_t": (ctypes.c_int64, "<i8"), "int32_t": (ctypes.c_int32, "<i4")}

CLUSTER_FIELDS = ["stream", "id", "col_from", "first_record", "n_points", "n_columns", "firing_min", "firing_max", "min_x", "min_y", "min_z",
                  "max_x", "max_y", "max_z"]
STREAM_FIELDS = ["id_from", "id_to", "lost_columns", "first_record", "n_records", "first_cluster", "n_clusters", "error", "pad"]


@pytest.fixture(scope="module")
def lib():
    from continuous_clustering_amd import build, load_library, take
    build.build()
    load_library()
    return take._lib()


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cc_hip.h")).read(), flags=re.S)


def header_struct(name):
    """[(field, C type)] of `typedef struct name { ... } name;` in include/cc_hip.h, in declaration order."""
    body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (name, name), header_text(), flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    return fields


@pytest.mark.parametrize("name,size,order", [("cc_take_cluster", 64, CLUSTER_FIELDS), ("cc_take_cluster_stream", 56, STREAM_FIELDS)])
def test_struct_layouts_match_header(name, size, order):
    from continuous_clustering_amd import take
    cstruct, dtype = {"cc_take_cluster": (take.TakeCluster, take.TAKE_CLUSTER_DTYPE),
                      "cc_take_cluster_stream": (take.TakeClusterStream, take.TAKE_CLUSTER_STREAM_DTYPE)}[name]
    fields = header_struct(name)
    # what a C compiler makes of the header's declarations (natural alignment), rebuilt from the parsed text
    Rebuilt = type("Rebuilt", (ctypes.Structure,), {"_fields_": [(f, C_TYPES[t][0]) for f, t in fields]})
    assert ctypes.sizeof(Rebuilt) == ctypes.sizeof(cstruct) == dtype.itemsize == size
    assert [f for f, _ in fields] == [f for f, _ in cstruct._fields_] == list(dtype.names) == order
    end = 0
    for f, t in fields:
        off = getattr(Rebuilt, f).offset
        assert off == end, f                                              # no padding anywhere: the kernel stores whole 16-byte quarters
        end = off + ctypes.sizeof(C_TYPES[t][0])
        assert getattr(cstruct, f).offset == off, f
        assert dtype.fields[f][1] == off and dtype.fields[f][0].str == C_TYPES[t][1], f
        assert getattr(cstruct, f).size == ctypes.sizeof(C_TYPES[t][0]), f
    assert end == size


def test_header_declares_the_flags_and_both_functions():
    txt = header_text()
    assert re.search(r"CC_TAKE_CLUSTERS_WITH_POINTS\s*=\s*0\s*,\s*CC_TAKE_CLUSTERS_DESCRIPTORS_ONLY\s*=\s*1", txt)
    assert re.search(r"int\s+cc_engine_take_clusters\s*\(\s*cc_engine\s*\*\s*e\s*,\s*uint32_t\s+min_points\s*,\s*int\s+flags", txt)
    assert re.search(r"int\s+cc_engine_take_clusters_cursor\s*\(\s*cc_engine\s*\*\s*e\s*,\s*int\s+stream\s*,\s*int64_t\s*\*\s*next_id", txt)


def test_package_reexports_the_cluster_take_names():
    import continuous_clustering_amd as cca
    assert cca.TAKE_CLUSTER_DTYPE is cca.take.TAKE_CLUSTER_DTYPE and cca.TAKE_CLUSTER_DTYPE.itemsize == 64
    assert cca.TAKE_CLUSTER_STREAM_DTYPE is cca.take.TAKE_CLUSTER_STREAM_DTYPE and cca.TAKE_CLUSTER_STREAM_DTYPE.itemsize == 56
    for name in ("TAKE_CLUSTER_DTYPE", "TAKE_CLUSTER_STREAM_DTYPE"):
        assert name in cca.__all__
    for m in ("take_clusters", "take_clusters_size", "take_clusters_cursor"):
        assert callable(getattr(cca.Engine, m)) and getattr(cca.Engine, m) is getattr(cca.take, m)
    err = cca.TakeCapacityError("x", 5, np.zeros(1, dtype=cca.TAKE_CLUSTER_STREAM_DTYPE), needed_clusters=3)
    assert (err.needed, err.needed_clusters, err.code) == (5, 3, cca.capi.CC_ERR_CAPACITY)
    assert cca.TakeCapacityError("x", 5, None).needed_clusters == 0      # (a point take has no descriptors)
    assert (cca.take.TAKE_CLUSTERS_WITH_POINTS, cca.take.TAKE_CLUSTERS_DESCRIPTORS_ONLY) == (0, 1)


def test_functions_are_exported_and_refuse_a_null_engine(lib):
    from continuous_clustering_amd import capi, take
    for n in ("cc_engine_take_clusters", "cc_engine_take_clusters_cursor"):
        assert hasattr(lib, n), n
    table = np.full(1, -7, dtype=np.int64).repeat(7).view(take.TAKE_CLUSTER_STREAM_DTYPE)
    before = table.tobytes()
    n, m, a, b, c = (ctypes.c_int64(-7) for _ in range(5))
    assert lib.cc_engine_take_clusters(None, 21, 0, None, 0, None, 0, None, table.ctypes.data, ctypes.byref(n),
                                       ctypes.byref(m)) == capi.CC_ERR_INVALID_ARGUMENT
    assert lib.cc_engine_take_clusters_cursor(None, 0, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == capi.CC_ERR_INVALID_ARGUMENT
    assert (n.value, m.value, a.value, b.value, c.value) == (-7,) * 5 and table.tobytes() == before
