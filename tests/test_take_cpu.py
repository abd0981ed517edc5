"""CPU: the hand-over ABI (cc_engine_take_points / _take_cursor / _take_seek, include/cc_hip.h) as far as it can be checked without a device:
struct layouts in the header, in ctypes and in the numpy dtypes agree; pointcloud2_fields() tiles the 32 bytes; the three functions are
exported and refuse a NULL engine."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_TYPES = {"float": (ctypes.c_float, "<f4"), "uint32_t": (ctypes.c_uint32, "<u4"), "uint16_t": (ctypes.c_uint16, "<u2"),
           "uint8_t": (ctypes.c_uint8, "|u1"), "int64_t": (ctypes.c_int64, "<i8"), "int32_t": (ctypes.c_int32, "<i4")}


@pytest.fixture(scope="module")
def lib():
    from continuous_clustering_amd import build, load_library, take
    build.build()
    load_library()
    return take._lib()


def header_struct(name):
    """[(field, C type)] of `typedef struct name { ... } name;` in include/cc_hip.h, in declaration order."""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cc_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (name, name), txt, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    return fields


@pytest.mark.parametrize("name,size", [("cc_take_point", 32), ("cc_take_stream", 48)])
def test_struct_layouts_match_header(name, size):
    from continuous_clustering_amd import take
    cstruct, dtype = {"cc_take_point": (take.TakePoint, take.TAKE_POINT_DTYPE), "cc_take_stream": (take.TakeStream, take.TAKE_STREAM_DTYPE)}[name]
    fields = header_struct(name)
    # what a C compiler makes of the header's declarations (natural alignment), rebuilt from the parsed text
    Rebuilt = type("Rebuilt", (ctypes.Structure,), {"_fields_": [(f, C_TYPES[t][0]) for f, t in fields]})
    assert ctypes.sizeof(Rebuilt) == ctypes.sizeof(cstruct) == dtype.itemsize == size
    assert [f for f, _ in fields] == [f for f, _ in cstruct._fields_] == list(dtype.names)
    for f, t in fields:
        off = getattr(Rebuilt, f).offset
        assert getattr(cstruct, f).offset == off, f
        assert dtype.fields[f][1] == off and dtype.fields[f][0].str == C_TYPES[t][1], f
        assert getattr(cstruct, f).size == ctypes.sizeof(C_TYPES[t][0]), f


def test_package_reexports_the_take_names():
    import continuous_clustering_amd as cca
    assert cca.TAKE_POINT_DTYPE is cca.take.TAKE_POINT_DTYPE and cca.TAKE_POINT_DTYPE.itemsize == 32
    assert cca.pointcloud2_fields is cca.take.pointcloud2_fields
    for m in ("take_points", "take_cursor", "take_seek"):
        assert callable(getattr(cca.Engine, m))
    assert issubclass(cca.TakeCapacityError, cca.EngineError)


def test_pointcloud2_fields_cover_the_record_without_overlap():
    from continuous_clustering_amd import take
    size = {2: 1, 4: 2, 6: 4, 7: 4}  # sensor_msgs/PointField: UINT8, UINT16, UINT32, FLOAT32
    fields = take.pointcloud2_fields()
    assert [f[0] for f in fields] == list(take.TAKE_POINT_DTYPE.names)
    assert [f[0] for f in fields[:3]] == ["x", "y", "z"] and all(f[2] == 7 for f in fields[:4])
    used = np.zeros(32, dtype=np.int32)
    for name, off, datatype, count in fields:
        assert count == 1 and off % size[datatype] == 0, name
        used[off:off + size[datatype]] += 1
        assert take.TAKE_POINT_DTYPE.fields[name][1] == off and take.TAKE_POINT_DTYPE.fields[name][0].itemsize == size[datatype]
    assert (used == 1).all()


def test_functions_are_exported_and_refuse_a_null_engine(lib):
    from continuous_clustering_amd import capi, take
    for n in ("cc_engine_take_points", "cc_engine_take_cursor", "cc_engine_take_seek"):
        assert hasattr(lib, n), n
    table = np.zeros(1, dtype=take.TAKE_STREAM_DTYPE)
    n, a, b = ctypes.c_int64(-7), ctypes.c_int64(-7), ctypes.c_int64(-7)
    assert lib.cc_engine_take_points(None, 0, 0, None, 0, None, table.ctypes.data, ctypes.byref(n)) == capi.CC_ERR_INVALID_ARGUMENT
    assert lib.cc_engine_take_cursor(None, 0, 0, ctypes.byref(a), ctypes.byref(b)) == capi.CC_ERR_INVALID_ARGUMENT
    assert lib.cc_engine_take_seek(None, 0, -1, 0) == capi.CC_ERR_INVALID_ARGUMENT
    assert (n.value, a.value, b.value) == (-7, -7, -7)
    assert take.TAKE_CLUSTERED == 0 and take.TAKE_SEGMENTED == 1
    assert (take.TAKE_ALL_RETURNS, take.TAKE_NOT_GROUND, take.TAKE_WITH_ID) == (0, 1, 2)
