"""CPU: the replay evaluator's ABI (cc_replay_eval_*, include/cc_kitti.h) as far as it can be checked without a device: the struct layouts in
the header, in ctypes and in the numpy dtypes agree; every function is exported and refuses a NULL handle or engine; replay.replay takes the
`scatter` keyword and rejects a value it does not know."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_TYPES = {"double": (ctypes.c_double, "<f8"), "int64_t": (ctypes.c_int64, "<i8"), "int32_t": (ctypes.c_int32, "<i4")}
FUNCTIONS = ("cc_replay_eval_create", "cc_replay_eval_destroy", "cc_replay_eval_original_index", "cc_replay_eval_add_frame",
             "cc_replay_eval_set_active", "cc_replay_eval_seek", "cc_replay_eval_step", "cc_replay_eval_counters",
             "cc_replay_eval_evaluate_slots", "cc_replay_eval_slot_arrays")


@pytest.fixture(scope="module")
def lib():
    from continuous_clustering_amd import build, evaluation, load_library
    build.build()
    load_library()
    return evaluation._replay_lib()


def header_struct(header, name):
    """[(field, C type)] of `typedef struct name { ... } name;` in include/<header>, in declaration order (the parser of test_take_cpu.py)."""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s;" % (name, name), txt, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    return fields


def rebuilt(header, name):
    """what a C compiler makes of the header's declarations (natural alignment): (ctypes.Structure, flat [(path, offset, numpy str)])"""
    members, flat = [], []
    for f, t in header_struct(header, name):
        if t in C_TYPES:
            members.append((f, C_TYPES[t][0], None))
        else:  # a struct declared in cc_hip.h, by value
            inner, inner_flat = rebuilt("cc_hip.h", t)
            members.append((f, inner, inner_flat))
    cls = type("Rebuilt_" + name, (ctypes.Structure,), {"_fields_": [(f, c) for f, c, _ in members]})
    for (f, c, inner_flat), (_, t) in zip(members, header_struct(header, name)):
        off = getattr(cls, f).offset
        if inner_flat is None:
            flat.append(((f,), off, C_TYPES[t][1]))
        else:
            flat += [((f,) + path, off + o, s) for path, o, s in inner_flat]
    return cls, flat


def flat_ctypes(cls, base=0, prefix=()):
    out = []
    for f, c in cls._fields_:
        off = base + getattr(cls, f).offset
        if issubclass(c, ctypes.Structure):
            out += flat_ctypes(c, off, prefix + (f,))
        else:
            out.append((prefix + (f,), off, ctypes.sizeof(c)))
    return out


def flat_dtype(dt, base=0, prefix=()):
    out = []
    for f in dt.names:
        sub, off = dt.fields[f][0], base + dt.fields[f][1]
        if sub.names:
            out += flat_dtype(sub, off, prefix + (f,))
        else:
            out.append((prefix + (f,), off, sub.str))
    return out


@pytest.mark.parametrize("name,size", [("cc_replay_record", 56), ("cc_replay_stream", 48)])
def test_struct_layouts_match_header(name, size):
    from continuous_clustering_amd import evaluation
    cstruct, dtype = {"cc_replay_record": (evaluation.ReplayRecord, evaluation.REPLAY_RECORD_DTYPE),
                      "cc_replay_stream": (evaluation.ReplayStream, evaluation.REPLAY_STREAM_DTYPE)}[name]
    cls, flat = rebuilt("cc_kitti.h", name)
    assert ctypes.sizeof(cls) == ctypes.sizeof(cstruct) == dtype.itemsize == size
    assert [(p, o) for p, o, _ in flat] == [(p, o) for p, o, _ in flat_ctypes(cstruct)]
    assert flat == flat_dtype(dtype)
    assert [s for _, _, s in flat_ctypes(cstruct)] == [np.dtype(s).itemsize for _, _, s in flat]


def test_record_is_two_ints_and_the_frame_result():
    from continuous_clustering_amd import evaluation
    assert [f for f, _ in header_struct("cc_kitti.h", "cc_replay_record")] == ["stream", "frame", "r"]
    assert tuple(f for f, _ in header_struct("cc_hip.h", "cc_eval_frame_result")) == evaluation.RESULT_FIELDS
    assert evaluation.REPLAY_RECORD_DTYPE.fields["r"][1] == 8
    txt = open(os.path.join(ROOT, "include", "cc_kitti.h")).read()
    for n, v in (("ALREADY_EVALUATED", evaluation.REPLAY_ERR_ALREADY_EVALUATED), ("TOO_FAR_AHEAD", evaluation.REPLAY_ERR_TOO_FAR_AHEAD)):
        assert int(re.search(r"#define CC_REPLAY_ERR_%s (\d+)" % n, txt).group(1)) == v
    assert len(set(evaluation.REPLAY_ERROR_TEXT)) == 2 and all(v > 9 for v in evaluation.REPLAY_ERROR_TEXT)  # (apart from the CC_ERR_* codes)


def test_functions_are_declared_exported_and_refuse_null(lib):
    from continuous_clustering_amd import capi, evaluation
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cc_kitti.h")).read(), flags=re.S)
    for n in FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % n, txt), n
        assert hasattr(lib, n), n
    inv = capi.CC_ERR_INVALID_ARGUMENT
    h = ctypes.c_void_p(0x1234)
    assert lib.cc_replay_eval_create(ctypes.byref(h), None, 4, 1000, 2) == inv   # NULL engine
    assert lib.cc_replay_eval_create(None, None, 4, 1000, 2) == inv
    lib.cc_replay_eval_destroy(None)
    assert lib.cc_replay_eval_original_index(None, 0, 0) is None
    sem, eu = np.zeros(4, np.uint16), np.zeros(4, np.uint32)
    assert lib.cc_replay_eval_add_frame(None, 0, 0, 4, sem.ctypes.data, eu.ctypes.data) == inv
    assert lib.cc_replay_eval_set_active(None, 0, 1) == inv
    assert lib.cc_replay_eval_seek(None, 0, 0, 0) == inv
    table = np.zeros(1, dtype=evaluation.REPLAY_STREAM_DTYPE)
    rec = np.zeros(1, dtype=evaluation.REPLAY_RECORD_DTYPE)
    n = ctypes.c_int64(-7)
    assert lib.cc_replay_eval_step(None, None, rec.ctypes.data, 1, ctypes.byref(n), table.ctypes.data) == inv
    assert n.value == -7
    v = [ctypes.c_uint64(9) for _ in range(4)]
    assert lib.cc_replay_eval_counters(None, *[ctypes.byref(x) for x in v]) == inv
    assert [x.value for x in v] == [9] * 4
    fr = np.zeros(1, np.int32)
    assert lib.cc_replay_eval_evaluate_slots(None, 0, 1, fr.ctypes.data, rec.ctypes.data) == inv
    g, d = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.cc_replay_eval_slot_arrays(None, 0, 0, ctypes.byref(g), ctypes.byref(d)) == inv


def test_replay_takes_the_scatter_keyword(tmp_path):
    from continuous_clustering_amd import evaluation, replay
    p = inspect.signature(replay.replay).parameters["scatter"]
    assert p.default == "device"
    with pytest.raises(ValueError, match="scatter"):
        replay.replay(str(tmp_path), [0], scatter="host")
    # both values pass the check; with no sequence on this rank nothing else runs
    for v in ("device", "batched"):
        assert replay.replay(str(tmp_path), [], scatter=v) == ([], dict(streams=0, frames=0, cells_published=0))
    for m in ("original_index_ptr", "add_frame", "publish", "finish", "counters"):
        assert callable(getattr(evaluation.BatchedFrameScatter, m)), m
