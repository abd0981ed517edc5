"""CPU: the generic PointCloud2 decoder's host side (include/cc_points.h) and the numpy restatement the GPU tests compare against.

* every function the header declares is exported, and the device path refuses to run without a GPU;
* cc_points_layout_check accepts the layouts of the GPU tests and refuses one good layout with one field broken at a time;
* layout_from_pointcloud2 on the reference's RAW_POINT fields and on a padded xyzi cloud, and each of its refusals;
* points_ref against two hand-assembled messages with the expected outputs as literals;
* intensity mode 0 for all 256 bytes against what g++ computes for the reference's expression; modes 2 and 3 on special values;
* write_messages -> points_ref.decode is the identity, with garbage in every byte that is not a field.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import points_cases
import points_ref
from continuous_clustering_amd import EngineError, capi, points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "csrc", "points_intensity_probe.cpp")


@pytest.fixture(scope="module")
def lib():
    from continuous_clustering_amd import build, load_library
    build.build()
    load_library()
    return points._lib()


def test_header_symbols_are_exported_and_no_gpu_means_no_decoder(lib):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cc_points.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(cc_[a-z_0-9]+)\s*\(", txt)))
    assert "cc_points_decode" in names and "cc_points_layout_check" in names and len(names) == 11
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/cc_points.h but not exported by libcc_hip.so"
    assert ctypes.sizeof(points.Layout) == 56                                        # 2 x i32, 2 x i64, 6 x i32, 1 x i64
    import torch
    layout = points.raw_firing_layout(32)
    h = ctypes.c_void_p()
    rc = lib.cc_points_create(ctypes.byref(h), 0, 2, ctypes.byref(layout), 8, None)
    if torch.cuda.is_available():
        assert rc == capi.CC_OK
        lib.cc_points_destroy(h)
    else:
        assert rc == capi.CC_ERR_NO_DEVICE and not h.value
        assert b"no gfx950 device" in lib.cc_points_last_error()
    assert lib.cc_points_create(ctypes.byref(h), 0, 0, ctypes.byref(layout), 8, None) == capi.CC_ERR_INVALID_ARGUMENT
    assert lib.cc_points_create(ctypes.byref(h), 0, 2, ctypes.byref(layout), 0, None) == capi.CC_ERR_INVALID_ARGUMENT
    bad = layout.copy(rows=30)                                                       # a bad layout is refused before the device is looked for
    assert lib.cc_points_create(ctypes.byref(h), 0, 2, ctypes.byref(bad), 8, None) == capi.CC_ERR_INVALID_ARGUMENT
    assert b"rows" in lib.cc_points_last_error()


def test_layout_check_accepts_the_test_layouts_and_refuses_each_broken_field(lib):
    for name, layout in points_cases.all_layouts().items():
        assert lib.cc_points_layout_check(ctypes.byref(layout)) == capi.CC_OK, name
        assert points.kernel_path(layout) in (points.PATH_GATHER, points.PATH_ROWS, points.PATH_MESSAGES)
    assert points.kernel_path(points_cases.raw_firing()) == points.PATH_MESSAGES
    assert points.kernel_path(points_cases.raw_firing(128)) == points.PATH_MESSAGES and points.column_tile(points_cases.raw_firing(128)) == 8
    assert points.kernel_path(points_cases.column_major()) == points.PATH_GATHER
    good = points_cases.organised_row_major()[0]                                     # H 8, 22-byte points, fields at 3 / 7 / 13 / 17 (f32)
    H, C, rs, cs, mb = good.rows, good.columns, good.row_stride, good.column_stride, good.message_bytes
    assert mb == (H - 1) * rs + C * cs
    broken = [dict(rows=6), dict(rows=0), dict(rows=-4), dict(rows=132), dict(columns=0), dict(columns=-1), dict(row_stride=0),
              dict(row_stride=-rs), dict(column_stride=0), dict(column_stride=-22), dict(off_x=-1), dict(off_y=-3), dict(off_z=-4),
              dict(off_x=19), dict(off_y=20), dict(off_z=22),                        # the last point's field ends behind the message
              dict(off_intensity=-2), dict(off_intensity=19), dict(off_intensity=mb),
              dict(intensity_mode=4), dict(intensity_mode=-1), dict(message_bytes=mb - 2), dict(message_bytes=0),   # the last field byte is byte mb - 2
              dict(columns=C + 1), dict(rows=H + 4)]                                 # one more column / four more rows than the message holds
    for change in broken:
        bad = good.copy(**change)
        assert lib.cc_points_layout_check(ctypes.byref(bad)) == capi.CC_ERR_INVALID_ARGUMENT, change
        assert len(lib.cc_points_last_error()) > 10, change
        assert points.kernel_path(bad) == -1 and points.column_tile(bad) == -1
        with pytest.raises(EngineError):
            points.check_layout(bad)
    assert lib.cc_points_layout_check(ctypes.byref(good.copy(message_bytes=mb - 1))) == capi.CC_OK
    # a one-byte intensity field may end where a four-byte one may not
    assert lib.cc_points_layout_check(ctypes.byref(good.copy(off_intensity=21, intensity_mode=points.INTENSITY_U8))) == capi.CC_OK
    assert lib.cc_points_layout_check(ctypes.byref(good.copy(off_intensity=21))) == capi.CC_ERR_INVALID_ARGUMENT
    assert lib.cc_points_layout_check(ctypes.byref(good.copy(off_intensity=-1))) == capi.CC_OK
    assert lib.cc_points_layout_check(None) == capi.CC_ERR_INVALID_ARGUMENT
    # strides near 2^62 neither overflow the check nor the plan
    huge = points.Layout(rows=4, columns=2, row_stride=2 ** 61, column_stride=2 ** 60, off_x=0, off_y=4, off_z=8, off_intensity=-1,
                         intensity_mode=0, reverse_rows=0, message_bytes=2 ** 63 - 1)
    assert lib.cc_points_layout_check(ctypes.byref(huge)) == capi.CC_OK and points.kernel_path(huge) == points.PATH_ROWS
    assert points.column_tile(huge) == 1
    assert lib.cc_points_layout_check(ctypes.byref(huge.copy(row_stride=2 ** 62))) == capi.CC_ERR_INVALID_ARGUMENT


def test_layout_from_pointcloud2(lib):
    raw = points.layout_from_pointcloud2(128, 1, 37, 37, points.RAW_FIRING_FIELDS)
    assert (raw.off_x, raw.off_y, raw.off_z, raw.off_intensity) == (0, 4, 8, 20)
    assert (raw.rows, raw.columns, raw.row_stride, raw.column_stride, raw.message_bytes) == (128, 1, 37, 37, 128 * 37)
    assert raw.intensity_mode == points.INTENSITY_REFERENCE and raw.reverse_rows == 0
    assert bytes(points.raw_firing_layout(128)) == bytes(raw) and points.RAW_FIRING_POINT_STEP == 37
    end = max(off + points.DATATYPE_BYTES[dt] * cnt for _, off, dt, cnt in points.RAW_FIRING_FIELDS)
    assert end == 37 and [f[0] for f in points.RAW_FIRING_FIELDS] == ["x", "y", "z", "firing_index", "intensity",
                                                                       "globally_unique_point_index", "time_sec", "time_nsec"]
    # a padded organised cloud as the common drivers publish it: 32-byte points, rows padded to 64 bytes more
    F32, U16 = points.FLOAT32, points.UINT16
    fields = [("x", 0, F32, 1), ("y", 4, F32, 1), ("z", 8, F32, 1), ("intensity", 16, F32, 1), ("ring", 20, U16, 1), ("time", 24, F32, 1)]
    lay = points.layout_from_pointcloud2(16, 1800, 32, 1800 * 32 + 64, fields, intensity_mode=points.INTENSITY_F32_255, reverse_rows=True)
    assert lay.as_dict() == dict(rows=16, columns=1800, row_stride=57664, column_stride=32, off_x=0, off_y=4, off_z=8, off_intensity=16,
                                 intensity_mode=3, reverse_rows=1, message_bytes=15 * 57664 + 1800 * 32)
    assert points.kernel_path(lay) == points.PATH_ROWS
    no_i = points.layout_from_pointcloud2(16, 1, 32, 32, [f for f in fields if f[0] != "intensity"])
    assert no_i.off_intensity == -1
    # the reference's mode reads the first byte of any datatype
    assert points.layout_from_pointcloud2(16, 1, 32, 32, fields, intensity_mode=points.INTENSITY_REFERENCE).off_intensity == 16
    # refusals
    for missing in ("x", "y", "z"):
        with pytest.raises(ValueError, match=f"no field '{missing}'"):
            points.layout_from_pointcloud2(16, 1, 32, 32, [f for f in fields if f[0] != missing])
    with pytest.raises(ValueError, match="big-endian"):
        points.layout_from_pointcloud2(16, 1, 32, 32, fields, is_bigendian=True)
    for name in ("x", "y", "z"):
        wrong = [(n, o, points.FLOAT64 if n == name else dt, c) for n, o, dt, c in fields]
        with pytest.raises(ValueError, match="not FLOAT32"):
            points.layout_from_pointcloud2(16, 1, 32, 32, wrong)
    u8 = [(n, o, points.UINT8 if n == "intensity" else dt, c) for n, o, dt, c in fields]
    with pytest.raises(ValueError, match="intensity"):
        points.layout_from_pointcloud2(16, 1, 32, 32, fields, intensity_mode=points.INTENSITY_U8)         # FLOAT32 field, byte mode
    with pytest.raises(ValueError, match="intensity"):
        points.layout_from_pointcloud2(16, 1, 32, 32, u8, intensity_mode=points.INTENSITY_F32_UNIT)
    with pytest.raises(ValueError, match="intensity"):
        points.layout_from_pointcloud2(16, 1, 32, 32, [(n, o, U16 if n == "intensity" else dt, c) for n, o, dt, c in fields],
                                       intensity_mode=points.INTENSITY_F32_255)
    assert points.layout_from_pointcloud2(16, 1, 32, 32, u8, intensity_mode=points.INTENSITY_U8).intensity_mode == 1
    with pytest.raises(ValueError):
        points.layout_from_pointcloud2(16, 1, 32, 32, fields, intensity_mode=7)
    with pytest.raises(ValueError, match="rows"):
        points.layout_from_pointcloud2(18, 1, 32, 32, fields)                                             # rows not a multiple of 4
    with pytest.raises(ValueError):
        points.layout_from_pointcloud2(16, 4, 32, 100, fields)                                            # row_step below width * point_step
    with pytest.raises(ValueError, match="point_step"):
        points.layout_from_pointcloud2(16, 1, 16, 16, fields)                                             # intensity behind the point


# two messages of four 14-byte points: filler byte, x @1, y @5, z @9 (little-endian f32), intensity byte @13
MESSAGE_0 = [0xAA, 0x00, 0x00, 0x80, 0x3F, 0x00, 0x00, 0x00, 0xC0, 0x00, 0x00, 0x00, 0x3F, 0x01,   # 1.0, -2.0, 0.5; 1
             0xBB, 0x01, 0x00, 0xC0, 0x7F, 0x00, 0x00, 0x00, 0x80, 0x00, 0x00, 0x80, 0x7F, 0x00,   # NaN with payload 1, -0.0, +inf; 0
             0xCC, 0x01, 0x00, 0x00, 0x00, 0x78, 0x56, 0x34, 0x12, 0xFF, 0xFF, 0x7F, 0x7F, 0xFF,   # smallest denormal, 0x12345678, FLT_MAX; 255
             0xDD, 0x00, 0x00, 0x20, 0x41, 0x00, 0x00, 0xA0, 0xC1, 0xDB, 0x0F, 0x49, 0x40, 0x80]   # 10.0, -20.0, pi; 128
MESSAGE_1 = [0x11, 0x00, 0x00, 0x00, 0x40, 0x00, 0x00, 0x40, 0x40, 0x00, 0x00, 0x80, 0x40, 0x02,   # 2.0, 3.0, 4.0; 2
             0x22, 0xFF, 0xFF, 0xFF, 0xFF, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x80, 0xBF, 0x03,   # all-ones NaN, 0.0, -1.0; 3
             0x33, 0x00, 0x00, 0x80, 0xFF, 0x00, 0x00, 0xC8, 0x42, 0x00, 0x00, 0x7A, 0x44, 0x7F,   # -inf, 100.0, 1000.0; 127
             0x44, 0xCD, 0xCC, 0xCC, 0x3D, 0xCD, 0xCC, 0x4C, 0x3E, 0x9A, 0x99, 0x99, 0x3E, 0x64]   # 0.1f, 0.2f, 0.3f; 100
XYZ_0 = [[0x3F800000, 0xC0000000, 0x3F000000], [0x7FC00001, 0x80000000, 0x7F800000], [0x00000001, 0x12345678, 0x7F7FFFFF],
         [0x41200000, 0xC1A00000, 0x40490FDB]]
XYZ_1 = [[0x40000000, 0x40400000, 0x40800000], [0xFFFFFFFF, 0x00000000, 0xBF800000], [0xFF800000, 0x42C80000, 0x447A0000],
         [0x3DCCCCCD, 0x3E4CCCCD, 0x3E99999A]]
BYTES_0, BYTES_1 = [0x01, 0x00, 0xFF, 0x80], [0x02, 0x03, 0x7F, 0x64]
REFERENCE_0, REFERENCE_1 = [255, 0, 1, 128], [254, 253, 129, 156]                   # (b * 255) & 0xFF
QNAN = 0x7FC00000


def test_points_ref_against_hand_assembled_bytes():
    msg = np.array([MESSAGE_0 + [0xEE, 0xEE], MESSAGE_1 + [0x77, 0x77]], dtype=np.uint8)       # stride 58: two bytes behind each message
    lay = dict(rows=4, columns=1, row_stride=14, column_stride=14, off_x=1, off_y=5, off_z=9, off_intensity=13, intensity_mode=0,
               reverse_rows=0, message_bytes=56)
    poses = np.arange(24, dtype=np.float64).reshape(2, 12)
    out = points_ref.decode(msg, lay, message_poses=poses)
    assert out["xyz"].dtype == np.uint32 and out["xyz"].tolist() == [XYZ_0, XYZ_1]
    assert out["intensity"].dtype == np.uint8 and out["intensity"].tolist() == [REFERENCE_0, REFERENCE_1]
    assert np.array_equal(out["poses"], poses) and int(out["skipped_messages"]) == 0 and int(out["no_return_points"]) == 2
    assert out["xyz"].view(np.float32)[0, 0].tolist() == [1.0, -2.0, 0.5] and np.signbit(out["xyz"].view(np.float32)[0, 1, 1])
    # the byte verbatim, rows reversed, the second message skipped
    out = points_ref.decode(msg, dict(lay, intensity_mode=1, reverse_rows=1), skip=[False, True], message_poses=poses)
    assert out["xyz"].tolist() == [XYZ_0[::-1], [[QNAN] * 3] * 4]
    assert out["intensity"].tolist() == [BYTES_0[::-1], [0, 0, 0, 0]]
    assert np.array_equal(out["poses"], poses) and int(out["skipped_messages"]) == 1 and int(out["no_return_points"]) == 1
    # no intensity field
    assert points_ref.decode(msg, dict(lay, off_intensity=-1))["intensity"].tolist() == [[0] * 4] * 2
    # the same bytes as one organised message of 2 columns x 4 rows, column-major (column stride 58, row stride 14): column c is firing c
    org = dict(lay, columns=2, column_stride=58, message_bytes=58 + 56, intensity_mode=1)
    out = points_ref.decode(msg.reshape(1, 116), org, message_poses=poses[:1])
    assert out["xyz"].tolist() == [XYZ_0, XYZ_1] and out["intensity"].tolist() == [BYTES_0, BYTES_1]
    assert np.array_equal(out["poses"], poses[[0, 0]])                               # the message's pose for both firings
    # and as one row-major message of 4 columns x 2 rows (row stride 58, column stride 14): firing c holds point c of both halves
    org = dict(lay, rows=2, columns=4, row_stride=58, column_stride=14, message_bytes=58 + 56, intensity_mode=1)
    out = points_ref.decode(msg.reshape(1, 116), org)
    assert out["xyz"].tolist() == [[XYZ_0[c], XYZ_1[c]] for c in range(4)]
    assert out["intensity"].tolist() == [[BYTES_0[c], BYTES_1[c]] for c in range(4)]


def test_reference_intensity_equals_what_gxx_computes(tmp_path):
    exe = str(tmp_path / "points_intensity_probe")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-o", exe, PROBE], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    rows = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert [b for b, _ in rows] == list(range(256))
    got = points_ref.reference_intensity(np.arange(256))
    assert got.tolist() == [v for _, v in rows]
    assert got[[0, 1, 2, 127, 128, 255]].tolist() == [0, 255, 254, 129, 128, 1]
    # through the decode, and what the writer stores for a wanted value is its inverse
    lay = points.raw_firing_layout(256 // 2)
    want = np.arange(256, dtype=np.uint8).reshape(2, 128)
    msg = points.write_messages(np.zeros((2, 128, 3), dtype=np.float32), want, lay)
    assert np.array_equal(msg.reshape(2, 128, 37)[:, :, 20], (256 - want.astype(np.int64)) & 0xFF)
    assert np.array_equal(points_ref.decode(msg, lay)["intensity"], want)


SPECIAL = [np.nan, np.inf, -np.inf, -0.5, -3.0, 0.0, 0.999, 1.0, 1.004, 1e20, 255.9, 0.5]
UNIT_WANT = [0, 0, 0, 129, 3, 0, 254, 255, 0, 0, 230, 127]      # trunc(v * 255) as int32, low byte: -127 -> 129, -765 -> 3, 256 -> 0, 65254 -> 230
SCALE_WANT = [0, 255, 0, 0, 0, 0, 0, 1, 1, 255, 255, 0]         # clamped to [0, 255], truncated


def test_float_intensity_modes_on_special_values():
    bits = np.array(SPECIAL, dtype=np.float32).view(np.uint32)
    assert points_ref.unit_intensity(bits).tolist() == UNIT_WANT
    assert points_ref.scale255_intensity(bits).tolist() == SCALE_WANT
    assert points_ref.unit_intensity(np.array([0xFFC00001, 0x7F800001], dtype=np.uint32)).tolist() == [0, 0]     # other NaNs
    assert points_ref.scale255_intensity(np.array([0xFFC00001, 0x7F800001], dtype=np.uint32)).tolist() == [0, 0]
    # beyond the int32 range: 0; inside it the low byte of the integer, 255000 = 996 * 256 + 24
    assert points_ref.unit_intensity(np.array([-8.5e6, 8.5e6, 1000.0], dtype=np.float32).view(np.uint32)).tolist() == [0, 0, 24]
    # through write_messages (a float intensity array is written verbatim) and the decode
    xyz = np.zeros((1, 12, 3), dtype=np.float32)
    for mode, want in ((points.INTENSITY_F32_UNIT, UNIT_WANT), (points.INTENSITY_F32_255, SCALE_WANT)):
        lay = points.layout_from_pointcloud2(12, 1, 16, 16, points_cases.XYZI_FIELDS, intensity_mode=mode)
        msg = points.write_messages(xyz, np.array(SPECIAL, dtype=np.float32).reshape(1, 12), lay, fill=0x5A)
        assert points_ref.decode(msg, lay)["intensity"].tolist() == [want]
        # uint8 values survive the writer's float encoding in both modes
        every = np.resize(np.arange(256, dtype=np.uint8), (22, 12))
        msg = points.write_messages(np.zeros((22, 12, 3), dtype=np.float32), every, lay)
        assert np.array_equal(points_ref.decode(msg, lay)["intensity"], every)


def test_write_messages_then_numpy_decode_is_the_identity(lib):
    rng = np.random.default_rng(14)
    for name, layout in points_cases.all_layouts().items():
        for stride in (layout.message_bytes, layout.message_bytes + 1, (layout.message_bytes + 15) // 16 * 16 + 16):
            xyz, inten = points_cases.random_firings(rng, (2, 3), layout)
            msg = points.write_messages(xyz, inten, layout, stride=stride, fill=rng)
            assert msg.shape == (2, 3, stride) and msg.dtype == np.uint8
            out = points_ref.decode(msg, layout)
            assert np.array_equal(out["xyz"], xyz), (name, stride)
            assert np.array_equal(out["intensity"], inten if layout.off_intensity >= 0 else np.zeros_like(inten)), (name, stride)
            # the filler is filler: other garbage, same fields, same decode
            other = points.write_messages(xyz.view(np.float32), inten, layout, stride=stride, fill=0xC3)
            field_bytes = layout.rows * layout.columns * (12 + (0 if layout.off_intensity < 0 else 4 if layout.intensity_mode >= 2 else 1))
            assert np.array_equal(other, msg) == (field_bytes == stride), (name, stride)   # equal only where no byte is filler
            again = points_ref.decode(other, layout)
            assert np.array_equal(again["xyz"], xyz) and np.array_equal(again["intensity"], out["intensity"]), (name, stride)
    with pytest.raises(ValueError):
        points.write_messages(np.zeros((3, 32, 3), dtype=np.float32), np.zeros((3, 32), dtype=np.uint8), points_cases.raw_firing(),
                              stride=32 * 37 - 1)
    with pytest.raises(ValueError):                                                  # 7 firings into messages of tile + 6 columns
        points.write_messages(np.zeros((7, 8, 3), dtype=np.float32), np.zeros((7, 8), dtype=np.uint8), points_cases.organised_row_major()[0])
