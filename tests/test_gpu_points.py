"""GPU: the generic PointCloud2 decoder (include/cc_points.h) — bit-equal to the numpy restatement of its specification
(tests/points_ref.py) for every path of the kernel, at every alignment of the message bytes, with garbage in every byte that is not a
field, and refusing what it cannot run."""
import numpy as np
import pytest

import points_cases
import points_ref
from continuous_clustering_amd import capi, points

pytestmark = pytest.mark.gpu

CANARY_F32, CANARY_U8, SENTINEL_POSE = 12345.5, 0xA5, -77.25


def _outputs(dev, S, n, H):
    """Output arrays one firing larger than the call writes, filled with canaries."""
    import torch
    return dict(xyz=torch.full((S * n + 1, H, 3), CANARY_F32, dtype=torch.float32, device=dev),
                intensity=torch.full((S * n + 1, H), CANARY_U8, dtype=torch.uint8, device=dev),
                poses=torch.full((S * n + 1, 12), SENTINEL_POSE, dtype=torch.float64, device=dev))


def _decode_and_compare(dec, layout, msg, base, skip=None, poses=None, tag=None):
    """msg uint8 [S][M][stride] is put at byte `base` of a device buffer that ends with its last byte, decoded, and compared bit for bit
    with the numpy decode; the canary firing behind the outputs must be intact. Returns the reference."""
    import torch
    dev = torch.device("cuda")
    S, M, stride = msg.shape
    H, n = layout.rows, M * layout.columns
    buf = torch.empty(base + msg.size, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    buf[:base] = 0xEE
    buf[base:] = torch.from_numpy(msg.reshape(-1)).to(dev)
    d_skip = None if skip is None else torch.from_numpy(skip.astype(np.uint8)).to(dev)
    d_poses = None if poses is None else torch.from_numpy(poses).to(dev)
    out = _outputs(dev, S, n, H)
    torch.cuda.synchronize()
    rc = dec.decode_raw(M, buf[base:], stride, d_poses, d_skip, out["xyz"], out["intensity"], out["poses"])
    assert rc == capi.CC_OK, points._lib().cc_points_last_error()
    dec.sync()
    ref = points_ref.decode(msg, layout, skip=skip, message_poses=poses)
    got_xyz = out["xyz"].cpu().numpy().view(np.uint32)
    got_i, got_p = out["intensity"].cpu().numpy(), out["poses"].cpu().numpy()
    bad = np.argwhere(got_xyz[:-1].reshape(S, n, H, 3) != ref["xyz"])
    assert bad.size == 0, f"{tag}: {len(bad)} xyz words differ, first (stream, firing, row, axis) {bad[0]}"
    assert np.array_equal(got_i[:-1].reshape(S, n, H), ref["intensity"]), tag
    if poses is None:
        assert (got_p == SENTINEL_POSE).all(), tag                                   # the caller's poses stay
    else:
        assert np.array_equal(got_p[:-1].reshape(S, n, 12).view(np.uint64), ref["poses"].view(np.uint64)), tag
    assert (got_xyz[-1] == np.float32(CANARY_F32).view(np.uint32)).all() and (got_i[-1] == CANARY_U8).all(), tag
    assert (got_p[-1] == SENTINEL_POSE).all(), tag
    return ref


def _messages(layout, S, M, stride, seed):
    rng = np.random.default_rng(seed)
    xyz, inten = points_cases.random_firings(rng, (S, M), layout)
    return points.write_messages(xyz, inten, layout, stride=stride, fill=rng), xyz, inten


@pytest.mark.parametrize("mode", [points.INTENSITY_REFERENCE, points.INTENSITY_U8], ids=["reference", "u8"])
def test_raw_firing_message_at_every_alignment(mode):
    """The reference's own firing message (37-byte points): base at byte 0, 1, 2, 3 of a 16-byte-aligned buffer, strides H * 37, odd,
    a multiple of 4 and a multiple of 16 — every alignment of the first and the last staged word, with the array ending at the
    buffer's last byte."""
    S, M = 3, 9
    layout = points_cases.raw_firing(32, mode)
    assert points.kernel_path(layout) == points.PATH_MESSAGES and layout.message_bytes == 32 * 37
    dec = points.PointsDecoder(S, layout, max_messages=M)
    skip = np.zeros((S, M), dtype=bool)
    skip[0, 4] = skip[2, 0] = skip[2, 8] = True
    poses = np.random.default_rng(5).normal(size=(S, M, 12))
    seen = set()
    for stride in (32 * 37, 32 * 37 + 1, 32 * 37 + 4, 32 * 37 + 16):
        assert (stride % 2, stride % 4 == 0, stride % 16 == 0) in ((0, True, True), (1, False, False), (0, True, False))
        msg, _, inten = _messages(layout, S, M, stride, stride)
        seen |= set(np.unique(inten).tolist())
        for base in (0, 1, 2, 3):
            ref = _decode_and_compare(dec, layout, msg, base, skip=skip, poses=poses, tag=(stride, base))
            assert np.isnan(ref["xyz"].view(np.float32)[0, 4]).all() and ref["no_return_points"].min() > 0
    assert len(seen) == 256                                                          # all 256 intensity bytes went through
    dec.close()


def test_raw_firing_message_128_rows_more_than_one_workgroup():
    """128 rows: 8 messages per workgroup, so 9 messages are two workgroups, the second with one message; no poses, no skip."""
    layout = points_cases.raw_firing(128)
    assert points.column_tile(layout) == 8
    dec = points.PointsDecoder(2, layout, max_messages=9)
    for base, stride in ((0, 128 * 37), (3, 128 * 37 + 5)):
        msg, _, _ = _messages(layout, 2, 9, stride, 40 + base)
        _decode_and_compare(dec, layout, msg, base, tag=(stride, base))
    dec.close()


def test_aligned_xyzi_unit_intensity():
    """16-byte points at a 16-byte-aligned base: float intensities in [0, 1] and, verbatim, the special values."""
    layout = points_cases.aligned_xyzi(64)
    S, M = 2, 5
    rng = np.random.default_rng(8)
    xyz, _ = points_cases.random_firings(rng, (S, M), layout)
    special = np.array([np.nan, np.inf, -np.inf, -0.5, -3.0, 0.0, 0.999, 1.0, 1.004, 1e20, 255.9, 0.5, -8.5e6, 1000.0], dtype=np.float32)
    inten = rng.uniform(0, 1, (S, M, 64)).astype(np.float32)
    inten[:, :, :special.size] = special
    msg = points.write_messages(xyz, inten, layout, fill=rng)
    dec = points.PointsDecoder(S, layout, max_messages=M)
    ref = _decode_and_compare(dec, layout, msg, 0, poses=rng.normal(size=(S, M, 12)))
    assert ref["intensity"][0, 0, :special.size].tolist() == [0, 0, 0, 129, 3, 0, 254, 255, 0, 0, 230, 127, 0, 24]
    _decode_and_compare(dec, layout, msg, 5)                                         # the same bytes off the alignment
    dec.close()


def test_organised_row_major_cloud():
    """H = 8, 22-byte points with every field at an odd offset, rows padded by 3 bytes, tile + 6 columns (two column tiles, the last
    partial), rows reversed, intensity on a 0..255 scale; skipped messages first, last and a whole skipped stream."""
    layout, tile = points_cases.organised_row_major(8)
    assert layout.columns == tile + 6 and layout.row_stride == layout.columns * 22 + 3 and layout.reverse_rows == 1
    S, M = 3, 4
    rng = np.random.default_rng(9)
    xyz, _ = points_cases.random_firings(rng, (S, M), layout)
    inten = rng.uniform(-20, 300, (S, M * layout.columns, 8)).astype(np.float32)
    inten[0, :14, 0] = [np.nan, np.inf, -np.inf, -0.5, -3.0, 0.0, 0.999, 1.0, 1.004, 1e20, 255.9, 0.5, 255.0, 254.999]
    skip = np.zeros((S, M), dtype=bool)
    skip[0, 0] = skip[0, M - 1] = True
    skip[1, :] = True
    poses = rng.normal(size=(S, M, 12))
    dec = points.PointsDecoder(S, layout, max_messages=M)
    for base, extra in ((0, 0), (1, 0), (2, 7), (0, 16 - layout.message_bytes % 16)):
        msg = points.write_messages(xyz, inten, layout, stride=layout.message_bytes + extra, fill=rng)
        ref = _decode_and_compare(dec, layout, msg, base, skip=skip, poses=poses, tag=(base, extra))
        assert ref["skipped_messages"].tolist() == [2, M, 0]
    assert (ref["poses"][2, :layout.columns] == poses[2, 0]).all() and (ref["poses"][2, layout.columns] == poses[2, 1]).all()
    c = dec.counters()
    assert [x["skipped_messages"] for x in c] == [4 * 2, 4 * M, 0]                   # once per message, whatever its columns
    assert [x["no_return_points"] for x in c] == (4 * ref["no_return_points"]).tolist()
    dec.close()


def test_column_major_cloud_and_no_intensity():
    """column_stride > row_stride (H = 4, C = 5): the generic addressing, gathered byte by byte; and a layout without intensity."""
    layout = points_cases.column_major(4, 5)
    assert points.kernel_path(layout) == points.PATH_GATHER
    S, M = 2, 7
    dec = points.PointsDecoder(S, layout, max_messages=M)
    skip = np.zeros((S, M), dtype=bool)
    skip[1, 3] = True
    for base, extra in ((0, 0), (3, 1)):
        msg, _, inten = _messages(layout, S, M, layout.message_bytes + extra, 70 + base)
        ref = _decode_and_compare(dec, layout, msg, base, skip=skip, poses=np.random.default_rng(3).normal(size=(S, M, 12)), tag=base)
        assert np.array_equal(ref["intensity"][0], inten[0])                          # the byte verbatim
    dec.close()
    layout = points_cases.no_intensity(4)
    dec = points.PointsDecoder(1, layout, max_messages=300)
    msg, _, _ = _messages(layout, 1, 300, layout.message_bytes, 71)                   # 256 messages per workgroup: two workgroups
    ref = _decode_and_compare(dec, layout, msg, 1)
    assert not ref["intensity"].any()
    dec.close()


def test_results_do_not_depend_on_the_path():
    """The same firings written as a row-major cloud, as a column-major cloud and as single-column messages take the three paths of the
    kernel and come back the same."""
    rng = np.random.default_rng(21)
    H, C, M = 8, 5, 3
    F32 = points.FLOAT32
    fields = [("x", 1, F32, 1), ("y", 5, F32, 1), ("z", 9, F32, 1), ("intensity", 13, points.UINT8, 1)]
    rows = points.layout_from_pointcloud2(H, C, 15, C * 15 + 1, fields, intensity_mode=points.INTENSITY_U8)
    cols = points.Layout(rows=H, columns=C, row_stride=15, column_stride=H * 15 + 1, off_x=1, off_y=5, off_z=9, off_intensity=13,
                         intensity_mode=points.INTENSITY_U8, reverse_rows=0, message_bytes=(H - 1) * 15 + (C - 1) * (H * 15 + 1) + 15)
    single = points.layout_from_pointcloud2(H, 1, 15, 15, fields, intensity_mode=points.INTENSITY_U8)
    assert [points.kernel_path(x) for x in (rows, cols, single)] == [points.PATH_ROWS, points.PATH_GATHER, points.PATH_MESSAGES]
    xyz, inten = points_cases.random_firings(rng, (1, M), rows)                      # M * C firings
    for layout in (rows, cols, single):
        msg = points.write_messages(xyz, inten, layout, fill=rng)
        dec = points.PointsDecoder(1, layout, max_messages=msg.shape[1])
        ref = _decode_and_compare(dec, layout, msg, 1, tag=points.kernel_path(layout))
        assert np.array_equal(ref["xyz"], xyz) and np.array_equal(ref["intensity"], inten)
        dec.close()


def test_counters_after_two_calls_and_poses_left_alone():
    """Two calls, the second with fewer messages than max_messages (its own stream stride); NULL message poses leave d_poses as it was."""
    layout = points_cases.raw_firing(32, points.INTENSITY_U8)
    S, M = 3, 6
    dec = points.PointsDecoder(S, layout, max_messages=M)
    msg, _, _ = _messages(layout, S, M, layout.message_bytes + 3, 90)
    skip = np.zeros((S, M), dtype=bool)
    skip[0, 0] = skip[0, 5] = skip[1, 2] = True
    first = _decode_and_compare(dec, layout, msg, 2, skip=skip, poses=np.random.default_rng(4).normal(size=(S, M, 12)))
    assert dec.counters(0) == dict(skipped_messages=2, no_return_points=int(first["no_return_points"][0]))
    msg2 = np.ascontiguousarray(msg[:, :4])
    second = _decode_and_compare(dec, layout, msg2, 1, skip=skip[:, :4], poses=None)   # the sentinel-filled poses stay untouched
    for s in range(S):
        assert dec.counters(s) == dict(skipped_messages=int(first["skipped_messages"][s] + second["skipped_messages"][s]),
                                       no_return_points=int(first["no_return_points"][s] + second["no_return_points"][s])), s
    assert dec.counters(0)["skipped_messages"] == 3 and dec.counters(2)["skipped_messages"] == 0
    dec.close()


def test_bad_arguments_are_refused_not_run():
    import torch
    from continuous_clustering_amd import Engine, EngineError
    layout = points_cases.raw_firing(32)
    M, S, H = 4, 2, 32
    cfg = capi.Config.vls128()
    e64 = Engine(cfg, 64, 2)
    dec = points.PointsDecoder(S, layout, max_messages=M, hip_stream=e64.hip_stream())
    with pytest.raises(EngineError) as ei:                                           # the engine's rows are not the layout's
        dec.check_engine(e64)
    assert ei.value.code == capi.CC_ERR_INVALID_ARGUMENT and "rows" in str(ei.value)
    e3 = Engine(cfg, 32, 3)
    with pytest.raises(EngineError) as ei:                                           # stream count differs
        dec.check_engine(e3)
    assert ei.value.code == capi.CC_ERR_INVALID_ARGUMENT and "streams" in str(ei.value)
    e2 = Engine(cfg, 32, 2)
    dec.check_engine(e2)
    with pytest.raises(EngineError) as ei:                                           # a layout cc_points_layout_check refuses
        points.PointsDecoder(S, layout.copy(off_z=34), max_messages=M)
    assert ei.value.code == capi.CC_ERR_INVALID_ARGUMENT and "field z" in str(ei.value)
    dev = torch.device("cuda")
    err = points._lib().cc_points_last_error
    stride = layout.message_bytes
    pk = torch.zeros((S, M + 1, stride), dtype=torch.uint8, device=dev)
    out = _outputs(dev, S, M + 1, H)
    xyz, inten, poses = out["xyz"], out["intensity"], out["poses"]
    mposes = torch.zeros((S, M + 1, 12), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    bad = capi.CC_ERR_INVALID_ARGUMENT
    assert dec.decode_raw(M + 1, pk, stride, None, None, xyz, inten, poses) == bad and b"n_messages" in err()      # more than max_messages
    assert dec.decode_raw(0, pk, stride, None, None, xyz, inten, poses) == bad and b"n_messages" in err()          # fewer than one
    assert dec.decode_raw(-1, pk, stride, None, None, xyz, inten, poses) == bad and b"n_messages" in err()
    assert dec.decode_raw(1, pk, stride - 1, None, None, xyz, inten, poses) == bad and b"message_stride" in err()  # below message_bytes
    assert dec.decode_raw(1, None, stride, None, None, xyz, inten, poses) == bad and b"required" in err()          # no messages
    assert dec.decode_raw(1, pk, stride, None, None, None, inten, poses) == bad and b"required" in err()           # no xyz
    assert dec.decode_raw(1, pk, stride, None, None, xyz, None, poses) == bad and b"required" in err()             # no intensity
    assert dec.decode_raw(1, pk, stride, mposes, None, xyz, inten, None) == bad and b"required" in err()           # message poses, no poses
    assert dec.decode_raw(1, pk, stride, None, None, xyz.view(-1)[1:], inten, poses) == bad and b"misaligned" in err()
    assert dec.decode_raw(1, pk, stride, None, None, xyz, inten.view(-1)[1:], poses) == bad and b"misaligned" in err()
    assert dec.decode_raw(1, pk, stride, None, None, xyz, inten, poses.view(-1)[1:]) == bad and b"misaligned" in err()
    assert dec.decode_raw(1, pk, stride, mposes.view(-1)[1:], None, xyz, inten, poses) == bad and b"misaligned" in err()
    dec.sync()
    # nothing was launched: the outputs are as they were, the counters zero
    assert bool((xyz == CANARY_F32).all()) and bool((inten == CANARY_U8).all()) and bool((poses == SENTINEL_POSE).all())
    assert dec.counters() == [dict(skipped_messages=0, no_return_points=0)] * S
    # and a good call still runs, with the messages at an odd address
    assert dec.decode_raw(1, pk.view(-1)[1:], stride, None, None, xyz, inten, None) == capi.CC_OK
    dec.sync()
    written = xyz.view(-1)[: S * H * 3]                                              # [2][1][32][3]: the stream stride of a 1-message call
    assert bool((written == 0).all()) and bool((xyz.view(-1)[S * H * 3:] == CANARY_F32).all())
    dec.close()
    for e in (e2, e3, e64):
        e.close()
