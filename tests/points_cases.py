"""The message layouts the generic PointCloud2 decoder tests share (tests/test_points_cpu.py, tests/test_gpu_points.py): the smallest
shapes at which each path of the kernel can go wrong. Needs the built library (the column tile is asked of it), no device."""
from __future__ import annotations

import numpy as np

from continuous_clustering_amd import points

XYZI_FIELDS = [("x", 0, points.FLOAT32, 1), ("y", 4, points.FLOAT32, 1), ("z", 8, points.FLOAT32, 1), ("intensity", 12, points.FLOAT32, 1)]
# a 22-byte point with every field at an odd offset
ODD_FIELDS = [("x", 3, points.FLOAT32, 1), ("y", 7, points.FLOAT32, 1), ("z", 13, points.FLOAT32, 1), ("intensity", 17, points.FLOAT32, 1)]


def raw_firing(rows=32, mode=points.INTENSITY_REFERENCE) -> points.Layout:
    """The reference's own firing message: 37-byte points, floats at odd addresses from the second point on."""
    return points.raw_firing_layout(rows, intensity_mode=mode)


def aligned_xyzi(rows=64) -> points.Layout:
    return points.layout_from_pointcloud2(rows, 1, 16, 16, XYZI_FIELDS, intensity_mode=points.INTENSITY_F32_UNIT)


def organised_row_major(rows=8):
    """(layout, tile): 22-byte points, rows padded by 3 bytes, tile + 6 columns (more than one tile and a partial last one), rows
    reversed, intensity on a 0..255 scale."""
    def make(columns):
        return points.layout_from_pointcloud2(rows, columns, 22, columns * 22 + 3, ODD_FIELDS, intensity_mode=points.INTENSITY_F32_255,
                                              reverse_rows=True)
    tile = points.column_tile(make(1000))
    layout = make(tile + 6)
    assert points.kernel_path(layout) == points.PATH_ROWS and points.column_tile(layout) == tile and tile > 1
    return layout, tile


def column_major(rows=4, columns=5) -> points.Layout:
    """column_stride > row_stride: 19-byte points, the rows of a column back to back, columns padded by 2 bytes."""
    row_stride, column_stride = 19, rows * 19 + 2
    return points.Layout(rows=rows, columns=columns, row_stride=row_stride, column_stride=column_stride, off_x=0, off_y=5, off_z=10,
                         off_intensity=15, intensity_mode=points.INTENSITY_U8, reverse_rows=0,
                         message_bytes=(rows - 1) * row_stride + (columns - 1) * column_stride + 19)


def no_intensity(rows=4) -> points.Layout:
    return points.layout_from_pointcloud2(rows, 1, 12, 12, XYZI_FIELDS[:3])


def all_layouts() -> dict:
    return {"raw_firing_reference": raw_firing(), "raw_firing_u8": raw_firing(mode=points.INTENSITY_U8), "aligned_xyzi": aligned_xyzi(),
            "organised_row_major": organised_row_major()[0], "column_major": column_major(), "no_intensity": no_intensity()}


def random_firings(rng, lead, layout):
    """xyz as random bit patterns (NaNs, infinities and denormals among them, plus a few planted) and random intensities."""
    F = lead[-1] * layout.columns
    xyz = rng.integers(0, 2 ** 32, (*lead[:-1], F, layout.rows, 3), dtype=np.uint64).astype(np.uint32)
    flat = xyz.reshape(-1, 3)
    special = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800001, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001], dtype=np.uint32)
    at = np.arange(0, flat.shape[0], 7)
    flat[at, 0] = special[np.arange(at.size) % 8]
    flat[1::5] = np.array([1.5, -2.25, 0.125], dtype=np.float32).view(np.uint32)
    inten = rng.integers(0, 256, (*lead[:-1], F, layout.rows), dtype=np.uint8)
    return xyz, inten
