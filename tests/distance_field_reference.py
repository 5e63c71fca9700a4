"""The CPU statement of vk_volume_classify_cells, vk_grid_distance_transform and vk_volume_distance_field (include/vk.h): a
voxel-hashed volume classified into a dense grid of cells, the exact squared Euclidean distance of every cell to the nearest
site cell, and the clearance field in metres — in numpy, on an oracle.HostVolume. There is no upstream counterpart, so this
file is the definition.

The classes and the squared distances are integers. The float field is float32 with one rounding per operation in the
order vk.h gives — numpy's float32 arithmetic and its correctly rounded square root are exactly that — so no tolerance
exists and the device is held to it bit for bit (tests/test_gpu_distance_field.py).

It also holds the case table of grids the CPU and the GPU tests share."""
import numpy as np

import register_reference as RR
from vulcan_amd import vk_types as T

f32 = np.float32
UNKNOWN, FREE, OCCUPIED = T.CELL_UNKNOWN, T.CELL_FREE, T.CELL_OCCUPIED
BEYOND = T.VK_FIELD_BEYOND
NONE = 1 << 29                  # no site within reach, while the passes run

# name: (origin, dims (nx, ny, nz), stride, max_cells) on merge_reference.view_state(orc, "a", ...)
GRIDS = {
    "stride-1": ((-96, -80, 96), (192, 160, 64), 1, 16),
    "stride-2": ((-96, -80, 96), (96, 80, 32), 2, 12),
    "stride-4": ((-96, -80, 96), (48, 40, 16), 4, 8),
    "ragged": ((-37, -21, 107), (67, 45, 33), 1, 20),
}
SMALL = ((-12, -10, 118), (24, 20, 18), 1)      # the grid the brute force is run on


def classify(hv, origin, dims, stride=1, occupied_below=0.0, table=None):
    """uint8 [nz, ny, nx]: the class of every cell. Driven from the blocks the chain walk finds, as the device is: a cell
    lies in one block, since the origin is a multiple of the stride."""
    origin, dims = np.asarray(origin, dtype=np.int64), np.asarray(dims, dtype=np.int64)
    assert stride in (1, 2, 4, 8) and (origin % stride == 0).all()
    table = RR.block_table(hv) if table is None else table
    nx, ny, nz = (int(d) for d in dims)
    classes = np.full((nz, ny, nx), UNKNOWN, dtype=np.uint8)
    per = 8 // stride                                                       # cells of a block along an axis
    threshold = f32(occupied_below)
    for block, slot in table.items():
        if not all(-32768 <= c <= 32767 for c in block):
            continue
        first = (8 * np.asarray(block, dtype=np.int64) - origin) // stride  # the block's first cell
        if (first + per <= 0).any() or (first >= dims).any():
            continue
        voxels = hv.voxels[slot * 512:(slot + 1) * 512]
        observed = (voxels["distance_weight"] != 0).reshape(8, 8, 8)         # [z, y, x]
        with np.errstate(invalid="ignore"):
            occupied = observed & (voxels["distance"].reshape(8, 8, 8) <= threshold)
        fold = lambda bits: bits.reshape(per, stride, per, stride, per, stride).any(axis=(1, 3, 5))
        cells = np.where(fold(occupied), OCCUPIED, np.where(fold(observed), FREE, UNKNOWN)).astype(np.uint8)
        lo, hi = np.maximum(first, 0), np.minimum(first + per, dims)
        classes[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = cells[lo[2] - first[2]:hi[2] - first[2], lo[1] - first[1]:hi[1] - first[1],
                                                               lo[0] - first[0]:hi[0] - first[0]]
    return classes


def _pass(values, axis, max_cells):
    """min over offsets |k| <= max_cells along `axis` of values shifted by k, plus k^2; cells outside the grid do not exist"""
    length = values.shape[axis]
    best = values.copy()
    for k in range(1, min(max_cells, length - 1) + 1):
        square = np.int32(k * k)
        here, there = [slice(None)] * 3, [slice(None)] * 3
        here[axis], there[axis] = slice(0, length - k), slice(k, length)
        here, there = tuple(here), tuple(there)
        best[here] = np.minimum(best[here], values[there] + square)
        best[there] = np.minimum(best[there], values[here] + square)
    return best


def transform(classes, site_mask, max_cells):
    """int32 [nz, ny, nx]: d2 of every cell. Three separable passes, x, then y, then z, then the threshold."""
    assert 0 <= site_mask <= 7 and 1 <= max_cells <= 256
    values = np.where((classes & site_mask) != 0, 0, NONE).astype(np.int32)
    for axis in (2, 1, 0):
        values = np.minimum(_pass(values, axis, max_cells), NONE)
    return np.where(values > max_cells * max_cells, BEYOND, values).astype(np.int32)


def brute_force(classes, site_mask, max_cells):
    """the same by the definition's own words: the minimum over all sites"""
    nz, ny, nx = classes.shape
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    best = np.full(classes.shape, BEYOND, dtype=np.int64)
    for sk, sj, si in np.argwhere((classes & site_mask) != 0):
        best = np.minimum(best, (k - sk) ** 2 + (j - sj) ** 2 + (i - si) ** 2)
    return np.where(best > max_cells * max_cells, BEYOND, best).astype(np.int32)


def metres(d2, stride, voxel_length):
    """float32: (sqrtf((float)d2) * (float)stride) * voxel_length, +inf beyond the cap"""
    beyond = d2 == BEYOND
    root = np.sqrt(np.where(beyond, 0, d2).astype(f32))
    assert root.dtype == f32
    out = (root * f32(stride)) * f32(voxel_length)
    assert out.dtype == f32
    return np.where(beyond, f32(np.inf), out)


def field(classes, site_mask, max_cells, stride, voxel_length, signed=False):
    """(d2 int32, distance float32) of a class grid"""
    d2 = transform(classes, site_mask, max_cells)
    distance = metres(d2, stride, voxel_length)
    if signed:
        inside = metres(transform(classes, 7 ^ site_mask, max_cells), stride, voxel_length)
        distance = np.where((classes & site_mask) != 0, -inside, distance)
    return d2, distance


def distance_field(hv, origin, dims, stride=1, max_cells=256, occupied_below=0.0, site_mask=OCCUPIED, signed=False, table=None):
    """(classes, d2, distance) as vk_volume_distance_field writes them"""
    classes = classify(hv, origin, dims, stride, occupied_below, table)
    return (classes,) + field(classes, site_mask, max_cells, stride, hv.voxel_length, signed)


def chained(orc, origins, seed=3, ghost=None):
    """A HostVolume of one bucket whose chain holds a block at each of `origins` in order (an origin given twice: the chain
    walk finds the first), with random voxels — a third unobserved, distances in [-1, 1]. `ghost`: the origin of one more
    entry with a block that no chain reaches."""
    count = len(origins) + (1 if ghost is not None else 0)
    hv = orc.HostVolume(1, count + 2, voxel_length=0.008, truncation_length=0.04)
    rng = np.random.default_rng(seed)
    hv.voxels["distance"] = rng.uniform(-1, 1, len(hv.voxels)).astype(f32)
    hv.voxels["distance_weight"] = rng.integers(0, 3, len(hv.voxels))
    hv.hash_entries["data"], hv.hash_entries["next"] = -1, -1
    for index, origin in enumerate(origins):
        hv.hash_entries["block"]["origin"][index] = origin
        hv.hash_entries["data"][index] = index
        hv.hash_entries["next"][index] = index + 1 if index + 1 < len(origins) else -1
    if ghost is not None:
        hv.hash_entries["block"]["origin"][len(origins)] = ghost
        hv.hash_entries["data"][len(origins)] = len(origins)
    return hv


def grid_around(table, stride, most=(96, 96, 48)):
    """(origin, dims) of an aligned grid over the middle of the blocks of `table`, a block more on every side, at most
    `most` cells per axis"""
    blocks = np.array(list(table), dtype=np.int64)
    lo, hi = 8 * (blocks.min(0) - 1), 8 * (blocks.max(0) + 2)
    dims = np.minimum((hi - lo) // stride, most)
    origin = ((lo + hi) // 2 - dims * stride // 2) // stride * stride
    return tuple(int(o) for o in origin), tuple(int(d) for d in dims)


def grid_for_box(lo, hi, stride, voxel_length):
    """(origin, dims) of the smallest aligned grid that covers the metric box: api.grid_for_box's statement"""
    first = np.floor(np.asarray(lo, dtype=np.float64) / voxel_length / stride).astype(np.int64)
    last = np.floor(np.asarray(hi, dtype=np.float64) / voxel_length / stride).astype(np.int64)
    return tuple(int(f) * stride for f in first), tuple(int(n) for n in last - first + 1)
