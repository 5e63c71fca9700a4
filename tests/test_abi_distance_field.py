"""The host side of the clearance field's entry points (include/vk.h at vk_volume_distance_field): every refusal the header
lists comes back as VK_ERR_ARGUMENT from addresses that are no memory — nothing may be enqueued, no GPU is needed or
touched — and the structs and constants of vulcan_amd/vk_types.py are the header's."""
import ctypes as C
import os
import re

from abi_support import fake_volume
from vulcan_amd import vk_types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE, ODD2, ODD8 = C.c_void_p(4096), C.c_void_p(4096 + 2), C.c_void_p(4096 + 8)
NAN, INF = float("nan"), float("inf")


def grid(origin=(0, 0, 0), dims=(8, 8, 8), stride=1):
    return T.CellGrid.make(origin, dims, stride)


def params(flags=0, site_mask=4, max_cells=16, occupied_below=0.0):
    return T.DistanceFieldParams(flags, site_mask, max_cells, occupied_below)


def ref(s):
    return C.byref(s) if s is not None else None


BAD_GRIDS = ([dict(stride=s) for s in (0, 3, 5, 6, 16, -1, -2)] +
             [dict(origin=o, stride=s) for o, s in (((1, 0, 0), 2), ((0, 2, 0), 4), ((0, 0, 4), 8), ((-3, 0, 0), 2))] +
             [dict(origin=o) for o in (((1 << 20) + 1, 0, 0), (0, -(1 << 20) - 1, 0), (0, 0, 1 << 30))] +
             [dict(origin=(0, (1 << 20) + 8, 0), stride=8)] +
             [dict(dims=d) for d in ((0, 8, 8), (8, -1, 8), (8, 8, 1025), (1024, 1024, 129), (1024, 1024, 1024), (1 << 30, 4, 4))])
GOOD_GRIDS = [dict(origin=(1 << 20, -(1 << 20), 0), stride=8), dict(dims=(1024, 1024, 128)), dict(dims=(1, 1, 1), origin=(-37, 5, 3))]


def test_the_structs_and_constants_are_the_headers():
    with open(os.path.join(ROOT, "include", "vk.h"), encoding="utf-8") as header:
        text = header.read()
    cells = re.search(r"enum \{ VK_CELL_UNKNOWN = (\d+), VK_CELL_FREE = (\d+), VK_CELL_OCCUPIED = (\d+) \};", text)
    assert tuple(int(g) for g in cells.groups()) == (T.CELL_UNKNOWN, T.CELL_FREE, T.CELL_OCCUPIED) == (1, 2, 4)
    assert int(re.search(r"enum \{ VK_FIELD_SIGNED = (\d+) \};", text).group(1)) == T.VK_FIELD_SIGNED
    assert re.search(r"#define VK_FIELD_BEYOND INT32_MAX", text) and T.VK_FIELD_BEYOND == (1 << 31) - 1
    assert int(re.search(r"#define VK_ABI_VERSION (\d+)", text).group(1)) == T.VK_ABI_VERSION == 7
    assert C.sizeof(T.CellGrid) == 32 and C.sizeof(T.DistanceFieldParams) == 16
    assert [name for name, _ in T.CellGrid._fields_] == re.findall(r"int32_t (\w+)(?:\[3\])?;", re.search(
        r"typedef struct vk_cell_grid \{(.*?)\} vk_cell_grid;", text, re.S).group(1))
    assert [name for name, _ in T.DistanceFieldParams._fields_] == re.findall(r"(?:int32_t|float)\s+(\w+);", re.search(
        r"typedef struct vk_distance_field_params \{(.*?)\} vk_distance_field_params;", text, re.S).group(1))
    assert T.CellGrid.origin.offset == 0 and T.CellGrid.dims.offset == 12 and T.CellGrid.stride.offset == 24
    assert T.DistanceFieldParams.occupied_below.offset == 12


def test_classify_cells_validates_before_touching_a_device():
    from vulcan_amd import api
    lib = api.lib()

    def call(v=fake_volume(), g=grid(), occupied_below=0.0, classes=ONE):
        return lib.vk_volume_classify_cells(ref(v), ref(g), occupied_below, classes, None)

    assert call(v=None) == -1 and call(g=None) == -1 and call(classes=None) == -1
    for field, value in (("hash_entries", None), ("voxel_length", 0.0), ("main_block_count", 0), ("voxels", (1 << 20) + 8)):
        broken = fake_volume()
        setattr(broken, field, value)
        assert call(v=broken) == -1, field
    for bad in BAD_GRIDS:
        assert call(g=grid(**bad)) == -1, bad
    for threshold in (NAN, INF, -INF, 1.5, -1.0001):
        assert call(occupied_below=threshold) == -1, threshold


def test_the_transform_validates_before_touching_a_device():
    from vulcan_amd import api
    lib = api.lib()

    def dims3(*d):
        return (C.c_int32 * 3)(*d)

    def call(classes=ONE, dims=dims3(8, 8, 8), site_mask=4, max_cells=16, d2=ONE, workspace=ONE):
        return lib.vk_grid_distance_transform(classes, dims, site_mask, max_cells, d2, workspace, None)

    assert call(classes=None) == -1 and call(dims=None) == -1 and call(d2=None) == -1 and call(workspace=None) == -1
    for d in ((0, 8, 8), (8, -1, 8), (8, 8, 1025), (1024, 1024, 129), (1 << 30, 4, 4)):
        assert call(dims=dims3(*d)) == -1, d
        assert lib.vk_grid_distance_transform_workspace_bytes(dims3(*d)) == 0
    assert lib.vk_grid_distance_transform_workspace_bytes(None) == 0
    for site_mask in (0, 8, -1, 1 << 16):
        assert call(site_mask=site_mask) == -1
    for max_cells in (0, -1, 257, 1 << 30):
        assert call(max_cells=max_cells) == -1
    assert call(d2=ODD2) == -1 and call(workspace=ODD8) == -1
    # the workspace holds the passes' intermediates (2 and 4 bytes per cell), a class grid, and two flag bytes per grid row and
    # 64 cells of it, each part on a 256-byte boundary
    def part(n):
        return (n + 255) // 256 * 256
    for d in ((1, 1, 1), (8, 8, 8), (67, 45, 33), (1024, 1024, 128)):
        cells = d[0] * d[1] * d[2]
        size = lib.vk_grid_distance_transform_workspace_bytes(dims3(*d))
        assert size == part(2 * cells) + part(4 * cells) + part(cells) + 2 * part((d[0] + 63) // 64 * d[1] * d[2])


def test_the_distance_field_validates_before_touching_a_device():
    from vulcan_amd import api
    lib = api.lib()

    def call(v=fake_volume(), g=grid(), p=params(), classes=ONE, d2=ONE, distance=ONE, workspace=ONE):
        return lib.vk_volume_distance_field(ref(v), ref(g), ref(p), classes, d2, distance, workspace, None)

    def size(g=grid(), p=params()):
        return lib.vk_volume_distance_field_workspace_bytes(ref(g), ref(p))

    assert call(v=None) == -1 and call(g=None) == -1 and call(p=None) == -1 and call(distance=None) == -1 and call(workspace=None) == -1
    for field, value in (("hash_entries", None), ("voxel_length", 0.0), ("main_block_count", 0), ("voxels", (1 << 20) + 8),
                         ("counters", None), ("excess_block_count", -1)):
        broken = fake_volume()
        setattr(broken, field, value)
        assert call(v=broken) == -1, field
    for bad in BAD_GRIDS:
        assert call(g=grid(**bad)) == -1 and size(g=grid(**bad)) == 0, bad
    for good in GOOD_GRIDS:
        assert size(g=grid(**good)) > 0, good
    for bad in ([dict(site_mask=m) for m in (0, 8, -1, 1 << 16)] + [dict(max_cells=m) for m in (0, -1, 257, 1 << 30)] +
                [dict(flags=f) for f in (2, 3, -1, 1 << 16)] + [dict(occupied_below=t) for t in (NAN, INF, -INF, 1.5, -1.0001)]):
        assert call(p=params(**bad)) == -1 and size(p=params(**bad)) == 0, bad
    for good in (dict(flags=1), dict(site_mask=7), dict(site_mask=1), dict(max_cells=256), dict(max_cells=1), dict(occupied_below=-1.0),
                 dict(occupied_below=1.0)):
        assert size(p=params(**good)) == size() > 0, good
    assert size(g=None) == 0 and size(p=None) == 0
    assert call(d2=ODD2) == -1 and call(distance=ODD2) == -1 and call(workspace=ODD8) == -1
