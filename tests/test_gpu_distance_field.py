"""vk_volume_classify_cells, vk_grid_distance_transform and vk_volume_distance_field on the device against their CPU
statement (tests/distance_field_reference.py). The volume starts from an uploaded oracle state; classes and squared
distances are integers and the float field is one defined sequence of float32 operations, so everything is compared bit for
bit — the floats as uint32 — with no tolerance. Every output is allocated with a guard tail that has to keep its pattern, and
tests/test_distance_field_reference.py shows that the case grids reach every outcome."""
import ctypes as C

import numpy as np
import pytest

import carve_rays_reference as CC
import distance_field_reference as DF
import merge_reference as M
import register_reference as RR
import release_reference as R
from gpu_support import OTHER, SAME, api, assert_untouched, device_copy, overwrite, sync  # noqa: F401
from vulcan_amd import vk_types as T

pytestmark = pytest.mark.gpu

TAIL = 64                         # guard elements behind every output
RAGGED = DF.GRIDS["ragged"]
CENTRE = (-8, -8, 123)            # a voxel of the surface's rippled zero crossing: lines along x and y leave and re-enter it
_STATE = {}


def world(api, orc, sizes=SAME[0]):
    """(host volume, its block table, device copy) of the test view at these table sizes: once, only read"""
    if sizes not in _STATE:
        hv = M.view_state(orc, "a", *sizes)
        _STATE[sizes] = (hv, RR.block_table(hv), device_copy(api, hv))
    return _STATE[sizes]


def guarded(shape, dtype, fill, seed):
    """a device tensor of prod(shape) + TAIL elements, overwritten; (tensor, its tail as it has to stay)"""
    import torch
    count = int(np.prod(shape))
    t = torch.empty(count + TAIL, dtype=dtype, device="cuda")
    overwrite(t, fill, seed)
    return t, t[count:].clone()


def run(api, dv, origin, dims, stride, max_cells, occupied_below=0.0, site_mask=4, signed=False, classes=True, d2=True, fill="noise"):
    """one vk_volume_distance_field through the library's own entry point, into guarded outputs and a workspace that were
    overwritten with `fill` (0xFF bytes, or noise): (classes, d2, distance as uint32) as numpy arrays [nz, ny, nx]"""
    import torch
    lib = api.lib()
    grid = T.CellGrid.make(origin, dims, stride)
    params = T.DistanceFieldParams(T.VK_FIELD_SIGNED if signed else 0, site_mask, max_cells, occupied_below)
    shape = tuple(int(d) for d in dims)[::-1]
    count = int(np.prod(shape))
    size = lib.vk_volume_distance_field_workspace_bytes(C.byref(grid), C.byref(params))
    assert size > 0
    workspace, workspace_tail = guarded((size,), torch.uint8, fill, 11)
    out_c, tail_c = guarded(shape, torch.uint8, fill, 12) if classes else (None, None)
    out_d2, tail_d2 = guarded(shape, torch.int32, fill, 13) if d2 else (None, None)
    out_f, tail_f = guarded(shape, torch.float32, fill, 14)
    api.check(lib.vk_volume_distance_field(C.byref(dv.desc()), C.byref(grid), C.byref(params), api._ptr(out_c), api._ptr(out_d2),
                                           api._ptr(out_f), api._ptr(workspace), api.stream()), "vk_volume_distance_field")
    sync()
    for out, tail in ((workspace, workspace_tail), (out_c, tail_c), (out_d2, tail_d2), (out_f, tail_f)):
        if out is not None:
            assert torch.equal(out[-TAIL:].view(torch.uint8), tail.view(torch.uint8)), "a guard tail was written"
    return (None if out_c is None else out_c[:count].cpu().numpy().reshape(shape),
            None if out_d2 is None else out_d2[:count].cpu().numpy().reshape(shape),
            out_f[:count].cpu().numpy().view(np.uint32).reshape(shape))


def assert_is_statement(got, want, what=""):
    classes, d2, distance = got
    if classes is not None:
        assert np.array_equal(classes, want[0]), f"classes {what}"
    if d2 is not None:
        assert np.array_equal(d2, want[1]), f"d2 {what}"
    assert np.array_equal(distance, want[2].view(np.uint32)), f"distance {what}"


def check(api, dv, hv, table, origin, dims, stride, max_cells, occupied_below=0.0, site_mask=4, signed=False, **kw):
    want = DF.distance_field(hv, origin, dims, stride, max_cells, occupied_below, site_mask, signed, table=table)
    got = run(api, dv, origin, dims, stride, max_cells, occupied_below, site_mask, signed, **kw)
    assert_is_statement(got, want, f"{origin} {dims} stride {stride} cap {max_cells}")
    return want


@pytest.mark.parametrize("sizes", [SAME[0], OTHER[0]], ids=["long-chains", "other-bucket-count"])
@pytest.mark.parametrize("name", list(DF.GRIDS))
def test_the_case_grids_bit_for_bit(api, orc, sizes, name):
    hv, table, dv = world(api, orc, sizes)
    origin, dims, stride, max_cells = DF.GRIDS[name]
    classes, d2, _ = check(api, dv, hv, table, origin, dims, stride, max_cells)
    counts = [int((classes == c).sum()) for c in (DF.UNKNOWN, DF.FREE, DF.OCCUPIED)]
    print(name, "unknown, free, occupied", counts, "beyond", int((d2 == DF.BEYOND).sum()))
    assert min(counts) > 100 and ((d2 != DF.BEYOND) & (d2 != 0)).sum() > 1000
    assert_untouched(dv, hv)
    assert dv.host_voxels().tobytes() == hv.voxels.tobytes()


@pytest.mark.parametrize("max_cells", [1, 2, 9, 16, 256])
def test_the_cap(api, orc, max_cells):
    hv, table, dv = world(api, orc)
    origin, dims, stride, _ = RAGGED
    _, d2, _ = check(api, dv, hv, table, origin, dims, stride, max_cells)
    assert ((d2 == DF.BEYOND).any()) == (max_cells < 20)


@pytest.mark.parametrize("signed", [False, True], ids=["unsigned", "signed"])
@pytest.mark.parametrize("site_mask", [4, 1, 2, 3, 7])
def test_the_site_masks_and_the_sign(api, orc, site_mask, signed):
    hv, table, dv = world(api, orc)
    origin, dims, stride, max_cells = DF.GRIDS["stride-2"]
    _, _, distance = check(api, dv, hv, table, origin, dims, stride, max_cells, site_mask=site_mask, signed=signed)
    assert (distance < 0).any() == signed
    if signed and site_mask == 7:
        assert np.isneginf(distance).all()


@pytest.mark.parametrize("occupied_below", [-0.25, 0.0, 0.25])
def test_the_occupancy_threshold(api, orc, occupied_below):
    hv, table, dv = world(api, orc)
    origin, dims, stride, max_cells = RAGGED
    classes = check(api, dv, hv, table, origin, dims, stride, max_cells, occupied_below=occupied_below)[0]
    _STATE.setdefault("occupied", {})[occupied_below] = int((classes == DF.OCCUPIED).sum())
    seen = _STATE["occupied"]
    assert all(seen[a] < seen[b] for a in seen for b in seen if a < b)


SHAPES = [(1, 1, 1), (70, 1, 1), (1, 70, 1), (1, 1, 70)] + [tuple(n if a == axis else (5, 3, 4)[a] for a in range(3))
                                                           for axis in range(3) for n in (63, 64, 65, 257)]


@pytest.mark.parametrize("dims", SHAPES, ids=["x".join(str(n) for n in s) for s in SHAPES])
def test_shapes_at_which_a_tiled_pass_can_go_wrong(api, orc, dims):
    hv, table, dv = world(api, orc)
    origin = tuple(CENTRE[a] - dims[a] // 2 for a in range(3))
    for max_cells in (5, 256):
        classes = check(api, dv, hv, table, origin, dims, 1, max_cells, classes=max_cells == 5, d2=max_cells == 256)[0]
    assert (classes == DF.OCCUPIED).any() and (max(dims) == 1 or (classes != DF.OCCUPIED).any())


@pytest.mark.parametrize("stride", [1, 2, 4, 8])
def test_a_grid_inside_one_block_and_one_that_meets_none(api, orc, stride):
    hv, table, dv = world(api, orc)
    inside = next(block for block, slot in table.items()
                  if (hv.voxels[slot * 512:(slot + 1) * 512]["distance_weight"] != 0).all()
                  and 0 < (hv.voxels[slot * 512:(slot + 1) * 512]["distance"] <= 0).sum() < 512)
    per = 8 // stride
    dims = (per, max(per - 1, 1), max(per - 2, 1))
    origin = tuple(8 * inside[a] + stride * (per - dims[a]) for a in range(3))
    classes = check(api, dv, hv, table, origin, dims, stride, 3)[0]
    assert (classes != DF.UNKNOWN).all() and (classes == DF.OCCUPIED).any()
    classes, d2, distance = check(api, dv, hv, table, (4096, -4096, 8192), (9, 7, 5), stride, 256)
    assert (classes == DF.UNKNOWN).all() and (d2 == DF.BEYOND).all() and np.isposinf(distance).all()


@pytest.mark.parametrize("stride", [1, 8])
def test_a_grid_cut_by_the_int16_block_range(api, orc, stride):
    """blocks at both ends of the range, the far one's twin by truncation, a second block of one origin and a block that no
    chain reaches: beyond block 32767 and before block -32768 nothing exists"""
    origins = [(32767, 0, 0), (-32768, 0, 0), (32766, 0, 0), (32767, 0, 0), (-32768, 1, 0), (-32767, 0, -1)]
    hv = DF.chained(orc, origins, ghost=(32766, 1, 0))
    dv = device_copy(api, hv)
    table = RR.block_table(hv)
    assert len(table) == 5
    for origin in ((262144 - 24, -8, -8), (-262144 - 16, -8, -8)):
        dims = (40 // stride, 24 // stride, 16 // stride)
        classes = check(api, dv, hv, table, origin, dims, stride, 256, site_mask=6)[0]
        outside = classes[:, :, 24 // stride:] if origin[0] > 0 else classes[:, :, :16 // stride]
        assert (outside == DF.UNKNOWN).all() and (classes != DF.UNKNOWN).any()


def test_the_separate_entry_points_against_the_combined_one(api, orc):
    import torch
    hv, table, dv = world(api, orc)
    origin, dims, stride, max_cells = DF.GRIDS["stride-2"]
    want = DF.distance_field(hv, origin, dims, stride, max_cells, table=table)
    field = dv.distance_field(origin, dims, stride, max_cells=max_cells, squared=True)
    classes = dv.classify_cells(origin, dims, stride)
    d2 = api.distance_transform(classes, T.CELL_OCCUPIED, max_cells)
    unknown = api.distance_transform(classes, T.CELL_UNKNOWN, max_cells)
    sync()
    assert torch.equal(classes, field.classes) and torch.equal(d2, field.squared_cells)
    assert np.array_equal(classes.cpu().numpy(), want[0]) and np.array_equal(d2.cpu().numpy(), want[1])
    assert np.array_equal(field.distance.cpu().numpy().view(np.uint32), want[2].view(np.uint32))
    assert np.array_equal(unknown.cpu().numpy(), DF.transform(want[0], T.CELL_UNKNOWN, max_cells))
    assert field.squared_cells.shape == tuple(dims)[::-1] and field.stride == stride and field.origin == origin
    assert field.cell_length == float(np.float32(stride) * np.float32(hv.voxel_length))
    # metres become cells on the host, rounded up and clamped
    metric = dv.distance_field(origin, dims, stride, max_distance=(max_cells - 0.5) * field.cell_length)
    assert metric.squared_cells is None and torch.equal(metric.distance, field.distance)
    assert dv.grid_for_box((-0.1, -0.05, 1.0), (0.1, 0.05, 1.2), 4) == DF.grid_for_box((-0.1, -0.05, 1.0), (0.1, 0.05, 1.2), 4, hv.voxel_length)


@pytest.mark.parametrize("fill", ["ones", "noise"])
@pytest.mark.parametrize("outputs", ["all", "distance-only"])
def test_dirty_buffers_and_optional_outputs(api, orc, fill, outputs):
    hv, table, dv = world(api, orc)
    origin, dims, stride, max_cells = RAGGED
    every = outputs == "all"
    for signed in (False, True):
        check(api, dv, hv, table, origin, dims, stride, max_cells, signed=signed, classes=every, d2=every, fill=fill)


def test_after_release_blocks(api, orc):
    hv = M.view_state(orc, "a", *SAME[0])
    released = R.release_blocks(hv, *R.helper_arguments(R.RULES["no-surface"]))[0]
    assert released > 0
    dv = device_copy(api, hv)
    origin, dims, stride, max_cells = DF.GRIDS["stride-2"]
    classes = check(api, dv, hv, RR.block_table(hv), origin, dims, stride, max_cells)[0]
    assert (classes == DF.OCCUPIED).sum() > 1000


def test_after_carve_rays(api, orc):
    hv = R.clone(orc, CC.scenario(orc)[0])
    dv = device_copy(api, hv)
    table = RR.block_table(hv)
    origin, dims = DF.grid_around(table, 2)
    classes, d2, _ = check(api, dv, hv, table, origin, dims, 2, 12)
    carved = hv.voxels["distance"][hv.voxels["distance_weight"] != 0] == 1.0
    print("grid", origin, dims, "carved voxels", int(carved.sum()), "free cells", int((classes == DF.FREE).sum()))
    assert carved.sum() > 1000 and (classes == DF.FREE).sum() > 1000 and (classes == DF.OCCUPIED).sum() > 100
