"""The CPU statement of vk_volume_carve_rays (tests/carve_rays_reference.py) against what any definition of the call must
give: its cell walk is integrate_rays' walk, one ray along an axis carves the cells one can count by hand, the shared ray sets
reach every branch, a ray carves a cell once and only in front of its measurement, the order of the rays changes no byte,
nothing but carved voxels changes, carving and fusing one ray share (almost) no cell, and a wall that is no longer there
disappears from what cast_rays sees. No GPU: the device is held to the same statement in tests/test_gpu_carve_rays.py."""
import ctypes as C

import numpy as np
import pytest

from abi_support import fake_volume
import carve_rays_reference as CV
from carve_rays_reference import state_but_voxels
import cast_reference as CR
import integrate_rays_reference as IR
import register_reference as RR
import release_reference as R
from vulcan_amd import vk_types as T

f32 = np.float32
SMALL, LARGE = ((509, 4096), (509, 4096)), ((4093, 2048), (509, 4096))
# The scenario: of 19 200 rays every one hits the back wall after three carves; |t - back range| median 7.60e-4 m, 99th
# percentile 4.19e-3 m, 5.14e-3 m at worst, measured on this statement. Asserted: twice the measured maximum, the margin for
# nothing more than another host libm or numpy build (as test_integrate_rays_reference.py does).
SCENARIO_BOUND = 2 * 5.14e-3


def test_the_statements_walk_is_integrate_rays_walk(orc):
    """with ta = max(r - tr, 0) and tb = r + tr the walk of this statement is integrate_rays_reference.walk, cell for cell"""
    hv = CR.volume(orc)
    rays, ranges = IR.all_rays(orc, False)
    o, n, r, kind = IR.carried(hv, rays, ranges, None, IR.R_MIN, IR.R_MAX, False)
    fused = kind == IR.INTEGRATED
    o, n, r, tr = o[fused], n[fused], r[fused], f32(5)
    who, cells = IR.walk(o, n, r, tr)
    mine, my_cells, leaves = CV.walk(o, n, np.fmax(r - tr, f32(0)), r + tr)
    assert len(who) > 100000 and np.array_equal(who, mine) and np.array_equal(cells, my_cells)
    assert leaves.dtype == f32 and len(leaves) == len(who)


def one_row(t_from):
    """the ray +x from (0.5, 0.5, 0.5) voxels with r = 40.25 and tr = 5 in a volume that holds blocks (1, 0, 0) and (2, 0, 0)"""
    import oracle.oracle as orc
    hv = orc.HostVolume(61, 16, voxel_length=2.0 ** -7, truncation_length=5 * 2.0 ** -7)
    # a measurement at x = 15.5 from x = 8.5 allocates the two blocks; then every voxel is made Voxel::Empty() again
    IR.integrate(hv, np.array([[8.5, 0.5, 0.5, 1, 0, 0]], dtype=f32), np.array([7.0], dtype=f32), r_min=1.0, r_max=100.0, flags=IR.VOXEL_UNITS)
    table = RR.block_table(hv)
    assert sorted(table) == [(1, 0, 0), (2, 0, 0)]
    hv.voxels[:] = np.zeros((), dtype=T.voxel_dtype)
    hv.voxels["distance"] = 1
    before = state_but_voxels(hv)
    out = CV.carve(hv, np.array([[0.5, 0.5, 0.5, 2.0, 0, 0]], dtype=f32), np.array([40.25], dtype=f32), r_min=1.0, r_max=100.0,
                   t_from=t_from, flags=CV.VOXEL_UNITS)
    assert state_but_voxels(hv) == before and RR.block_table(hv) == table       # cells 0 .. 7 and 24 .. 34 are not created
    carved = {}
    for index in np.flatnonzero(out.N):
        slot, voxel = divmod(int(index), 512)
        origin = [o for o, s in table.items() if s == slot][0]
        assert voxel >> 3 == 0 and origin[1:] == (0, 0)
        carved[8 * origin[0] + voxel] = int(out.N[index])
        assert hv.voxels["distance"][index] == 1 and hv.voxels["distance_weight"][index] == 1
    assert int((hv.voxels["distance_weight"] != 0).sum()) == len(carved)
    return carved, out


def test_one_ray_by_hand():
    # te = 35.25, at x = 35.75: cell 35 straddles it and is the band walk's; 24 .. 34 lie in absent blocks
    carved, out = one_row(0.0)
    assert carved == {c: 1 for c in range(8, 24)}
    assert out.counts == (1, 0, 0, 0, 0, 2, 16, 16) and out.branches["absent"] == 3 and out.branches["present"] == 2
    # t0 = 10.5: the walk starts at p = 0.5 + 10.5 = 11.0, which is cell 11 by the definition's floorf (cell 10 ends at
    # x = 11 and is left at t = 10.5 exactly); t0 = 10.25 starts inside cell 10
    carved, out = one_row(10.5)
    assert carved == {c: 1 for c in range(11, 24)} and out.counts == (1, 0, 0, 0, 0, 2, 13, 13)
    carved, out = one_row(10.25)
    assert carved == {c: 1 for c in range(10, 24)} and out.counts == (1, 0, 0, 0, 0, 2, 14, 14)
    # nothing to carve: the carve would start where the band does, or behind it
    carved, out = one_row(35.25)
    assert carved == {} and out.counts == (0, 1, 0, 0, 0, 0, 0, 0)


@pytest.fixture(scope="module")
def everything(orc):
    """the statement on all sets into the scene volume, as the GPU tests carve them"""
    hv = R.clone(orc, CR.volume(orc))
    return hv, CV.carve(hv, *CV.all_rays(orc, False))


@pytest.mark.parametrize("sizes", [SMALL, LARGE], ids=["509-buckets", "4093-buckets"])
def test_a_ray_carves_a_cell_once_in_front_of_its_measurement(orc, sizes):
    hv = R.clone(orc, CR.volume(orc, sizes))
    rays, ranges = CV.all_rays(orc, False)
    out = CV.carve(hv, rays, ranges)
    assert len(out.ray) > 100000
    keys = np.concatenate([out.ray[:, None], out.cell], -1)
    assert len(np.unique(keys, axis=0)) == len(keys)                               # every ray carves a cell at most once
    order = np.lexsort((np.arange(len(out.ray)), out.segment))                     # the cells of a segment in walk order
    segment, cells = out.segment[order], out.cell[order]
    same = segment[1:] == segment[:-1]
    assert same.sum() > 50000 and (np.abs(cells[1:] - cells[:-1]).sum(-1)[same] == 1).all()
    # every carved cell's centre lies in front of the measurement: raw > 0
    o, n, r, _ = IR.carried(hv, rays, ranges, None, CV.R_MIN, CV.R_MAX, False)
    e = out.cell.astype(f32) + f32(0.5)
    oo, nn = o[out.ray], n[out.ray]
    raw = r[out.ray] - (((e[:, 0] - oo[:, 0]) * nn[:, 0] + (e[:, 1] - oo[:, 1]) * nn[:, 1]) + (e[:, 2] - oo[:, 2]) * nn[:, 2])
    print("least raw of a carved cell, in voxels", float(raw.min()))
    assert (raw > 0).all()


def test_the_ray_sets_reach_every_branch(orc, everything):
    hv, out = everything
    b = out.branches
    print("counts", out.counts, b)
    for name, least in (("ties", 1000), ("zero_component", 1000), ("negative_step", 1000), ("nothing_to_carve", 100),
                        ("outside_int16", 100), ("absent", 100000), ("present", 10000), ("outside_block", 100), ("straddling", 1000),
                        ("shared_voxels", 1000)):
        assert b[name] >= least, name
    assert b["cut_short"] == 0 and b["most_on_a_voxel"] >= 4096
    carved, nothing, unmeasured, invalid, cut, blocks, voxels, carves = out.counts
    assert invalid == 25 and unmeasured >= 12 and carved + nothing + unmeasured + invalid == len(CV.all_rays(orc, False)[1])
    assert carves == len(out.ray) == int(out.N.sum()) and voxels == int((out.N > 0).sum()) and blocks > 500
    # the cap reached: the scene's voxels carry a weight of 2, so a cap of 3 is met by every carved voxel that was observed
    capped = R.clone(orc, CR.volume(orc))
    low = CV.carve(capped, *CV.all_rays(orc, False), cap=3.0)
    print("cap 3", low.branches["cap_reached"], "cap 16", b["cap_reached"])
    assert low.branches["cap_reached"] > 10000 and int(capped.voxels["distance_weight"][low.N > 0].max()) == 3
    # rays cut short at a small max_blocks carve less, and say so
    short = CV.carve(R.clone(orc, CR.volume(orc)), *CV.all_rays(orc, False), max_blocks=4)
    print("max_blocks 4", short.counts)
    assert short.counts[4] > 10000 and short.counts[7] < carves and short.counts[:4] == out.counts[:4]
    assert (short.N <= out.N).all()
    # the voxel-units form carves the same map wherever / L gave the same numbers
    units = CV.carve(R.clone(orc, CR.volume(orc)), *CV.all_rays(orc, True), r_min=CV.bounds(True)[0], r_max=CV.bounds(True)[1],
                     flags=CV.VOXEL_UNITS)
    assert units.counts[3] == 25 and abs(units.counts[0] - carved) <= 2


def test_the_order_of_the_rays_changes_no_byte(orc, everything):
    hv, out = everything
    other = R.clone(orc, CR.volume(orc))
    again = CV.carve(other, *CV.permuted(*CV.all_rays(orc, False)))
    assert again.counts == out.counts and np.array_equal(again.N, out.N)
    assert other.voxels.tobytes() == hv.voxels.tobytes() and state_but_voxels(other) == state_but_voxels(hv)


def test_what_the_call_does_not_touch(orc, everything):
    hv, out = everything
    before = CR.volume(orc)
    assert state_but_voxels(hv) == state_but_voxels(before)
    assert (before.voxels["color_weight"] != 0).sum() > 1000
    assert hv.voxels["color"].tobytes() == before.voxels["color"].tobytes()
    assert np.array_equal(hv.voxels["color_weight"], before.voxels["color_weight"])
    kept = out.N == 0
    assert hv.voxels[kept].tobytes() == before.voxels[kept].tobytes()
    changed = ~kept
    assert (hv.voxels["distance_weight"][changed] > before.voxels["distance_weight"][changed]).sum() > 1000
    assert (hv.voxels["distance"][changed] >= before.voxels["distance"][changed]).all()


def test_carving_and_fusing_share_no_cell(orc):
    """the cells one ray both carves and visits in its band: at or below 1 per 1 000 rays (a rounding at a face)"""
    hv = R.clone(orc, CR.volume(orc))
    rays, ranges = IR.all_rays(orc, False)
    out = CV.carve(hv, rays, ranges)
    o, n, r, kind = IR.carried(hv, rays, ranges, None, IR.R_MIN, IR.R_MAX, False)
    fused = np.flatnonzero(kind == IR.INTEGRATED)
    who, cells = IR.walk(o[fused], n[fused], r[fused], f32(5))
    band = np.concatenate([fused[who][:, None], cells], -1)
    carved = np.concatenate([out.ray[:, None], out.cell], -1)
    both = len(band) + len(carved) - len(np.unique(np.concatenate([band, carved]), axis=0))
    print("cells both carved and fused by one ray", both, "of", len(carved), "carves by", out.counts[0], "rays")
    assert len(carved) > 50000 and both * 1000 <= out.counts[0]


def test_a_wall_that_is_no_longer_there(orc):
    rays, front, back = CV.scenario_rays()
    assert (back - front).min() >= 4 * R.TRUNCATION and back.max() < CV.R_MAX     # along every ray, and inside the depth range
    hv, counts, cast = CV.scenario(orc)
    print("counts", counts)
    assert int(hv.counters[T.VK_CTR_DROPPED]) == 0 and all(c[7] == 0 for c in counts[:2] + counts[3::2])     # no visit lost
    assert all(c[0] == len(front) and c[4] == 0 and c[7] > 100000 for c in counts[2::2])                    # every ray carved
    hit = cast.status == CR.HIT
    d = np.abs(cast.t.astype(np.float64) - back)
    print("hits %.4f" % hit.mean(), "|t - back| median %.3g m, 99th percentile %.3g m, max %.3g m"
          % (np.median(d[hit]), np.percentile(d[hit], 99), d[hit].max()))
    assert (hit & (d <= SCENARIO_BOUND)).mean() >= 0.95
    # the control: without the carves the front wall is still what a ray hits first
    _, _, still = CV.scenario(orc, carving=False)
    near = (still.status == CR.HIT) & (still.t < (front + back) / 2)
    print("control: hits nearer than the midpoint %.4f" % near.mean())
    assert near.mean() >= 0.95


def test_the_library_validates_before_touching_a_device():
    """every refusal vk.h lists, with addresses that are no memory: nothing may be enqueued (no GPU is needed, or touched)"""
    from vulcan_amd import api
    lib = api.lib()
    one, odd = C.c_void_p(4096), C.c_void_p(4096 + 8)
    assert C.sizeof(T.CarveRaysParams) == 24

    def params(flags=0, max_blocks=1024, r_min=0.1, r_max=5.0, t_from=0.0, cap=16.0):
        return T.CarveRaysParams(flags, max_blocks, r_min, r_max, t_from, cap)

    def call(v=fake_volume(), rays=one, ranges=one, count=8, pose=None, p=params(), counts=one, workspace=one):
        return lib.vk_volume_carve_rays(C.byref(v) if v else None, rays, ranges, count, pose, C.byref(p) if p else None, counts,
                                        workspace, None)

    assert call(v=None) == -1 and call(p=None) == -1 and call(counts=None) == -1 and call(workspace=None) == -1
    for field, value in (("hash_entries", None), ("voxel_length", 0.0), ("main_block_count", 0), ("voxels", (1 << 20) + 8),
                         ("truncation_length", 0.008 * 64.5)):
        broken = fake_volume()
        setattr(broken, field, value)
        assert call(v=broken) == -1, field
    for flags in (4, 7, 8, -1, 1 << 16):
        assert call(p=params(flags=flags)) == -1
    for max_blocks in (0, -1, 4097, 1 << 30):
        assert call(p=params(max_blocks=max_blocks)) == -1
    for cap in (0.5, 0.0, 32768.0, float("nan"), float("inf")):
        assert call(p=params(cap=cap)) == -1
    for r_min, r_max in ((-0.001, 5.0), (1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (0.0, float("nan")), (float("nan"), 5.0),
                         (float("-inf"), 5.0), (0.0, 0.0)):
        assert call(p=params(r_min=r_min, r_max=r_max)) == -1
    for t_from in (-0.001, float("nan"), float("inf"), float("-inf")):
        assert call(p=params(t_from=t_from)) == -1
    assert call(count=-1) == -1 and call(count=(1 << 22) + 1) == -1
    assert call(rays=None) == -1 and call(ranges=None) == -1 and call(workspace=odd) == -1
    # count == 0 launches nothing, whatever else is allowed, but is checked like any call
    for flags in (0, 1, 2, 3):
        assert call(count=0, p=params(flags=flags)) == 0
    assert call(count=0, rays=None, ranges=None) == 0 and call(count=0, p=params(max_blocks=1)) == 0
    assert call(count=0, p=params(max_blocks=4096, cap=32767.0, t_from=3.0)) == 0 and call(count=0, p=params(cap=1.0)) == 0
    assert call(count=0, counts=None) == -1 and call(count=0, workspace=None) == -1 and call(count=0, p=params(max_blocks=4097)) == -1
    assert lib.vk_volume_carve_rays_workspace_bytes(0, 0) == 0 and lib.vk_volume_carve_rays_workspace_bytes(8, -1) == 0
    assert lib.vk_volume_carve_rays_workspace_bytes(509, 96) >= 605 * (512 * 4 + 1)
