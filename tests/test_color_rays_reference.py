"""The CPU statement of vk_volume_color_rays (tests/color_rays_reference.py) against what any definition of the call must
give: its cell walk is integrate_rays' walk, one ray along an axis colours the cells one can count by hand, the shared ray sets
with seeded colours reach every branch, the order of the rays changes no byte, nothing but the colour and the colour weight of
visited voxels near a surface changes, and a map built from rays alone carries the colours of its rays into what cast_rays
and the mesh see. No GPU: the device is held to the same statement in tests/test_gpu_color_rays.py.

MEASURED HERE on the scenario (19 200 rays fused and coloured once, band = the truncation length): all rays hit again,
18 980 of their samples carry a colour weight; the colour difference, the largest of the three channels, against the paint at
the new hit is 0.0023 in the median, 0.0085 at the 99th percentile and 0.0130 at worst, against the ray's own colour 0.0128 at
worst. All 19 557 vertices of the mesh carry a colour, 0.0025 from the paint at the vertex in the median, 0.0095 at the 99th
percentile and 0.0158 at worst. With band = two voxels the figures at the hit are the same to four places and 18 976 samples
carry a colour weight. Asserted: twice each measured maximum, the margin for nothing more than another host libm or numpy
build."""
import ctypes as C

import numpy as np
import pytest

from abi_support import fake_volume
import cast_reference as CR
import color_rays_reference as CO
import extract_attributes_reference as A
import integrate_rays_reference as IR
import register_reference as RR
import release_reference as R
from carve_rays_reference import state_but_voxels
from vulcan_amd import vk_types as T

f32 = np.float32
CAST_BOUND = 2 * 0.0130           # |colour of the sample at the new hit - paint there|, the largest channel
OWN_BOUND = 2 * 0.0128            # |colour of the sample at the new hit - the ray's own colour|
MESH_BOUND = 2 * 0.0158           # |colour of a vertex - paint at the vertex|


def test_the_statements_walk_is_integrate_rays_walk(orc):
    """with b = tr the ends are integrate_rays' and the walk is integrate_rays_reference.walk, cell for cell"""
    hv = CR.volume(orc)
    rays, ranges = IR.all_rays(orc, False)
    o, n, r, kind = IR.carried(hv, rays, ranges, None, IR.R_MIN, IR.R_MAX, False)
    fused = kind == IR.INTEGRATED
    o, n, r, tr = o[fused], n[fused], r[fused], f32(5)
    who, cells = IR.walk(o, n, r, tr)
    mine, my_cells, _ = CO.CV.walk(o, n, *CO.ends(r, tr))
    assert len(who) > 100000 and np.array_equal(who, mine) and np.array_equal(cells, my_cells)


def one_row(band):
    """the ray +x from (0.5, 2.5, 3.5) voxels with r = 20.25, fused with tr = 5 and then coloured (0.25, 0.5, 1.0)"""
    import oracle.oracle as orc
    hv = orc.HostVolume(61, 16, voxel_length=2.0 ** -7, truncation_length=5 * 2.0 ** -7)
    rays, ranges = np.array([[0.5, 2.5, 3.5, 3.0, 0, 0]], dtype=f32), np.array([20.25], dtype=f32)
    IR.integrate(hv, rays, ranges, r_min=1.0, r_max=100.0, flags=IR.VOXEL_UNITS)
    table = RR.block_table(hv)
    assert sorted(table) == [(1, 0, 0), (2, 0, 0), (3, 0, 0)]                     # cells 15 .. 25
    before = R.clone(orc, hv)
    out = CO.color(hv, rays, ranges, np.array([[0.25, 0.5, 1.0]], dtype=f32), r_min=1.0, r_max=100.0, band=band, flags=CO.VOXEL_UNITS)
    assert state_but_voxels(hv) == state_but_voxels(before)
    assert hv.voxels["distance"].tobytes() == before.voxels["distance"].tobytes()
    assert np.array_equal(hv.voxels["distance_weight"], before.voxels["distance_weight"])
    cell = {}
    for index in range(len(hv.voxels)):
        slot, voxel = divmod(index, 512)
        origin = [o for o, s in table.items() if s == slot]
        if origin:
            assert origin[0][1:] == (0, 0)
            if voxel >> 3 == 3 * 8 + 2:                                             # the row y = 2, z = 3
                cell[8 * origin[0][0] + (voxel & 7)] = index
    coloured = {c for c, index in cell.items() if hv.voxels["color_weight"][index] != 0}
    changed = np.flatnonzero(hv.voxels.view(np.uint8).reshape(-1, 20) != before.voxels.view(np.uint8).reshape(-1, 20))
    assert len(np.unique(changed // 20)) == len(coloured) == int((hv.voxels["color_weight"] != 0).sum())
    for c in coloured:
        assert hv.voxels["color"][cell[c]].tolist() == [0.25, 0.5, 1.0] and hv.voxels["color_weight"][cell[c]] == 1
    return hv, cell, coloured, out


def test_one_ray_by_hand():
    # the measurement lies at x = 20.75; band 2: ta = 18.25 at x = 18.75, tb = 22.25 at x = 22.75
    hv, cell, coloured, out = one_row(2.0)
    assert coloured == set(range(18, 23))
    assert out.counts == (1, 0, 0, 0, 1, 5, 0, 0)                                  # all five in block (2, 0, 0)
    # band 5: the walk is the one that fused the ray, cells 15 .. 25; cell 15's centre lies 5.25 in front of the measurement,
    # its stored distance is min(1, 5.25 / 5) = 1: visited, not near a surface, refused
    hv, cell, coloured, out = one_row(5.0)
    assert hv.voxels["distance"][cell[15]] == 1 and hv.voxels["distance_weight"][cell[15]] == 1
    assert coloured == set(range(16, 26))
    assert out.counts == (1, 0, 0, 0, 2, 10, 1, 0)                                 # block (1, 0, 0) holds cell 15 alone


def seeded(orc):
    rays, ranges = IR.all_rays(orc, False)
    return rays, ranges, CO.colors_for(len(ranges))


@pytest.fixture(scope="module")
def everything(orc):
    """the statement on all sets with seeded colours into the scene volume, as the GPU tests colour them"""
    hv = R.clone(orc, CR.volume(orc))
    return hv, CO.color(hv, *seeded(orc))


def test_the_ray_sets_reach_every_branch(orc, everything):
    hv, out = everything
    b = out.branches
    print("counts", out.counts, b)
    coloured, no_colour, unmeasured, invalid, blocks, voxels, not_near, lost = out.counts
    rays, ranges, colors = seeded(orc)
    assert len(ranges) == 27597 and coloured + no_colour + unmeasured + invalid == len(ranges)
    assert invalid == 25 and unmeasured >= 12 and no_colour > 500 and coloured > 20000
    bad = ~((colors >= 0) & (colors <= 1)).all(-1)
    assert np.isnan(colors).any(-1).sum() > 100 and (colors < 0).any(-1).sum() > 100 and (colors > 1).any(-1).sum() > 100
    assert no_colour <= bad.sum() and (colors == 0).all(-1).sum() > 100 and (colors == 1).all(-1).sum() > 100
    for name, least in (("ta_clamped", 100), ("outside_int16", 100), ("lost", 10000), ("shared_voxels", 10000), ("not_near", 1000),
                        ("continued", 10000)):
        assert b[name] >= least, name
    assert b["most_on_a_voxel"] >= 3000
    assert lost == b["lost"] and voxels + not_near == int((out.N > 0).sum()) and blocks > 500
    assert b["visits"] == b["outside_int16"] + b["lost"] + int(out.N.sum())
    # Here: 26 695 rays coloured, 346 152 visits of present blocks, 45 702 lost, 165 250 voxels in 639 blocks updated, 13 105
    # not near a surface, 87 219 voxels with N >= 2, 3 977 on one voxel. Which rays lack a colour follows the seed and the
    # strides of colors_for, so the structure is asserted and not these digits.
    assert b["first_colour"] == 0                # every scene voxel near a surface has a colour: the scenario takes that branch
    # a stored colour is a mean of colours in [0, 1]
    stored = hv.voxels["color"][out.near]
    assert stored.min() >= 0 and stored.max() <= 1
    # the cap reached: the scene's voxels carry a colour weight, so a cap of 3 is met
    capped = R.clone(orc, CR.volume(orc))
    low = CO.color(capped, rays, ranges, colors, cap=3.0)
    print("cap 3", low.branches["cap_reached"], "cap 16", b["cap_reached"])
    assert low.branches["cap_reached"] > 10000 and int(capped.voxels["color_weight"][low.near].max()) == 3
    # one observation: the same voxels, a weight that grows by 1
    once = R.clone(orc, CR.volume(orc))
    single = CO.color(once, rays, ranges, colors, flags=CO.ONE_OBSERVATION)
    assert single.counts == out.counts and np.array_equal(single.N, out.N)
    before = CR.volume(orc).voxels["color_weight"][single.near]
    assert np.array_equal(once.voxels["color_weight"][single.near], np.minimum(before + 1, 16))
    # the voxel-units form colours the same map wherever / L gave the same numbers
    rays_v, ranges_v = IR.all_rays(orc, True)
    units = CO.color(R.clone(orc, CR.volume(orc)), rays_v, ranges_v, colors, r_min=IR.bounds(True)[0], r_max=IR.bounds(True)[1],
                     flags=CO.VOXEL_UNITS)
    assert units.counts[3] == 25 and abs(units.counts[0] - coloured) <= 2


def test_the_order_of_the_rays_changes_no_byte(orc, everything):
    hv, out = everything
    other = R.clone(orc, CR.volume(orc))
    again = CO.color(other, *CO.permuted(*seeded(orc)))
    assert again.counts == out.counts and np.array_equal(again.N, out.N) and np.array_equal(again.S, out.S)
    assert other.voxels.tobytes() == hv.voxels.tobytes() and state_but_voxels(other) == state_but_voxels(hv)


def test_what_the_call_does_not_touch(orc, everything):
    hv, out = everything
    before = CR.volume(orc)
    assert state_but_voxels(hv) == state_but_voxels(before)
    assert hv.voxels["distance"].tobytes() == before.voxels["distance"].tobytes()
    assert np.array_equal(hv.voxels["distance_weight"], before.voxels["distance_weight"])
    kept = np.ones(len(hv.voxels), dtype=bool)
    kept[out.near] = False
    assert (out.N[kept] > 0).sum() == out.counts[6]                              # visited, not near: kept
    assert hv.voxels[kept].tobytes() == before.voxels[kept].tobytes()
    assert (hv.voxels["color_weight"][out.near] > 0).all()
    assert (np.abs(before.voxels["distance"][out.near]) < 1).all()


def colour_error(got, want):
    return np.abs(got.astype(np.float64) - want.astype(np.float64)).max(-1)


@pytest.mark.parametrize("band", [None, CO.TWO_VOXELS], ids=["truncation-length", "two-voxels"])
def test_a_map_from_rays_has_colours(orc, band):
    rays, t, colors = CO.scenario_rays(orc)
    assert len(t) == 19200 and (t > 0.1).all() and colors.min() >= 0.1 - 1e-6 and colors.max() <= 0.9 + 1e-6
    hv, counts, cast = CO.scenario(orc, band)
    print("counts", counts)
    assert int(hv.counters[T.VK_CTR_DROPPED]) == 0 and counts[0][7] == 0
    coloured, no_colour, unmeasured, invalid, blocks, voxels, not_near, lost = counts[1]
    assert (coloured, no_colour, unmeasured, invalid, lost) == (len(t), 0, 0, 0, 0)
    assert voxels > 50000 and (not_near < 100 if band else not_near > 1000)
    hit = cast.status == CR.HIT
    carries = hit & (cast.samples["color_weight"] != 0)
    at_hit = colour_error(cast.samples["color"], CO.paint(CO.hit_points(rays, cast.t)))[carries]
    own = colour_error(cast.samples["color"], colors)[carries]
    print("hit again %d, carry a colour weight %d (%.4f)" % (hit.sum(), carries.sum(), carries.mean()))
    print("against the paint at the new hit: median %.4f, 99th percentile %.4f, max %.4f; against the ray's own colour: max %.4f"
          % (np.median(at_hit), np.percentile(at_hit, 99), at_hit.max(), own.max()))
    assert hit.all() and carries.mean() >= 0.95
    assert at_hit.max() <= CAST_BOUND and own.max() <= OWN_BOUND


def test_without_the_call_a_map_from_rays_has_no_colour(orc):
    """the control: the same sequence without color_rays leaves every sample's colour weight 0"""
    hv, counts, cast = CO.scenario(orc, coloring=False)
    assert (cast.status == CR.HIT).all() and (cast.samples["color_weight"] == 0).all()
    assert (hv.voxels["color_weight"] == 0).all()
    coloured = CO.scenario(orc)[2]
    assert np.array_equal(coloured.t, cast.t) and np.array_equal(coloured.status, cast.status)   # the surface is the same


def test_the_mesh_of_a_map_from_rays_has_colours(orc):
    hv = CO.scenario(orc)[0]
    points, faces, skipped = orc.extract_mesh(hv, True, True)
    statistics = {}
    colors, _ = A.extract_attributes(orc, hv, True, True, statistics)
    carries = (colors != 0).any(-1)                                              # the paint is nowhere (0, 0, 0)
    error = colour_error(colors, CO.paint(points))[carries]
    print("vertices %d, with a colour %d (%.4f), none by the statistics %d" % (len(points), carries.sum(), carries.mean(), statistics["color_none"]))
    print("against the paint at the vertex: median %.4f, 99th percentile %.4f, max %.4f" % (np.median(error), np.percentile(error, 99), error.max()))
    assert skipped == 0 and len(points) > 10000 and int((~carries).sum()) == statistics["color_none"]
    assert carries.mean() >= 0.95 and error.max() <= MESH_BOUND


def test_the_library_validates_before_touching_a_device():
    """every refusal vk.h lists, with addresses that are no memory: nothing may be enqueued (no GPU is needed, or touched)"""
    from vulcan_amd import api
    lib = api.lib()
    one, odd = C.c_void_p(4096), C.c_void_p(4096 + 8)
    assert C.sizeof(T.ColorRaysParams) == 24

    def params(flags=0, r_min=0.1, r_max=5.0, band=0.04, cap=16.0):
        return T.ColorRaysParams(flags, r_min, r_max, band, cap, 0)

    def call(v=fake_volume(), rays=one, ranges=one, colors=one, count=8, pose=None, p=params(), counts=one, workspace=one):
        return lib.vk_volume_color_rays(C.byref(v) if v else None, rays, ranges, colors, count, pose, C.byref(p) if p else None,
                                        counts, workspace, None)

    L = fake_volume().voxel_length
    assert call(v=None) == -1 and call(p=None) == -1 and call(counts=None) == -1 and call(workspace=None) == -1
    for field, value in (("hash_entries", None), ("voxel_length", 0.0), ("main_block_count", 0), ("voxels", (1 << 20) + 8),
                         ("truncation_length", L * 64.5)):
        broken = fake_volume()
        setattr(broken, field, value)
        assert call(v=broken) == -1, field
    for flags in (4, 7, 8, -1, 1 << 16):
        assert call(p=params(flags=flags)) == -1
    for cap in (0.5, 0.0, 32768.0, float("nan"), float("inf")):
        assert call(p=params(cap=cap)) == -1
    for r_min, r_max in ((-0.001, 5.0), (1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (0.0, float("nan")), (float("nan"), 5.0),
                         (float("-inf"), 5.0), (0.0, 0.0)):
        assert call(p=params(r_min=r_min, r_max=r_max)) == -1
    for band in (0.0, -0.01, float("nan"), float("inf"), float("-inf"), L * 64.5):
        assert call(p=params(band=band)) == -1
    assert call(p=params(flags=1, band=64.5)) == -1 and call(count=0, p=params(flags=1, band=64.0)) == 0
    assert call(count=-1) == -1 and call(count=(1 << 21) + 1) == -1
    assert call(rays=None) == -1 and call(ranges=None) == -1 and call(colors=None) == -1 and call(workspace=odd) == -1
    # count == 0 launches nothing, whatever else is allowed, but is checked like any call
    for flags in (0, 1, 2, 3):
        assert call(count=0, p=params(flags=flags)) == 0
    assert call(count=0, rays=None, ranges=None, colors=None) == 0 and call(count=0, p=params(cap=32767.0, band=L * 63)) == 0
    assert call(count=0, counts=None) == -1 and call(count=0, workspace=None) == -1 and call(count=0, p=params(band=0.0)) == -1
    assert lib.vk_volume_color_rays_workspace_bytes(0, 0) == 0 and lib.vk_volume_color_rays_workspace_bytes(8, -1) == 0
    assert lib.vk_volume_color_rays_workspace_bytes(509, 96) >= 605 * (512 * 16 + 1)
    # the pass events: five of them, or none
    assert lib.vk_volume_color_rays_time_next(None, 0) == 0 and lib.vk_volume_color_rays_time_next(None, 5) == -1
