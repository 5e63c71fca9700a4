"""vk_volume_color_rays on the device against its CPU statement (tests/color_rays_reference.py), bit for bit. The volume starts
from an uploaded oracle state, the device makes the call, and it must hold the voxel bytes and the eight counts the statement
leaves on the host — and the hash entries, visibility bytes, free list, allocation arrays and public counters it started
from, which the call must not touch. What rays that share a voxel add up are integers and everything else is one defined
sequence of float32 operations, so there is no tolerance anywhere in this file. The ray sets are integrate_rays' (a)-(g) with
color_rays_reference.colors_for's seeded colours; tests/test_color_rays_reference.py shows that they reach every branch of
the definition but a voxel's first colour, which the scenario reaches."""
import ctypes as C

import numpy as np
import pytest

import cast_reference as CR
import color_rays_reference as CO
import extract_attributes_reference as A
import integrate_rays_reference as IR
import merge_reference as M
import release_reference as R
from gpu_support import OTHER, SAME, api, assert_same_state, assert_volume_equal, device_copy, on_device, sync  # noqa: F401
from ray_call_support import RayCall
from vulcan_amd import vk_types as T

pytestmark = pytest.mark.gpu

FORMS = [0, CO.VOXEL_UNITS, CO.ONE_OBSERVATION, CO.VOXEL_UNITS | CO.ONE_OBSERVATION]
ONE_VOXEL, TWO_VOXELS = float(np.float32(R.VOXEL)), CO.TWO_VOXELS
all_rays = CO.all_rays
CALL = RayCall(CO.color, all_rays, "_color_rays_call", "max_color_weight", CO.keywords, voxels_only=True)
start, statement, call, both = CALL.start, CALL.statement, CALL.call, CALL.both


@pytest.mark.parametrize("target", ["scene", "fresh"])
@pytest.mark.parametrize("sizes", [SAME, OTHER], ids=["long-chains", "other-bucket-count"])
@pytest.mark.parametrize("flags", FORMS, ids=["metres", "voxel-units", "metres-one-observation", "voxel-units-one-observation"])
def test_bit_for_bit(api, orc, sizes, flags, target):
    _, hv, want = both(api, orc, sizes, target, flags)
    print(want.branches)
    coloured, no_colour, unmeasured, invalid, blocks, voxels, not_near, lost = want.counts
    assert coloured > 20000 and no_colour > 500 and unmeasured >= 12 and invalid == 25
    if target == "fresh":                             # nothing exists: nothing changes, and every visit is lost
        assert (blocks, voxels, not_near) == (0, 0, 0) and lost == want.branches["visits"] - want.branches["outside_int16"] > 300000
        assert hv.voxels.tobytes() == start(orc, sizes, target).voxels.tobytes()
    else:
        assert blocks > 500 and voxels > 100000 and not_near > 1000 and lost > 10000
        assert want.branches["most_on_a_voxel"] >= 3000 and want.branches["shared_voxels"] > 10000


def test_the_cap_reached(api, orc):
    _, hv, want = both(api, orc, SAME, "scene", 0, cap=3.0)
    assert want.branches["cap_reached"] > 10000 and int(hv.voxels["color_weight"][want.near].max()) == 3


@pytest.mark.parametrize("flags", [0, CO.VOXEL_UNITS], ids=["metres", "voxel-units"])
def test_a_pose_on_the_device(api, orc, flags):
    want, _, _ = CALL.a_pose_on_the_device(api, orc, SAME, flags)
    assert want.counts[0] > 20000 and want.counts[5] > 10000


@pytest.mark.parametrize("band", [ONE_VOXEL, TWO_VOXELS, None], ids=["one-voxel", "two-voxels", "truncation-length"])
def test_the_band(api, orc, band):
    _, _, want = both(api, orc, SAME, "scene", 0, band=band)
    _, full = statement(orc, SAME, "scene", 0)
    print("band", band, "visits", want.branches["visits"], "of", full.branches["visits"])
    assert want.counts[:4] == full.counts[:4] and 10000 < want.counts[5] <= full.counts[5]
    assert band is None or want.branches["visits"] < full.branches["visits"]


def test_the_order_of_the_rays_does_not_matter(api, orc):
    hv, want = statement(orc, SAME, "scene", 0)
    rays, ranges, colors = CO.permuted(*all_rays(orc, False))
    dv = device_copy(api, start(orc, SAME, "scene"))
    assert call(dv, on_device(rays), on_device(ranges), on_device(colors), None, 0) == want.counts
    assert_same_state(dv, hv)
    # and two calls from the same start state leave the same bytes: nothing depends on timing
    again = device_copy(api, start(orc, SAME, "scene"))
    assert call(again, on_device(rays), on_device(ranges), on_device(colors), None, 0) == want.counts
    sync()
    assert again.host_voxels().tobytes() == dv.host_voxels().tobytes() and np.array_equal(again.host_entries(), dv.host_entries())


def hitting(orc, count, extra=0):
    """`count` + `extra` rays from the middle of (a) that hit, with their ranges and seeded colours that are colours"""
    rays, ranges = IR.pixel_hits(orc)
    hit = np.flatnonzero(ranges > 0)
    hit = hit[len(hit) // 2:][:count + extra]
    colors = np.random.default_rng(29).uniform(0, 1, (count + extra, 3)).astype(np.float32)
    return np.ascontiguousarray(rays[hit]), np.ascontiguousarray(ranges[hit]), colors


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_ragged_counts(api, orc, count):
    rays, ranges, colors = hitting(orc, count, 64)
    hv = start(orc, SAME, "scene")
    want = CO.color(hv, rays[:count], ranges[:count], colors[:count])
    dv = device_copy(api, start(orc, SAME, "scene"))
    got = call(dv, on_device(rays), on_device(ranges), on_device(colors), None, 0, count=count)    # the buffers hold 64 rays more
    assert got == want.counts and got[0] == count and got[5] > 0
    assert_same_state(dv, hv)


def test_the_fields_do_not_carry(api, orc):
    """2^21 copies of one hitting ray with the colour (1, 1, 1): every sum of a visited voxel reaches 2^31 and its N 2^21, the
    most a call can bring, and neither carries into the field above it. The statement of k copies of a ray is k times the
    S and N of one, folded."""
    copies = 1 << 21
    ray, distance, _ = hitting(orc, 1)
    white = np.ones((1, 3), dtype=np.float32)
    one = CO.color(start(orc, SAME, "scene"), ray, distance, white, band=TWO_VOXELS)
    assert one.counts[0] == 1 and 3 <= int(one.N.sum()) <= 12 and int(one.N.max()) == 1 and (one.S[one.N > 0] == 1024).all()
    hv = start(orc, SAME, "scene")
    want = CO.Result()
    want.branches = {}
    CO.fold(hv, want, one.S * copies, one.N * copies, (copies, 0, 0, 0), one.branches["lost"] * copies, 16.0, False)
    assert int(want.S.max()) == 1 << 31 and int(want.N.max()) == 1 << 21 and want.counts[5] >= 3
    assert (hv.voxels["color_weight"][want.near] == 16).all()
    dv = device_copy(api, start(orc, SAME, "scene"))
    got = call(dv, on_device(np.repeat(ray, copies, axis=0)), on_device(np.repeat(distance, copies)),
               on_device(np.repeat(white, copies, axis=0)), None, 0, band=TWO_VOXELS)
    print("counts", got, want.counts)
    assert got == want.counts
    assert_same_state(dv, hv)


def test_inputs_and_refusals(api, orc):
    import torch
    hv = start(orc, SAME, "scene")
    dv = device_copy(api, hv)
    lib = api.lib()
    rays, ranges, colors = hitting(orc, 64)
    rays_dev, ranges_dev, colors_dev = on_device(rays), on_device(ranges), on_device(colors)
    counts = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    workspace = torch.full((lib.vk_volume_color_rays_workspace_bytes(dv.main, dv.excess),), 0xA5, dtype=torch.uint8, device="cuda")
    sync()
    at = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731

    def params(flags=0, r_min=0.01, r_max=5.0, band=0.04, cap=16.0):
        return T.ColorRaysParams(flags, r_min, r_max, band, cap, 0)

    def color(v="volume", r=rays_dev, g=ranges_dev, k=colors_dev, count=64, p=params(), c=counts, w=workspace, w_offset=0):
        desc = dv.desc() if v == "volume" else v
        w_ptr = None if w is None else C.c_void_p(w.data_ptr() + w_offset)
        return lib.vk_volume_color_rays(C.byref(desc) if desc else None, at(r), at(g), at(k), count, None, C.byref(p) if p else None,
                                        at(c), w_ptr, api.stream())

    def changed(**fields):
        desc = dv.desc()
        for name, value in fields.items():
            setattr(desc, name, value)
        return desc

    assert color(v=None) == -1 and color(p=None) == -1 and color(c=None) == -1 and color(w=None) == -1
    assert color(v=changed(voxels=None)) == -1 and color(v=changed(main_block_count=0)) == -1
    assert color(v=changed(voxel_length=0.0)) == -1 and color(v=changed(voxels=dv.desc().voxels + 8)) == -1
    assert color(v=changed(truncation_length=65 * hv.voxel_length)) == -1
    for flags in (4, 7, -1, 1 << 16):
        assert color(p=params(flags=flags)) == -1
    for cap in (0.5, 32768.0, float("nan"), -1.0):
        assert color(p=params(cap=cap)) == -1
    for r_min, r_max in ((-0.001, 5.0), (1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (0.0, float("nan")), (float("nan"), 5.0),
                         (float("-inf"), 5.0), (0.0, 0.0)):
        assert color(p=params(r_min=r_min, r_max=r_max)) == -1
    for band in (0.0, -0.001, float("nan"), float("inf"), 64.5 * hv.voxel_length):
        assert color(p=params(band=band)) == -1
    assert color(p=params(flags=CO.VOXEL_UNITS, band=64.5)) == -1
    assert color(count=-1) == -1 and color(count=(1 << 21) + 1) == -1
    assert color(r=None) == -1 and color(g=None) == -1 and color(k=None) == -1
    assert color(w_offset=8) == -1
    # count == 0 launches nothing and leaves the counts alone, but is checked like any call
    assert color(count=0) == 0 and color(count=0, r=None, g=None, k=None) == 0 and color(count=0, c=None) == -1
    sync()
    assert bool((counts == 0x5A5A5A5A).all()) and bool((workspace == 0xA5).all())
    assert_same_state(dv, hv)
    # the class refuses what is no float32 [N, 6] with a float32 [N] and a float32 [N, 3], and an empty batch is no call
    with pytest.raises(api.VkError):
        dv.color_rays(rays_dev.double(), ranges_dev, colors_dev)
    with pytest.raises(api.VkError):
        dv.color_rays(rays_dev, ranges_dev[:5], colors_dev)
    with pytest.raises(api.VkError):
        dv.color_rays(rays_dev, ranges_dev, colors_dev[:5])
    with pytest.raises(api.VkError):
        dv.color_rays(rays_dev, ranges_dev, rays_dev)
    assert dv.color_rays(rays_dev[:0], ranges_dev[:0], colors_dev[:0]) == (0,) * 8
    assert_same_state(dv, hv)
    # a call that colours leaves its inputs as they were
    got = dv.color_rays(rays_dev, ranges_dev, colors_dev, r_min=0.01)
    sync()
    assert got[0] == 64 and got[5] > 0
    assert rays_dev.cpu().numpy().tobytes() == rays.tobytes() and ranges_dev.cpu().numpy().tobytes() == ranges.tobytes()
    assert colors_dev.cpu().numpy().tobytes() == colors.tobytes()


@pytest.mark.parametrize("band", [None, TWO_VOXELS], ids=["truncation-length", "two-voxels"])
def test_a_map_from_rays_has_colours(api, orc, band):
    """the scenario of tests/test_color_rays_reference.py through the class methods: every call's counts, the volume, what
    cast_rays sees and the coloured mesh at the end equal the CPU run bit for bit"""
    hv, counts, want = CO.scenario(orc, band)
    rays, t, colors = CO.scenario_rays(orc)
    rays_dev, t_dev, colors_dev = on_device(rays), on_device(t), on_device(colors)
    dv = device_copy(api, M.fresh(orc, *CO.SIZES))
    got = [dv.integrate_rays(rays_dev, t_dev, one_observation=True), dv.color_rays(rays_dev, t_dev, colors_dev, band=band, one_observation=True)]
    assert got == counts
    assert_same_state(dv, hv)
    hits = dv.cast_rays(rays_dev)
    sync()
    assert np.array_equal(hits.status.cpu().numpy(), want.status)
    assert np.array_equal(hits.t.cpu().numpy().view(np.uint32), want.t.view(np.uint32))
    assert hits.samples.cpu().numpy().tobytes() == want.samples.tobytes()
    assert (want.status == CR.HIT).all() and (want.samples["color_weight"] != 0).mean() >= 0.95
    ex = api.Extractor(dv)
    ex.all_allocated, ex.interpolate = True, True
    mesh = ex.extract(colors=True)
    sync()
    want_points, want_faces, _ = orc.extract_mesh(hv, True, True)
    want_colors, _ = A.extract_attributes(orc, hv, True, True)
    got_points, got_faces = mesh.host()
    got_colors, _ = mesh.host_attributes()
    assert len(want_points) > 10000 and np.array_equal(got_points.view(np.uint32), want_points.view(np.uint32))
    assert np.array_equal(got_faces, want_faces)
    assert np.array_equal(np.ascontiguousarray(got_colors).view(np.uint32), np.ascontiguousarray(want_colors).view(np.uint32))


def test_the_visible_list_survives(api, orc):
    """set_view, color_rays, then a colour integration of the same view: the statement with no SetView in between"""
    hv = M.view_state(orc, "a", 509, 4096)
    dv = device_copy(api, hv)
    hf = M.frame_at(orc, 25, color=np.random.default_rng(3).random((R.H, R.W, 3), dtype=np.float32))
    df = api.Frame(hf.depth, hf.depth_projection, hf.depth_to_world, color=hf.color)
    for _ in range(3):
        hv.set_view(hf, orc.POLICY_MAXKEY)
    dv.set_view(df, rounds=3)
    # rays that end on what view "a" fused: its own pixel rays with the ranges the statement of cast_rays gives them
    rays = IR.pixel_rays()[0]
    ranges = CR.cast(hv, rays).t
    colors = CO.colors_for(len(ranges))
    want = CO.color(hv, rays, ranges, colors, r_min=0.1)
    got = dv.color_rays(on_device(rays), on_device(ranges), on_device(colors))
    print("counts", got)
    assert got == want.counts and got[5] > 10000
    assert dv.requests_ahead is None or dv.requests_ahead.valid == 0
    orc.integrate_depth(hv, hf)                       # ColorIntegrator::Integrate is both passes (color_integrator.cu:144-148)
    orc.integrate_color(hv, hf)
    api.ColorIntegrator(dv).integrate(df)
    assert_volume_equal(dv, hv)


def test_refused_while_a_frame_is_announced(api, orc):
    hv = M.view_state(orc, "a", 509, 4096)
    dv = device_copy(api, hv)
    hf = R.frame_at(orc, 25)
    dv.set_view(api.Frame(hf.depth, hf.depth_projection, hf.depth_to_world), rounds=3)
    out = api.Frame(np.zeros((R.H, R.W), np.float32), hf.depth_projection, hf.depth_to_world)
    nf = R.frame_at(orc, 12)
    api.Tracer(dv).trace(out, next_frame=api.Frame(nf.depth, nf.depth_projection, nf.depth_to_world))
    sync()
    assert dv.requests_ahead is not None and dv.requests_ahead.valid == 1
    rays, ranges, colors = all_rays(orc, False)
    rays, ranges, colors = on_device(rays[:256]), on_device(ranges[:256]), on_device(colors[:256])
    before = (dv.host_entries(), dv.host_voxels().tobytes(), dv.read_counters())
    with pytest.raises(api.VkError):
        dv.color_rays(rays, ranges, colors)
    sync()
    after = (dv.host_entries(), dv.host_voxels().tobytes(), dv.read_counters())
    for a, b in zip(before, after):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    dv.cancel_requests_ahead(rounds=3)
    assert dv.color_rays(rays, ranges, colors)[0] > 0
