"""vk_volume_carve_rays on the device against its CPU statement (tests/carve_rays_reference.py), bit for bit. The volume starts
from an uploaded oracle state, the device makes the call, and it must hold the voxel bytes and the eight counts the statement
leaves on the host — and the hash entries, visibility bytes, free list, allocation arrays and public counters it started
from, which the call must not touch. What rays that share a voxel add up is a count and everything else is one defined
sequence of float32 operations, so there is no tolerance anywhere in this file. The ray sets are integrate_rays' (a)-(g) and
(h), the scene's pixel rays with ranges beyond the fused surface; tests/test_carve_rays_reference.py shows that they reach
every branch of the definition."""
import ctypes as C

import numpy as np
import pytest

import carve_rays_reference as CV
import cast_reference as CR
import integrate_rays_reference as IR
import merge_reference as M
import release_reference as R
from gpu_support import OTHER, SAME, api, assert_same_state, assert_volume_equal, device_copy, on_device, sync  # noqa: F401
from ray_call_support import RayCall
from vulcan_amd import vk_types as T

pytestmark = pytest.mark.gpu

FORMS = [0, CV.VOXEL_UNITS, CV.ONE_OBSERVATION, CV.VOXEL_UNITS | CV.ONE_OBSERVATION]
CALL = RayCall(CV.carve, CV.all_rays, "_carve_rays_call", "max_distance_weight", CV.keywords, voxels_only=True)
start, statement, call, both = CALL.start, CALL.statement, CALL.call, CALL.both


@pytest.mark.parametrize("target", ["scene", "fresh"])
@pytest.mark.parametrize("sizes", [SAME, OTHER], ids=["long-chains", "other-bucket-count"])
@pytest.mark.parametrize("flags", FORMS, ids=["metres", "voxel-units", "metres-one-observation", "voxel-units-one-observation"])
def test_bit_for_bit(api, orc, sizes, flags, target):
    _, hv, want = both(api, orc, sizes, target, flags)
    print(want.branches)
    carved, nothing, unmeasured, invalid, cut, blocks, voxels, carves = want.counts
    assert carved > 40000 and nothing > 100 and unmeasured >= 12 and invalid == 25 and cut == 0
    if target == "fresh":                                                  # nothing exists: nothing is carved, nothing changes
        assert (blocks, voxels, carves) == (0, 0, 0)
        assert hv.voxels.tobytes() == start(orc, sizes, target).voxels.tobytes()
    else:
        assert blocks > 500 and voxels > 100000 and carves > voxels
        assert want.branches["most_on_a_voxel"] >= 4096 and want.branches["shared_voxels"] > 1000


def test_the_cap_reached(api, orc):
    _, hv, want = both(api, orc, SAME, "scene", 0, cap=3.0)
    assert want.branches["cap_reached"] > 10000 and int(hv.voxels["distance_weight"][want.N > 0].max()) == 3


@pytest.mark.parametrize("flags", [0, CV.VOXEL_UNITS], ids=["metres", "voxel-units"])
def test_a_pose_on_the_device(api, orc, flags):
    want, _, _ = CALL.a_pose_on_the_device(api, orc, SAME, flags)
    assert want.counts[0] > 40000 and want.counts[6] > 10000


@pytest.mark.parametrize("max_blocks", [1, 2, 12])
def test_rays_cut_short(api, orc, max_blocks):
    _, _, want = both(api, orc, SAME, "scene", 0, max_blocks=max_blocks)
    _, full = statement(orc, SAME, "scene", 0)
    print("cut short", want.counts[4], "of", want.counts[0], "carves", want.counts[7], "of", full.counts[7])
    assert 1000 < want.counts[4] < want.counts[0] and want.counts[7] < full.counts[7]
    assert want.counts[:4] == full.counts[:4]


def test_a_carve_that_starts_beyond_every_band(api, orc):
    # every te lies below r_max - tr: nothing is carved and the volume is unchanged
    _, hv, want = both(api, orc, SAME, "scene", 0, t_from=5.0)
    assert want.counts[0] == 0 and want.counts[1] > 40000 and want.counts[4:] == (0, 0, 0, 0)
    assert hv.voxels.tobytes() == start(orc, SAME, "scene").voxels.tobytes()
    # and one that starts in the middle of the rays carves less than one from the origin
    _, _, part = both(api, orc, SAME, "scene", 0, t_from=1.0)
    assert 0 < part.counts[7] < statement(orc, SAME, "scene", 0)[1].counts[7]


def test_the_order_of_the_rays_does_not_matter(api, orc):
    hv, want = statement(orc, SAME, "scene", 0)
    rays, ranges = CV.permuted(*CV.all_rays(orc, False))
    dv = device_copy(api, start(orc, SAME, "scene"))
    assert call(dv, on_device(rays), on_device(ranges), None, 0) == want.counts
    assert_same_state(dv, hv)
    # and two calls from the same start state leave the same bytes: nothing depends on timing
    again = device_copy(api, start(orc, SAME, "scene"))
    assert call(again, on_device(rays), on_device(ranges), None, 0) == want.counts
    sync()
    assert again.host_voxels().tobytes() == dv.host_voxels().tobytes() and np.array_equal(again.host_entries(), dv.host_entries())


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_ragged_counts(api, orc, count):
    first = CV.spans(orc)["h"].start + 9000                                 # rays from the middle of (h): they pass the surface
    rays, ranges = CV.all_rays(orc, False)
    rays, ranges = rays[first:first + count + 64], ranges[first:first + count + 64]
    assert (ranges[:count] > 0).all()
    hv = start(orc, SAME, "scene")
    want = CV.carve(hv, rays[:count], ranges[:count])
    dv = device_copy(api, start(orc, SAME, "scene"))
    got = call(dv, on_device(rays), on_device(ranges), None, 0, count=count)       # the buffers hold 64 rays more
    assert got == want.counts and got[0] == count and got[7] > 0
    assert_same_state(dv, hv)


def test_inputs_and_refusals(api, orc):
    import torch
    hv = start(orc, SAME, "scene")
    dv = device_copy(api, hv)
    lib = api.lib()
    rays, ranges = CV.all_rays(orc, False)
    at_h = CV.spans(orc)["h"].start + 9000
    rays, ranges = rays[at_h:at_h + 64], ranges[at_h:at_h + 64]
    rays_dev, ranges_dev = on_device(rays), on_device(ranges)
    counts = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    workspace = torch.full((lib.vk_volume_carve_rays_workspace_bytes(dv.main, dv.excess),), 0xA5, dtype=torch.uint8, device="cuda")
    sync()
    at = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731

    def params(flags=0, max_blocks=1024, r_min=0.01, r_max=5.0, t_from=0.0, cap=16.0):
        return T.CarveRaysParams(flags, max_blocks, r_min, r_max, t_from, cap)

    def carve(v="volume", r=rays_dev, g=ranges_dev, count=64, p=params(), c=counts, w=workspace, w_offset=0):
        desc = dv.desc() if v == "volume" else v
        w_ptr = None if w is None else C.c_void_p(w.data_ptr() + w_offset)
        return lib.vk_volume_carve_rays(C.byref(desc) if desc else None, at(r), at(g), count, None, C.byref(p) if p else None,
                                        at(c), w_ptr, api.stream())

    def changed(**fields):
        desc = dv.desc()
        for name, value in fields.items():
            setattr(desc, name, value)
        return desc

    assert carve(v=None) == -1 and carve(p=None) == -1 and carve(c=None) == -1 and carve(w=None) == -1
    assert carve(v=changed(voxels=None)) == -1 and carve(v=changed(main_block_count=0)) == -1
    assert carve(v=changed(voxel_length=0.0)) == -1 and carve(v=changed(voxels=dv.desc().voxels + 8)) == -1
    assert carve(v=changed(truncation_length=65 * hv.voxel_length)) == -1
    for flags in (4, 7, -1, 1 << 16):
        assert carve(p=params(flags=flags)) == -1
    for max_blocks in (0, -1, 4097, 1 << 20):
        assert carve(p=params(max_blocks=max_blocks)) == -1
    for cap in (0.5, 32768.0, float("nan"), -1.0):
        assert carve(p=params(cap=cap)) == -1
    for r_min, r_max in ((-0.001, 5.0), (1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (0.0, float("nan")), (float("nan"), 5.0),
                         (float("-inf"), 5.0), (0.0, 0.0)):
        assert carve(p=params(r_min=r_min, r_max=r_max)) == -1
    for t_from in (-0.001, float("nan"), float("inf")):
        assert carve(p=params(t_from=t_from)) == -1
    assert carve(count=-1) == -1 and carve(count=(1 << 22) + 1) == -1
    assert carve(r=None) == -1 and carve(g=None) == -1
    assert carve(w_offset=8) == -1
    # count == 0 launches nothing and leaves the counts alone, but is checked like any call
    assert carve(count=0) == 0 and carve(count=0, r=None, g=None) == 0 and carve(count=0, c=None) == -1
    sync()
    assert bool((counts == 0x5A5A5A5A).all()) and bool((workspace == 0xA5).all())
    assert_same_state(dv, hv)
    # the class refuses what is no float32 [N, 6] with a float32 [N], and an empty batch is no call
    with pytest.raises(api.VkError):
        dv.carve_rays(rays_dev.double(), ranges_dev)
    with pytest.raises(api.VkError):
        dv.carve_rays(rays_dev, ranges_dev[:5])
    assert dv.carve_rays(rays_dev[:0], ranges_dev[:0]) == (0,) * 8
    assert_same_state(dv, hv)
    # a call that carves leaves its inputs as they were
    got = dv.carve_rays(rays_dev, ranges_dev, r_min=0.01)
    sync()
    assert got[0] == 64 and got[7] > 0
    assert rays_dev.cpu().numpy().tobytes() == rays.tobytes() and ranges_dev.cpu().numpy().tobytes() == ranges.tobytes()


def test_a_wall_that_is_no_longer_there(api, orc):
    """the scenario of tests/test_carve_rays_reference.py through the class methods: every call's counts, the volume and
    what cast_rays sees at the end equal the CPU run bit for bit"""
    hv, counts, want = CV.scenario(orc)
    rays, front, back = CV.scenario_rays()
    rays_dev, front_dev, back_dev = on_device(rays), on_device(front), on_device(back)
    dv = device_copy(api, M.fresh(orc, *CV.SIZES))
    got = [dv.integrate_rays(rays_dev, front_dev, one_observation=True)]
    for _ in range(CV.REPEATS):
        got.append(dv.integrate_rays(rays_dev, back_dev, one_observation=True))
        got.append(dv.carve_rays(rays_dev, back_dev, one_observation=True))
    assert got == counts
    assert_same_state(dv, hv)
    hits = dv.cast_rays(rays_dev, color=False)
    sync()
    assert np.array_equal(hits.status.cpu().numpy(), want.status)
    assert np.array_equal(hits.t.cpu().numpy().view(np.uint32), want.t.view(np.uint32))
    assert (want.status == CR.HIT).mean() >= 0.95 and (np.abs(want.t - back)[want.status == CR.HIT] < 0.02).all()


def test_the_visible_list_survives(api, orc):
    """set_view, carve_rays, then an integration of the same view: the statement with no SetView in between"""
    hv = M.view_state(orc, "a", 509, 4096)
    dv = device_copy(api, hv)
    hf = R.frame_at(orc, 25)
    df = api.Frame(hf.depth, hf.depth_projection, hf.depth_to_world)
    for _ in range(3):
        hv.set_view(hf, orc.POLICY_MAXKEY)
    dv.set_view(df, rounds=3)
    # rays that pass through what view "a" fused: its own pixel rays, measured well behind the ripple
    rays = IR.pixel_rays()[0]
    ranges = np.full(len(rays), 2.5, dtype=np.float32)
    want = CV.carve(hv, rays, ranges, r_min=0.1)
    got = dv.carve_rays(on_device(rays), on_device(ranges))
    print("counts", got)
    assert got == want.counts and got[7] > 100000
    assert dv.requests_ahead is None or dv.requests_ahead.valid == 0
    orc.integrate_depth(hv, hf)
    api.DepthIntegrator(dv).integrate(df)
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
    rays, ranges = CV.all_rays(orc, False)
    rays, ranges = on_device(rays[:256]), on_device(ranges[:256])
    before = (dv.host_entries(), dv.host_voxels().tobytes(), dv.read_counters())
    with pytest.raises(api.VkError):
        dv.carve_rays(rays, ranges)
    sync()
    after = (dv.host_entries(), dv.host_voxels().tobytes(), dv.read_counters())
    for a, b in zip(before, after):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    dv.cancel_requests_ahead(rounds=3)
    assert dv.carve_rays(rays, ranges)[0] > 0
