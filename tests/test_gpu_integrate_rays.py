"""vk_volume_integrate_rays on the device against its CPU statement (tests/integrate_rays_reference.py), bit for bit. The
volume starts from an uploaded oracle state, the device makes the call, and it must hold the hash entries, visibility bytes,
free list, voxel bytes, public counters and the eight counts the statement leaves on the host. What rays that share a voxel
add up is an integer and everything else is one defined sequence of float32 operations, so there is no tolerance anywhere in
this file. The ray sets are the statement's (a)-(g): the fusing camera's 160 x 120 pixel rays with the ranges cast_rays gives
them, 4 096 copies of one ray, axis-parallel and diagonal rays from lattice points, random rays, rays without a measurement,
invalid rays and rays at the end of the block coordinates; tests/test_integrate_rays_reference.py shows that they reach every
branch of the definition."""
import ctypes as C

import numpy as np
import pytest

import cast_reference as CR
import integrate_rays_reference as IR
import merge_reference as M
import release_reference as R
from gpu_support import OTHER, SAME, api, assert_same_state, device_copy, on_device, sync  # noqa: F401
from ray_call_support import RayCall
from vulcan_amd import vk_types as T

pytestmark = pytest.mark.gpu

FORMS = [0, IR.VOXEL_UNITS, IR.ONE_OBSERVATION, IR.VOXEL_UNITS | IR.ONE_OBSERVATION]
CALL = RayCall(IR.integrate, IR.all_rays, "_integrate_rays_call", "max_distance_weight", IR.keywords, voxels_only=False)
start, statement, call, both = CALL.start, CALL.statement, CALL.call, CALL.both


@pytest.mark.parametrize("target", ["scene", "fresh"])
@pytest.mark.parametrize("sizes", [SAME, OTHER], ids=["long-chains", "other-bucket-count"])
@pytest.mark.parametrize("flags", FORMS, ids=["metres", "voxel-units", "metres-one-observation", "voxel-units-one-observation"])
def test_bit_for_bit(api, orc, sizes, flags, target):
    _, hv, want = both(api, orc, sizes, target, flags)
    print(want.branches)
    integrated, unmeasured, invalid, allocated, rounds, blocks, voxels, lost = want.counts
    assert integrated > 20000 and unmeasured >= 12 and invalid == 25 and allocated > 100 and blocks > 1000 and voxels > 100000
    assert want.branches["most_on_a_voxel"] >= 4096 and want.branches["shared_voxels"] > 1000
    if target == "fresh":
        assert int(hv.voxels["distance_weight"].max()) == (1 if flags & IR.ONE_OBSERVATION else 16)


@pytest.mark.parametrize("flags", [0, IR.VOXEL_UNITS], ids=["metres", "voxel-units"])
def test_a_pose_on_the_device(api, orc, flags):
    want, with_identity, without = CALL.a_pose_on_the_device(api, orc, SAME, flags)
    assert want.counts[0] > 20000 and want.counts[6] > 100000
    assert np.array_equal(with_identity.hash_entries, without.hash_entries)


def test_allocation_limits(api, orc):
    # no round: a fixed map is updated, nothing is allocated and every visit of an absent block is lost
    _, hv, want = both(api, orc, SAME, "scene", 0, max_rounds=0)
    assert want.counts[3] == 0 and want.counts[4] == 0 and want.counts[7] > 1000 and want.counts[6] > 10000
    assert np.array_equal(hv.hash_entries, CR.volume(orc, SAME).hash_entries)
    _, _, want = both(api, orc, SAME, "fresh", 0, max_rounds=0)
    assert want.counts[3:7] == (0, 0, 0, 0)
    _, _, want = both(api, orc, OTHER, "fresh", 0, max_rounds=1)
    assert want.counts[4] == 1 and want.counts[3] > 100 and want.counts[7] > 0
    # a pool that runs dry: the handle pass's exhaustion, VK_CTR_DROPPED raised
    small = ((61, 16), (509, 4096))
    _, hv, want = both(api, orc, small, "fresh", 0)
    print("dropped", int(hv.counters[T.VK_CTR_DROPPED]))
    assert hv.counters[T.VK_CTR_DROPPED] > 0 and want.counts[3] <= 77 and want.counts[7] > 100000


def test_the_order_of_the_rays_does_not_matter(api, orc):
    hv, want = statement(orc, SAME, "scene", 0)
    rays, ranges = IR.permuted(*IR.all_rays(orc, False))
    dv = device_copy(api, start(orc, SAME, "scene"))
    assert call(dv, on_device(rays), on_device(ranges), None, 0) == want.counts
    assert_same_state(dv, hv)
    # and two calls on the same inputs leave the same bytes: nothing depends on timing
    again = device_copy(api, start(orc, SAME, "scene"))
    assert call(again, on_device(rays), on_device(ranges), None, 0) == want.counts
    sync()
    assert again.host_voxels().tobytes() == dv.host_voxels().tobytes() and np.array_equal(again.host_entries(), dv.host_entries())


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_ragged_counts(api, orc, count):
    first = 9000                                                            # pixel rays from the middle of (a)
    rays, ranges = IR.all_rays(orc, False)
    rays, ranges = rays[first:first + count + 64], ranges[first:first + count + 64]
    assert (ranges[:count] > 0).all()
    hv = start(orc, SAME, "scene")
    want = IR.integrate(hv, rays[:count], ranges[:count])
    dv = device_copy(api, start(orc, SAME, "scene"))
    got = call(dv, on_device(rays), on_device(ranges), None, 0, count=count)       # the buffers hold 64 rays more
    assert got == want.counts and got[0] == count
    assert_same_state(dv, hv)


@pytest.mark.parametrize("count", [(1 << 21) - 1, 1 << 21], ids=["one-word-sums", "two-word-sums"])
def test_both_accumulator_layouts(api, orc, count):
    """below 2^21 rays a voxel's count and sum share one 64-bit word, from there on they are two: the last count of the one
    form and the first of the other, most of the rays without a measurement, 2 000 pixel rays and the 4 096 copies with one"""
    spans = IR.spans(orc)
    rays, ranges = IR.all_rays(orc, False)
    rays = np.concatenate([rays[9000:11000], rays[spans["b"]], np.repeat(rays[9000:9001], count - 6096, axis=0)])
    ranges = np.concatenate([ranges[9000:11000], ranges[spans["b"]], np.zeros(count - 6096, dtype=np.float32)])
    hv = start(orc, SAME, "scene")
    want = IR.integrate(hv, rays, ranges)
    assert want.counts[:3] == (6096, count - 6096, 0) and want.branches["most_on_a_voxel"] >= 4096
    dv = device_copy(api, start(orc, SAME, "scene"))
    assert call(dv, on_device(rays), on_device(ranges), None, 0) == want.counts
    assert_same_state(dv, hv)


def test_what_stays_untouched(api, orc):
    before = start(orc, OTHER, "scene")
    hv, want = statement(orc, OTHER, "scene", 0)
    dv = device_copy(api, start(orc, OTHER, "scene"))
    rays, ranges = IR.all_rays(orc, False)
    rays_dev, ranges_dev = on_device(rays), on_device(ranges)
    assert call(dv, rays_dev, ranges_dev, None, 0) == want.counts
    sync()
    assert rays_dev.cpu().numpy().tobytes() == rays.tobytes() and ranges_dev.cpu().numpy().tobytes() == ranges.tobytes()
    got = R.clone(orc, hv)
    got.hash_entries[:], got.voxels[:] = dv.host_entries(), dv.host_voxels()
    was, now = R.block_voxels(before), R.block_voxels(got)
    empty = np.zeros(512, dtype=T.voxel_dtype)
    empty["distance"] = 1
    changed = 0
    for origin, data in now.items():
        old = np.frombuffer(was.get(origin, empty.tobytes()), dtype=T.voxel_dtype)
        new = np.frombuffer(data, dtype=T.voxel_dtype)
        assert new["color"].tobytes() == old["color"].tobytes() and np.array_equal(new["color_weight"], old["color_weight"])
        slot = R.find(got, origin)
        visited = want.N[slot * 512:(slot + 1) * 512] > 0
        assert new[~visited].tobytes() == old[~visited].tobytes()           # a voxel without a count keeps all its bytes
        changed += int(visited.any())
    assert changed == want.counts[5] and len(now) == len(was) + want.counts[3] and set(was) <= set(now)


def test_refusals_leave_everything_as_given(api, orc):
    import torch
    hv = start(orc, SAME, "scene")
    dv = device_copy(api, hv)
    lib = api.lib()
    rays, ranges = IR.all_rays(orc, False)
    rays, ranges = on_device(rays[:64]), on_device(ranges[:64])
    counts = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    workspace = torch.full((lib.vk_volume_integrate_rays_workspace_bytes(dv.main, dv.excess),), 0xA5, dtype=torch.uint8, device="cuda")
    sync()
    at = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731

    def params(flags=0, max_rounds=8, r_min=0.01, r_max=5.0, cap=16.0):
        return T.IntegrateRaysParams(flags, max_rounds, r_min, r_max, cap, 0)

    def integrate(v="volume", r=rays, g=ranges, count=64, p=params(), c=counts, w=workspace, w_offset=0):
        desc = dv.desc() if v == "volume" else v
        w_ptr = None if w is None else C.c_void_p(w.data_ptr() + w_offset)
        return lib.vk_volume_integrate_rays(C.byref(desc) if desc else None, at(r), at(g), count, None, C.byref(p) if p else None,
                                            at(c), w_ptr, api.stream())

    def changed(**fields):
        desc = dv.desc()
        for name, value in fields.items():
            setattr(desc, name, value)
        return desc

    assert integrate(v=None) == -1 and integrate(p=None) == -1 and integrate(c=None) == -1 and integrate(w=None) == -1
    assert integrate(v=changed(voxels=None)) == -1 and integrate(v=changed(main_block_count=0)) == -1
    assert integrate(v=changed(voxel_length=0.0)) == -1 and integrate(v=changed(voxels=dv.desc().voxels + 8)) == -1
    assert integrate(v=changed(truncation_length=65 * hv.voxel_length)) == -1
    for flags in (4, 7, -1, 1 << 16):
        assert integrate(p=params(flags=flags)) == -1
    for max_rounds in (-1, 65, 1 << 20):
        assert integrate(p=params(max_rounds=max_rounds)) == -1
    for cap in (0.5, 32768.0, float("nan"), -1.0):
        assert integrate(p=params(cap=cap)) == -1
    for r_min, r_max in ((-0.001, 5.0), (1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (0.0, float("nan")), (float("nan"), 5.0),
                         (float("-inf"), 5.0), (0.0, 0.0)):
        assert integrate(p=params(r_min=r_min, r_max=r_max)) == -1
    assert integrate(count=-1) == -1 and integrate(count=(1 << 22) + 1) == -1
    assert integrate(r=None) == -1 and integrate(g=None) == -1
    assert integrate(w_offset=8) == -1
    # count == 0 launches nothing and leaves the counters' bytes alone, but is checked like any call
    assert integrate(count=0) == 0 and integrate(count=0, r=None, g=None) == 0 and integrate(count=0, c=None) == -1
    sync()
    assert bool((counts == 0x5A5A5A5A).all()) and bool((workspace == 0xA5).all())
    assert_same_state(dv, hv)
    # the class refuses what is no float32 [N, 6] with a float32 [N], and an empty batch is no call
    with pytest.raises(api.VkError):
        dv.integrate_rays(rays.double(), ranges)
    with pytest.raises(api.VkError):
        dv.integrate_rays(rays, ranges[:5])
    assert dv.integrate_rays(rays[:0], ranges[:0]) == (0,) * 8
    assert_same_state(dv, hv)


def test_cast_then_integrate_then_cast(api, orc):
    """the device's closure: cast_rays in the scene volume, integrate_rays into a fresh volume, cast_rays there — each step
    against its CPU statement, through the class methods"""
    src = CR.volume(orc, SAME)
    rays = IR.pixel_rays()[0]
    first = CR.cast(src, rays, max_steps=500)
    hv = M.fresh(orc, *SAME[0])
    want = IR.integrate(hv, rays, first.t, r_min=0.1, flags=IR.ONE_OBSERVATION)
    second = CR.cast(hv, rays, max_steps=500)

    ds, dv = device_copy(api, src), device_copy(api, M.fresh(orc, *SAME[0]))
    rays_dev = on_device(rays)
    hits = ds.cast_rays(rays_dev, color=False)
    sync()
    assert np.array_equal(hits.t.cpu().numpy().view(np.uint32), first.t.view(np.uint32))
    assert dv.integrate_rays(rays_dev, hits.t, one_observation=True) == want.counts
    assert_same_state(dv, hv)
    again = dv.cast_rays(rays_dev, color=False)
    sync()
    assert np.array_equal(again.status.cpu().numpy(), second.status)
    assert np.array_equal(again.t.cpu().numpy().view(np.uint32), second.t.view(np.uint32))
    hit, hit_again = first.status == CR.HIT, second.status == CR.HIT
    print("hits", int(hit.sum()), "hit again", int((hit & hit_again).sum()))
    assert hit.sum() > 10000


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
    rays, ranges = IR.all_rays(orc, False)
    rays, ranges = on_device(rays[:256]), on_device(ranges[:256])
    before = (dv.host_entries(), dv.host_voxels().tobytes(), dv.read_counters())
    with pytest.raises(api.VkError):
        dv.integrate_rays(rays, ranges)
    sync()
    after = (dv.host_entries(), dv.host_voxels().tobytes(), dv.read_counters())
    for a, b in zip(before, after):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    dv.cancel_requests_ahead(rounds=3)
    assert dv.integrate_rays(rays, ranges)[0] > 0
