"""The CPU statement of vk_volume_cast_rays (tests/cast_reference.py) against what any definition of the call must give: the
fusing camera's pixel rays hit where the reference's raycast says, each hit carries vk_volume_sample's sample, a back face is
not reported, bounds on t and on the steps end a ray as MISS and STEPS, and the shared ray sets reach every outcome and every
branch of the march. No GPU: the device is held to the same statement in tests/test_gpu_cast.py."""
import ctypes as C

import numpy as np
import pytest

from abi_support import fake_volume
import cast_reference as CR
import merge_reference as M
import register_reference as RR
import sample_reference as S
from vulcan_amd import vk_types as T

f32 = np.float32
# |t (n . optical axis) - the oracle's raycast depth| over the pixels both hit, in metres. Measured on the 80x60 grid:
# 0.0232 at worst, 99th percentile 0.00963, all of it on the rim of the image, where the reference's trilinear sample blends
# in the unobserved voxels beside the observed region (distance 1, it does not look at weights; the statement's sample
# needs every USED voxel observed). Three grid pixels in from the rim: 1.92e-4 at worst, 99th percentile 1.18e-4, median
# 1.0e-5 — both marches end with the same two refinement steps, but from different last steps. Asserted: twice the measured
# maxima, the margin for nothing more than another host libm or numpy build.
DEPTH_BOUND, INNER_DEPTH_BOUND = 2 * 0.0232, 2 * 1.92e-4


@pytest.fixture(scope="module")
def hv(orc):
    return CR.volume(orc)


@pytest.fixture(scope="module")
def pixels(orc, hv):
    """the statement on set (a)"""
    return CR.cast(hv, CR.ray_sets(orc, False)["a"])


@pytest.fixture(scope="module")
def everything(orc, hv):
    """the statement on all sets, as the GPU tests cast them"""
    return CR.cast(hv, CR.all_rays(orc, False))


def test_pixel_rays_hit_from_the_free_side_with_the_samples_of_their_hits(orc, hv, pixels):
    hit = pixels.status == CR.HIT
    print("rays", len(hit), "hits", int(hit.sum()), "steps at most", int(pixels.steps.max()))
    assert hit.sum() > 1000
    assert pixels.armed[hit].all()                                     # armed by an observed positive value
    assert (pixels.t[hit] > 0).all() and not pixels.t[~hit].any()
    at = pixels.origin[hit] + pixels.t_voxels[hit, None] * pixels.direction[hit]
    samples, gradients = S.sample(hv, at, voxel_units=True)
    assert pixels.samples[hit].tobytes() == samples.tobytes()
    assert pixels.gradients[hit].tobytes() == gradients.tobytes()
    assert (samples["distance_weight"] != 0).sum() > 1000 and (gradients[:, 3] != 0).sum() > 1000
    # the hit lies on the zero set: within the README's TSDF tolerance where the second refinement step found a sample
    print("worst |D| at a hit", float(np.abs(samples["distance"][samples["distance_weight"] != 0]).max()))


def test_it_agrees_with_the_reference_raycast(orc, hv, pixels):
    """the oracle's trace of the same volume at the fusing view, on the pixels of (a)"""
    frame = CR.fusing_frame(orc)
    depth = orc.trace(hv, frame)[0]
    _, xs, ys = CR.pixel_rays()
    depth = depth[ys, xs]
    seen, hit = depth > 0, pixels.status == CR.HIT
    lost = seen & ~hit
    print("oracle depth > 0 at", int(seen.sum()), "of", len(seen), "; not a hit of the statement:", int(lost.sum()))
    assert seen.sum() > 1000
    assert lost.sum() <= 0.05 * seen.sum()
    both = seen & hit
    along_axis = pixels.t[both] * pixels.direction[both, 2]            # the camera looks down +z of the volume's frame
    error = np.abs(along_axis.astype(np.float64) - depth[both])
    print("pixels both hit", int(both.sum()), "max |dz| %.3g m, 99th percentile %.3g m" % (error.max(), np.percentile(error, 99)))
    assert error.max() <= DEPTH_BOUND
    inner = (both & (xs >= 3 * CR.GRID) & (xs < RR.W - 3 * CR.GRID) & (ys >= 3 * CR.GRID) & (ys < RR.H - 3 * CR.GRID))[both]
    print("three grid pixels in from the rim:", int(inner.sum()), "max |dz| %.3g m, 99th percentile %.3g m, median %.3g m"
          % (error[inner].max(), np.percentile(error[inner], 99), np.median(error[inner])))
    assert inner.sum() > 1000 and error[inner].max() <= INNER_DEPTH_BOUND


def test_a_back_face_is_not_reported(orc, hv, pixels):
    sets = CR.ray_sets(orc, True)
    twins = CR.cast(hv, sets["b"], voxel_units=True, t_max=CR.bounds(True)[1])
    assert len(sets["b"]) == (pixels.status == CR.HIT).sum()
    hit = twins.status == CR.HIT
    print("twins", len(hit), "hit", int(hit.sum()), np.bincount(twins.status, minlength=4))
    # the surface lies 3 voxels back along the twin: nothing is reported there (or before it), a voxel of margin beyond
    assert not (hit & (twins.t_voxels < 4.0)).any()
    # they start behind the surface, walk out through it unarmed and are armed in the free space in front of it
    assert twins.armed.all() and twins.branches["behind_steps"] > 1000


def test_rays_that_cannot_hit(orc, hv):
    sets = CR.ray_sets(orc, False)
    away = CR.cast(hv, sets["e"])
    assert (away.status == CR.MISS).all() and away.branches["present"] == 0 and away.branches["absent"] > 0
    bad = CR.cast(hv, sets["f"])
    assert len(bad.status) == 25 and (bad.status == CR.INVALID).all()
    for pose in (None, T.Transform.identity()):
        assert (CR.cast(hv, CR.ray_sets(orc, True)["f"], pose=pose, voxel_units=True, t_max=625.0).status == CR.INVALID).all()
    for result in (away, bad):
        assert not result.t.any() and (result.samples["distance"] == 1).all() and not result.samples["distance_weight"].any()
        assert not result.gradients.any() and not result.samples["color"].any()


def test_the_bounds_end_a_ray(orc, hv, pixels):
    rays = CR.ray_sets(orc, False)["a"]
    hit = pixels.status == CR.HIT
    short = CR.cast(hv, rays, t_max=np.where(hit, pixels.t / f32(2), f32(1)))
    assert (short.status[hit] == CR.MISS).all() and not short.t.any()
    one = CR.cast(hv, rays, max_steps=1)
    assert (one.status[hit] == CR.STEPS).all() and not one.t.any()
    # a t_min behind the surface: the ray starts unarmed inside the wall and reports nothing it did not cross from the front
    late = CR.cast(hv, rays, t_min=float(pixels.t[hit].max()) + 0.02)
    assert not (late.status == CR.HIT).any()


def test_the_ray_sets_are_not_vacuous(orc, hv, everything):
    """conditions on the statement that the GPU tests rely on"""
    sets, spans = CR.ray_sets(orc, False), CR.spans(orc)
    print({name: len(rays) for name, rays in sets.items()})
    assert len(sets["a"]) == 4800 and len(sets["b"]) > 1000 and len(sets["c"]) == 3000 and len(sets["d"]) == 1500
    assert len(sets["e"]) == 256 and len(sets["f"]) == 25
    counts = np.bincount(everything.status, minlength=4)
    print("miss, hit, steps, invalid", counts, everything.branches)
    assert counts[CR.HIT] > 1000 and counts[CR.MISS] > 1000 and counts[CR.STEPS] >= 10 and counts[CR.INVALID] == 25
    for name, least in (("absent", 1000), ("exit_at_zero", 100), ("present", 1000), ("unobserved", 100), ("window", 1000),
                        ("armed_steps", 1000), ("behind_steps", 1000), ("refined_twice", 1000)):
        assert everything.branches[name] >= least, name
    assert everything.branches["window_sampled"] < everything.branches["window"]        # a window voxel without a sample
    # (c) and (d) hit too, and (d) marches along an axis: two components of n are 0
    for name in "cd":
        assert (everything.status[spans[name]] == CR.HIT).sum() >= 100
    assert ((everything.direction[spans["d"]] == 0).sum(-1) == 2).all()
    # the voxel-units form of the sets ends the same way wherever * L / L gave the origin back
    units = CR.cast(hv, CR.all_rays(orc, True), voxel_units=True, t_max=CR.bounds(True)[1])
    same = (CR.all_rays(orc, True)[:, :3] == everything.origin).all(-1)
    print("origins that survive the conversion: %.1f %%" % (100.0 * same.mean()))
    assert same.sum() > 1000 and np.array_equal(units.status[same], everything.status[same])
    assert units.t_voxels[same].tobytes() == everything.t_voxels[same].tobytes()


def test_a_pose_carries_the_rays(orc, hv, pixels):
    """rays given in a frame the pose carries into the volume's hit what the carried rays hit: the same surface points, to
    the rounding of the carry"""
    import merge_pose_reference as MP
    pose = MP.generic()
    rays = CR.ray_sets(orc, False)["a"]
    m = pose.inverse().matrix().astype(np.float64)
    moved = rays.copy()
    moved[:, :3] = (rays[:, :3] @ m[:3, :3].T + m[:3, 3]).astype(f32)
    moved[:, 3:] = (rays[:, 3:] @ m[:3, :3].T).astype(f32)
    got = CR.cast(hv, moved, pose=pose)
    both = (got.status == CR.HIT) & (pixels.status == CR.HIT)
    print("hits", int((got.status == CR.HIT).sum()), "worst |dt|", float(np.abs(got.t[both] - pixels.t[both]).max()))
    assert both.sum() > 0.99 * (pixels.status == CR.HIT).sum()
    assert np.abs(got.t[both] - pixels.t[both]).max() < 1e-4


def test_an_empty_volume_gives_all_miss(orc):
    empty = M.fresh(orc, 509, 4096)
    got = CR.cast(empty, CR.all_rays(orc, False))
    finite = slice(0, len(got.status) - 25)
    assert (got.status[finite] == CR.MISS).all() and (got.status[len(got.status) - 25:] == CR.INVALID).all()
    assert got.branches["present"] == 0 and not got.t.any()


def test_the_library_validates_before_touching_a_device():
    """every refusal vk.h lists, with addresses that are no memory: nothing may be enqueued (no GPU is needed, or touched)"""
    from vulcan_amd import api
    lib = api.lib()
    one, odd = C.c_void_p(4096), C.c_void_p(4096 + 8)

    def params(flags=0, max_steps=500, t_min=0.0, t_max=5.0):
        return T.CastParams(flags, max_steps, t_min, t_max)

    def call(v=fake_volume(), rays=one, count=8, pose=None, p=params(), t_out=one, status=one, samples=one, gradients=one):
        return lib.vk_volume_cast_rays(C.byref(v) if v else None, rays, count, pose, C.byref(p) if p else None, t_out, status, samples,
                                       gradients, None)

    assert call(v=None) == -1 and call(p=None) == -1
    broken = fake_volume()
    broken.hash_entries = None
    assert call(v=broken) == -1
    broken = fake_volume()
    broken.voxel_length = 0.0
    assert call(v=broken) == -1
    for flags in (4, 8, -1, 1 << 16):
        assert call(p=params(flags=flags)) == -1
    assert call(count=-1) == -1
    assert call(rays=None) == -1
    assert call(t_out=None) == -1 and call(status=None) == -1
    assert call(gradients=odd) == -1 and call(samples=None, gradients=odd) == -1
    for max_steps in (0, -1, 65537, 1 << 30):
        assert call(p=params(max_steps=max_steps)) == -1
    for t_min, t_max in ((-0.001, 5.0), (1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (0.0, float("nan")), (float("nan"), 5.0),
                         (float("-inf"), 5.0), (0.0, 0.0)):
        assert call(p=params(t_min=t_min, t_max=t_max)) == -1
    # count == 0 launches nothing, whatever the flags allow, but is checked like any call
    for flags in (0, 1, 2, 3):
        assert call(count=0, p=params(flags=flags)) == 0
    assert call(count=0, rays=None) == 0 and call(count=0, samples=None, gradients=None) == 0
    assert call(count=0, p=params(max_steps=1)) == 0 and call(count=0, p=params(max_steps=65536)) == 0
    assert call(count=0, t_out=None) == -1 and call(count=0, status=None) == -1 and call(count=0, p=params(max_steps=0)) == -1
