"""The CPU statement of vk_volume_register_rays (tests/register_rays_reference.py) on the project's own scene: one ray by hand,
the loop on a displaced sweep, every branch of the definition reached, and the host checks of the built library.

The figures the method gave before any of this was written (a numpy script built from register_reference.sample / jacobian /
system / step on cast_reference.volume and its 19 200 pixel rays with cast_rays' ranges, displaced by
merge_pose_reference.generic(), 26.0 mm / 11.2 degrees from the identity start): the full sweep ends with code 1 after 7 steps
at 0.065 mm / 0.0082 degrees from the truth, residuals 5 331 -> 18 783, rms 0.52 -> 0.00093; every 16th ray: 8 steps, 0.061 mm /
0.0069 degrees; started at the truth it settles at the same point in 2 steps. The bounds below, 0.1 mm and 0.012 degrees within
10 steps, leave the statement about 1.5x."""
import ctypes as C

import numpy as np

from abi_support import fake_volume
import integrate_rays_reference as IR
import merge_pose_reference as MP
import register_rays_reference as RY
import register_reference as RR
from vulcan_amd import vk_types as T

f32 = np.float32
MAX_STEPS, MAX_METRES, MAX_DEGREES = 10, 0.1e-3, 0.012


def test_one_ray_by_hand(orc):
    """a ray along +z from a point in front of the wall, in voxel units at the identity: every quantity spelled out"""
    world = RY.world(orc)
    hv = world.hv
    rays, ranges = IR.pixel_hits(orc)
    one = len(ranges) // 2 + 37
    L = f32(hv.voxel_length)
    d = rays[one, 3:]
    length = np.sqrt(f32(f32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
    n = d / length
    r = ranges[one] / L
    e = (rays[one, :3] / L) + r * n
    g = e - f32(0.5)
    b = np.floor(g)
    fx, fy, fz = g - b
    base = b.astype(np.int64)
    v = []
    for k in range(8):
        p = base + np.array([k & 1, (k >> 1) & 1, k >> 2])
        slot = world.table[tuple(int(c) for c in p >> 3)]
        cell = hv.voxels[slot * 512 + (p[2] & 7) * 64 + (p[1] & 7) * 8 + (p[0] & 7)]
        assert cell["distance_weight"] != 0
        v.append(f32(cell["distance"]))
    lerp = lambda t, a, c: a + t * (c - a)   # noqa: E731
    x00, x10, x01, x11 = lerp(fx, v[0], v[1]), lerp(fx, v[2], v[3]), lerp(fx, v[4], v[5]), lerp(fx, v[6], v[7])
    y0, y1 = lerp(fy, x00, x10), lerp(fy, x01, x11)
    D = lerp(fz, y0, y1)
    gz = y1 - y0
    gy = lerp(fz, x10 - x00, x11 - x01)
    gx = lerp(fz, lerp(fy, v[1] - v[0], v[3] - v[2]), lerp(fy, v[5] - v[4], v[7] - v[6]))
    iv = f32(1.0) / L
    J = np.array([e[1] * gz - e[2] * gy, e[2] * gx - e[0] * gz, e[0] * gy - e[1] * gx, gx * iv, gy * iv, gz * iv], dtype=f32)
    got = RY.terms(world, rays[one:one + 1], ranges[one:one + 1], T.Transform.identity())
    print("e", e, "D", D, "gradient", gx, gy, gz, "J", J)
    assert D.dtype == f32 and abs(D) < 0.05 and gz < 0                              # a hit of cast_rays lies on the zero set
    assert got.counts == (1, 1, 1, 0) and got.valid[0] == 1
    assert got.r.view(np.uint32)[0] == np.array([D], dtype=f32).view(np.uint32)[0]
    assert np.array_equal(got.J[0].view(np.uint32), J.view(np.uint32))
    total, absolute = RY.system(got)
    assert total[42] == float(f32(D * D)) and total[36] == float(f32(J[0] * D)) and total[20] == float(f32(J[5] * J[5]))


def test_undisplaced_rays_at_the_identity(orc):
    rays, ranges = IR.pixel_hits(orc)
    got = RY.terms(RY.world(orc), rays, ranges, T.Transform.identity())
    total, _ = RY.system(got)
    rms = float(np.sqrt(total[42] / got.counts[2]))
    print("counts", got.counts, "rms", rms)
    assert got.counts == (19200, 18785, 18785, 0)
    assert abs(rms - 0.00114) < 0.00001


def _loop(orc, every=1, start=None):
    rays, ranges, truth = RY.displaced_sweep(orc)
    out = RY.register(orc, RY.world(orc), rays[::every], ranges[::every], T.Transform.identity() if start is None else start, iterations=20)
    metres, degrees = RR.pose_error(out.pose, truth)
    print("every %d: steps %d code %d, %.4f mm %.5f degrees; residuals and rms per step %s" % (every, out.steps, out.code, metres * 1e3, degrees,
                                                                                           out.history))
    return out, metres, degrees


def test_the_full_sweep_from_the_identity(orc):
    start_error = RR.pose_error(T.Transform.identity(), MP.generic())
    print("start: %.1f mm %.1f degrees" % (start_error[0] * 1e3, start_error[1]))
    out, metres, degrees = _loop(orc)
    assert out.code == 1 and out.steps <= MAX_STEPS
    assert metres < MAX_METRES and degrees < MAX_DEGREES
    assert out.history[0][0] < out.history[-1][0] and out.history[0][1] > 0.3 and out.history[-1][1] < 0.002


def test_every_sixteenth_ray(orc):
    out, metres, degrees = _loop(orc, every=16)
    assert out.counts[0] == 1200
    assert out.code == 1 and out.steps <= MAX_STEPS
    assert metres < MAX_METRES and degrees < MAX_DEGREES


def test_started_at_the_truth_it_stays(orc):
    out, metres, degrees = _loop(orc, start=MP.generic())
    assert out.code == 1 and out.steps <= 3
    assert metres < MAX_METRES and degrees < MAX_DEGREES


def test_every_branch_is_reached(orc):
    world = RY.world(orc)
    for voxel_units in (False, True):
        rays, ranges = IR.all_rays(orc, voxel_units)
        r_min, r_max = IR.bounds(voxel_units)
        for pose in (T.Transform.identity(), MP.generic()):
            got = RY.terms(world, rays, ranges, pose, RY.BAND, r_min, r_max, voxel_units)
            print("voxel units", voxel_units, "counts", got.counts, got.branches)
            assert len(ranges) > 27000 and got.counts[0] + got.branches["unmeasured"] + got.counts[3] == len(ranges)
            for name in ("invalid", "unmeasured", "absent_block", "unweighted_corner", "outside_band", "leaves_1", "leaves_2", "leaves_3"):
                assert got.branches[name] > 0, name
            assert got.counts[2] > 1000 and got.counts[1] > got.counts[2]


def test_a_sweep_ten_metres_away_has_no_overlap(orc):
    rays, ranges, _ = RY.displaced_sweep(orc)
    start = T.Transform.translate(10.0, 0.0, 0.0) * MP.generic()
    out = RY.register(orc, RY.world(orc), rays, ranges, start, iterations=5)
    print("counts", out.counts, "steps", out.steps, "code", out.code)
    assert (out.steps, out.code) == (1, RY.NO_OVERLAP) and out.counts == (19200, 0, 0, 0)
    assert bytes(out.pose) == bytes(start) and not out.update.any()


def test_the_library_validates_before_touching_a_device():
    """every refusal vk.h lists, with addresses that are no memory: nothing may be enqueued (no GPU is needed, or touched)"""
    from vulcan_amd import api
    lib = api.lib()
    one, odd = C.c_void_p(4096), C.c_void_p(4096 + 8)
    assert C.sizeof(T.RegisterRaysParams) == 24

    def params(flags=0, iterations=20, r_min=0.1, r_max=5.0, band=0.75):
        return T.RegisterRaysParams(flags, iterations, r_min, r_max, band, 0)

    def call(v=fake_volume(), rays=one, ranges=one, count=8, pose=one, p=params(), system=one, state=one, counts=one, update=one,
             workspace=one):
        return lib.vk_volume_register_rays(C.byref(v) if v else None, rays, ranges, count, pose, C.byref(p) if p else None, system, state,
                                           counts, update, workspace, None)

    def system_call(v=fake_volume(), rays=one, ranges=one, count=8, pose=one, p=params(), system=one, counts=one, workspace=one):
        return lib.vk_volume_register_rays_system(C.byref(v) if v else None, rays, ranges, count, pose, C.byref(p) if p else None, system,
                                                  counts, workspace, None)

    def terms_call(v=fake_volume(), rays=one, ranges=one, count=8, pose=one, p=params(), residuals=one, jacobians=one, valid=one,
                   workspace=one):
        return lib.vk_volume_register_rays_terms(C.byref(v) if v else None, rays, ranges, count, pose, C.byref(p) if p else None,
                                                 residuals, jacobians, valid, workspace, None)

    for fn in (call, system_call, terms_call):
        assert fn(v=None) == -1 and fn(p=None) == -1 and fn(pose=None) == -1 and fn(workspace=None) == -1
        for field, value in (("hash_entries", None), ("voxel_length", 0.0), ("main_block_count", 0), ("voxels", (1 << 20) + 8)):
            broken = fake_volume()
            setattr(broken, field, value)
            assert fn(v=broken) == -1, field
        for flags in (2, 3, 4, -1, 1 << 16):
            assert fn(p=params(flags=flags)) == -1
        for iterations in (0, -1, 65):
            assert fn(p=params(iterations=iterations)) == -1
        for band in (0.0, -0.5, 1.5, float("nan"), float("inf")):
            assert fn(p=params(band=band)) == -1
        for r_min, r_max in ((-0.001, 5.0), (1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (0.0, float("nan")), (float("nan"), 5.0),
                             (float("-inf"), 5.0), (0.0, 0.0)):
            assert fn(p=params(r_min=r_min, r_max=r_max)) == -1
        assert fn(count=-1) == -1 and fn(count=(1 << 22) + 1) == -1
        assert fn(rays=None) == -1 and fn(ranges=None) == -1 and fn(workspace=odd) == -1
        # count == 0 launches nothing, whatever else is allowed, but is checked like any call
        for flags in (0, 1):
            assert fn(count=0, p=params(flags=flags, iterations=64, band=1.0)) == 0
        assert fn(count=0, rays=None, ranges=None) == 0
        assert fn(count=0, workspace=None) == -1 and fn(count=0, p=params(band=0.0)) == -1 and fn(count=0, pose=None) == -1
    for name in ("system", "state", "counts"):
        assert call(**{name: None}) == -1 and call(count=0, **{name: None}) == -1
    assert call(count=0, update=None) == 0
    for name in ("system", "counts"):
        assert system_call(**{name: None}) == -1
    for name in ("residuals", "jacobians", "valid"):
        assert terms_call(**{name: None}) == -1
    size = lib.vk_volume_register_rays_workspace_bytes
    assert size(-1) == 0 and size((1 << 22) + 1) == 0
    assert size(1) >= 128 and size(1 << 22) >= 128 * ((1 << 22) // 1024) and size(1 << 22) <= 1 << 20
