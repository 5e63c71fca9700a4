"""vk_volume_cast_rays on the device against its CPU statement (tests/cast_reference.py). The volume starts from an uploaded
oracle state; a ray's outcome, its t and the sample at its hit are one defined sequence of float32 operations, so status and
t are compared as uint32, samples as bytes and gradients as uint32, with no tolerance. The ray sets are the statement's
(a)-(f): the fusing camera's pixel rays, their twins from behind the surface, random rays around the mesh, axis-parallel rays
from block faces, rays that leave, and invalid rays; tests/test_cast_reference.py shows that they reach every outcome and
every branch of the march."""
import ctypes as C

import numpy as np
import pytest

import cast_reference as CR
import merge_pose_reference as MP
import sample_reference as S
from gpu_support import OTHER, SAME, api, device_copy, on_device, sync  # noqa: F401
from vulcan_amd import vk_types as T

pytestmark = pytest.mark.gpu

FORMS = [0, CR.VOXEL_UNITS, CR.DISTANCE_ONLY, CR.VOXEL_UNITS | CR.DISTANCE_ONLY]
_HOST, _DEVICE, _STATE = {}, {}, {}


def volumes(api, orc, sizes=SAME):
    """(host, device) of the statement's volume: the call only reads it, so one upload per table size serves every test
    (test_the_volume_is_only_read holds it to that)"""
    if sizes not in _DEVICE:
        _HOST[sizes] = CR.volume(orc, sizes)
        _DEVICE[sizes] = device_copy(api, _HOST[sizes])
    return _HOST[sizes], _DEVICE[sizes]


def statement(orc, hv, flags, pose=None, **bounds):
    """the statement on all_rays in the form `flags`, once per volume, form, pose and bounds"""
    key = (hv.main, hv.excess, flags, None if pose is None else bytes(pose), tuple(sorted(bounds.items())))
    if key not in _STATE:
        units = bool(flags & CR.VOXEL_UNITS)
        bounds.setdefault("t_max", CR.bounds(units)[1])
        _STATE[key] = CR.cast(hv, CR.all_rays(orc, units), pose=pose, voxel_units=units, color=not flags & CR.DISTANCE_ONLY, **bounds)
    return _STATE[key]


def call(dd, rays, pose, flags, **kw):
    kw.setdefault("t_max", CR.bounds(bool(flags & CR.VOXEL_UNITS))[1])
    kw.setdefault("max_steps", CR.MAX_STEPS)
    return dd._cast_call(rays, pose, flags, **kw)


def raw(t, status, samples, gradients):
    sync()
    return (t.cpu().numpy().view(np.uint32).copy(), status.cpu().numpy().view(np.uint32).copy(),
            None if samples is None else samples.cpu().numpy().tobytes(),
            None if gradients is None else gradients.cpu().numpy().view(np.uint32).copy())


def wanted(want, span=slice(None)):
    return (want.t[span].view(np.uint32), want.status[span].view(np.uint32), want.samples[span].tobytes(),
            want.gradients[span].view(np.uint32))


def assert_same(got, want):
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0], want[0])
    assert got[2] == want[2]
    assert np.array_equal(got[3], want[3])


@pytest.mark.parametrize("sizes", [SAME, OTHER], ids=["long-chains", "other-bucket-count"])
@pytest.mark.parametrize("flags", FORMS, ids=["metres", "voxel-units", "metres-distance-only", "voxel-units-distance-only"])
def test_bit_for_bit(api, orc, sizes, flags):
    hv, dd = volumes(api, orc, sizes)
    want = statement(orc, hv, flags)
    rays = on_device(CR.all_rays(orc, bool(flags & CR.VOXEL_UNITS)))
    got = raw(*call(dd, rays, None, flags))
    counts = np.bincount(want.status, minlength=4)
    print("rays", len(rays), "miss, hit, steps, invalid", counts, "with gradient", int((want.gradients[:, 3] != 0).sum()))
    assert counts[CR.HIT] > 1000 and counts[CR.MISS] >= 100 and counts[CR.STEPS] >= 10 and counts[CR.INVALID] == 25
    assert_same(got, wanted(want))
    if flags & CR.DISTANCE_ONLY:
        assert not want.samples["color"].any() and not want.samples["color_weight"].any()
    else:
        assert (want.samples["color_weight"] != 0).sum() > 1000


@pytest.mark.parametrize("flags", [0, CR.VOXEL_UNITS], ids=["metres", "voxel-units"])
def test_a_pose_on_the_device(api, orc, flags):
    import torch
    hv, dd = volumes(api, orc)
    rays = on_device(CR.all_rays(orc, bool(flags & CR.VOXEL_UNITS)))
    want = statement(orc, hv, flags, MP.generic())
    got = raw(*call(dd, rays, MP.generic(), flags))
    counts = np.bincount(want.status, minlength=4)
    print("miss, hit, steps, invalid", counts)
    assert counts[CR.HIT] > 1000 and counts[CR.MISS] >= 100
    assert_same(got, wanted(want))
    # a device buffer that already holds the pose: the same call
    pose_dev = torch.as_tensor(np.frombuffer(bytes(MP.generic()), dtype=np.uint8).copy()).cuda()
    again = raw(*call(dd, rays, pose_dev, flags))
    assert_same(again, got)
    # the identity pose is no pose, on the finite rays (the last 25 are the invalid ones)
    without, identity = raw(*call(dd, rays, None, flags)), raw(*call(dd, rays, T.Transform.identity(), flags))
    finite = len(rays) - 25
    assert np.array_equal(identity[0][:finite], without[0][:finite]) and np.array_equal(identity[1][:finite], without[1][:finite])
    assert identity[2][:20 * finite] == without[2][:20 * finite] and np.array_equal(identity[3][:finite], without[3][:finite])
    assert_same(identity, wanted(statement(orc, hv, flags, T.Transform.identity())))


def test_the_hit_carries_the_sample_of_its_point(api, orc):
    """voxel units, no pose: vk_volume_sample at the numpy float32 o + t n of the device's hits returns the device's own
    samples and gradients"""
    _, dd = volumes(api, orc)
    rays = CR.all_rays(orc, True)
    t, status, samples, gradients = raw(*call(dd, on_device(rays), None, CR.VOXEL_UNITS))
    hit = status == CR.HIT
    assert hit.sum() > 1000
    with np.errstate(all="ignore"):
        d = rays[:, 3:]
        n = d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
        points = rays[:, :3] + t.view(np.float32)[:, None] * n
    assert points.dtype == np.float32
    at = dd._sample_call(on_device(points[hit]), None, S.VOXEL_UNITS)
    sync()
    assert at[0].cpu().numpy().tobytes() == np.frombuffer(samples, dtype=np.uint8).reshape(-1, 20)[hit].tobytes()
    assert np.array_equal(at[1].cpu().numpy().view(np.uint32), gradients[hit])
    assert (gradients[hit][:, 3] != 0).sum() > 1000


@pytest.mark.parametrize("count", [1, 63, 65, 257, 4099])
def test_ragged_counts(api, orc, count):
    import torch
    hv, dd = volumes(api, orc)
    want = statement(orc, hv, 0)
    # from the middle of (a) on: pixel rays, then their twins
    first = 3000
    rays = on_device(CR.all_rays(orc, False)[first:first + count + 64])
    span = slice(first, first + count)

    def buffers(samples=True, gradients=True):
        return (torch.full((count + 64,), -7.5, dtype=torch.float32, device="cuda"),
                torch.full((count + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda"),
                torch.full((count + 64, 20), 0xA5, dtype=torch.uint8, device="cuda") if samples else None,
                torch.full((count + 64, 4), -7.5, dtype=torch.float32, device="cuda") if gradients else None)

    out = buffers()
    call(dd, rays, None, 0, count=count, out=out)
    got, untouched = raw(*out), raw(*buffers())
    assert_same((got[0][:count], got[1][:count], got[2][:20 * count], got[3][:count]), wanted(want, span))
    assert np.array_equal(got[0][count:], untouched[0][count:]) and np.array_equal(got[1][count:], untouched[1][count:])
    assert got[2][20 * count:] == untouched[2][20 * count:] and np.array_equal(got[3][count:], untouched[3][count:])
    # a null optional output: the others hold the same bytes, and the same tail is left alone
    for samples, gradients in ((False, True), (True, False), (False, False)):
        alone = buffers(samples, gradients)
        call(dd, rays, None, 0, count=count, out=alone)
        alone = raw(*alone)
        assert np.array_equal(alone[0], got[0]) and np.array_equal(alone[1], got[1])
        assert alone[2] is None or alone[2] == got[2]
        assert alone[3] is None or np.array_equal(alone[3], got[3])


def test_null_outputs(api, orc):
    hv, dd = volumes(api, orc)
    want = wanted(statement(orc, hv, 0))
    rays = on_device(CR.all_rays(orc, False))
    t, status, samples, gradients = raw(*call(dd, rays, None, 0, gradients=False))
    assert gradients is None and np.array_equal(t, want[0]) and np.array_equal(status, want[1]) and samples == want[2]
    t, status, samples, gradients = raw(*call(dd, rays, None, 0, samples=False))
    assert samples is None and np.array_equal(t, want[0]) and np.array_equal(status, want[1]) and np.array_equal(gradients, want[3])
    t, status, samples, gradients = raw(*call(dd, rays, None, 0, samples=False, gradients=False))
    assert samples is None and gradients is None and np.array_equal(t, want[0]) and np.array_equal(status, want[1])


def test_the_bounds_end_a_ray(api, orc):
    hv, dd = volumes(api, orc)
    rays = on_device(CR.all_rays(orc, False))
    full = statement(orc, hv, 0)
    one = statement(orc, hv, 0, max_steps=1)
    assert (one.status[full.status == CR.HIT] == CR.STEPS).all()
    assert_same(raw(*call(dd, rays, None, 0, max_steps=1)), wanted(one))
    # 0.9 m: short of the wall for most pixel rays, enough for the bump
    short = statement(orc, hv, 0, t_max=0.9)
    counts = np.bincount(short.status, minlength=4)
    print("t_max 0.9: miss, hit, steps, invalid", counts)
    assert (short.status[(full.status == CR.HIT) & (full.t > np.float32(0.95))] == CR.MISS).all() and counts[CR.HIT] >= 100
    assert_same(raw(*call(dd, rays, None, 0, t_max=0.9)), wanted(short))
    late = statement(orc, hv, 0, t_min=0.5)
    assert_same(raw(*call(dd, rays, None, 0, t_min=0.5)), wanted(late))


def test_the_volume_is_only_read(api, orc):
    hv, dd = volumes(api, orc)

    def state():
        return (dd.host_voxels().tobytes(), dd.host_entries().tobytes(), dd.counters.cpu().numpy().tobytes(),
                dd.host_visibility().tobytes(), dd.free_voxel_blocks.cpu().numpy().tobytes())

    before = state()
    for flags in FORMS:
        call(dd, on_device(CR.all_rays(orc, bool(flags & CR.VOXEL_UNITS))), MP.generic() if flags == 0 else None, flags)
    sync()
    assert state() == before
    assert before[0] == hv.voxels.tobytes() and before[1] == hv.hash_entries.tobytes()


def test_the_class_method(api, orc):
    hv, dd = volumes(api, orc)
    want = statement(orc, hv, 0, max_steps=500)
    rays = on_device(CR.all_rays(orc, False))
    result = dd.cast_rays(rays, gradient=True)
    sync()
    assert_same(raw(result.t, result.status, result.samples, result.gradients), wanted(want))
    assert int(result.hit.sum()) == int((want.status == CR.HIT).sum())
    assert result.color.shape == (len(rays), 3) and result.gradient.shape == (len(rays), 3)
    plain = dd.cast_rays(rays, color=False)
    assert plain.color is None and plain.gradient is None and bool((plain.t == result.t).all())
    with pytest.raises(api.VkError):
        dd.cast_rays(rays.double())
    with pytest.raises(api.VkError):
        dd.cast_rays(rays.reshape(-1))


def test_arguments_are_checked_on_the_host(api, orc):
    import torch
    hv, dd = volumes(api, orc)
    lib = api.lib()
    rays = on_device(CR.all_rays(orc, False)[:64])
    t_out = torch.full((64,), -7.5, dtype=torch.float32, device="cuda")
    status = torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    samples = torch.full((64, 20), 0xA5, dtype=torch.uint8, device="cuda")
    gradients = torch.full((65, 4), -7.5, dtype=torch.float32, device="cuda")
    sync()
    at = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731

    def params(flags=0, max_steps=500, t_min=0.0, t_max=5.0):
        return T.CastParams(flags, max_steps, t_min, t_max)

    def cast(v="volume", r=rays, count=64, p=params(), t=t_out, st=status, s=samples, g=gradients, g_offset=0):
        desc = dd.desc() if v == "volume" else v
        g_ptr = None if g is None else C.c_void_p(g.data_ptr() + g_offset)
        return lib.vk_volume_cast_rays(C.byref(desc) if desc else None, at(r), count, None, C.byref(p) if p else None, at(t), at(st),
                                       at(s), g_ptr, api.stream())

    def changed(**fields):
        desc = dd.desc()
        for name, value in fields.items():
            setattr(desc, name, value)
        return desc

    assert cast(v=None) == -1 and cast(p=None) == -1
    assert cast(v=changed(voxels=None)) == -1 and cast(v=changed(main_block_count=0)) == -1 and cast(v=changed(voxel_length=0.0)) == -1
    for flags in (4, 7, -1):
        assert cast(p=params(flags=flags)) == -1
    assert cast(count=-1) == -1 and cast(r=None) == -1 and cast(t=None) == -1 and cast(st=None) == -1
    assert cast(g_offset=4) == -1 and cast(g_offset=8) == -1 and cast(s=None, g_offset=12) == -1
    for max_steps in (0, -5, 65537):
        assert cast(p=params(max_steps=max_steps)) == -1
    for t_min, t_max in ((-1.0, 5.0), (1.0, 1.0), (3.0, 2.0), (0.0, float("inf")), (float("nan"), 5.0), (0.0, float("nan"))):
        assert cast(p=params(t_min=t_min, t_max=t_max)) == -1
    assert cast(count=0) == 0 and cast(count=0, r=None) == 0 and cast(count=0, t=None) == -1
    sync()
    # nothing was launched: the outputs hold their sentinel, the volume its bytes
    assert bool((t_out == -7.5).all()) and bool((status == 0x5A5A5A5A).all())
    assert bool((samples == 0xA5).all()) and bool((gradients == -7.5).all())
    assert dd.host_voxels().tobytes() == hv.voxels.tobytes() and np.array_equal(dd.host_entries(), hv.hash_entries)
    assert cast() == 0 and cast(s=None) == 0 and cast(g=None) == 0 and cast(s=None, g=None) == 0 and cast(g_offset=16) == 0
    assert cast(p=params(max_steps=65536)) == 0 and cast(p=params(max_steps=1)) == 0
    sync()
