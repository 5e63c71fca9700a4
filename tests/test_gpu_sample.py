"""vk_volume_sample on the device against its CPU statement (tests/sample_reference.py). The volume starts from an uploaded
oracle state; a sample and a gradient are one defined sequence of float32 operations each, so samples are compared as bytes
and gradients as uint32, with no tolerance. The point sets are the statement's (a)-(f): mesh vertices, points around them,
voxel centres at the rim of the observed region, points on block faces with integral coordinates, points far from any
block, and non-finite coordinates; tests/test_sample_reference.py shows that they reach every outcome."""
import ctypes as C

import numpy as np
import pytest

import merge_pose_reference as MP
import merge_reference as M
import sample_reference as S
from gpu_support import OTHER, SAME, api, device_copy, on_device, pair_on_device, sync  # noqa: F401
from vulcan_amd import vk_types as T

pytestmark = pytest.mark.gpu

FORMS = [0, S.VOXEL_UNITS, S.DISTANCE_ONLY, S.VOXEL_UNITS | S.DISTANCE_ONLY]
_STATE = {}


def volumes(api, orc, sizes=SAME):
    """(host dst, host src, device dst, device src) of the register tests' pair"""
    return pair_on_device(api, orc, MP.generic(), sizes)


def statement(orc, hv, flags, pose=None):
    """the statement at all_points in the form `flags`, once per volume, form and pose"""
    key = (hv.main, hv.excess, flags, None if pose is None else bytes(pose))
    if key not in _STATE:
        units = bool(flags & S.VOXEL_UNITS)
        _STATE[key] = S.sample(hv, S.all_points(orc, units), pose=pose, voxel_units=units, color=not flags & S.DISTANCE_ONLY)
    return _STATE[key]


def raw(samples, gradients):
    sync()
    return (None if samples is None else samples.cpu().numpy().tobytes(),
            None if gradients is None else gradients.cpu().numpy().view(np.uint32).copy())


def assert_is_statement(got, want):
    samples, gradients = got
    assert samples == want[0].tobytes()
    assert np.array_equal(gradients, want[1].view(np.uint32))


@pytest.mark.parametrize("sizes", [SAME, OTHER], ids=["long-chains", "other-bucket-count"])
@pytest.mark.parametrize("flags", FORMS, ids=["metres", "voxel-units", "metres-distance-only", "voxel-units-distance-only"])
def test_bit_for_bit(api, orc, sizes, flags):
    hd, _, dd, _ = volumes(api, orc, sizes)
    want = statement(orc, hd, flags)
    points = on_device(S.all_points(orc, bool(flags & S.VOXEL_UNITS)))
    got = raw(*dd._sample_call(points, None, flags))
    d, g = want[0]["distance_weight"] != 0, want[1][:, 3] != 0
    print("points", len(points), "with distance", int(d.sum()), "with gradient", int(g.sum()), "with colour", int((want[0]["color_weight"] != 0).sum()))
    assert d.sum() > 1000 and g.sum() > 1000
    assert_is_statement(got, want)
    if flags & S.DISTANCE_ONLY:
        assert not want[0]["color"].any() and not want[0]["color_weight"].any()


@pytest.mark.parametrize("flags", [0, S.VOXEL_UNITS], ids=["metres", "voxel-units"])
def test_a_pose_on_the_device(api, orc, flags):
    hd, _, dd, _ = volumes(api, orc)
    units = bool(flags & S.VOXEL_UNITS)
    points = on_device(S.all_points(orc, units))
    want = statement(orc, hd, flags, MP.generic())
    got = raw(*dd._sample_call(points, MP.generic(), flags))
    print("with distance", int((want[0]["distance_weight"] != 0).sum()), "with gradient", int((want[1][:, 3] != 0).sum()))
    assert (want[0]["distance_weight"] != 0).sum() > 1000 and (want[1][:, 3] != 0).sum() > 1000
    assert_is_statement(got, want)
    # a device buffer that already holds the pose: the same call
    import torch
    pose_dev = torch.as_tensor(np.frombuffer(bytes(MP.generic()), dtype=np.uint8).copy()).cuda()
    again = raw(*dd._sample_call(points, pose_dev, flags))
    assert again[0] == got[0] and np.array_equal(again[1], got[1])
    # the identity pose is no pose, on the finite points (the last twelve are the non-finite ones and 1e30)
    without = raw(*dd._sample_call(points, None, flags))
    identity = raw(*dd._sample_call(points, T.Transform.identity(), flags))
    finite = len(points) - 12
    assert identity[0][:20 * finite] == without[0][:20 * finite] and np.array_equal(identity[1][:finite], without[1][:finite])
    assert_is_statement(identity, statement(orc, hd, flags, T.Transform.identity()))


@pytest.mark.parametrize("count", [1, 63, 65, 257, 4099])
def test_ragged_counts(api, orc, count):
    import torch
    hd, _, dd, _ = volumes(api, orc)
    want = statement(orc, hd, 0)
    # from the middle of (a)-(b) on: vertices, then points around them
    first = 19000
    points = on_device(S.all_points(orc, False)[first:first + count + 64])

    def buffers():
        return (torch.full((count + 64, 20), 0xA5, dtype=torch.uint8, device="cuda"),
                torch.full((count + 64, 4), -7.5, dtype=torch.float32, device="cuda"))

    samples, gradients = buffers()
    dd._sample_call(points, None, 0, count=count, out=(samples, gradients))
    got = raw(samples, gradients)
    assert got[0][:20 * count] == want[0][first:first + count].tobytes()
    assert np.array_equal(got[1][:count], want[1][first:first + count].view(np.uint32))
    untouched = raw(*buffers())
    assert got[0][20 * count:] == untouched[0][20 * count:] and np.array_equal(got[1][count:], untouched[1][count:])
    # one output alone (the other pointer is null): the same bytes, and the same tail left alone
    samples_alone, gradients_alone = buffers()
    dd._sample_call(points, None, 0, count=count, out=(samples_alone, None))
    dd._sample_call(points, None, 0, count=count, out=(None, gradients_alone))
    assert raw(samples_alone, None)[0] == got[0] and np.array_equal(raw(None, gradients_alone)[1], got[1])
    # again: the same bytes
    samples, gradients = buffers()
    dd._sample_call(points, None, 0, count=count, out=(samples, gradients))
    again = raw(samples, gradients)
    assert again[0] == got[0] and np.array_equal(again[1], got[1])


def test_the_volume_is_only_read(api, orc):
    hd, _, dd, _ = volumes(api, orc)
    before = (dd.host_voxels().tobytes(), dd.host_entries().tobytes(), dd.counters.cpu().numpy().tobytes(),
              dd.host_visibility().tobytes(), dd.free_voxel_blocks.cpu().numpy().tobytes())
    for flags in FORMS:
        dd._sample_call(on_device(S.all_points(orc, bool(flags & S.VOXEL_UNITS))), MP.generic() if flags == 0 else None, flags)
    sync()
    after = (dd.host_voxels().tobytes(), dd.host_entries().tobytes(), dd.counters.cpu().numpy().tobytes(),
             dd.host_visibility().tobytes(), dd.free_voxel_blocks.cpu().numpy().tobytes())
    assert before == after
    assert before[0] == hd.voxels.tobytes() and before[1] == hd.hash_entries.tobytes()


def test_the_devices_own_mesh_lies_on_the_zero_set(api, orc):
    """bound: 1e-4, the README's TSDF tolerance (the statement measures 4.6e-6 at the oracle's vertices)"""
    _, _, dd, _ = volumes(api, orc)
    extractor = api.Extractor(dd)
    extractor.all_allocated = True
    mesh = extractor.extract()
    result = dd.sample(mesh.points.contiguous(), color=False)
    worst = float(result.distance.abs().max())
    print("vertices", len(mesh.points), "worst |D|", worst, "metres", float(result.metres().abs().max()))
    assert len(mesh.points) > 10000
    assert bool((result.distance_weight != 0).all())
    assert worst <= 1e-4
    assert result.color is None and result.gradient is None
    full = dd.sample(mesh.points.contiguous(), gradient=True)
    assert bool((full.distance == result.distance).all()) and full.color.shape == (len(mesh.points), 3)
    assert full.gradient.shape == (len(mesh.points), 3) and bool((full.gradient_valid == 1).sum() > 10000)
    assert float(full.metres()[0]) == pytest.approx(float(full.distance[0]) * dd.truncation_length, abs=1e-9)


def test_a_fresh_merge_is_the_samples_of_its_centres(api, orc):
    """merge(src, pose) into an empty volume: every voxel of every block it allocates is the sample of src at the voxel's
    centre carried back, through the running average from weight 0: the value itself, the weight capped at 16. Compared on
    the device."""
    import torch
    _, hs, _, ds = volumes(api, orc)
    fresh = device_copy(api, M.fresh(orc, 4093, 4096))
    counts = fresh.merge(ds, pose=MP.generic())
    entries = fresh.host_entries()
    held = np.flatnonzero(entries["data"] >= 0)
    print("counts", counts, "blocks", len(held))
    assert counts[4] == 0 and len(held) == counts[2] and counts[7] > 100000
    origins = entries["block"]["origin"][held].astype(np.int64)
    centres = ((8 * origins[:, None, :] + MP.OFFSETS[None]).astype(np.float32) + np.float32(0.5)).reshape(-1, 3)
    at = (entries["data"][held].astype(np.int64)[:, None] * 512 + np.arange(512)[None]).reshape(-1)
    samples, _ = ds._sample_call(on_device(centres), MP.generic().inverse(), S.VOXEL_UNITS, gradients=False)
    want = samples.clone()
    weights = want.view(torch.int16)[:, 8:10]
    weights.clamp_(max=16)
    got = fresh.voxels.view(-1, 20)[torch.as_tensor(at).cuda()]
    sampled = int((weights[:, 0] != 0).sum())
    print("voxels with a distance sample", sampled)
    assert sampled == counts[7]
    assert bool(torch.equal(got, want))


def test_arguments_are_checked_on_the_host(api, orc):
    import torch
    hd, _, dd, _ = volumes(api, orc)
    lib = api.lib()
    points = on_device(S.all_points(orc, False)[:64])
    samples = torch.full((64, 20), 0xA5, dtype=torch.uint8, device="cuda")
    gradients = torch.full((65, 4), -7.5, dtype=torch.float32, device="cuda")
    sync()
    good = T.SampleParams(0, 0)
    at = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731

    def call(v="volume", p=points, count=64, params=good, s=samples, g=gradients, g_offset=0):
        desc = dd.desc() if v == "volume" else v
        g_ptr = None if g is None else C.c_void_p(g.data_ptr() + g_offset)
        return lib.vk_volume_sample(C.byref(desc) if desc else None, at(p), count, None, C.byref(params) if params else None, at(s),
                                    g_ptr, api.stream())

    def changed(**fields):
        desc = dd.desc()
        for name, value in fields.items():
            setattr(desc, name, value)
        return desc

    assert call(v=None) == -1 and call(params=None) == -1
    assert call(v=changed(voxels=None)) == -1 and call(v=changed(main_block_count=0)) == -1 and call(v=changed(voxel_length=0.0)) == -1
    for flags in (4, 7, -1):
        assert call(params=T.SampleParams(flags, 0)) == -1
    assert call(count=-1) == -1 and call(p=None) == -1 and call(s=None, g=None) == -1
    assert call(g_offset=4) == -1 and call(g_offset=8) == -1 and call(s=None, g_offset=12) == -1
    assert call(count=0) == 0 and call(count=0, p=None) == 0
    sync()
    # nothing was launched: the outputs hold their sentinel, the volume its bytes
    assert bool((samples == 0xA5).all()) and bool((gradients == -7.5).all())
    assert dd.host_voxels().tobytes() == hd.voxels.tobytes() and np.array_equal(dd.host_entries(), hd.hash_entries)
    assert call() == 0 and call(s=None) == 0 and call(g=None) == 0 and call(g_offset=16) == 0
    sync()
    # through the class: what is no [N, 3] float32 device tensor is refused
    with pytest.raises(api.VkError):
        dd.sample(points.double())
    with pytest.raises(api.VkError):
        dd.sample(points.reshape(-1))
