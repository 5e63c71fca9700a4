"""vk_volume_register_rays on the device against its CPU statement (tests/register_rays_reference.py). The volume starts from an
uploaded oracle state. The per-ray terms are one defined sequence of float32 operations and equal the statement's bit for bit;
the sums are added in float32 in the device's own fixed order and are held to the bound the depth tracker's system is held to
(gpu_support.assert_system: 2e-5 of the sum of the absolute terms); a pose after the loop is held to 2e-5 per entry, the
project's standing bound for a tracked pose against the oracle. The rays are integrate_rays' sets (a)-(g), which reach every
branch of the definition (tests/test_register_rays_reference.py), and the displaced sweep of register_rays_reference."""
import numpy as np
import pytest

import cast_reference as CR
import integrate_rays_reference as IR
import map_life as ML
import merge_pose_reference as MP
import merge_reference as M
import register_rays_reference as RY
import register_reference as RR
import release_reference as R
from gpu_support import OTHER, SAME, api, assert_system, device_copy, form, on_device, same_bits, sync, world  # noqa: F401
from vulcan_amd import vk_types as T

pytestmark = pytest.mark.gpu

RUN = 512                                      # the rays of one workgroup: one row of partial sums
RAGGED = (1, 63, 64, 65, 255, 256, 257, RUN + 1)
_WANT, _LOOP = {}, {}


def pose_of(name):
    return MP.generic() if name == "generic" else T.Transform.identity()


def statement(orc, sizes, units, pose, permuted=False):
    """(rays, ranges, the statement's Terms) of all_rays in the form: once per case, never changed"""
    key = (sizes, units, pose, permuted)
    if key not in _WANT:
        rays, ranges = IR.all_rays(orc, units)
        if permuted:
            rays, ranges = IR.permuted(rays, ranges)
        _, r_min, r_max = form(units)
        _WANT[key] = (rays, ranges, RY.terms(world(orc, sizes), rays, ranges, pose_of(pose), RY.BAND, r_min, r_max, units))
    return _WANT[key]


def statement_loop(orc):
    """the statement's 20 steps from the identity on the displaced sweep: once"""
    if "loop" not in _LOOP:
        rays, ranges, _ = RY.displaced_sweep(orc)
        _LOOP["loop"] = RY.register(orc, RY.world(orc), rays, ranges, T.Transform.identity(), iterations=20)
    return _LOOP["loop"]


def device_terms(dv, rays, ranges, pose, units, count=None, out=None):
    flags, r_min, r_max = form(units)
    valid, residuals, jacobians = dv._register_rays_terms_call(rays, ranges, pose, RY.BAND, flags, r_min, r_max, count, out)
    return valid.cpu().numpy(), residuals.cpu().numpy(), jacobians.cpu().numpy()


def assert_terms(got, want, count=None):
    valid, residuals, jacobians = got
    count = len(want.valid) if count is None else count
    assert np.array_equal(valid[:count], want.valid[:count])
    assert same_bits(residuals[:count], want.r[:count])
    assert same_bits(jacobians[:count], want.J[:count])


@pytest.mark.parametrize("sizes", [SAME, OTHER], ids=["long-chains", "other-bucket-count"])
@pytest.mark.parametrize("units", [False, True], ids=["metres", "voxel-units"])
@pytest.mark.parametrize("pose", ["generic", "identity"])
def test_terms_bit_for_bit(api, orc, sizes, units, pose):
    rays, ranges, want = statement(orc, sizes, units, pose)
    dv = device_copy(api, world(orc, sizes).hv)
    got = device_terms(dv, on_device(rays), on_device(ranges), pose_of(pose), units)
    print("counts", want.counts, "valid on the device", int(got[0].sum()), want.branches)
    assert want.counts[2] > 1000 and want.counts[3] == 25
    assert_terms(got, want)


def test_ragged_counts(api, orc):
    """the ragged last wave and the ragged last row: the terms and the counts of the first `count` rays of the shuffled sets,
    the outputs pre-filled with noise, and nothing past `count` written"""
    import torch
    rays, ranges, want = statement(orc, SAME, False, "generic", permuted=True)
    dv = device_copy(api, world(orc, SAME).hv)
    d_rays, d_ranges = on_device(rays), on_device(ranges)
    flags, r_min, r_max = form(False)
    for count in RAGGED:
        size = count + 2 * RUN
        generator = torch.Generator(device="cuda").manual_seed(count)
        noise = (torch.randint(1, 255, (size,), dtype=torch.uint8, device="cuda", generator=generator),
                 torch.rand(size, device="cuda", generator=generator) + 1, torch.rand((size, 6), device="cuda", generator=generator) + 1)
        before = tuple(t.cpu().numpy() for t in noise)
        got = device_terms(dv, d_rays, d_ranges, MP.generic(), False, count, noise)
        assert_terms(got, want, count)
        for after, was in zip(got, before):
            assert np.array_equal(after[count:], was[count:]), count
        _, counts = dv._register_rays_system_call(d_rays, d_ranges, MP.generic(), RY.BAND, flags, r_min, r_max, count)
        kinds = IR.carried(world(orc, SAME).hv, rays[:count], ranges[:count], MP.generic(), r_min, r_max, False)[3]
        print("count", count, "counts", counts)
        assert counts[0] == int((kinds == IR.INTEGRATED).sum()) and counts[3] == int((kinds == IR.INVALID).sum())
        assert counts[2] == int(want.valid[:count].sum()) and counts[2] <= counts[1] <= counts[0]


@pytest.mark.parametrize("sizes", [SAME, OTHER], ids=["long-chains", "other-bucket-count"])
def test_system(api, orc, sizes):
    rays, ranges, want = statement(orc, sizes, False, "generic")
    total, absolute = RY.system(want)
    dv = device_copy(api, world(orc, sizes).hv)
    d_rays, d_ranges = on_device(rays), on_device(ranges)
    flags, r_min, r_max = form(False)
    got, counts = dv._register_rays_system_call(d_rays, d_ranges, MP.generic(), RY.BAND, flags, r_min, r_max)
    print("counts", counts, want.counts)
    assert counts == want.counts
    assert_system(got, total, absolute)
    again, counts_again = dv._register_rays_system_call(d_rays, d_ranges, MP.generic(), RY.BAND, flags, r_min, r_max)
    assert again.tobytes() == got.tobytes() and counts_again == counts


def test_system_of_more_rows_than_the_narrow_sum_takes(api, orc):
    """beyond 1 024 rows of partial sums the sum runs 1024 lanes wide: the sets twenty times over, 1 079 rows; every sum and
    every count is twenty times the statement's"""
    rays, ranges, want = statement(orc, SAME, False, "generic")
    times = 20
    assert times * len(ranges) > 1024 * RUN
    total, absolute = RY.system(want)
    dv = device_copy(api, world(orc, SAME).hv)
    flags, r_min, r_max = form(False)
    d_rays, d_ranges = on_device(np.tile(rays, (times, 1))), on_device(np.tile(ranges, times))
    got, counts = dv._register_rays_system_call(d_rays, d_ranges, MP.generic(), RY.BAND, flags, r_min, r_max)
    print("counts", counts, want.counts)
    assert counts == tuple(times * c for c in want.counts)
    assert_system(got, times * total, times * absolute)
    again, counts_again = dv._register_rays_system_call(d_rays, d_ranges, MP.generic(), RY.BAND, flags, r_min, r_max)
    assert again.tobytes() == got.tobytes() and counts_again == counts


def test_a_permuted_sweep_gives_the_permuted_terms(api, orc):
    rays, ranges, want = statement(orc, SAME, False, "generic")
    order = np.random.default_rng(5).permutation(len(ranges))               # integrate_rays_reference.permuted's
    shuffled = IR.permuted(rays, ranges)
    assert np.array_equal(shuffled[1].view(np.uint32), ranges[order].view(np.uint32))
    dv = device_copy(api, world(orc, SAME).hv)
    valid, residuals, jacobians = device_terms(dv, on_device(shuffled[0]), on_device(shuffled[1]), MP.generic(), False)
    assert np.array_equal(valid, want.valid[order]) and same_bits(residuals, want.r[order]) and same_bits(jacobians, want.J[order])
    # and the sums of the permuted sweep are held to the same float64 sums
    flags, r_min, r_max = form(False)
    got, counts = dv._register_rays_system_call(on_device(shuffled[0]), on_device(shuffled[1]), MP.generic(), RY.BAND, flags, r_min, r_max)
    assert counts == want.counts
    assert_system(got, *RY.system(want))


def test_loop_from_the_identity(api, orc):
    want = statement_loop(orc)
    rays, ranges, truth = RY.displaced_sweep(orc)
    hv = RY.world(orc).hv
    dv = device_copy(api, hv)
    d_rays, d_ranges = on_device(rays), on_device(ranges)
    pose, state, counts, system, _ = dv._register_rays_call(d_rays, d_ranges, T.Transform.identity(), 20, RY.BAND, 0, RY.R_MIN, RY.R_MAX)
    print("state", state, "statement", want.steps, want.code, "counts", counts, want.counts)
    print("pose: worst entry", float(np.abs(pose.matrix() - want.pose.matrix()).max()),
          "inverse", float(np.abs(pose.inverse_matrix() - want.pose.inverse_matrix()).max()), "error", RR.pose_error(pose, truth))
    assert state == (want.steps, want.code) and want.code == 1
    assert np.abs(pose.matrix() - want.pose.matrix()).max() <= 2e-5
    assert np.abs(pose.inverse_matrix() - want.pose.inverse_matrix()).max() <= 2e-5
    # the volume is only read
    sync()
    assert dv.host_voxels().tobytes() == hv.voxels.tobytes() and np.array_equal(dv.host_entries(), hv.hash_entries)

    # through the class, from a 4x4 array: the same call, and the pose stays on the device
    result = dv.register_rays(d_rays, d_ranges, pose=np.eye(4), r_min=RY.R_MIN, r_max=RY.R_MAX)
    print(result)
    assert bytes(result.pose) == bytes(pose) and (result.steps, result.converged, result.overlap) == (state[0], True, True)
    assert result.residuals == counts[2] and result.rms == pytest.approx(np.sqrt(system[42] / counts[2]))
    assert bytes(result.device_pose.cpu().numpy().tobytes()) == bytes(pose)
    assert dv.register_rays(d_rays, d_ranges, r_min=RY.R_MIN, r_max=RY.R_MAX).steps == state[0]     # no pose: the identity


def test_three_steps(api, orc):
    want = statement_loop(orc)
    rays, ranges, _ = RY.displaced_sweep(orc)
    dv = device_copy(api, RY.world(orc).hv)
    pose, state, _, _, _ = dv._register_rays_call(on_device(rays), on_device(ranges), T.Transform.identity(), 3, RY.BAND, 0, RY.R_MIN, RY.R_MAX)
    after = want.poses[3]
    print("state", state, "worst entry", float(np.abs(pose.matrix() - after.matrix()).max()))
    assert state == (3, 0)
    assert np.abs(pose.matrix() - after.matrix()).max() <= 2e-5
    assert np.abs(pose.inverse_matrix() - after.inverse_matrix()).max() <= 2e-5


def test_no_overlap(api, orc):
    rays, ranges, _ = RY.displaced_sweep(orc)
    dv = device_copy(api, RY.world(orc).hv)
    start = T.Transform.translate(10.0, 0.0, 0.0) * MP.generic()
    d_rays, d_ranges = on_device(rays), on_device(ranges)
    pose, state, counts, _, update = dv._register_rays_call(d_rays, d_ranges, start, 5, RY.BAND, 0, RY.R_MIN, RY.R_MAX)
    print("state", state, "counts", counts)
    assert state == (1, T.VK_REGISTER_NO_OVERLAP) and counts == (19200, 0, 0, 0)
    assert bytes(pose) == bytes(start) and not update.any()
    result = dv.register_rays(d_rays, d_ranges, pose=start, r_min=RY.R_MIN, r_max=RY.R_MAX)
    assert not result.overlap and not result.converged and result.residuals == 0 and bytes(result.pose) == bytes(start)
    # no rays: no call
    none = dv.register_rays(d_rays[:0], d_ranges[:0], pose=start)
    assert (none.steps, none.converged, none.overlap, none.residuals) == (0, False, False, 0) and bytes(none.pose) == bytes(start)


@pytest.mark.parametrize("fill", ["ones", "noise"])
def test_a_dirty_workspace(api, orc, fill):
    """workspace, counts, system, update and the pose buffer overwritten before the call: the same bytes come out"""
    import torch
    rays, ranges, _ = RY.displaced_sweep(orc)
    dv = device_copy(api, RY.world(orc).hv)
    d_rays, d_ranges = on_device(rays), on_device(ranges)
    arguments = (d_rays, d_ranges, T.Transform.identity(), 20, RY.BAND, 0, RY.R_MIN, RY.R_MAX)
    clean = dv._register_rays_call(*arguments)
    clean_system = dv._register_rays_system_call(d_rays, d_ranges, MP.generic(), RY.BAND, 0, RY.R_MIN, RY.R_MAX)
    b = dv._register_rays_buffers
    generator = torch.Generator(device="cuda").manual_seed(3)

    def dirty():
        for name in ("workspace", "counts", "system", "update", "pose"):
            raw = b[name].view(torch.uint8)
            if fill == "ones":
                raw.fill_(1)
            else:
                raw.copy_(torch.randint(0, 256, raw.shape, dtype=torch.uint8, device="cuda", generator=generator))

    dirty()
    again = dv._register_rays_call(*arguments)
    assert bytes(again[0]) == bytes(clean[0]) and again[1] == clean[1] and again[2] == clean[2]
    assert again[3].tobytes() == clean[3].tobytes() and again[4].tobytes() == clean[4].tobytes()
    dirty()
    system_again = dv._register_rays_system_call(d_rays, d_ranges, MP.generic(), RY.BAND, 0, RY.R_MIN, RY.R_MAX)
    assert system_again[0].tobytes() == clean_system[0].tobytes() and system_again[1] == clean_system[1]


@pytest.mark.parametrize("step", ["release_blocks", "carve_rays"])
def test_the_state_another_operation_left(api, orc, step):
    """behind release_blocks (the pool rebuilt, the table compacted) and behind carve_rays (voxels near the surface rewritten)
    on the same volume: the terms are the statement's on the state that operation left, and the call changes no byte of it"""
    hv = R.clone(orc, CR.volume(orc))
    dv = device_copy(api, hv)
    side = ML.DeviceSide(api, {"map": dv})
    record = ML.release_blocks("unobserved+no-surface") if step == "release_blocks" else ML.carve_rays(0)
    want_counts = record.host(orc, {"map": hv})
    got_counts = record.device(orc, side, want_counts)
    print(record, "counts", got_counts, want_counts)
    assert ML.same(got_counts, want_counts) and record.work(want_counts)
    sync()
    assert dv.host_voxels().tobytes() == hv.voxels.tobytes()
    rays, ranges = IR.all_rays(orc, False)
    _, r_min, r_max = form(False)
    want = RY.terms(RY.Map(hv), rays, ranges, MP.generic(), RY.BAND, r_min, r_max, False)
    got = device_terms(dv, on_device(rays), on_device(ranges), MP.generic(), False)
    print("counts", want.counts, "against the untouched scene", statement(orc, SAME, False, "generic")[2].counts)
    assert want.counts[2] > 1000 and want.counts != statement(orc, SAME, False, "generic")[2].counts
    assert_terms(got, want)
    dv._register_rays_call(on_device(rays), on_device(ranges), T.Transform.identity(), 2, RY.BAND, 0, r_min, r_max)
    sync()
    assert dv.host_voxels().tobytes() == hv.voxels.tobytes() and np.array_equal(dv.host_entries(), hv.hash_entries)


def test_localise_then_map(api, orc):
    """the found pose is handed, on the device, to integrate_rays into a fresh volume; cast_rays from the true pose then agrees
    with the source map's ranges within one voxel length on the rays both hit"""
    rays, ranges, truth = RY.displaced_sweep(orc)
    dv = device_copy(api, RY.world(orc).hv)
    d_rays, d_ranges = on_device(rays), on_device(ranges)
    result = dv.register_rays(d_rays, d_ranges, r_min=RY.R_MIN, r_max=RY.R_MAX)
    print(result, "error", RR.pose_error(result.pose, truth))
    assert result.converged and hasattr(result.device_pose, "data_ptr")
    fresh = device_copy(api, M.fresh(orc, 509, 4096))
    counts = fresh.integrate_rays(d_rays, d_ranges, pose=result.device_pose, r_min=RY.R_MIN, r_max=RY.R_MAX)
    hits = fresh.cast_rays(d_rays, pose=truth, t_max=CR.T_MAX, max_steps=CR.MAX_STEPS, color=False)
    t, status = hits.t.cpu().numpy(), hits.status.cpu().numpy()
    both = (status == CR.HIT) & (ranges > 0)
    error = np.abs(t[both] - ranges[both])
    print("integrated", counts, "both hit", int(both.sum()), "worst", float(error.max()), "voxel", R.VOXEL)
    assert counts[0] == 19200 and both.sum() > 15000
    assert error.max() <= float(np.float32(R.VOXEL))
