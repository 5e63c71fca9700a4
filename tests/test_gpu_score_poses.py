"""vk_volume_score_poses and vk_volume_score_poses_best on the device against their CPU statement
(tests/score_poses_reference.py). The volume starts from an uploaded oracle state. A pair's D is register_rays' defined sequence
of float32 operations and a score's sums are integers, so all six fields of every score equal the statement's bit for bit: no
tolerance anywhere except the pose after localize_rays' refinement, which is vk_volume_register_rays' and is held to its bound
(2e-5 per entry, tests/test_gpu_register_rays.py). The rays are integrate_rays' sets (a)-(g), which reach every branch of the
definition (tests/test_register_rays_reference.py), and the far sweep of score_poses_reference."""
import ctypes as C

import numpy as np
import pytest

import cast_reference as CR
import integrate_rays_reference as IR
import map_life as ML
import merge_pose_reference as MP
import register_rays_reference as RY
import register_reference as RR
import release_reference as R
import score_poses_reference as SP
from gpu_support import OTHER, SAME, api, device_copy, form, on_device, sync, world  # noqa: F401
from vulcan_amd import vk_types as T

pytestmark = pytest.mark.gpu

RAY_COUNTS = (1, 63, 64, 65, 255, 256, 257, 513)               # ragged last waves and ray tiles (256 rays)
POSE_COUNTS = (1, 63, 64, 65, 130)                             # ragged pose tiles (8) and sum columns (32)
SPARE = 64                                                     # scores allocated past pose_count
_WANT, _RAGGED, _LOOP = {}, {}, {}


def many_poses():
    """130 poses: the eight, and 122 spread over the grid"""
    poses = SP.eight_poses() + SP.grid()[1][3::21][:122]
    assert len(poses) == max(POSE_COUNTS)
    return poses


def poses_on_device(poses):
    import torch
    return torch.from_numpy(np.frombuffer(b"".join(bytes(p) for p in poses), dtype=np.uint8).copy()).cuda()


def statement(orc, sizes, units, permuted=False):
    """(rays, ranges, the statement's scores at the eight poses) of all_rays in the form: once per case, never changed"""
    key = (sizes, units, permuted)
    if key not in _WANT:
        rays, ranges = IR.all_rays(orc, units)
        if permuted:
            rays, ranges = IR.permuted(rays, ranges)
        _, r_min, r_max = form(units)
        _WANT[key] = (rays, ranges, SP.score(world(orc, sizes), rays, ranges, SP.eight_poses(), SP.BAND, r_min, r_max, units))
    return _WANT[key]


def device_scores(dv, rays, ranges, poses, pose_count, units=False, count=None, scores=None, workspace=None):
    """the structured array of the first `pose_count` scores, and the raw bytes of the whole scores buffer"""
    flags, r_min, r_max = form(units)
    out = dv._score_poses_call(rays, ranges, poses, pose_count, SP.BAND, flags, r_min, r_max, count, scores, workspace)
    raw = out.cpu().numpy().tobytes()
    return np.frombuffer(raw[:pose_count * 32], dtype=SP.SCORE), raw


def noise(size, seed):
    import torch
    return torch.randint(0, 256, (size,), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


@pytest.mark.parametrize("sizes", [SAME, OTHER], ids=["long-chains", "other-bucket-count"])
@pytest.mark.parametrize("units", [False, True], ids=["metres", "voxel-units"])
def test_scores_bit_for_bit(api, orc, sizes, units):
    rays, ranges, want = statement(orc, sizes, units)
    dv = device_copy(api, world(orc, sizes).hv)
    got, _ = device_scores(dv, on_device(rays), on_device(ranges), poses_on_device(SP.eight_poses()), 8, units)
    for k in range(8):
        print(k, tuple(got[k]), tuple(want[k]))
    assert want["residuals"][:2].min() > 1000 and want["invalid"].min() > 0 and (want["sum_abs"][:2] > want["sum_squares"][:2]).all()
    assert got.tobytes() == want.tobytes()


def ragged_statement(orc, count):
    """the statement's scores of the first `count` rays of the shuffled sets at the 130 poses"""
    if count not in _RAGGED:
        rays, ranges = IR.permuted(*IR.all_rays(orc, False))
        _, r_min, r_max = form(False)
        _RAGGED[count] = SP.score(world(orc, SAME), rays[:count], ranges[:count], many_poses(), SP.BAND, r_min, r_max, False)
    return _RAGGED[count]


@pytest.mark.parametrize("count", RAY_COUNTS)
def test_ragged_counts(api, orc, count):
    """ragged last waves, ray tiles and pose tiles: the scores buffer and the workspace pre-filled with noise, the scores
    buffer longer than pose_count, and nothing past pose_count written"""
    rays, ranges = IR.permuted(*IR.all_rays(orc, False))
    want = ragged_statement(orc, count)
    dv = device_copy(api, world(orc, SAME).hv)
    d_rays, d_ranges, d_poses = on_device(rays), on_device(ranges), poses_on_device(many_poses())
    for pose_count in POSE_COUNTS:
        scores = noise((pose_count + SPARE) * 32, 1000 * count + pose_count)
        before = scores.cpu().numpy().tobytes()
        workspace = noise(api.lib().vk_volume_score_poses_workspace_bytes(count, pose_count), 7 * count + pose_count)
        assert workspace.data_ptr() % 16 == 0 and workspace.numel() >= 32 * pose_count
        got, raw = device_scores(dv, d_rays, d_ranges, d_poses, pose_count, False, count, scores, workspace)
        assert got.tobytes() == want[:pose_count].tobytes(), (count, pose_count)
        assert raw[pose_count * 32:] == before[pose_count * 32:], (count, pose_count)
    print("count", count, "residuals per pose", want["residuals"][:8], "most", want["residuals"].max())


def test_the_counts_are_register_rays_counts(api, orc):
    """per pose, the four counts are what vk_volume_register_rays_system writes at that pose: the new code against the old"""
    rays, ranges, want = statement(orc, SAME, False)
    dv = device_copy(api, world(orc, SAME).hv)
    d_rays, d_ranges = on_device(rays), on_device(ranges)
    got, _ = device_scores(dv, d_rays, d_ranges, poses_on_device(SP.eight_poses()), 8)
    flags, r_min, r_max = form(False)
    for k, pose in enumerate(SP.eight_poses()):
        _, counts = dv._register_rays_system_call(d_rays, d_ranges, pose, SP.BAND, flags, r_min, r_max)
        print(k, counts, tuple(got[k]))
        assert counts == (got[k]["measured"], got[k]["sampled"], got[k]["residuals"], got[k]["invalid"])


def one_residual_test(orc):
    """(rays, ranges, poses) for test_one_residual_test, checked on the CPU: 513 rays spread over the displaced sweep; its truth,
    the identity and seven of the eight poses. Once."""
    if "cut" not in _LOOP:
        rays, ranges, truth = RY.displaced_sweep(orc)
        rays, ranges = np.ascontiguousarray(rays[::37][:513]), np.ascontiguousarray(ranges[::37][:513])
        poses = [truth, T.Transform.identity()] + SP.eight_poses()[1:]
        assert len(ranges) == 513 and len(poses) == 9
        # the equality below says something only if the test has residuals to sum and a sampled ray to refuse
        assert RY.terms(RY.world(orc), rays, ranges, truth).counts[2] >= 257
        assert any(RY.terms(RY.world(orc), rays, ranges, pose).branches["outside_band"] > 0 for pose in poses)
        _LOOP["cut"] = (rays, ranges, poses)
    return _LOOP["cut"]


@pytest.mark.parametrize("count", [1, 63, 257, 513])
def test_one_residual_test(api, orc, count):
    """the two entry points share one residual test on the device: at every pose, score_poses' six numbers are what
    vk_volume_register_rays_terms and vk_volume_register_rays_system give there for the same rays. 9 poses are one past a pose
    tile; the counts are inside a wave, past score_poses' workgroup of 256 and past register_rays' of 512."""
    rays, ranges, poses = one_residual_test(orc)
    dv = device_copy(api, RY.world(orc).hv)
    d_rays, d_ranges = on_device(rays[:count]), on_device(ranges[:count])
    got, _ = device_scores(dv, d_rays, d_ranges, poses_on_device(poses), len(poses), False, count)
    flags, r_min, r_max = form(False)
    for k, pose in enumerate(poses):
        valid, residuals, _ = dv._register_rays_terms_call(d_rays, d_ranges, pose, SP.BAND, flags, r_min, r_max, count)
        _, counts = dv._register_rays_system_call(d_rays, d_ranges, pose, SP.BAND, flags, r_min, r_max, count)
        valid, residuals = valid.cpu().numpy() != 0, residuals.cpu().numpy()
        sum_abs, sum_squares = SP.quantised(residuals[valid])              # float32, then int64
        want = (counts[0], counts[1], int(valid.sum()), counts[3], int(sum_abs.sum()), int(sum_squares.sum()))
        print(count, k, tuple(got[k]), want)
        assert tuple(int(x) for x in got[k]) == want and counts[2] == want[2]


def test_permuted_rays_permuted_poses_and_a_second_call(api, orc):
    rays, ranges, want = statement(orc, SAME, False)
    shuffled = IR.permuted(rays, ranges)
    dv = device_copy(api, world(orc, SAME).hv)
    d_poses = poses_on_device(SP.eight_poses())
    first, _ = device_scores(dv, on_device(rays), on_device(ranges), d_poses, 8)
    again, _ = device_scores(dv, on_device(rays), on_device(ranges), d_poses, 8)
    other_rays, _ = device_scores(dv, on_device(shuffled[0]), on_device(shuffled[1]), d_poses, 8)
    assert first.tobytes() == want.tobytes() and again.tobytes() == first.tobytes() and other_rays.tobytes() == first.tobytes()
    order = np.random.default_rng(11).permutation(8)
    assert not np.array_equal(order, np.arange(8))
    other_poses, _ = device_scores(dv, on_device(rays), on_device(ranges), poses_on_device([SP.eight_poses()[k] for k in order]), 8)
    assert other_poses.tobytes() == want[order].tobytes()
    # through the class, from a list of Transforms and from a device tensor of them
    flags, r_min, r_max = form(False)
    for poses in (SP.eight_poses(), d_poses):
        scored = dv.score_poses(on_device(rays), on_device(ranges), poses, r_min=r_min, r_max=r_max)
        assert len(scored) == 8 and scored.host().tobytes() == want.tobytes()
        assert np.allclose(scored.mean_abs, SP.mean_abs(want)) and np.allclose(scored.rms ** 2, want["sum_squares"] / 1048576.0 / want["residuals"])
    none = dv.score_poses(on_device(rays)[:0], on_device(ranges)[:0], SP.eight_poses())            # no rays: no call
    assert none.host().tobytes() == bytes(8 * 32) and none.best() == (-1, None)


def test_the_volume_keeps_its_bytes(api, orc):
    rays, ranges, _ = statement(orc, SAME, False)
    hv = world(orc, SAME).hv
    dv = device_copy(api, hv)
    device_scores(dv, on_device(rays), on_device(ranges), poses_on_device(SP.eight_poses()), 8)
    sync()
    assert dv.host_voxels().tobytes() == hv.voxels.tobytes() and np.array_equal(dv.host_entries(), hv.hash_entries)


@pytest.mark.parametrize("step", ["release_blocks", "carve_rays"])
def test_the_state_another_operation_left(api, orc, step):
    """behind release_blocks (the pool rebuilt, the table compacted) and behind carve_rays (voxels near the surface rewritten)
    on the same volume: the scores are the statement's on the state that operation left, and the call changes no byte of it"""
    hv = R.clone(orc, CR.volume(orc))
    dv = device_copy(api, hv)
    side = ML.DeviceSide(api, {"map": dv})
    record = ML.release_blocks("unobserved+no-surface") if step == "release_blocks" else ML.carve_rays(0)
    want_counts = record.host(orc, {"map": hv})
    got_counts = record.device(orc, side, want_counts)
    assert ML.same(got_counts, want_counts) and record.work(want_counts)
    sync()
    assert dv.host_voxels().tobytes() == hv.voxels.tobytes()
    rays, ranges = IR.all_rays(orc, False)
    _, r_min, r_max = form(False)
    poses = SP.eight_poses()[:4]
    want = SP.score(RY.Map(hv), rays, ranges, poses, SP.BAND, r_min, r_max, False)
    got, _ = device_scores(dv, on_device(rays), on_device(ranges), poses_on_device(poses), 4)
    untouched = statement(orc, SAME, False)[2][:4]
    print("scores", [tuple(s) for s in want], "against the untouched scene", [tuple(s) for s in untouched])
    assert want["residuals"].max() > 1000 and want.tobytes() != untouched.tobytes()
    assert got.tobytes() == want.tobytes()
    sync()
    assert dv.host_voxels().tobytes() == hv.voxels.tobytes() and np.array_equal(dv.host_entries(), hv.hash_entries)


def _table(rows):
    out = np.zeros(len(rows), dtype=SP.SCORE)
    for k, (residuals, sum_abs) in enumerate(rows):
        out[k]["residuals"], out[k]["sum_abs"], out[k]["measured"], out[k]["sampled"] = residuals, sum_abs, 1 << 20, 1 << 20
    return out


TABLES = {
    "most-residuals": [(5, 10), (9, 500), (7, 1)],
    "then-least-sum": [(9, 500), (9, 499), (9, 501)],
    "then-least-index": [(3, 7), (9, 499), (9, 499), (9, 499)],
    "beyond-32-bits": [(9, 1 << 41), (9, (1 << 41) - 1)],
    "one": [(9, 5)],
    "nothing": [(0, 0), (0, 0)],
    "last-of-many": [(4, 50)] * 2999 + [(4, 49)],
    "first-of-many": [(4, 50)] * 3000,
    "across-waves": [(k % 1500, 7) for k in range(3000)],
}


@pytest.mark.parametrize("name", sorted(TABLES))
def test_best_orders_like_the_statement(api, name):
    """vk_volume_score_poses_best on score tables written by hand: the total order, and -1 with pose_out's bytes left alone"""
    import torch
    table = _table(TABLES[name])
    count = len(table)
    poses = [T.Transform.translate(float(k), 0.0, 0.0) for k in range(count)]
    scored = api.PoseScores(torch.from_numpy(np.frombuffer(table.tobytes(), dtype=np.uint8).copy()).cuda(), poses_on_device(poses), count, "cuda")
    top = int(table["residuals"].max())
    for min_residuals in sorted({1, max(top, 1), top + 1}):
        want = SP.best(table, min_residuals)
        best, pose_out = torch.full((1,), 77, dtype=torch.int32, device="cuda"), noise(128, count)
        before = pose_out.cpu().numpy().tobytes()
        scored._best_call(min_residuals, best, pose_out)
        got = int(best.cpu()[0])
        print(name, "min_residuals", min_residuals, "best", got, want)
        assert got == want
        assert pose_out.cpu().numpy().tobytes() == (bytes(poses[want]) if want >= 0 else before)
        index, device_pose = scored.best(min_residuals)
        assert index == want and (device_pose is None if want < 0 else device_pose.cpu().numpy().tobytes() == bytes(poses[want]))


def search_loop(orc):
    """the statement's search and its 20 steps from the candidate it names: once"""
    if "loop" not in _LOOP:
        s = SP.search(orc)
        k = SP.best(s["scores"], 600)
        _LOOP["loop"] = (k, RY.register(orc, RY.world(orc), s["rays"], s["ranges"], s["poses"][k], iterations=20))
    return _LOOP["loop"]


def test_the_grid_scores_and_best(api, orc):
    """2 625 poses x 1 200 rays: every score, the best, its pose's bytes, and no best above its residuals"""
    s = SP.search(orc)
    dv = device_copy(api, RY.world(orc).hv)
    scored = dv.score_poses(on_device(s["rays"]), on_device(s["ranges"]), s["poses"], r_min=SP.R_MIN, r_max=SP.R_MAX)
    assert scored.host().tobytes() == s["scores"].tobytes()
    want = SP.best(s["scores"], 600)
    index, device_pose = scored.best(600)
    print("best", index, s["labels"][index], tuple(scored.host()[index]))
    assert index == want and s["labels"][index] == SP.BEST and device_pose.cpu().numpy().tobytes() == bytes(s["poses"][want])
    assert scored.best(716)[0] == want and scored.best(717) == (-1, None) and SP.best(s["scores"], 717) == -1


def test_localise_from_far_away(api, orc):
    s = SP.search(orc)
    k, want = search_loop(orc)
    hv = RY.world(orc).hv
    dv = device_copy(api, hv)
    d_rays, d_ranges = on_device(s["rays"]), on_device(s["ranges"])
    # register_rays alone, from the identity, finds nothing to hold on to: the test needs the feature
    alone = dv.register_rays(d_rays, d_ranges, r_min=SP.R_MIN, r_max=SP.R_MAX)
    print("alone", alone)
    assert not alone.overlap and not alone.converged
    result = dv.localize_rays(d_rays, d_ranges, s["poses"], r_min=SP.R_MIN, r_max=SP.R_MAX)
    print(result, "best", result.best_index, "statement", k, want.steps, want.code, "error", RR.pose_error(result.pose, s["truth"]))
    print("pose: worst entry", float(np.abs(result.pose.matrix() - want.pose.matrix()).max()))
    assert result.best_index == k and s["labels"][k] == SP.BEST
    assert (result.steps, result.converged, result.overlap) == (want.steps, want.code == 1, True) and want.code == 1
    assert np.abs(result.pose.matrix() - want.pose.matrix()).max() <= 2e-5
    assert np.abs(result.pose.inverse_matrix() - want.pose.inverse_matrix()).max() <= 2e-5
    assert result.device_pose.cpu().numpy().tobytes() == bytes(result.pose)
    sync()
    assert dv.host_voxels().tobytes() == hv.voxels.tobytes() and np.array_equal(dv.host_entries(), hv.hash_entries)
    with pytest.raises(api.VkError):
        dv.localize_rays(d_rays, d_ranges, s["poses"][:40], min_residuals=1000, r_min=SP.R_MIN, r_max=SP.R_MAX)
    assert C.sizeof(T.Transform) == 128
