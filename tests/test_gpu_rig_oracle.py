"""The rig Track of more than one camera (BASELINE configs[4]) against its oracle: tests/golden/rig_views.json holds what
oracle.rig_track(increment="rig") computes for the eight-camera ring at 160 x 120 — every step's update and per-view
packed systems, the final poses, the step count (tests/golden/make_rig_views.py; tests/test_oracle_rig.py holds the
oracle itself). Before this file the device's rig arithmetic with more than one view had only been compared with
itself, on the one ring (0 / 180 degrees) whose symmetry hides that upstream's per-camera ApplyUpdate bends a rig.

One process, one GPU, no peers: the stage solve bit for bit, the eight views stage by stage, and the hooked Track of
each view with the other seven played back from the file. 75 pixel groups per view; every test is a few dozen small
launches."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_rig_views as rv  # noqa: E402
from gpu_support import _without_parameter, api, sync  # noqa: F401
from vulcan_amd import vk_types as T  # noqa: E402

pytestmark = pytest.mark.gpu

NAME = "eight_160x120"
RING, W, H, _ = rv.RECORDED[NAME]
POSE_BOUND = 2e-5          # the project's bound for a free-running Track against the oracle's (tests/test_gpu_parity.py)
ERROR_BOUND = 5e-4         # the project's bound for a rig's pose after a Track (tests/test_gpu_rig_two_ranks.py)
RIGIDITY_BOUND = 4.1e-5    # two poses within POSE_BOUND of an oracle whose own rigidity is 1.2e-7


@pytest.fixture(scope="module")
def golden():
    assert os.path.exists(rv.FILE), "run python tests/golden/make_rig_views.py"
    track = rv.load()["rigs"][NAME]["tracks"][0]
    assert track["rigidity"] <= 1.2e-7 and track["error"] < 5e-7        # what RIGIDITY_BOUND allows for
    return track


@pytest.fixture(scope="module")
def views(api):
    """Per camera of the ring: (keyframe at the truth, frame — the same image — displaced with the whole rig)."""
    out = []
    k, error = rv.projection(W), rv.errors()[0]
    for rank, truth in enumerate(rv.truths(RING)):
        key = api.Frame(rv.view_depth(rank, W, H), k, truth)
        key.compute_normals()
        out.append((key, api.Frame(key.depth, k, error * truth, normals=key.normals)))
    sync()
    return out


def starts():
    return [rv.errors()[0] * truth for truth in rv.truths(RING)]


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


def max_pose_difference(poses, golden):
    return max(float(np.abs(np.array(p.m[:], dtype=np.float32) - np.float32(want)).max()) for p, want in zip(poses, golden["poses"]))


@pytest.mark.parametrize("translation", (True, False), ids=("translation", "rotation_only"))
@pytest.mark.parametrize("system", ("real", "zero", "rank_deficient"))
def test_rig_solve_update_matches_at_every_ring_pose(api, orc, golden, system, translation):
    """vk_icp_solve_update_rig against orc.icp_solve_update(increment="rig") on the same packed system — the ring's own
    first summed system, an all-zero one, a rank-deficient one — at each of the eight cameras' start poses: the update,
    Twc.m and Twc.inv bit for bit, state = {1 step, converged iff |update| < 1e-6}. The rig form must also really
    differ from the camera form wherever the system is not zero (else this test could not tell them apart)."""
    import torch
    n = 6 if translation else 3
    count = n * (n + 1) // 2
    total = rv.unpack27(np.float32(golden["systems"][0][0]))
    for values in golden["systems"][0][1:]:
        total = total + rv.unpack27(np.float32(values))                 # float32, rank order
    packed, grad = total[:count].copy(), total[36:36 + n].copy()
    if system == "zero":
        packed[:], grad[:] = 0, 0
    elif system == "rank_deficient":
        packed, grad = _without_parameter(packed, grad, n, n - 2)
    dh = torch.zeros(36, dtype=torch.float32, device="cuda")
    dh[:count] = torch.from_numpy(packed)
    dg = torch.zeros(6, dtype=torch.float32, device="cuda")
    dg[:n] = torch.from_numpy(grad)
    differs = 0
    for rank, start in enumerate(starts()):
        want, want_update, norm = orc.icp_solve_update(packed, grad, start, translation, increment="rig")
        camera, _, _ = orc.icp_solve_update(packed, grad, start, translation, increment="camera")
        differs += bytes(camera) != bytes(want)
        pose = torch.from_numpy(np.frombuffer(bytes(start), dtype=np.uint8).copy()).cuda()
        state = torch.zeros(2, dtype=torch.int32, device="cuda")
        upd = torch.full((6,), 7.0, dtype=torch.float32, device="cuda")
        api.check(api.lib().vk_icp_solve_update_rig(api._ptr(dh), api._ptr(dg), int(translation), api._ptr(pose),
                                                    api._ptr(state), api._ptr(upd), api.stream()), "vk_icp_solve_update_rig")
        sync()
        got = T.Transform.from_buffer_copy(pose.cpu().numpy().tobytes())
        print(f"{system} translation={translation} rank {rank}: |update| {norm:.3e}, "
              f"m {np.abs(np.array(got.m[:]) - np.array(want.m[:])).max():.3e}, "
              f"inv {np.abs(np.array(got.inv[:]) - np.array(want.inv[:])).max():.3e}")
        assert np.array_equal(bits(upd.cpu().numpy()), bits(want_update)), rank
        assert np.array_equal(bits(got.m[:]), bits(want.m[:])), rank
        assert np.array_equal(bits(got.inv[:]), bits(want.inv[:])), rank
        assert state.cpu().numpy().tolist() == [1, 1 if norm < 1e-6 else 0]
        # a second call on a converged state is a no-op (tracker.cpp:162)
        if norm < 1e-6:
            api.check(api.lib().vk_icp_solve_update_rig(api._ptr(dh), api._ptr(dg), int(translation), api._ptr(pose),
                                                        api._ptr(state), api._ptr(upd), api.stream()), "vk_icp_solve_update_rig")
            sync()
            assert pose.cpu().numpy().tobytes() == bytes(got) and state.cpu().numpy().tolist() == [1, 1]
    if system == "zero":
        assert norm == 0
    else:
        assert differs >= 6         # every camera that is not at yaw 0 / 180, at the least


def staged_rig_loop(api, views, solve):
    """The rig's Track stage by stage in one process: per step vk_icp_compute_system for each view at its device pose,
    the eight 48-float systems added in rank order in float32, `solve` (a stage solve of the library) on each pose.
    Returns (poses, steps, per-step updates)."""
    import torch
    trackers = []
    for (key, frame), start in zip(views, starts()):
        t = api.DepthTracker()
        t.keyframe = key
        api.check(api.lib().vk_transform_upload(api._ptr(t.pose), api._ref(start), api.stream()), "vk_transform_upload")
        trackers.append(t)
    total = torch.zeros(48, dtype=torch.float32, device="cuda")
    updates = []
    for _ in range(20):
        for t, (_, frame) in zip(trackers, views):
            t.compute_system(frame, pose_on_device=True)
        total.copy_(trackers[0].system)
        for t in trackers[1:]:
            total.add_(t.system)                                        # float32, rank order
        for t in trackers:
            api.check(solve(api._ptr(total[:36]), api._ptr(total[36:42]), 1, api._ptr(t.pose), api._ptr(t.state),
                            api._ptr(t.update), api.stream()), "stage solve")
        sync()
        states = [t.state.cpu().numpy().tolist() for t in trackers]
        assert all(s == states[0] for s in states)                      # one system, one solve: one state
        updates.append(trackers[0].update.cpu().numpy().copy())
        assert all(np.array_equal(bits(t.update.cpu().numpy()), bits(updates[-1])) for t in trackers)
        if states[0][1]:
            break
    poses = [T.Transform.from_buffer_copy(t.pose.cpu().numpy().tobytes()) for t in trackers]
    return poses, states[0][0], updates


def test_eight_views_stage_by_stage(api, views, golden):
    """Every final pose within 2e-5 per entry of the oracle's, the oracle's step count, the truth to 5e-4 and a rig that
    is still rigid (4.1e-5). The same loop with the plain stage solve — upstream's per-camera ApplyUpdate — must FAIL
    the rigidity bound (it bends the ring by 7.6e-3), or the bound above would prove nothing."""
    poses, steps, updates = staged_rig_loop(api, views, api.lib().vk_icp_solve_update_rig)
    difference, error, rigidity = max_pose_difference(poses, golden), rv.error_of(poses, RING), rv.rigidity_of(poses, RING)
    update_difference = max(float(np.abs(u - np.float32(w)).max()) for u, w in zip(updates, golden["updates"]))
    print(f"rig form: steps {steps} (oracle {golden['steps']}), pose - oracle {difference:.3e}, update - oracle "
          f"{update_difference:.3e}, error {error:.3e}, rigidity {rigidity:.3e}")
    camera_poses, camera_steps, _ = staged_rig_loop(api, views, api.lib().vk_icp_solve_update)
    camera_error, camera_rigidity = rv.error_of(camera_poses, RING), rv.rigidity_of(camera_poses, RING)
    print(f"camera form: steps {camera_steps}, error {camera_error:.3e}, rigidity {camera_rigidity:.3e}")
    assert steps == golden["steps"]
    assert difference <= POSE_BOUND
    assert error < ERROR_BOUND
    assert rigidity <= RIGIDITY_BOUND
    for p in poses:
        np.testing.assert_allclose(p.matrix().astype(np.float64) @ p.inverse_matrix().astype(np.float64), np.eye(4), atol=1e-5)
    assert camera_rigidity > RIGIDITY_BOUND and camera_steps < 20


@pytest.mark.parametrize("rank", range(8))
def test_hooked_track_of_each_view_with_the_others_played_back(api, views, golden, rank):
    """DepthTracker.track with a reduce hook and rig_increment=True, alone: at call s the hook replaces the system by the
    rank-ordered float32 sum of the tracker's own system and the file's systems of the other seven views at step s (calls
    past the recorded steps repeat the last record: steps after convergence are no-ops). The pose is the oracle's for
    that view to 2e-5 after the oracle's number of steps. The same hooked Track without the opt-in (the camera form) is
    run for the record and printed, not asserted: test_eight_views_stage_by_stage holds the proof that the forms differ."""
    import torch
    recorded = [[rv.unpack27(np.float32(v)) for v in step] for step in golden["systems"]]
    key, frame = views[rank]
    want = np.float32(golden["poses"][rank])
    out = {}
    for rig_increment in (True, False):
        calls, own_difference = [], []

        def hook(system):
            step = recorded[min(len(calls), len(recorded) - 1)]
            own = system.cpu().numpy().copy()
            own_difference.append(float(np.abs(own - step[rank]).max() / np.abs(step[rank]).max()))
            total = None
            for r in range(len(step)):
                term = own if r == rank else step[r]
                total = term.copy() if total is None else total + term
            system.copy_(torch.from_numpy(total))
            calls.append(1)

        tracker = api.DepthTracker()
        tracker.keyframe = key
        tracker.reduce_hook = hook
        tracker.rig_increment = rig_increment
        frame.depth_to_world = starts()[rank]
        got = tracker.track(frame)
        sync()
        steps, converged = (int(v) for v in tracker.state.cpu().numpy())
        out[rig_increment] = (float(np.abs(np.array(got.m[:], dtype=np.float32) - want).max()), steps, converged, len(calls))
        if rig_increment:
            # while the recorded steps last the tracker's own system is the file's for this view, to float32 sums' rounding
            print(f"rank {rank}: own system - oracle's, relative, per call {['%.1e' % d for d in own_difference[:len(recorded)]]}")
    frame.depth_to_world = starts()[rank]
    print(f"rank {rank}: rig form (pose - oracle, steps, converged, hook calls) {out[True]}, camera form {out[False]}")
    difference, steps, converged, calls = out[True]
    assert converged == 1 and steps == golden["steps"] and calls >= steps
    assert difference <= POSE_BOUND


def test_rig_increment_needs_a_hook(api, views):
    tracker = api.DepthTracker()
    tracker.keyframe = views[0][0]
    tracker.rig_increment = True
    with pytest.raises(ValueError):
        tracker.track(views[0][1])
    views[0][1].depth_to_world = starts()[0]
