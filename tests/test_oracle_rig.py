"""The oracle of the rig Track (oracle.rig_track; BASELINE configs[4]: several cameras, one normal system, one solve, the
same world-frame increment applied to every camera), and the finding it was written for: upstream's ApplyUpdate
(depth_tracker.cpp:22-86, increment="camera") turns one update into a DIFFERENT world-frame motion per camera —
Tinc(1,2) = +u0 is no rotation to first order, and what Gram-Schmidt makes of Tinc * Twc depends on Twc — so every rig
but the 0/180 pair converges, bent, 6-8 mm from the truth. increment="rig" applies the pose-independent motion
D(u) = rigid_from(Tinc(u)). Rings and scenes: tests/golden/make_rig_views.py, at 160 x 120."""
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_rig_views as rv  # noqa: E402
from vulcan_amd import vk_types as T  # noqa: E402

W, H = 160, 120
BOUND = 5e-4            # the project's bound for a rig's pose after a Track (tests/test_gpu_rig_two_ranks.py)


def bits(t):
    return bytes(t)


@pytest.fixture(scope="module")
def tracked(orc):
    """(poses, steps, error, rigidity) per (ring, increment): computed once, shared."""
    out = {}
    for ring, increment in itertools.product(rv.RINGS, ("camera", "rig")):
        keys, frames = rv.oracle_rig(orc, ring, W, H, rv.errors()[0])
        poses, steps, _ = orc.rig_track(keys, frames, increment=increment)
        out[ring, increment] = (poses, steps, rv.error_of(poses, ring), rv.rigidity_of(poses, ring))
    return out


@pytest.mark.parametrize("increment", ["camera", "rig"])
@pytest.mark.parametrize("translation_enabled", [True, False])
@pytest.mark.parametrize("rank", [0, 3])
def test_one_view_is_icp_track_bit_for_bit(orc, increment, translation_enabled, rank):
    """A rig of one camera is a plain tracker, for both increments (the device's world == 1 keeps vk_icp_track's bits
    the same way): pose, step count, last update and every step's system."""
    keys, frames = rv.oracle_rig(orc, "eight", W, H, rv.errors()[0])
    key, frame = keys[rank], frames[rank]
    start = frame.depth_to_world
    record = []
    poses, steps, update = orc.rig_track([key], [frame], 20, translation_enabled, increment, record)
    assert bits(frame.depth_to_world) == bits(poses[0])
    frame.depth_to_world = start
    want, want_steps = orc.icp_track(key, frame, 20, translation_enabled)
    assert steps == want_steps and len(record) == steps and 2 <= steps <= 20
    assert bits(poses[0]) == bits(want)
    assert np.array_equal(record[-1]["update"], update)
    frame.depth_to_world = start
    hessian, gradient = orc.icp_system(key, frame, translation_enabled)
    assert np.array_equal(record[0]["systems"][0], orc.packed_system(hessian, gradient))


def test_one_view_solve_update_camera_bits_unchanged(orc):
    """increment="camera" is orc_icp_solve_update: the default argument and the explicit one are the same call."""
    rng = np.random.default_rng(3)
    J = rng.standard_normal((200, 6)).astype(np.float32)
    Hm = (J.T @ J).astype(np.float32)
    h = np.array([Hm[r, c] for r in range(6) for c in range(r + 1)], dtype=np.float32)
    g = (J.T @ (1e-3 * rng.standard_normal(200).astype(np.float32))).astype(np.float32)
    pose = rv.truths("eight")[3]
    a, b = orc.icp_solve_update(h, g, pose), orc.icp_solve_update(h, g, pose, increment="camera")
    assert bits(a[0]) == bits(b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    c = orc.icp_solve_update(h, g, pose, increment="rig")
    assert np.array_equal(a[1], c[1]) and a[2] == c[2]            # the same solve; only the application differs
    assert bits(a[0]) != bits(c[0])


@pytest.mark.parametrize("ring", ["pair_90", "eight"])
def test_camera_increment_bends_the_rig(tracked, ring):
    """The finding, pinned: the loop converges (fewer than 20 steps) on a rig that is bent and wrong."""
    _, steps, error, rigidity = tracked[ring, "camera"]
    print(ring, "camera", steps, error, rigidity)
    assert steps < 20
    assert error > 1e-3 and rigidity > 1e-3


@pytest.mark.parametrize("ring", list(rv.RINGS))
def test_rig_increment_recovers_the_truth(tracked, ring):
    _, steps, error, rigidity = tracked[ring, "rig"]
    print(ring, "rig", steps, error, rigidity)
    assert steps == 3
    assert error < BOUND and rigidity < BOUND


def test_the_aligned_pair_passes_either_way(tracked):
    """0/180 is the one ring whose symmetry hides the bend — and the only one the suite had."""
    for increment in ("camera", "rig"):
        _, _, error, rigidity = tracked["pair_180", increment]
        assert error < BOUND and rigidity < BOUND


def expm_so3(u):
    """exp([u]x), float64 (Rodrigues)"""
    u = np.asarray(u, dtype=np.float64)
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    a = np.linalg.norm(u)
    if a == 0:
        return np.eye(3)
    return np.eye(3) + np.sin(a) / a * K + (1 - np.cos(a)) / (a * a) * (K @ K)


UPDATES = [(1e-2, 0, 0, 0, 0, 0), (0, 1e-2, 0, 0, 0, 0), (0, 0, 1e-2, 0, 0, 0), (6e-3, -5e-3, 4e-3, 1e-3, 2e-3, -3e-3),
           (-3e-4, 2e-4, 1e-4, 0.01, -0.02, 0.03), (1e-6, -1e-6, 1e-6, 0, 0, 0), (0, 0, 0, 0, 0, 0)]


@pytest.mark.parametrize("u", UPDATES)
def test_increment_is_a_rotation_and_the_exponential_to_first_order(orc, u):
    """D(u) against float64: orthonormal to 1e-6, within |u|^2 of exp([u]x) (Gram-Schmidt of I + [u]x + the sign slip's
    symmetric part is first-order exact; float32 rounding, 1.2e-7 per entry, is allowed for on top), the translation is
    u[3:] unchanged, and the stored inverse is the inverse."""
    D = orc.icp_rig_increment(np.array(u, dtype=np.float32))
    m, inv = D.matrix().astype(np.float64), D.inverse_matrix().astype(np.float64)
    R = m[:3, :3]
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-6
    rotation = np.asarray(u[:3], dtype=np.float64)
    assert np.abs(R - expm_so3(rotation)).max() <= rotation @ rotation + 2.0 ** -22
    assert np.array_equal(m[:3, 3].astype(np.float32), np.array(u[3:], dtype=np.float32))
    assert np.abs(m @ inv - np.eye(4)).max() <= 1e-6
    assert np.array_equal(m[3], [0, 0, 0, 1])


def test_camera_increment_is_not_the_exponential(orc):
    """What the test above would say of upstream's form: at the identity pose rigid_from(Tinc * I) is D(u), but at
    another pose the motion it applies, rigid_from(Tinc * Twc) * Twc^-1, is O(|u0|) away from exp([u]x) — the bend."""
    u = np.array([1e-2, 0, 0, 0, 0, 0], dtype=np.float32)
    h = np.array([1.0 if r == c else 0.0 for r in range(6) for c in range(r + 1)], dtype=np.float32)
    g = -u                                                     # H = I: the solve returns update = -g = u
    for pose, bent in ((T.Transform.identity(), False), (rv.truths("pair_90")[1], True)):
        out, update, _ = orc.icp_solve_update(h, g, pose, increment="camera")
        assert np.array_equal(update, u)
        motion = out.matrix().astype(np.float64) @ pose.inverse_matrix().astype(np.float64)
        off = np.abs(motion[:3, :3] - expm_so3(u[:3])).max()
        assert (off > 1e-3) == bent, off
        rig, _, _ = orc.icp_solve_update(h, g, pose, increment="rig")
        motion = rig.matrix().astype(np.float64) @ pose.inverse_matrix().astype(np.float64)
        assert np.abs(motion[:3, :3] - expm_so3(u[:3])).max() <= float(u[:3] @ u[:3]) + 1e-6     # |u|^2 + float32 products


def test_increment_does_not_depend_on_the_pose(orc):
    """The motion the rig form applies, P_new * P_old^-1, is D(u) for every pose of the eight-camera ring (to the
    rounding of two float32 4x4 products and a Gram-Schmidt: 1e-6), displaced or not."""
    u = np.array([6e-3, -5e-3, 4e-3, 1e-3, 2e-3, -3e-3], dtype=np.float32)
    h = np.array([1.0 if r == c else 0.0 for r in range(6) for c in range(r + 1)], dtype=np.float32)
    D = orc.icp_rig_increment(u).matrix().astype(np.float64)
    for truth in rv.truths("eight"):
        for pose in (truth, rv.errors()[0] * truth, T.Transform.translate(0.4, -0.3, 1.2) * truth):
            out, update, _ = orc.icp_solve_update(h, -u, pose, increment="rig")
            assert np.array_equal(update, u)
            motion = out.matrix().astype(np.float64) @ pose.inverse_matrix().astype(np.float64)
            assert np.abs(motion - D).max() <= 1e-6


@pytest.mark.parametrize("ring", ["three", "eight"])
def test_order_of_the_sum(orc, tracked, ring):
    """Permuting the views moves the summed system by its last bits at most (27 float32 additions of same-signed or
    cancelling terms: 8 ulp of the largest term per entry is generous) and never changes the step count."""
    n = len(rv.RINGS[ring])
    first = None
    for order in (tuple(range(n)), tuple(reversed(range(n))), tuple(np.random.default_rng(5).permutation(n))):
        keys, frames = rv.oracle_rig(orc, ring, W, H, rv.errors()[0])
        record = []
        poses, steps, _ = orc.rig_track([keys[i] for i in order], [frames[i] for i in order], record=record)
        assert steps == tracked[ring, "rig"][1]
        systems = record[0]["systems"]
        total = systems[0].copy()
        for s in systems[1:]:
            total = total + s
        if first is None:
            first, scale = total, np.abs(np.stack(systems)).max(axis=0)
        else:
            assert np.all(np.abs(total - first) <= 8 * np.spacing(scale.astype(np.float32)) * n)
        back = [None] * n
        for slot, i in enumerate(order):
            back[i] = poses[slot]
        assert rv.error_of(back, ring) < BOUND


@pytest.mark.parametrize("increment", ["camera", "rig"])
@pytest.mark.parametrize("translation_enabled", [True, False])
def test_zero_system_leaves_the_pose(orc, increment, translation_enabled):
    """A view made entirely of holes contributes H = 0, g = 0; alone it solves to update = 0 and the pose stands."""
    keys, frames = rv.oracle_rig(orc, "pair_90", W, H, rv.errors()[0], holes=(0, 1))
    hessian, gradient = orc.icp_system(keys[1], frames[1], translation_enabled)
    assert not hessian.any() and not gradient.any()
    starts = [f.depth_to_world for f in frames]
    poses, steps, update = orc.rig_track(keys, frames, 20, translation_enabled, increment)
    assert steps == 1 and not update.any()
    for pose, start in zip(poses, starts):
        assert np.abs(pose.matrix() - start.matrix()).max() <= 2e-7          # re-orthonormalised, not moved
        assert np.isfinite(pose.matrix()).all() and np.isfinite(pose.inverse_matrix()).all()


def test_rotation_only_rig(orc):
    """translation_enabled=False: a 3 x 3 solve, update[3:] = 0; a rig that is only rotated comes back."""
    ring = "four"
    turn = T.Transform.rotate(0.999995, 0.002, -0.0015, 0.001)
    keys, frames = rv.oracle_rig(orc, ring, W, H, turn)
    record = []
    poses, steps, update = orc.rig_track(keys, frames, 20, False, "rig", record)
    assert steps < 20 and all(not r["update"][3:].any() for r in record)
    assert all(not s[6:21].any() and not s[39:42].any() for r in record for s in r["systems"])
    assert rv.error_of(poses, ring) < BOUND and rv.rigidity_of(poses, ring) < BOUND


@pytest.mark.parametrize("ring,blind", [("pair_90", 1), ("eight", 0), ("eight", 5)])
def test_a_blind_camera_is_carried_by_the_others(orc, ring, blind):
    """One camera sees nothing: its system is zero, the others' solve moves it too, and the whole rig — the blind
    camera included — ends at the truth."""
    keys, frames = rv.oracle_rig(orc, ring, W, H, rv.errors()[0], holes=(blind,))
    record = []
    poses, steps, _ = orc.rig_track(keys, frames, record=record)
    assert all(not r["systems"][blind].any() for r in record)
    assert steps < 20
    assert rv.error_of(poses, ring) < BOUND and rv.rigidity_of(poses, ring) < BOUND


def test_communicator_opts_a_tracker_in_only_on_a_real_rig():
    """Communicator.track selects the hook path's rig form (DepthTracker.rig_increment) when the rig has more than one
    rank, and leaves a tracker of a one-rank communicator as it is (no GPU: the tracker here only records the call)."""
    from vulcan_amd import comm

    class Recorder:
        rig_increment = False
        comm = None

        def track(self, frame):
            return (frame, self.rig_increment, self.comm)

    for world, want in ((1, False), (2, True), (8, True)):
        c, t = comm.Communicator.without_rccl(0, world), Recorder()
        assert c.track(t, "frame") == ("frame", want, c)
