"""The CPU statement of vk_volume_score_poses (tests/score_poses_reference.py) on the project's own scene: one (pose, ray) pair
by hand, the scores against register_rays_reference.terms, the search from far away, the order of _best, and the host checks
of the built library.

The figures the method gave before any of this was written (register_rays_reference on cast_reference.volume, its 19 200 pixel
rays with cast_rays' ranges displaced by translate(0.12, -0.09, 0.06) * yaw(25) * pitch(-8), 161.6 mm / 26.2 degrees from the
identity): register from the identity finds 1 541 residuals, then none, and ends with NO_OVERLAP after 2 steps, 0.56 m from the
truth. Every 16th ray scored at the 2 625 candidates of score_poses_reference.grid() (none closer to the truth than 45.8 mm
and 5.4 degrees) ranks candidate (20, -10, (0.16, -0.08, 0.08)) first with sampled 797, residuals 716, sum_abs 237 758 401;
register from it: 5 steps, 0.0752 mm, 0.0068 degrees, as from each of the eight best-ranked candidates."""
import ctypes as C

import numpy as np

from abi_support import fake_volume
import integrate_rays_reference as IR
import merge_pose_reference as MP
import register_rays_reference as RY
import register_reference as RR
import score_poses_reference as SP
from vulcan_amd import vk_types as T

f32 = np.float32
MAX_STEPS, MAX_METRES, MAX_DEGREES = 10, 0.1e-3, 0.012          # vk_volume_register_rays' bounds (test_register_rays_reference.py)


def test_one_pair_by_hand(orc):
    """a pixel ray in metres at generic(): the carried ray, the endpoint, the eight voxels, D and its two integer terms"""
    world = RY.world(orc)
    hv = world.hv
    rays, ranges = IR.pixel_hits(orc)
    pose = MP.generic()
    whole = RY.terms(world, rays, ranges, pose)
    one = int(np.flatnonzero(whole.valid)[len(np.flatnonzero(whole.valid)) // 2])
    L = f32(hv.voxel_length)
    m = pose.matrix()
    o, d = rays[one, :3], rays[one, 3:]
    carried = lambda a, w: [f32(f32(f32(m[r, 0] * a[0] + m[r, 1] * a[1]) + m[r, 2] * a[2]) + w * m[r, 3]) for r in range(3)]   # noqa: E731
    got = RY.terms(world, rays[one:one + 1], ranges[one:one + 1], pose)
    assert got.counts == (1, 1, 1, 0)
    D = got.r[0]
    # the endpoint, from the statement's own carried ray (integrate_rays_reference.carried), then the sample by hand
    oo, nn, rr, kind = IR.carried(hv, rays[one:one + 1], ranges[one:one + 1], pose, SP.R_MIN, SP.R_MAX, False)
    assert kind[0] == IR.INTEGRATED and rr[0] == ranges[one] / L
    # (a few metres times float32's 6e-8, several roundings: 1e-5 m)
    assert np.allclose(oo[0] * L, carried(o, f32(1)), atol=1e-5) and np.allclose(nn[0], carried(d, f32(0)) / np.linalg.norm(carried(d, f32(0))), atol=1e-5)
    e = oo[0] + rr[0] * nn[0]
    g = e - f32(0.5)
    b = np.floor(g)
    fx, fy, fz = g - b
    base = b.astype(np.int64)
    v = []
    for k in range(8):
        p = base + np.array([k & 1, (k >> 1) & 1, k >> 2])
        cell = hv.voxels[world.table[tuple(int(c) for c in p >> 3)] * 512 + (p[2] & 7) * 64 + (p[1] & 7) * 8 + (p[0] & 7)]
        assert cell["distance_weight"] != 0
        v.append(f32(cell["distance"]))
    lerp = lambda t, a, c: a + t * (c - a)   # noqa: E731
    by_hand = lerp(fz, lerp(fy, lerp(fx, v[0], v[1]), lerp(fx, v[2], v[3])), lerp(fy, lerp(fx, v[4], v[5]), lerp(fx, v[6], v[7])))
    assert by_hand.dtype == f32 and by_hand.view(np.uint32) == D.view(np.uint32) and abs(D) < SP.BAND
    a = int(np.rint(np.float64(abs(D)) * 1048576.0))             # the product with 2^20 is exact in float32 and in float64
    s = int(np.rint(np.float64(f32(D * D)) * 1048576.0))
    s_one = SP.score(world, rays[one:one + 1], ranges[one:one + 1], [pose])[0]
    print("ray", one, "e", e, "D", D, "terms", a, s)
    assert a > 0 and tuple(s_one) == (1, 1, 1, 0, a, s)
    assert abs(a / 1048576.0 - abs(float(D))) <= 0.5 / 1048576.0 and abs(s / 1048576.0 - float(D) ** 2) <= 0.5 / 1048576.0 + 1e-7 * float(D) ** 2


def test_a_score_is_the_terms_counts_and_sums(orc):
    world = RY.world(orc)
    rays, ranges, _ = RY.displaced_sweep(orc)
    poses = [T.Transform.identity(), MP.generic()]
    scores = SP.score(world, rays, ranges, poses)
    for pose, s in zip(poses, scores):
        t = RY.terms(world, rays, ranges, pose)
        total, _ = RY.system(t)
        n = t.counts[2]
        print(tuple(s), "rms^2", total[42] / n, s["sum_squares"] / 1048576.0 / n, "mean |D|", SP.mean_abs(scores[:1]))
        assert (s["measured"], s["sampled"], s["residuals"], s["invalid"]) == t.counts and n > 1000
        # half a unit per term: |sum_squares / 2^20 - sum D^2| <= n / 2^21
        assert abs(s["sum_squares"] / 1048576.0 / n - total[42] / n) <= 0.5 / 1048576.0
        assert abs(s["sum_abs"] / 1048576.0 / n - float(np.abs(t.r[t.valid != 0].astype(np.float64)).sum()) / n) <= 0.5 / 1048576.0
        # the bounds vk.h states: a term <= 2^20, so a pose's sum <= 2^20 * count
        assert 0 <= s["sum_squares"] <= s["sum_abs"] <= n << 20


def test_the_grid_is_far_from_the_truth(orc):
    labels, poses = SP.grid()
    truth = SP.far_truth()
    start = RR.pose_error(T.Transform.identity(), truth)
    errors = np.array([RR.pose_error(p, truth) for p in poses])
    print("start %.1f mm %.1f degrees; nearest candidate %.1f mm, %.1f degrees" % (start[0] * 1e3, start[1], errors[:, 0].min() * 1e3,
                                                                                  errors[:, 1].min()))
    assert len(poses) == 2625 and labels[0] == (-30, -10, (-0.16, -0.16, -0.16)) and labels[1][2] == (-0.16, -0.16, -0.08)
    assert abs(start[0] * 1e3 - 161.6) < 0.05 and abs(start[1] - 26.2) < 0.05
    assert abs(errors[:, 0].min() * 1e3 - 45.8) < 0.05 and abs(errors[:, 1].min() - 5.4) < 0.05


def test_register_rays_alone_fails_from_the_identity(orc):
    rays, ranges, truth = RY.displaced_sweep(orc, SP.far_truth())
    out = RY.register(orc, RY.world(orc), rays, ranges, T.Transform.identity(), iterations=20)
    metres, _ = RR.pose_error(out.pose, truth)
    print("steps", out.steps, "code", out.code, "history", out.history, "%.2f m" % metres)
    assert (out.steps, out.code) == (2, RY.NO_OVERLAP) and [h[0] for h in out.history] == [1541, 0]
    assert abs(metres - 0.56) < 0.005
    s = SP.search(orc)
    sparse = RY.register(orc, RY.world(orc), s["rays"], s["ranges"], T.Transform.identity(), iterations=20)
    assert sparse.code == RY.NO_OVERLAP


def test_the_search_finds_a_start_that_converges(orc):
    s = SP.search(orc)
    scores = s["scores"]
    assert len(s["ranges"]) == 1200 and len(scores) == 2625
    k = SP.best(scores, 600)
    print("best", k, s["labels"][k], tuple(scores[k]))
    assert s["labels"][k] == SP.BEST
    assert (scores[k]["sampled"], scores[k]["residuals"], scores[k]["sum_abs"]) == (797, 716, 237758401)
    out = RY.register(orc, RY.world(orc), s["rays"], s["ranges"], s["poses"][k], iterations=20)
    metres, degrees = RR.pose_error(out.pose, s["truth"])
    print("steps %d code %d, %.4f mm %.5f degrees" % (out.steps, out.code, metres * 1e3, degrees))
    assert out.code == 1 and out.steps <= MAX_STEPS and metres < MAX_METRES and degrees < MAX_DEGREES
    assert out.steps == 5 and abs(metres * 1e3 - 0.0752) < 0.0005 and abs(degrees - 0.0068) < 0.0005


def test_the_eight_best_ranked_converge(orc):
    s = SP.search(orc)
    scores = s["scores"]
    order = np.lexsort((np.arange(len(scores)), scores["sum_abs"], -scores["residuals"].astype(np.int64)))
    assert int(order[0]) == SP.best(scores, 1)
    for k in order[1:8]:
        out = RY.register(orc, RY.world(orc), s["rays"], s["ranges"], s["poses"][int(k)], iterations=20)
        metres, degrees = RR.pose_error(out.pose, s["truth"])
        print(int(k), s["labels"][int(k)], tuple(scores[int(k)]), out.steps, "%.4f mm %.5f degrees" % (metres * 1e3, degrees))
        assert out.code == 1 and metres < MAX_METRES and degrees < MAX_DEGREES


def _scores(rows):
    out = np.zeros(len(rows), dtype=SP.SCORE)
    for k, (residuals, sum_abs) in enumerate(rows):
        out[k]["residuals"], out[k]["sum_abs"], out[k]["measured"] = residuals, sum_abs, 1000
    return out


def test_the_order_of_best():
    assert SP.best(_scores([(5, 10), (9, 500), (7, 1)]), 1) == 1                        # most residuals first
    assert SP.best(_scores([(9, 500), (9, 499), (9, 501)]), 1) == 1                     # then the smallest sum_abs
    assert SP.best(_scores([(3, 7), (9, 499), (9, 499), (9, 499)]), 1) == 1             # then the smallest index
    assert SP.best(_scores([(9, 1 << 41), (9, (1 << 41) - 1)]), 1) == 1                 # beyond 32 bits
    assert SP.best(_scores([(9, 5)]), 9) == 0 and SP.best(_scores([(9, 5)]), 10) == -1
    assert SP.best(_scores([(0, 0), (0, 0)]), 1) == -1
    assert SP.best(_scores([(4, 1), (6, 9), (5, 2)]), 7) == -1                          # all below min_residuals


def test_a_sweep_ten_metres_away_scores_nothing(orc):
    rays, ranges, _ = RY.displaced_sweep(orc)
    poses = [T.Transform.translate(10.0, 0.0, 0.0) * p for p in (T.Transform.identity(), MP.generic(), SP.grid()[1][7])]
    scores = SP.score(RY.world(orc), rays[::16], ranges[::16], poses)
    for s in scores:
        assert tuple(s) == (1200, 0, 0, 0, 0, 0)
    assert SP.best(scores, 1) == -1


def test_the_library_validates_before_touching_a_device():
    """every refusal vk.h lists, with addresses that are no memory: nothing may be enqueued (no GPU is needed, or touched)"""
    from vulcan_amd import api
    lib = api.lib()
    one, odd = C.c_void_p(4096), C.c_void_p(4096 + 8)
    assert C.sizeof(T.ScorePosesParams) == 24 and C.sizeof(T.PoseScore) == 32

    def params(flags=0, min_residuals=1, r_min=0.1, r_max=5.0, band=0.75):
        return T.ScorePosesParams(flags, min_residuals, r_min, r_max, band, 0)

    def call(v=fake_volume(), rays=one, ranges=one, count=8, poses=one, pose_count=8, p=params(), scores=one, workspace=one):
        return lib.vk_volume_score_poses(C.byref(v) if v else None, rays, ranges, count, poses, pose_count, C.byref(p) if p else None,
                                         scores, workspace, None)

    def best(scores=one, poses=one, pose_count=8, p=params(), best=one, pose_out=one):
        return lib.vk_volume_score_poses_best(scores, poses, pose_count, C.byref(p) if p else None, best, pose_out, None)

    assert call(v=None) == -1 and call(p=None) == -1 and call(poses=None) == -1 and call(workspace=None) == -1 and call(scores=None) == -1
    for field, value in (("hash_entries", None), ("voxel_length", 0.0), ("main_block_count", 0), ("voxels", (1 << 20) + 8)):
        broken = fake_volume()
        setattr(broken, field, value)
        assert call(v=broken) == -1, field
    for flags in (2, 3, 4, -1, 1 << 16):
        assert call(p=params(flags=flags)) == -1 and best(p=params(flags=flags)) == -1
    for min_residuals in (0, -1, -(1 << 31)):
        assert call(p=params(min_residuals=min_residuals)) == -1 and best(p=params(min_residuals=min_residuals)) == -1
    for band in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        assert call(p=params(band=band)) == -1
    for r_min, r_max in ((-0.001, 5.0), (1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (0.0, float("nan")), (float("nan"), 5.0),
                         (float("-inf"), 5.0), (0.0, 0.0)):
        assert call(p=params(r_min=r_min, r_max=r_max)) == -1
    assert call(count=-1) == -1 and call(count=(1 << 22) + 1) == -1
    for pose_count in (0, -1, 65537, 1 << 30):
        assert call(pose_count=pose_count) == -1 and call(count=0, pose_count=pose_count) == -1 and best(pose_count=pose_count) == -1
    # the product: 1 << 28 is the last one allowed (checked with count == 0's twin below: nothing may be enqueued here)
    assert call(count=(1 << 22), pose_count=65) == -1 and call(count=(1 << 12) + 1, pose_count=65536) == -1
    assert call(count=(1 << 14) + 1, pose_count=1 << 14) == -1
    assert call(rays=None) == -1 and call(ranges=None) == -1 and call(workspace=odd) == -1
    # count == 0 launches nothing, whatever else is allowed, but is checked like any call
    for flags in (0, 1):
        assert call(count=0, p=params(flags=flags, min_residuals=1 << 30, band=1.0)) == 0
    assert call(count=0, rays=None, ranges=None) == 0 and call(count=0, pose_count=65536) == 0 and call(count=0, pose_count=1) == 0
    assert call(count=0, workspace=None) == -1 and call(count=0, p=params(band=0.0)) == -1 and call(count=0, poses=None) == -1
    assert call(count=0, scores=None) == -1 and call(count=0, workspace=odd) == -1
    for name in ("scores", "poses", "p", "best", "pose_out"):
        assert best(**{name: None}) == -1, name
    size = lib.vk_volume_score_poses_workspace_bytes
    assert size(-1, 8) == 0 and size((1 << 22) + 1, 1) == 0 and size(8, 0) == 0 and size(8, 65537) == 0 and size(1 << 22, 65) == 0
    assert size(0, 1) >= 16 and size(1, 1) >= 32 and size(1 << 12, 65536) <= 1 << 28 and size(1200, 2625) % 16 == 0
