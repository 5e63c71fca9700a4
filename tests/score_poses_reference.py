"""The CPU statement of vk_volume_score_poses and vk_volume_score_poses_best (include/vk.h): what a sweep of range rays
scores at each of many candidate poses T_volume_rays, and which candidate explains it best — in numpy, on
register_rays_reference.terms. There is no upstream counterpart, so this file is the definition.

Per (pose, ray) the terms are vk_volume_register_rays' word for word: the float32 D of a residual is terms(...).r, and a
score holds that call's four counts and two INTEGER sums over the residuals, rint(|D| * 2^20) and rint((D * D) * 2^20), both
taken in float32 (the product with 2^20 is exact, D * D is rounded once) and added as int64. Integer sums commute, so the
device is held to every field bit for bit (tests/test_gpu_score_poses.py)."""
import itertools

import numpy as np

import merge_pose_reference as MP
import register_rays_reference as RY
import scenes
from vulcan_amd import vk_types as T

f32 = np.float32
BAND, R_MIN, R_MAX = RY.BAND, RY.R_MIN, RY.R_MAX
UNIT = f32(1048576.0)
SCORE = T.pose_score_dtype


def quantised(D):
    """(rint(|D| * 2^20), rint((D * D) * 2^20)) of float32 residuals, as int64"""
    D = np.asarray(D, dtype=f32)
    return np.rint(np.abs(D) * UNIT).astype(np.int64), np.rint((D * D) * UNIT).astype(np.int64)


def score_of(t):
    """the vk_pose_score of one register_rays_reference.Terms"""
    out = np.zeros((), dtype=SCORE)
    out["measured"], out["sampled"], out["residuals"], out["invalid"] = t.counts
    a, s = quantised(t.r[t.valid != 0])
    out["sum_abs"], out["sum_squares"] = a.sum(), s.sum()
    return out


def score(world, rays, ranges, poses, band=BAND, r_min=R_MIN, r_max=R_MAX, voxel_units=False):
    """the structured array [len(poses)] of vk_pose_score: `world` a register_rays_reference.Map, `poses` Transforms"""
    out = np.zeros(len(poses), dtype=SCORE)
    for k, pose in enumerate(poses):
        out[k] = score_of(RY.terms(world, rays, ranges, pose, band, r_min, r_max, voxel_units))
    return out


def best(scores, min_residuals):
    """the pose with the most residuals, then the smallest sum_abs, then the smallest index; -1 if it has too few"""
    if len(scores) == 0:
        return -1
    order = np.lexsort((np.arange(len(scores)), scores["sum_abs"], -scores["residuals"].astype(np.int64)))
    k = int(order[0])
    return k if scores["residuals"][k] >= min_residuals else -1


def mean_abs(scores):
    with np.errstate(all="ignore"):
        return np.where(scores["residuals"] > 0, scores["sum_abs"] / 1048576.0 / scores["residuals"], 0.0)


# ---- the search the CPU and the GPU tests share ------------------------------------------------------------------------

def pitch(degrees):
    """about x, written as merge_pose_reference.generic() writes its own"""
    a = np.deg2rad(degrees) / 2.0
    return T.Transform.rotate(np.cos(a), np.sin(a), 0.0, 0.0)


def far_truth():
    """161.6 mm and 26.2 degrees from the identity: too far for vk_volume_register_rays"""
    return T.Transform.translate(0.12, -0.09, 0.06) * scenes.yaw(25.0) * pitch(-8.0)


YAWS, PITCHES, SHIFTS = (-30, -20, -10, 0, 10, 20, 30), (-10, 0, 10), (-0.16, -0.08, 0.0, 0.08, 0.16)
EVERY = 16
BEST = (20, -10, (0.16, -0.08, 0.08))


def grid():
    """(labels, poses): 7 yaws x 3 pitches x 5^3 translations = 2 625 candidates, each translate * yaw * pitch"""
    labels = [(y, p, t) for y in YAWS for p in PITCHES for t in itertools.product(SHIFTS, SHIFTS, SHIFTS)]
    return labels, [T.Transform.translate(*t) * scenes.yaw(float(y)) * pitch(float(p)) for y, p, t in labels]


_SEARCH = {}


def search(orc):
    """the far sweep's every 16th ray scored at the grid, once per session and only read:
    dict(rays, ranges, truth, labels, poses, scores)"""
    if not _SEARCH:
        rays, ranges, truth = RY.displaced_sweep(orc, far_truth())
        rays, ranges = np.ascontiguousarray(rays[::EVERY]), np.ascontiguousarray(ranges[::EVERY])
        labels, poses = grid()
        _SEARCH.update(rays=rays, ranges=ranges, truth=truth, labels=labels, poses=poses,
                       scores=score(RY.world(orc), rays, ranges, poses))
        _SEARCH["scores"].setflags(write=False)
    return _SEARCH


def eight_poses():
    """the identity, generic() and six of the grid: what the device's bit-for-bit tests score"""
    _, poses = grid()
    return [T.Transform.identity(), MP.generic()] + [poses[k] for k in (0, 437, 1312, 2006, 2310, 2624)]
