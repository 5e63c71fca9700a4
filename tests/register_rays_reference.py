"""The CPU statement of vk_volume_register_rays (include/vk.h): the residual and Jacobian every range ray contributes at a pose
T_volume_rays, the normal system, one Gauss-Newton step and the loop — in numpy, on an oracle.HostVolume. There is no upstream
counterpart (the reference tracks pinhole depth images against a raycast keyframe), so this file is the definition.

The ray is integrate_rays_reference.carried's, the sample and the Jacobian are register_reference.sample / jacobian at the
ray's endpoint, the sums register_reference.system's and the step register_reference.step's. The per-ray terms are float32
with one rounding per operation, in the order vk.h gives: numpy's float32 arithmetic is exactly that, and the device is held
to them bit for bit (tests/test_gpu_register_rays.py). The sums are float64 sums of those float32 terms: the device adds in
float32 in its own fixed order and is held to the project's bound for a normal system."""
import numpy as np

import cast_reference as CR
import integrate_rays_reference as IR
import merge_pose_reference as MP
import register_reference as RR
from vulcan_amd import vk_types as T

f32 = np.float32
FAR = 1 << 30
NO_OVERLAP = RR.NO_OVERLAP
VOXEL_UNITS = T.VK_RAYS_VOXEL_UNITS
R_MIN, R_MAX = IR.R_MIN, IR.R_MAX
BAND = 0.75


class Map:
    """what does not depend on the pose: the volume's blocks"""

    def __init__(self, hv):
        self.hv = hv
        self.table = RR.block_table(hv)
        self.lookup = CR.Lookup(self.table)


class Terms:
    """valid [N] uint8, r [N], J [N, 6] (zeros where no residual exists), counts = (valid rays with a measurement, of those
    with a sample, residuals, invalid rays), and `branches`: how often each branch of the definition was taken"""

    def __init__(self, size):
        self.valid = np.zeros(size, dtype=np.uint8)
        self.r = np.zeros(size, dtype=f32)
        self.J = np.zeros((size, 6), dtype=f32)
        self.counts = (0, 0, 0, 0)
        self.branches = {}


def terms(world, rays, ranges, pose, band=BAND, r_min=R_MIN, r_max=R_MAX, voxel_units=False):
    """per ray i: valid, r, J. `world`: a Map. `pose`: a Transform, T_volume_rays."""
    hv = world.hv
    band = f32(band)
    o, n, r, kind = IR.carried(hv, rays, ranges, pose, r_min, r_max, voxel_units)
    out = Terms(len(r))
    measured = np.flatnonzero(kind == IR.INTEGRATED)
    with np.errstate(all="ignore"):
        e = o[measured] + r[measured, None] * n[measured]                                 # mul, add
        assert e.dtype == f32
        finite = np.isfinite(e).all(-1)
        at, e = measured[finite], e[finite]
        g = e - f32(0.5)
        b = np.floor(g)
        f = g - b
        base = np.clip(MP.to_int(b), -FAR, FAR)
        points = base[None] + MP.CORNERS[:, None, :]                                       # [8, N, 3]
        slots = world.lookup.slots((points >> 3).reshape(-1, 3)).reshape(8, -1)
        voxel = points & 7
        index = voxel[..., 2] * 64 + voxel[..., 1] * 8 + voxel[..., 0]
        there = slots >= 0
        got = hv.voxels[np.where(there, slots * 512 + index, 0)]
        weighted = got["distance_weight"] != 0
        exists = (there & weighted).all(0)
        v = [np.where(there[k], got["distance"][k], f32(0)) for k in range(8)]
        D, gradient = RR.sample(v, (f[:, 0], f[:, 1], f[:, 2]))
        valid = exists & (np.abs(D) < band)
        J = RR.jacobian((e[:, 0], e[:, 1], e[:, 2]), gradient, f32(1.0) / f32(hv.voxel_length))
    assert D.dtype == f32 and all(j.dtype == f32 for j in J)
    out.valid[at[valid]] = 1
    out.r[at[valid]] = D[valid]
    out.J[at[valid]] = np.stack(J, -1)[valid]
    out.counts = (len(measured), int(exists.sum()), int(valid.sum()), int((kind == IR.INVALID).sum()))
    leaves = ((base & 7) == 7).sum(-1)
    out.branches = dict(invalid=out.counts[3], unmeasured=int((kind == IR.NO_MEASUREMENT).sum()), not_finite=int((~finite).sum()),
                        absent_block=int((~there).any(0).sum()), unweighted_corner=int((there.all(0) & ~weighted.all(0)).sum()),
                        outside_band=int((exists & ~valid).sum()), leaves_1=int((leaves == 1).sum()), leaves_2=int((leaves == 2).sum()),
                        leaves_3=int((leaves == 3).sum()))
    return out


def system(t):
    """register_reference.system: (system[48] in float64, the sums of absolute terms in the same layout)"""
    return RR.system(t)


class Result:
    pass


def register(orc, world, rays, ranges, start, iterations=20, band=BAND, r_min=R_MIN, r_max=R_MAX, voxel_units=False):
    """the loop: `poses[k]` is the pose after k steps; system, counts and rms are the last evaluated step's"""
    out = Result()
    out.pose, out.steps, out.code, out.poses = T.Transform.from_matrices(start.matrix(), start.inverse_matrix()), 0, 0, []
    out.poses.append(out.pose)
    out.history = []
    for _ in range(iterations):
        evaluated = terms(world, rays, ranges, out.pose, band, r_min, r_max, voxel_units)
        out.system, out.absolute = system(evaluated)
        out.counts = evaluated.counts
        out.rms = float(np.sqrt(out.system[42] / out.counts[2])) if out.counts[2] else 0.0
        out.history.append((out.counts[2], out.rms))
        out.pose, out.update, out.code = RR.step(orc, out.system, out.counts, out.pose)
        out.steps += 1
        out.poses.append(out.pose)
        if out.code:
            break
    return out


# ---- the sweep the CPU and the GPU tests share -------------------------------------------------------------------------

_WORLD, _SWEEP = {}, {}


def world(orc):
    """cast_reference.volume (the bumps fused at the identity) as a Map: computed once, only read"""
    if "map" not in _WORLD:
        _WORLD["map"] = Map(CR.volume(orc))
    return _WORLD["map"]


def displaced_sweep(orc, truth=None):
    """(rays, ranges, truth): the volume's 19 200 pixel rays with cast_rays' ranges, re-expressed in a sensor frame displaced by
    `truth` = T_volume_rays (merge_pose_reference.generic()): registering them from the identity has to find `truth`. The
    change of frame is made in float64 and rounded once."""
    truth = MP.generic() if truth is None else truth
    key = bytes(truth)
    if key not in _SWEEP:
        rays, ranges = IR.pixel_hits(orc)
        back = np.linalg.inv(truth.matrix().astype(np.float64))
        there = np.zeros_like(rays)
        there[:, :3] = (rays[:, :3].astype(np.float64) @ back[:3, :3].T + back[:3, 3]).astype(f32)
        there[:, 3:] = (rays[:, 3:].astype(np.float64) @ back[:3, :3].T).astype(f32)
        _SWEEP[key] = (np.ascontiguousarray(there), np.ascontiguousarray(ranges, dtype=f32), truth)
    return _SWEEP[key]
