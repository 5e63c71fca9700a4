"""The CPU statement of vk_volume_cast_rays (include/vk.h): what an arbitrary ray through a volume hits first and how far
away — status, distance along the ray, and vk_volume_sample's voxel and gradient at the hit — in numpy, on an
oracle.HostVolume. The march rule is the reference raycast's (src/tracer.cu:317-451, restated in oracle/oracle_trace.c:249-359)
in voxel units, with two changes a query that must not miss geometry needs: an absent block is left through its exit face
(the reference steps a whole block length and can jump a corner), and a surface is reported only when the ray crosses it
from its observed free side. There is no upstream call for a ray that is no pixel of a camera, so this file is the definition.

Everything is float32 with one rounding per operation, in the order vk.h gives: numpy's float32 arithmetic is exactly that
(its sqrt and division are correctly rounded), so no tolerance exists and the device is held to it bit for bit
(tests/test_gpu_cast.py). The distance sample is sample_reference.sample's, the pose merge_pose_reference's rows.

It is vectorised over rays with a per-ray active mask, and it holds the ray sets the CPU and the GPU tests share."""
import numpy as np

import merge_pose_reference as MP
import register_reference as RR
import release_reference as R
import sample_reference as S
from vulcan_amd import vk_types as T

f32 = np.float32
FAR = 1 << 30
VOXEL_UNITS, DISTANCE_ONLY = T.VK_CAST_VOXEL_UNITS, T.VK_CAST_DISTANCE_ONLY
MISS, HIT, STEPS, INVALID = T.VK_RAY_MISS, T.VK_RAY_HIT, T.VK_RAY_STEPS, T.VK_RAY_INVALID
# what the tests cast with: 5 m, and a step bound that the longest walks through empty space reach (the pixel rays take 34)
T_MAX, MAX_STEPS = 5.0, 150


class Lookup:
    """register_reference.block_table as sorted keys: the pool slots of many blocks at once"""

    SHIFT = np.array([1, 1 << 16, 1 << 32])

    def __init__(self, table):
        origins = np.array(list(table), dtype=np.int64).reshape(-1, 3)
        keys = (origins + 32768) @ self.SHIFT
        order = np.argsort(keys)
        self.keys, self.values = keys[order], np.array(list(table.values()), dtype=np.int64)[order]

    def slots(self, blocks):
        """pool slots of the blocks [N, 3], -1 when absent: a coordinate outside the int16 range is"""
        inside = ((blocks >= -32768) & (blocks <= 32767)).all(-1)
        keys = np.where(inside, (blocks + 32768) @ self.SHIFT, -1)
        if len(self.keys) == 0:
            return np.full(len(blocks), -1, dtype=np.int64)
        at = np.minimum(np.searchsorted(self.keys, keys), len(self.keys) - 1)
        return np.where(inside & (self.keys[at] == keys), self.values[at], -1)


def distance_sample(hv, p, table):
    """(exists [N], distance [N]) of vk_volume_sample's distance sample at p [N, 3], in voxels, by the USED rule"""
    if len(p) == 0:
        return np.zeros(0, dtype=bool), np.zeros(0, dtype=f32)
    got, _ = S.sample(hv, p, voxel_units=True, color=False, table=table)
    return got["distance_weight"] != 0, got["distance"]


class Cast:
    """status [N] int32, t [N] float32 (t_out), samples [N] of vk_types.voxel_dtype, gradients [N, 4] float32, and what the
    tests ask about the march: `armed` [N] at the end, `steps` [N], `t_voxels` [N] (the march's t where it ended),
    `origin` and `direction` [N, 3] (o and n, in voxels), and how often each branch was taken"""


def cast(hv, rays, pose=None, t_min=0.0, t_max=T_MAX, max_steps=MAX_STEPS, voxel_units=False, color=True, table=None):
    """`rays` [N, 6]: origin, direction. `pose`: a Transform, T_volume_rays, or None. `t_max`: a number, or one per ray (the
    call takes one number: an array stands for that many calls). `table`: RR.block_table(hv), when the caller has it."""
    x = np.ascontiguousarray(rays, dtype=f32).reshape(-1, 6)
    count = len(x)
    table = RR.block_table(hv) if table is None else table
    lookup = Lookup(table)
    out = Cast()
    out.branches = dict(absent=0, exit_at_zero=0, present=0, unobserved=0, window=0, window_sampled=0, armed_steps=0,
                        behind_steps=0, refined_twice=0)
    with np.errstate(all="ignore"):
        L = f32(hv.voxel_length)
        tr = f32(hv.truncation_length) / L
        t0 = f32(t_min) if voxel_units else f32(t_min) / L
        t1 = np.broadcast_to(np.asarray(t_max, dtype=f32) if voxel_units else np.asarray(t_max, dtype=f32) / L, (count,))
        q, d = (x[:, :3] if voxel_units else x[:, :3] / L), x[:, 3:]
        o = q
        if pose is not None:
            r = MP.rows(pose.m, hv.voxel_length)
            o = MP.apply(r, q)
            d = np.stack([(r[a, 0] * d[:, 0] + r[a, 1] * d[:, 1]) + r[a, 2] * d[:, 2] for a in range(3)], -1)
        length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        n = d / length[:, None]
        valid = (np.abs(o) < f32(FAR)).all(-1) & np.isfinite(length) & np.isfinite(n).all(-1)
        assert o.dtype == f32 and n.dtype == f32 and t1.dtype == f32

        status = np.where(valid, -1, INVALID).astype(np.int32)
        t = np.full(count, t0, dtype=f32)
        armed = np.zeros(count, dtype=bool)
        steps = np.zeros(count, dtype=np.int64)
        active = np.flatnonzero(valid)
        while len(active):
            # 1, 2
            ended = ~(t[active] < t1[active])
            status[active[ended]] = MISS
            active = active[~ended]
            ended = steps[active] == max_steps
            status[active[ended]] = STEPS
            active = active[~ended]
            steps[active] += 1
            # 3
            p = o[active] + t[active, None] * n[active]
            ended = ~np.isfinite(p).all(-1)
            status[active[ended]] = MISS
            active, p = active[~ended], p[~ended]
            # 4
            c = np.clip(MP.to_int(np.floor(p)), -FAR, FAR)
            B = c >> 3
            slot = lookup.slots(B)
            absent = slot < 0
            # 5: leave the absent block through its exit face
            ia, pa, na, Ba = active[absent], p[absent], n[active[absent]], B[absent]
            s = np.full(len(ia), np.inf, dtype=f32)
            for a in range(3):
                face = (8 * Ba[:, a] + np.where(na[:, a] > 0, 8, 0)).astype(f32)
                s = np.where(na[:, a] != 0, np.fmin(s, (face - pa[:, a]) / na[:, a]), s)
            t[ia] = t[ia] + (np.fmax(s, f32(0)) + f32(0.5))
            out.branches["absent"] += len(ia)
            out.branches["exit_at_zero"] += int((s == 0).sum())
            # 6: the nearest voxel, then the trilinear sample near the surface
            ip, pp, cp = active[~absent], p[~absent], c[~absent] & 7
            u = hv.voxels[slot[~absent] * 512 + cp[:, 2] * 64 + cp[:, 1] * 8 + cp[:, 0]]
            observed = u["distance_weight"] != 0
            sdf = np.where(observed, u["distance"], f32(1))
            window = observed & (sdf <= f32(0.1)) & (sdf >= f32(-0.5))
            exists, distance = distance_sample(hv, pp[window], table)
            sdf[window] = np.where(exists, distance, sdf[window])
            armed[ip] |= observed & (sdf > 0)
            hit = observed & armed[ip] & (sdf <= 0)
            go = ~hit
            t[ip[go]] = t[ip[go]] + np.where(sdf[go] > 0, np.fmax(f32(1), tr * sdf[go]), f32(1))
            out.branches["present"] += len(ip)
            out.branches["unobserved"] += int((~observed).sum())
            out.branches["window"] += int(window.sum())
            out.branches["window_sampled"] += int(exists.sum())
            out.branches["armed_steps"] += int((go & observed & (sdf > 0)).sum())
            out.branches["behind_steps"] += int((go & observed & ~(sdf > 0)).sum())
            # the refinement
            ih = ip[hit]
            th = t[ih] + tr * sdf[hit]
            exists, distance = distance_sample(hv, o[ih] + th[:, None] * n[ih], table)
            t[ih] = np.where(exists, th + tr * distance, th)
            status[ih] = HIT
            out.branches["refined_twice"] += int(exists.sum())
            active = np.concatenate([ia, ip[go]])
        assert t.dtype == f32

        hits = status == HIT
        out.status, out.armed, out.steps, out.t_voxels, out.origin, out.direction = status, armed, steps, t, o, n
        out.t = np.where(hits, t if voxel_units else t * L, f32(0))
        out.samples = np.zeros(count, dtype=T.voxel_dtype)
        out.samples["distance"] = f32(1)                                                    # Voxel::Empty()
        out.gradients = np.zeros((count, 4), dtype=f32)
        if hits.any():
            out.samples[hits], out.gradients[hits] = S.sample(hv, o[hits] + t[hits, None] * n[hits], voxel_units=True, color=color,
                                                              table=table)
    assert out.t.dtype == f32
    return out


# ---- the ray sets the CPU and the GPU tests share ----------------------------------------------------------------------

GRID = 2                                                              # every second pixel of the 160x120 view: 80x60 rays
_SETS = {}


def volume(orc, sizes=((509, 4096), (509, 4096))):
    """the destination volume of register_reference.pair(orc, MP.generic()): the bumps fused at the identity"""
    return RR.pair(orc, MP.generic(), sizes)[0]


def fusing_frame(orc):
    return orc.HostFrame(RR.bumps(RR.W, RR.H), R.projection(), T.Transform.identity())


def pixel_rays():
    """the pixel rays of the camera that fused the volume (the identity pose: the origin is 0), on the 80x60 grid, as the
    raycast builds them (tracer.cu:335-341): (u / fx - cx / fx, v / fy - cy / fy, 1) at the pixel's centre"""
    k = R.projection()
    ys, xs = np.mgrid[0:RR.H:GRID, 0:RR.W:GRID]
    ifx, ify = f32(1) / f32(k.fx), f32(1) / f32(k.fy)
    u, v = xs.reshape(-1).astype(f32) + f32(0.5), ys.reshape(-1).astype(f32) + f32(0.5)
    rays = np.zeros((len(u), 6), dtype=f32)
    rays[:, 3], rays[:, 4], rays[:, 5] = ifx * u - f32(k.cx) * ifx, ify * v - f32(k.cy) * ify, 1
    return rays, xs.reshape(-1), ys.reshape(-1)


def ray_sets(orc, voxel_units):
    """{name: float32 [n, 6]} with origins in the unit asked for (metres, or voxels; a direction has no unit), on volume(orc):
    computed once. A set born in the other unit is converted in float32: whatever the conversion rounds to is a ray like
    any other to the statement."""
    if voxel_units in _SETS:
        return _SETS[voxel_units]
    hv = volume(orc)
    L = f32(hv.voxel_length)
    rng = np.random.default_rng(31)
    metres, voxels = {}, {}
    # (a) the fusing camera's pixel rays
    metres["a"] = pixel_rays()[0]
    # (b) the twins of (a)'s hits: from 3 voxels behind the hit, back at the camera
    first = cast(hv, metres["a"])
    hit = first.status == HIT
    behind = np.zeros((int(hit.sum()), 6), dtype=f32)
    behind[:, :3] = first.origin[hit] + (first.t_voxels[hit] + f32(3))[:, None] * first.direction[hit]
    behind[:, 3:] = -metres["a"][hit, 3:]
    voxels["b"] = behind
    # (c) from random origins within 0.3 m of mesh vertices, in random directions
    vertices = orc.extract_mesh(hv, all_allocated=True, interpolate=True)[0]
    around = np.zeros((3000, 6), dtype=f32)
    around[:, :3] = vertices[rng.integers(0, len(vertices), 3000)] + rng.uniform(-0.3, 0.3, (3000, 3))
    around[:, 3:] = rng.normal(size=(3000, 3))
    metres["c"] = around
    # (d) along an axis, from integral voxel coordinates on a face of a block at or next to a held block: n_a == 0 on two
    # axes, and a ray that starts on the face it leaves an absent block through takes an exit step of s == 0
    origins = np.array(list(RR.block_table(hv)), dtype=np.int64)
    along = np.zeros((1500, 6), dtype=f32)
    axis, sign = rng.integers(0, 3, 1500), rng.choice([-1.0, 1.0], 1500)
    start = 8 * (origins[rng.integers(0, len(origins), 1500)] + rng.integers(-2, 3, (1500, 3))) + rng.integers(0, 8, (1500, 3))
    start[np.arange(1500), axis] &= ~7
    along[:, :3] = start
    along[np.arange(1500), 3 + axis] = sign * rng.uniform(0.5, 2.0, 1500)
    voxels["d"] = along
    # (e) no block near, and none ahead
    away = np.zeros((256, 6), dtype=f32)
    away[:, :3] = rng.uniform(-0.5, 0.5, (256, 3)) + np.array([6.0, -7.0, 9.0])
    away[:, 3:] = away[:, :3] + rng.uniform(-0.2, 0.2, (256, 3)).astype(f32)
    metres["e"] = away
    # (f) a zero direction, then NaN, +-inf and 1e30 in each component of a ray of (a) that hits
    bad = np.repeat(metres["a"][hit][:1] + np.array([0.01, 0.02, 0.03, 0, 0, 0], dtype=f32), 25, axis=0)
    bad[0, 3:] = 0
    for k, value in enumerate((np.nan, np.inf, -np.inf, 1e30)):
        for a in range(6):
            bad[1 + 6 * k + a, a] = value
    metres["f"] = bad
    with np.errstate(all="ignore"):
        for name in "abcdef":
            if name in metres:
                voxels[name] = metres[name].copy()
                voxels[name][:, :3] = metres[name][:, :3] / L
            else:
                metres[name] = voxels[name].copy()
                metres[name][:, :3] = voxels[name][:, :3] * L
    _SETS[False], _SETS[True] = metres, voxels
    return _SETS[voxel_units]


def spans(orc):
    """{name: slice} of each set in all_rays"""
    sets, at, out = ray_sets(orc, False), 0, {}
    for name in "abcdef":
        out[name] = slice(at, at + len(sets[name]))
        at += len(sets[name])
    return out


def all_rays(orc, voxel_units):
    sets = ray_sets(orc, voxel_units)
    return np.ascontiguousarray(np.concatenate([sets[name] for name in "abcdef"]), dtype=f32)


def bounds(voxel_units, t_min=0.0, t_max=T_MAX, voxel_length=R.VOXEL):
    """(t_min, t_max) in the unit the form takes them in: metres, or voxels (a float32 division, as any caller's)"""
    if not voxel_units:
        return float(f32(t_min)), float(f32(t_max))
    return float(f32(t_min) / f32(voxel_length)), float(f32(t_max) / f32(voxel_length))
