"""The CPU statement of vk_volume_register (include/vk.h): the residual and Jacobian every source voxel contributes at a pose
T_dst_src, the normal system, one Gauss-Newton step and the loop — in numpy, on two oracle.HostVolume. There is no upstream
counterpart (its Volume is a process-wide singleton, src/volume.cu:17-21), so this file is the definition.

The per-voxel terms are float32 with one rounding per operation, in the order vk.h gives: numpy's float32 arithmetic is
exactly that, and the device is held to them bit for bit (tests/test_gpu_register.py). The sums are float64 sums of those
float32 terms: the device adds in float32 in its own fixed order and is held to the project's bound for a normal system.
The step is the colour trackers' (color_tracker.cpp:45-95): the unpivoted LDL^T, Tinc(update) * m and rigid_from in float32."""
import numpy as np

import merge_pose_reference as MP
import merge_reference as M
import release_reference as R
from vulcan_amd import vk_types as T

f32 = np.float32
NO_OVERLAP = 2
FAR = 1 << 30
PACKED = [(r, c) for r in range(6) for c in range(r + 1)]            # the lower triangle, row-major


def lerp(t, a, b):
    return a + t * (b - a)


def sample(v, f):
    """D and its gradient (per voxel) from the eight values v[k], k = kx + 2 ky + 4 kz, at the fractions f = (fx, fy, fz);
    every operand keeps its dtype, so float32 in gives vk.h's sequence of roundings and float64 in gives the same formulas"""
    fx, fy, fz = f
    x00, x10, x01, x11 = lerp(fx, v[0], v[1]), lerp(fx, v[2], v[3]), lerp(fx, v[4], v[5]), lerp(fx, v[6], v[7])
    y0, y1 = lerp(fy, x00, x10), lerp(fy, x01, x11)
    D = lerp(fz, y0, y1)
    gz = y1 - y0
    gy = lerp(fz, x10 - x00, x11 - x01)
    gx = lerp(fz, lerp(fy, v[1] - v[0], v[3] - v[2]), lerp(fy, v[5] - v[4], v[7] - v[6]))
    return D, (gx, gy, gz)


def jacobian(p, g, iv):
    """(x cross gradient, gradient / voxel_length): p in voxels, g per voxel"""
    gx, gy, gz = g
    return [p[1] * gz - p[2] * gy, p[2] * gx - p[0] * gz, p[0] * gy - p[1] * gx, gx * iv, gy * iv, gz * iv]


def block_table(hv):
    """{block origin: pool slot} over the blocks the chain walk finds"""
    table = {}
    for index in M.source_blocks(hv):
        table.setdefault(M.origin_of(hv, index), int(hv.hash_entries["data"][index]))
    return table


class Pair:
    """what does not depend on the pose: dst's blocks, the source blocks and their voxels"""

    def __init__(self, dst, src):
        assert f32(dst.voxel_length) == f32(src.voxel_length) and f32(dst.truncation_length) == f32(src.truncation_length)
        self.dst, self.src = dst, src
        self.table = block_table(dst)
        considered = M.source_blocks(src)
        self.considered = len(considered)
        self.slots = np.array([int(src.hash_entries["data"][i]) for i in considered], dtype=np.int64)
        origins = np.array([M.origin_of(src, i) for i in considered], dtype=np.int64).reshape(-1, 3)
        self.centres = ((8 * origins[:, None, :] + MP.OFFSETS[None]).astype(f32) + f32(0.5)).reshape(-1, 3)
        self.at = (self.slots[:, None] * 512 + np.arange(512)[None]).reshape(-1)         # q * 512 + i
        self.voxels = src.voxels[self.at]

    def slots_of(self, blocks):
        """pool slots of the blocks [N, 3], -1 when absent: a coordinate outside the int16 range is"""
        inside = ((blocks >= -32768) & (blocks <= 32767)).all(-1)
        keys = np.where(inside, (blocks + 32768) @ np.array([1, 1 << 16, 1 << 32]), -1)
        _, first, which = np.unique(keys, return_index=True, return_inverse=True)
        found = np.array([self.table.get(tuple(int(c) for c in blocks[k]), -1) if inside[k] else -1 for k in first], dtype=np.int64)
        return found[which.reshape(-1)]


class Terms:
    def __init__(self, size):
        self.valid = np.zeros(size, dtype=np.uint8)
        self.r = np.zeros(size, dtype=f32)
        self.J = np.zeros((size, 6), dtype=f32)
        self.counts = (0, 0, 0, 0)


def terms(pair, pose, band):
    """per source pool slot q and voxel i, at q * 512 + i: valid, r, J (zeros where no residual exists), and the counts"""
    dst, src = pair.dst, pair.src
    band = f32(band)
    out = Terms(src.max * 512)
    with np.errstate(all="ignore"):
        s = pair.voxels
        in_band = (s["distance_weight"] != 0) & (np.abs(s["distance"]) < band)
        at, s = pair.at[in_band], s[in_band]
        fwd = MP.rows(pose.m, dst.voxel_length)
        p = MP.apply(fwd, pair.centres[in_band])
        g = p - f32(0.5)
        b = np.floor(g)
        f = g - b
        base = np.clip(MP.to_int(b), -FAR, FAR)
        points = base[None] + MP.CORNERS[:, None, :]                                      # [8, N, 3]
        slots = pair.slots_of((points >> 3).reshape(-1, 3)).reshape(8, -1)
        voxel = points & 7
        index = voxel[..., 2] * 64 + voxel[..., 1] * 8 + voxel[..., 0]
        there = slots >= 0
        got = dst.voxels[np.where(there, slots * 512 + index, 0)]
        exists = (there & (got["distance_weight"] != 0)).all(0)
        v = [np.where(there[k], got["distance"][k], f32(0)) for k in range(8)]
        D, gradient = sample(v, (f[:, 0], f[:, 1], f[:, 2]))
        valid = exists & (np.abs(D) < band)
        r = D - s["distance"]
        J = jacobian((p[:, 0], p[:, 1], p[:, 2]), gradient, f32(1.0) / f32(dst.voxel_length))
    assert r.dtype == f32 and all(j.dtype == f32 for j in J)
    out.valid[at[valid]] = 1
    out.r[at[valid]] = r[valid]
    out.J[at[valid]] = np.stack(J, -1)[valid]
    out.counts = (pair.considered, int(in_band.sum()), int(valid.sum()), 0)
    return out


def system(t):
    """(system[48] in float64, the sums of absolute terms in the same layout: what the device's float32 sums are held to)"""
    J, r = t.J[t.valid != 0], t.r[t.valid != 0]
    total, absolute = np.zeros(48), np.zeros(48)
    for k, (row, col) in enumerate(PACKED):
        product = (J[:, row] * J[:, col]).astype(np.float64)
        total[k], absolute[k] = product.sum(), np.abs(product).sum()
    for i in range(6):
        product = (J[:, i] * r).astype(np.float64)
        total[36 + i], absolute[36 + i] = product.sum(), np.abs(product).sum()
    total[42] = absolute[42] = (r * r).astype(np.float64).sum()
    return total, absolute


def tinc(update):
    """color_tracker.cpp:45-65: the identity plus the proper skew matrix of update[0:3], update[3:6] the translation"""
    u = np.asarray(update, dtype=f32)
    m = np.eye(4, dtype=f32)
    m[0, 1], m[0, 2], m[0, 3] = -u[2], u[1], u[3]
    m[1, 0], m[1, 2], m[1, 3] = u[2], -u[0], u[4]
    m[2, 0], m[2, 1], m[2, 3] = -u[1], u[0], u[5]
    return m


def _normalized(a):
    dot = f32(0)
    for c in a:
        dot = f32(dot + f32(c * c))
    return a * f32(f32(1) / np.sqrt(dot))


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=f32)


def rigid_from(matrix):
    """color_tracker.cpp:69-95: Gram-Schmidt of the first two columns, Translate(t) * Rotate(R) and its inverse, float32"""
    matrix = np.asarray(matrix, dtype=f32)
    x_axis, y_axis = _normalized(matrix[:3, 0]), _normalized(matrix[:3, 1])
    z_axis = _cross(x_axis, y_axis)
    y_axis = _cross(z_axis, x_axis)
    translation, back, rotation = np.eye(4, dtype=f32), np.eye(4, dtype=f32), np.eye(4, dtype=f32)
    translation[:3, 3], back[:3, 3] = matrix[:3, 3], -matrix[:3, 3]
    rotation[:3, 0], rotation[:3, 1], rotation[:3, 2] = x_axis, y_axis, z_axis
    return T.Transform.from_matrices(T.Transform._matmul(translation, rotation), T.Transform._matmul(rotation.T.copy(), back))


def step(orc, total, counts, pose):
    """one step from the sums: (pose, update, code). A step without a residual leaves the pose alone."""
    if counts[2] == 0:
        return pose, np.zeros(6, dtype=f32), NO_OVERLAP
    H = np.zeros((6, 6), dtype=f32)
    for k, (row, col) in enumerate(PACKED):
        H[row, col] = H[col, row] = f32(total[k])
    update = -orc.ldlt_solve(H, np.asarray(total[36:42], dtype=f32))
    moved = rigid_from(T.Transform._matmul(tinc(update), pose.matrix())) if update.any() else pose      # a zero update: the bytes stay
    norm = f32(0)
    for u in update:
        norm = f32(norm + f32(u * u))
    return moved, update, 1 if np.sqrt(norm) < f32(1e-6) else 0


class Result:
    pass


def register(orc, dst, src, start, iterations=20, band=0.75, pair=None):
    """the loop: `poses[k]` is the pose after k steps; system and counts are the last evaluated step's"""
    pair = pair or Pair(dst, src)
    out = Result()
    out.pose, out.steps, out.code, out.poses = T.Transform.from_matrices(start.matrix(), start.inverse_matrix()), 0, 0, []
    out.poses.append(out.pose)
    for _ in range(iterations):
        evaluated = terms(pair, out.pose, band)
        out.system, out.absolute = system(evaluated)
        out.counts = evaluated.counts
        out.pose, out.update, out.code = step(orc, out.system, out.counts, out.pose)
        out.steps += 1
        out.poses.append(out.pose)
        if out.code:
            break
    return out


def pose_error(pose, truth):
    """(translation in metres, rotation in degrees) between two Transforms, in float64"""
    delta = np.linalg.inv(truth.matrix().astype(np.float64)) @ pose.matrix().astype(np.float64)
    skew = (delta[:3, :3] - delta[:3, :3].T) / 2.0                       # sin(angle) * axis: exact for small angles too
    sine, cosine = np.linalg.norm([skew[2, 1], skew[0, 2], skew[1, 0]]), (np.trace(delta[:3, :3]) - 1.0) / 2.0
    return (float(np.linalg.norm(pose.matrix()[:3, 3].astype(np.float64) - truth.matrix()[:3, 3].astype(np.float64))),
            float(np.degrees(np.arctan2(sine, cosine))))


# ---- the scene the CPU and the GPU tests share ------------------------------------------------------------------------

W, H = R.W, R.H
_PAIRS = {}


def bumps(w, h):
    """a wall at 1 m with a bump, a dent and a slope: nothing repeats, so the alignment has one answer (release_reference's
    ripple is periodic and locks one period off)"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    depth = (1.0 + 0.06 * np.exp(-((x - 0.375 * w) ** 2 + (y - 0.42 * h) ** 2) / (2 * (0.16 * w) ** 2))
             - 0.04 * np.exp(-((x - 0.69 * w) ** 2 + (y - 0.67 * h) ** 2) / (2 * (0.11 * w) ** 2)) + 0.03 * x / w)
    return depth.astype(f32)


def _fused(orc, size, pose, frames, seed):
    rng = np.random.default_rng(seed)
    hv = orc.HostVolume(*size, voxel_length=R.VOXEL, truncation_length=R.TRUNCATION)
    for _ in range(frames):
        frame = orc.HostFrame(bumps(W, H), R.projection(), pose, color=rng.random((H, W, 3), dtype=f32))
        for _ in range(8):
            hv.set_view(frame, orc.POLICY_MAXKEY)
        orc.integrate_depth(hv, frame)
        orc.integrate_color(hv, frame)
    return hv


def pair(orc, truth, sizes=((509, 4096), (509, 4096)), frames=(2, 3)):
    """(dst, src): the bumps fused twice at the identity (colour seed 11), and three times in a world frame displaced by
    `truth` = T_dst_src, that is at the camera pose truth^-1 (seed 12). Computed once per pose and sizes, handed out as copies.
    (`frames`: a source that has to equal the destination bit for bit takes as many frames as it: the running average of
    three equal samples, (2 d + d) / 3, is not always d in float32.)"""
    key = (bytes(truth), tuple(sizes[0]), tuple(sizes[1]), tuple(frames))
    if key not in _PAIRS:
        _PAIRS[key] = (_fused(orc, sizes[0], T.Transform.identity(), frames[0], 11), _fused(orc, sizes[1], truth.inverse(), frames[1], 12))
    return R.clone(orc, _PAIRS[key][0]), R.clone(orc, _PAIRS[key][1])
