"""The CPU statement of vk_volume_sample (include/vk.h): the trilinear sample of a volume's stored voxels at arbitrary points —
distance, colour and the two weights as a voxel, and the gradient of the distance — in numpy, on an oracle.HostVolume. There
is no upstream counterpart (the reference samples its volume only along camera rays), so this file is the definition.

Everything is float32 with one rounding per operation, in the order vk.h gives: numpy's float32 arithmetic is exactly that,
so no tolerance exists and the device is held to it bit for bit (tests/test_gpu_sample.py). The value is
merge_pose_reference's (the USED rule, an axis with f == 0 takes its base value), the gradient register_reference's.

It also holds the point sets the CPU and the GPU tests share."""
import numpy as np

import merge_pose_reference as MP
import merge_reference as M
import register_reference as RR
from vulcan_amd import vk_types as T

f32 = np.float32
FAR = 1 << 30
VOXEL_UNITS, DISTANCE_ONLY = T.VK_SAMPLE_VOXEL_UNITS, T.VK_SAMPLE_DISTANCE_ONLY


def slots_of(table, blocks):
    """pool slots of the blocks [N, 3], -1 when absent: a coordinate outside the int16 range is"""
    inside = ((blocks >= -32768) & (blocks <= 32767)).all(-1)
    keys = np.where(inside, (blocks + 32768) @ np.array([1, 1 << 16, 1 << 32]), -1)
    _, first, which = np.unique(keys, return_index=True, return_inverse=True)
    found = np.array([table.get(tuple(int(c) for c in blocks[k]), -1) if inside[k] else -1 for k in first], dtype=np.int64)
    return found[which.reshape(-1)]


def sample(hv, points, pose=None, voxel_units=False, color=True, table=None):
    """(samples [N] of vk_types.voxel_dtype, gradients [N, 4] float32) of `hv` at `points` [N, 3]. `pose`: a Transform,
    T_volume_points, or None. `table`: RR.block_table(hv), when the caller has it."""
    x = np.ascontiguousarray(points, dtype=f32).reshape(-1, 3)
    table = RR.block_table(hv) if table is None else table
    with np.errstate(all="ignore"):
        q = x if voxel_units else x / f32(hv.voxel_length)
        p = q if pose is None else MP.apply(MP.rows(pose.m, hv.voxel_length), q)
        finite = np.isfinite(p).all(-1)
        p = np.where(finite[:, None], p, f32(0))
        g = p - f32(0.5)
        b = np.floor(g)
        f = g - b
        base = np.clip(MP.to_int(b), -FAR, FAR)
        far = f != 0
        corners = base[None] + MP.CORNERS[:, None, :]                                    # [8, N, 3]
        slots = slots_of(table, (corners >> 3).reshape(-1, 3)).reshape(8, -1)
        voxel = corners & 7
        index = voxel[..., 2] * 64 + voxel[..., 1] * 8 + voxel[..., 0]
        there = (slots >= 0) & finite[None]
        got = hv.voxels[np.where(there, slots * 512 + index, 0)]
        used = np.stack([((MP.CORNERS[s] == 0) | far).all(-1) for s in range(8)])          # [8, N]
        read = there & used
        has_d = finite & (~used | (there & (got["distance_weight"] != 0))).all(0)
        has_c = finite & (~used | (there & (got["color_weight"] != 0))).all(0)
        least_d = np.where(read, got["distance_weight"], 32767).min(0)
        least_c = np.where(read, got["color_weight"], 32767).min(0)
        fx = [f[:, 0], f[:, 1], f[:, 2]]
        out = np.zeros(len(x), dtype=T.voxel_dtype)
        distance = MP.trilinear([np.where(read[s], got["distance"][s], f32(0)) for s in range(8)], fx)
        out["distance"] = np.where(has_d, distance, f32(1))                                # Voxel::Empty()
        out["distance_weight"] = np.where(has_d, least_d, 0)
        if color:
            for c in range(3):
                channel = MP.trilinear([np.where(read[s], got["color"][s, :, c], f32(0)) for s in range(8)], fx)
                out["color"][:, c] = np.where(has_c, channel, f32(0))
            out["color_weight"] = np.where(has_c, least_c, 0)
        # the gradient: all eight, no USED rule
        exists = (there & (got["distance_weight"] != 0)).all(0)
        _, gradient = RR.sample([np.where(there[k], got["distance"][k], f32(0)) for k in range(8)], fx)
        gradients = np.zeros((len(x), 4), dtype=f32)
        for a in range(3):
            assert gradient[a].dtype == f32
            gradients[:, a] = np.where(exists, gradient[a], f32(0))
        gradients[:, 3] = exists
    assert out["distance"].dtype == f32
    return out, gradients


def weighted_voxels(hv, limit=None):
    """(global voxel coordinates [N, 3], pool index [N]) of the voxels with distance_weight != 0, in pool order"""
    origin = {}
    for index in M.source_blocks(hv):
        origin.setdefault(int(hv.hash_entries["data"][index]), M.origin_of(hv, index))
    at = np.flatnonzero(hv.voxels["distance_weight"] != 0)
    at = at[np.isin(at // 512, list(origin))][:limit]
    origins = np.array([origin[int(slot)] for slot in at // 512], dtype=np.int64).reshape(-1, 3)
    return 8 * origins + MP.OFFSETS[at % 512], at


# ---- the point sets the CPU and the GPU tests share --------------------------------------------------------------------

_SETS = {}


def point_sets(orc, voxel_units):
    """{name: float32 [n, 3]} in the unit asked for (metres, or voxels), around the destination volume of
    register_reference.pair(orc, MP.generic()): computed once. A set born in the other unit is converted in float32:
    whatever the conversion rounds to is a point like any other to the statement."""
    if voxel_units in _SETS:
        return _SETS[voxel_units]
    hv = RR.pair(orc, MP.generic())[0]
    L = f32(hv.voxel_length)
    rng = np.random.default_rng(29)
    metres, voxels = {}, {}
    # (a) the oracle's mesh vertices
    vertices = orc.extract_mesh(hv, all_allocated=True, interpolate=True)[0]
    metres["a"] = vertices
    # (b) points within 20 mm of them
    metres["b"] = (vertices[rng.integers(0, len(vertices), 20000)] + rng.uniform(-0.02, 0.02, (20000, 3))).astype(f32)
    # (c) the centres of the weighted voxels with an unweighted or absent +1 neighbour, among the first 60 000 weighted ones
    coords, _ = weighted_voxels(hv, 60000)
    centres = coords.astype(f32) + f32(0.5)
    table = RR.block_table(hv)
    lacking = np.zeros(len(centres), dtype=bool)
    for a in range(3):
        lacking |= sample(hv, centres + np.eye(3, dtype=f32)[a], voxel_units=True, table=table)[0]["distance_weight"] == 0
    voxels["c"] = centres[lacking]
    # (d) on block faces, with p - 0.5 integral on one or two axes: b & 7 == 7 on an axis, dyadic fractions elsewhere
    faces = coords[((coords & 7) == 7).any(-1)][:1500]
    fractions = rng.integers(0, 16, faces.shape).astype(f32) / f32(16)
    fractions[np.arange(len(faces)), rng.integers(0, 3, len(faces))] = 0
    fractions[np.arange(len(faces)), rng.integers(0, 3, len(faces))] = 0
    voxels["d"] = faces.astype(f32) + f32(0.5) + fractions
    # (e) no block near
    metres["e"] = (rng.uniform(-0.5, 0.5, (256, 3)) + np.array([6.0, -7.0, 9.0])).astype(f32)
    # (f) NaN, +-inf and 1e30 in each coordinate of a vertex
    bad = np.repeat(vertices[:1], 12, axis=0)
    for k, value in enumerate((np.nan, np.inf, -np.inf, 1e30)):
        for a in range(3):
            bad[3 * k + a, a] = value
    metres["f"] = bad
    with np.errstate(all="ignore"):
        for name in "abcdef":
            if name in metres:
                voxels[name] = metres[name] / L
            else:
                metres[name] = voxels[name] * L
    _SETS[False], _SETS[True] = metres, voxels
    return _SETS[voxel_units]


def all_points(orc, voxel_units):
    sets = point_sets(orc, voxel_units)
    return np.ascontiguousarray(np.concatenate([sets[name] for name in "abcdef"]), dtype=f32)
