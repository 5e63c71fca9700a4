"""The CPU statement of vk_volume_merge_posed (include/vk.h): which blocks of the destination a source volume reaches through
a rigid pose, which of them a call allocates, and the destination's hash table, visibility bytes, pool, counters and voxels
afterwards — in numpy, on two oracle.HostVolume. The device is held to it bit for bit (tests/test_gpu_merge_pose.py); there
is no upstream counterpart (its Volume is a process-wide singleton, src/volume.cu:17-21), so this file is the definition.

Everything is float32 with one rounding per operation, in the order vk.h gives: numpy's float32 arithmetic is exactly that,
so no tolerance exists. The allocation rounds are merge_reference's with the candidate blocks in the place of the source
blocks, the running average is merge_reference.fuse_block with the trilinear sample in the place of the source voxel."""
import numpy as np

import merge_reference as M
import release_reference as R
from vulcan_amd import vk_types as T

SKIP_UNOBSERVED, CONTINUE = M.SKIP_UNOBSERVED, M.CONTINUE
f32 = np.float32
CLAMP = 40000
# voxel i = z*64 + y*8 + x of a block
OFFSETS = np.stack([np.arange(512) & 7, (np.arange(512) >> 3) & 7, np.arange(512) >> 6], -1)
CORNERS = np.array([[s & 1, (s >> 1) & 1, s >> 2] for s in range(8)])


def rows(matrix, voxel_length):
    """rows 0-2 of a column-major 4x4 (16 floats), the translation in voxels"""
    m = np.asarray(list(matrix), dtype=f32)
    assert np.isfinite(m[[a + 4 * c for a in range(3) for c in range(4)]]).all()
    return np.array([[m[a], m[4 + a], m[8 + a], m[12 + a] / f32(voxel_length)] for a in range(3)], dtype=f32)


def apply(r, c):
    """((r0 c0 + r1 c1) + r2 c2) + t per axis; c: float32 [..., 3]"""
    assert c.dtype == f32 and r.dtype == f32
    with np.errstate(all="ignore"):
        return np.stack([((r[a, 0] * c[..., 0] + r[a, 1] * c[..., 1]) + r[a, 2] * c[..., 2]) + r[a, 3] for a in range(3)], -1)


def to_int(x):
    """(int) as the device converts: saturating, NaN gives 0"""
    x = np.asarray(x, dtype=np.float64)
    return np.clip(np.where(np.isnan(x), 0.0, x), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def block_box(r, origin):
    """the blocks [lo, hi]^3 the eight corners of block `origin` reach through `r`, at most three per axis"""
    corners = (8 * np.asarray(origin, dtype=np.int64) + 8 * CORNERS).astype(f32)
    q = apply(r, corners)
    with np.errstate(all="ignore"):
        lo = np.clip(to_int(np.floor(np.fmin.reduce(q, 0) * f32(0.125))), -CLAMP, CLAMP)
        hi = np.clip(to_int(np.floor(np.fmax.reduce(q, 0) * f32(0.125))), -CLAMP, CLAMP)
    return lo, np.minimum(hi, lo + 2)


def centres(origin):
    return (8 * np.asarray(origin, dtype=np.int64) + OFFSETS).astype(f32) + f32(0.5)


def candidates_of(origin, fwd, back):
    """the destination blocks a source block with this origin reaches"""
    lo, hi = block_box(fwd, origin)
    first, last = (8 * np.asarray(origin)).astype(f32), (8 * np.asarray(origin) + 7).astype(f32)
    box = np.array([(bx, by, bz) for bz in range(lo[2], hi[2] + 1) for by in range(lo[1], hi[1] + 1) for bx in range(lo[0], hi[0] + 1)
                    if all(-32768 <= b <= 32767 for b in (bx, by, bz))], dtype=np.int64).reshape(-1, 3)
    cell = np.floor(apply(back, (8 * box[:, None, :] + OFFSETS[None]).astype(f32) + f32(0.5)))        # [blocks, 512, 3]
    reached = ((cell >= first) & (cell <= last)).all(-1).any(-1)
    return [tuple(int(b) for b in block) for block in box[reached]]


def lerp(f, a, b):
    with np.errstate(all="ignore"):
        return np.where(f == 0, a, a + f * (b - a))


def trilinear(v, f):
    """x, then y, then z over v[s], s = sx + 2 sy + 4 sz"""
    x = [lerp(f[0], v[2 * k], v[2 * k + 1]) for k in range(4)]
    y = [lerp(f[1], x[0], x[1]), lerp(f[1], x[2], x[3])]
    return lerp(f[2], y[0], y[1])


def samples(src, origin, back, find):
    """512 voxels: what the destination block at `origin` samples from src — value and weight per field, weight 0: none"""
    g = apply(back, centres(origin)) - f32(0.5)
    b = np.floor(g)
    f = g - b
    n0 = b.astype(np.int64)
    far = f != 0
    has_d, has_c = np.ones(512, bool), np.ones(512, bool)
    least_d, least_c = np.full(512, 32767, np.int64), np.full(512, 32767, np.int64)
    distance, color = [], []
    points = n0[None] + CORNERS[:, None, :]                              # [8, 512, 3]
    blocks = (points >> 3).reshape(-1, 3)
    _, first, which = np.unique(blocks @ np.array([1, 1 << 20, 1 << 40]), return_index=True, return_inverse=True)    # one key per block
    slots = np.array([find(block) for block in blocks[first]], dtype=np.int64)[which.reshape(-1)].reshape(8, 512)
    for s in range(8):
        used = ((CORNERS[s] == 0) | far).all(-1)
        voxel = points[s] & 7
        index = voxel[:, 2] * 64 + voxel[:, 1] * 8 + voxel[:, 0]
        slot = slots[s]
        there = used & (slot >= 0)
        got = np.zeros(512, dtype=T.voxel_dtype)
        got[there] = src.voxels[slot[there] * 512 + index[there]]
        has_d &= ~used | (there & (got["distance_weight"] != 0))
        has_c &= ~used | (there & (got["color_weight"] != 0))
        least_d = np.where(there, np.minimum(least_d, got["distance_weight"]), least_d)
        least_c = np.where(there, np.minimum(least_c, got["color_weight"]), least_c)
        distance.append(got["distance"])
        color.append(got["color"])
    out = np.zeros(512, dtype=T.voxel_dtype)
    fx = [f[:, 0], f[:, 1], f[:, 2]]
    out["distance"] = trilinear(distance, fx)
    for c in range(3):
        out["color"][:, c] = trilinear([v[:, c] for v in color], fx)
    out["distance_weight"] = np.where(has_d, least_d, 0)
    out["color_weight"] = np.where(has_c, least_c, 0)
    return out


class _Block:
    def __init__(self, voxels):
        self.voxels = voxels


def merge(dst, src, pose, flags=0, max_rounds=8, cap_d=16.0, cap_c=16.0, workspace=None):
    """Mutates `dst` as the call is defined; returns the eight counts. `pose`: a vk_types.Transform, T_dst_src. `workspace`:
    a dict standing for the device workspace — the considered source entries, the candidates and which of them are fused."""
    assert max_rounds >= 1 and 1 <= cap_d <= 32767 and 1 <= cap_c <= 32767
    assert f32(dst.voxel_length) == f32(src.voxel_length) and f32(dst.truncation_length) == f32(src.truncation_length)
    fwd, back = rows(pose.m, dst.voxel_length), rows(pose.inv, dst.voxel_length)
    skipped = 0
    if flags & CONTINUE:
        considered, candidates, done = workspace["considered"], workspace["candidates"], workspace["fused"]
    else:
        considered = M.source_blocks(src)
        if flags & SKIP_UNOBSERVED:
            observed = [i for i in considered if not M.unobserved(src, i)]
            skipped = len(considered) - len(observed)
            considered = observed
        candidates, done = {}, set()
        for i in considered:
            for origin in candidates_of(M.origin_of(src, i), fwd, back):
                candidates[origin] = True
        candidates = list(candidates)
    pending = [origin for origin in candidates if origin not in done]

    present_before = sum(1 for origin in pending if R.find(dst, origin) >= 0)
    rounds = 0
    for _ in range(max_rounds):
        winners = {}
        for origin in pending:
            if R.find(dst, origin) >= 0:
                continue
            bucket = M.bucket_of(origin, dst.main)
            kind = T.ALLOC_MAIN if dst.hash_entries["data"][bucket] == -1 else T.ALLOC_EXCESS
            key = M.request_key(kind, origin)
            if bucket not in winners or key > winners[bucket][0]:
                winners[bucket] = (key, kind, origin)
        if not winners:
            break
        rounds += 1
        for bucket, (_, kind, origin) in winners.items():
            dst.allocation_types[bucket] = kind
            dst.allocation_blocks["origin"][bucket] = origin
            dst.allocation_blocks["pad"][bucket] = kind
            if kind == T.ALLOC_MAIN:
                dst.block_visibility[bucket] = T.VISIBILITY_TRUE      # volume.cu:193-200
        dropped = int(dst.counters[T.VK_CTR_DROPPED])
        dst.handle_allocation_requests()
        if int(dst.counters[T.VK_CTR_DROPPED]) != dropped:
            break                                                       # DESIGN.md section 2, divergence 14

    found = {}

    def find(origin):                                                   # src is only read: one walk per block
        origin = tuple(int(c) for c in origin)
        if origin not in found:
            inside = all(-32768 <= c <= 32767 for c in origin)
            found[origin] = R.find(src, origin) if inside else -1
        return found[origin]

    fused = sampled = 0
    for origin in pending:
        slot = R.find(dst, origin)
        if slot < 0:
            continue
        sample = samples(src, origin, back, find)
        sampled += int((sample["distance_weight"] != 0).sum())
        M.fuse_block(dst, slot, _Block(sample), 0, cap_d, cap_c)
        done.add(origin)
        fused += 1
    if workspace is not None:
        workspace.update(considered=considered, candidates=candidates, fused=done)
    dst.counters[T.VK_CTR_VISIBLE] = 0
    dst.counters[T.VK_CTR_BANDED] = -1
    return len(considered), len(pending), fused, fused - present_before, len(pending) - fused, rounds, skipped, sampled


# ---- the poses the CPU and the GPU tests share ----------------------------------------------------------------------

def quarter_turn(shift_blocks=(0, 0, 0)):
    """90 degrees about z, then a translation of whole blocks: voxel centres go to voxel centres"""
    m = np.eye(4)
    m[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    m[:3, 3] = [float(f32(8 * s) * f32(M.VOXEL)) for s in shift_blocks]
    return T.Transform.from_matrices(m, np.linalg.inv(m))


def shift(voxels):
    """a translation by whole voxels; fl(fl(k * 0.008f) / 0.008f) == k for the k used (asserted where it is used)"""
    t = [float(f32(k) * f32(M.VOXEL)) for k in voxels]
    return T.Transform.translate(*t)


def generic():
    """yaw 10 degrees, pitch 5 degrees, t = (0.013, -0.021, 0.008) m"""
    a = np.deg2rad(5.0) / 2.0
    import scenes
    return T.Transform.translate(0.013, -0.021, 0.008) * scenes.yaw(10.0) * T.Transform.rotate(np.cos(a), np.sin(a), 0.0, 0.0)


def cloud(hv):
    """(global voxel coordinates [N, 3], voxels [N]) over the blocks of `hv`, sorted by coordinate"""
    coords, voxels = [], []
    for i in M.source_blocks(hv):
        slot = int(hv.hash_entries["data"][i])
        coords.append(8 * np.asarray(M.origin_of(hv, i), dtype=np.int64) + OFFSETS)
        voxels.append(hv.voxels[slot * 512:(slot + 1) * 512])
    coords, voxels = np.concatenate(coords), np.concatenate(voxels)
    order = np.lexsort(coords.T)
    return coords[order], voxels[order]
