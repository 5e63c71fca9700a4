"""The CPU statement of vk_volume_merge_resampled (include/vk.h): vk_volume_merge_posed between two volumes whose voxel
length, truncation length or both differ — in numpy, on two oracle.HostVolume. The device is held to it bit for bit
(tests/test_gpu_merge_resample.py); there is no upstream counterpart, so this file is the definition.

It is built on merge_pose_reference: the carry of a point, the lerps, the lattice and the poses are that module's, the
rounds and the running average merge_reference's. What is stated here is what the change of scale adds: the rows scaled by
the ratio of the voxel lengths, the n^3 sample points of a voxel, a source block's box of K^3 blocks, the rescaling of a
stored distance into the destination's truncation length, and the mean over the sub-samples.

Blocks are found by the definition and not by the bounds a device needs: a source block's box is taken from its corners
without the cap (that K holds every block of it is asserted, so a K too small fails here), and a lattice point's block is
looked up through the source's table, with no directory of D^3 blocks in between (a D too small shows as a difference from
the device). Everything is float32 with one rounding per operation, in the order vk.h gives."""
import numpy as np

import merge_pose_reference as MP
import merge_reference as M
import release_reference as R
from vulcan_amd import vk_types as T

SKIP_UNOBSERVED, CONTINUE = M.SKIP_UNOBSERVED, M.CONTINUE
f32 = np.float32
DIAGONAL = f32(1.7320508)


def ratios(dst, src):
    """(r_fwd, r_back, k): one float32 division each"""
    r_fwd, r_back = f32(src.voxel_length) / f32(dst.voxel_length), f32(dst.voxel_length) / f32(src.voxel_length)
    k = f32(src.truncation_length) / f32(dst.truncation_length)
    assert 0.25 <= r_fwd <= 4.0 and 0.25 <= r_back <= 4.0 and np.isfinite(k) and k > 0
    return r_fwd, r_back, k


def box_blocks(ratio):
    """K: blocks per axis that a block reaches at `ratio` voxels of the other lattice per voxel"""
    return min(8, int(f32(ratio) * DIAGONAL) + 2)


def directory_blocks(ratio):
    """D: what the device's fuse pass keeps per carried block (the statement looks every block up)"""
    return min(9, int(f32(ratio) * DIAGONAL + f32(0.125)) + 2)


def default_supersample(dst, src):
    return min(4, max(1, int(np.ceil(ratios(dst, src)[1] - 1e-6))))


def rows(matrix, ratio, voxel_length):
    """merge_pose_reference.rows with the rotation times `ratio`: at ratio 1.0f the same bits"""
    r = MP.rows(matrix, voxel_length)
    r[:, :3] = r[:, :3] * f32(ratio)
    return r


def offsets(n):
    """the n^3 sample points of a voxel from its centre, x fastest: float32 [n^3, 3]"""
    o = np.array([f32(2 * j + 1) / f32(2 * n) - f32(0.5) for j in range(n)], dtype=f32)
    return np.array([(o[jx], o[jy], o[jz]) for jz in range(n) for jy in range(n) for jx in range(n)], dtype=f32)


def candidates_of(origin, fwd, back, n, box):
    """the destination blocks a source block with this origin reaches: merge_pose_reference.candidates_of over the sample
    points of every voxel, the block's box taken whole"""
    corners = (8 * np.asarray(origin, dtype=np.int64) + 8 * MP.CORNERS).astype(f32)
    q = MP.apply(fwd, corners)
    with np.errstate(all="ignore"):
        lo = np.clip(MP.to_int(np.floor(np.fmin.reduce(q, 0) * f32(0.125))), -MP.CLAMP, MP.CLAMP)
        hi = np.clip(MP.to_int(np.floor(np.fmax.reduce(q, 0) * f32(0.125))), -MP.CLAMP, MP.CLAMP)
    assert (hi - lo <= box - 1).all(), ("a block's box spans more than K blocks", origin, lo, hi, box)
    first, last = (8 * np.asarray(origin)).astype(f32), (8 * np.asarray(origin) + 7).astype(f32)
    blocks = np.array([(bx, by, bz) for bz in range(lo[2], hi[2] + 1) for by in range(lo[1], hi[1] + 1) for bx in range(lo[0], hi[0] + 1)
                       if all(-32768 <= b <= 32767 for b in (bx, by, bz))], dtype=np.int64).reshape(-1, 3)
    centre = (8 * blocks[:, None, :] + MP.OFFSETS[None]).astype(f32) + f32(0.5)                        # [blocks, 512, 3]
    reached = np.zeros(len(blocks), bool)
    for o in offsets(n):
        cell = np.floor(MP.apply(back, centre + o))
        reached |= ((cell >= first) & (cell <= last)).all(-1).any(-1)
    return [tuple(int(b) for b in block) for block in blocks[reached]]


def sub_samples(src, points, back, find, k):
    """merge_pose_reference.samples at the 512 points `points` (float32 [512, 3], dst voxel units) in the place of the
    voxel centres, then the rescaling by k: (distance, colour [512, 3], distance weight, colour weight), weight 0: none"""
    g = MP.apply(back, points) - f32(0.5)
    b = np.floor(g)
    f = g - b
    n0 = np.clip(MP.to_int(b), -(1 << 30), 1 << 30)
    far = f != 0
    has_d, has_c, saturated = np.ones(512, bool), np.ones(512, bool), np.zeros(512, bool)
    least_d, least_c = np.full(512, 32767, np.int64), np.full(512, 32767, np.int64)
    distance, color = [], []
    lattice = n0[None] + MP.CORNERS[:, None, :]                          # [8, 512, 3]
    blocks = (lattice >> 3).reshape(-1, 3)
    _, first, which = np.unique(blocks @ np.array([1, 1 << 20, 1 << 40]), return_index=True, return_inverse=True)
    slots = np.array([find(block) for block in blocks[first]], dtype=np.int64)[which.reshape(-1)].reshape(8, 512)
    for s in range(8):
        used = ((MP.CORNERS[s] == 0) | far).all(-1)
        voxel = lattice[s] & 7
        index = voxel[:, 2] * 64 + voxel[:, 1] * 8 + voxel[:, 0]
        slot = slots[s]
        there = used & (slot >= 0)
        got = np.zeros(512, dtype=T.voxel_dtype)
        got[there] = src.voxels[slot[there] * 512 + index[there]]
        has_d &= ~used | (there & (got["distance_weight"] != 0))
        has_c &= ~used | (there & (got["color_weight"] != 0))
        saturated |= there & (got["distance"] >= f32(1.0))
        least_d = np.where(there, np.minimum(least_d, got["distance_weight"]), least_d)
        least_c = np.where(there, np.minimum(least_c, got["color_weight"]), least_c)
        distance.append(got["distance"])
        color.append(got["color"])
    fx = [f[:, 0], f[:, 1], f[:, 2]]
    d = MP.trilinear(distance, fx)
    c = np.stack([MP.trilinear([v[:, a] for v in color], fx) for a in range(3)], -1)
    if k != f32(1.0):
        with np.errstate(all="ignore"):
            if k < 1:
                has_d &= ~saturated
            d = k * d
            d = np.where(d >= 1, f32(1.0), d)
            has_d &= ~(d <= -1)
    return d.astype(f32), c.astype(f32), np.where(has_d, least_d, 0), np.where(has_c, least_c, 0)


def samples(src, origin, back, find, n, k):
    """512 voxels: what the destination block at `origin` samples from src — value and weight per field, weight 0: none.
    Per field the mean, in point order, of the sub-samples that exist, where more than half of the n^3 do."""
    centre = MP.centres(origin)
    count_d, count_c = np.zeros(512, np.int64), np.zeros(512, np.int64)
    sum_d, sum_c = np.zeros(512, f32), np.zeros((512, 3), f32)
    least_d, least_c = np.full(512, 32767, np.int64), np.full(512, 32767, np.int64)
    with np.errstate(all="ignore"):
        for o in offsets(n):
            d, c, wd, wc = sub_samples(src, centre + o, back, find, k)
            take = wd != 0
            sum_d = np.where(take, np.where(count_d == 0, d, sum_d + d), sum_d)          # the first, then + the next
            least_d = np.where(take, np.minimum(least_d, wd), least_d)
            count_d += take
            take = wc != 0
            sum_c = np.where(take[:, None], np.where((count_c == 0)[:, None], c, sum_c + c), sum_c)
            least_c = np.where(take, np.minimum(least_c, wc), least_c)
            count_c += take
        out = np.zeros(512, dtype=T.voxel_dtype)
        has_d, has_c = 2 * count_d > n ** 3, 2 * count_c > n ** 3
        out["distance"] = sum_d / count_d.astype(f32)
        out["color"] = sum_c / count_c.astype(f32)[:, None]
    out["distance_weight"] = np.where(has_d, least_d, 0)
    out["color_weight"] = np.where(has_c, least_c, 0)
    return out


def candidate_blocks(dst, src, pose, n, considered):
    """the candidates of the call, each once, in the order the considered source blocks reach them"""
    r_fwd, r_back, _ = ratios(dst, src)
    fwd, back = rows(pose.m, r_fwd, dst.voxel_length), rows(pose.inv, r_back, src.voxel_length)
    candidates = {}
    for i in considered:
        for origin in candidates_of(M.origin_of(src, i), fwd, back, n, box_blocks(r_fwd)):
            candidates[origin] = True
    return list(candidates)


def merge(dst, src, pose, supersample=1, flags=0, max_rounds=8, cap_d=16.0, cap_c=16.0, workspace=None):
    """Mutates `dst` as the call is defined; returns the eight counts. `pose`: a vk_types.Transform, T_dst_src. `workspace`:
    a dict standing for the device workspace — the considered source entries, the candidates and which of them are fused.
    (merge_pose_reference.merge's course: the candidates, its rounds, then a block's samples into the running average.)"""
    n = int(supersample)
    assert max_rounds >= 1 and 1 <= cap_d <= 32767 and 1 <= cap_c <= 32767 and 1 <= n <= 4
    r_fwd, r_back, k = ratios(dst, src)
    back = rows(pose.inv, r_back, src.voxel_length)
    skipped = 0
    if flags & CONTINUE:
        considered, candidates, done = workspace["considered"], workspace["candidates"], workspace["fused"]
    else:
        considered = M.source_blocks(src)
        if flags & SKIP_UNOBSERVED:
            observed = [i for i in considered if not M.unobserved(src, i)]
            skipped = len(considered) - len(observed)
            considered = observed
        candidates, done = candidate_blocks(dst, src, pose, n, considered), set()
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
        sample = samples(src, origin, back, find, n, k)
        sampled += int((sample["distance_weight"] != 0).sum())
        M.fuse_block(dst, slot, MP._Block(sample), 0, cap_d, cap_c)
        done.add(origin)
        fused += 1
    if workspace is not None:
        workspace.update(considered=considered, candidates=candidates, fused=done)
    dst.counters[T.VK_CTR_VISIBLE] = 0
    dst.counters[T.VK_CTR_BANDED] = -1
    return len(considered), len(pending), fused, fused - present_before, len(pending) - fused, rounds, skipped, sampled


# ---- the states the CPU and the GPU tests share ----------------------------------------------------------------------

def fresh(orc, main, excess, voxel_length, truncation_length):
    return orc.HostVolume(main, excess, voxel_length=voxel_length, truncation_length=truncation_length)


def cut(hv, keep_box):
    """`hv` with only the blocks whose origin lies in `keep_box` = ((lo x, y, z), (hi x, y, z)), inclusive"""
    R.release_blocks(hv, R.OUTSIDE_BOX, keep_lo=keep_box[0], keep_hi=keep_box[1])
    return hv


def dense(hv):
    """(least coordinate, the voxels of `hv` as a dense array [x, y, z] of vk_types.voxel_dtype, Voxel::Empty() where no
    block is) around the blocks of `hv`, with a margin of a block"""
    coords, voxels = MP.cloud(hv)
    least = coords.min(0) // 16 * 16 - 16
    shape = (coords.max(0) // 16 * 16 + 32) - least
    grid = np.zeros(tuple(int(s) for s in shape), dtype=T.voxel_dtype)
    grid["distance"] = 1
    at = coords - least
    grid[at[:, 0], at[:, 1], at[:, 2]] = voxels
    return least, grid


def ordered_mean_of_eight(source, coords, cap=16):
    """What a fresh volume of twice `source`'s voxel length holds at the voxels `coords` [N, 3] after a merge at the
    identity with n = 2, by plain slicing of a dense copy of the source and without a pose, a lattice or a table: per
    field the mean, x fastest, of the stored 2x2x2 source voxels that carry a weight where at least 5 do, with the
    smallest of their weights up to `cap`, Voxel::Empty() elsewhere. Returns voxels [N] of vk_types.voxel_dtype and, per
    field, how many voxels have some but fewer than 5 of the 8."""
    least, grid = dense(source)
    fine = 2 * coords - least                                            # the first of a dst voxel's 2x2x2 source voxels
    out, short = np.zeros(len(coords), dtype=T.voxel_dtype), {}
    with np.errstate(all="ignore"):
        for weight, field, channels in (("distance_weight", "distance", 1), ("color_weight", "color", 3)):
            count = np.zeros(len(coords), np.int64)
            total = np.zeros((len(coords), channels), f32)
            least_weight = np.full(len(coords), 32767, np.int64)
            for jz in range(2):
                for jy in range(2):
                    for jx in range(2):
                        got = grid[fine[:, 0] + jx, fine[:, 1] + jy, fine[:, 2] + jz]
                        value = got[field].reshape(len(coords), channels)
                        take = got[weight] != 0
                        total = np.where(take[:, None], np.where((count == 0)[:, None], value, total + value), total)
                        least_weight = np.where(take, np.minimum(least_weight, got[weight]), least_weight)
                        count += take
            exists = count >= 5
            mean = total / count.astype(f32)[:, None]
            empty = np.ones(1, f32) if channels == 1 else np.zeros(3, f32)
            out[field] = np.where(exists[:, None], mean, empty[None]).astype(f32).reshape(out[field].shape)
            out[weight] = np.where(exists, np.minimum(least_weight, cap), 0)
            short[field] = int(((count > 0) & ~exists).sum())
    return out, short
