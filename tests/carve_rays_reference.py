"""The CPU statement of vk_volume_carve_rays (include/vk.h): which voxels of a volume a batch of range rays carves — the
cells of existing blocks a ray crosses between t_from and the start of the band around its measurement — and what each holds
afterwards, in numpy, on an oracle.HostVolume. The ray, its range and the cell traversal are vk_volume_integrate_rays'
(tests/integrate_rays_reference.py); the observation a carve makes is the 1 the reference integrator writes in front of a
surface (min(1, d / truncation), src/depth_integrator.cu:54-74). There is no upstream call for a measurement that is no pixel
of a pinhole depth image, so this file is the definition.

Everything is float32 with one rounding per operation, in the order vk.h gives, and what rays that share a voxel add up is a
count: no result depends on the order of the rays, no tolerance exists and the device is held to it bit for bit
(tests/test_gpu_carve_rays.py).

It is vectorised over rays (the block walk) and over the visits of present blocks (the cell walk), and it holds the ray sets
and the scenario the CPU and the GPU tests share."""
import numpy as np

import cast_reference as CR
import integrate_rays_reference as IR
import merge_pose_reference as MP
import merge_reference as M
import register_reference as RR
import release_reference as R
from vulcan_amd import vk_types as T

f32 = np.float32
FAR = IR.FAR
VOXEL_UNITS, ONE_OBSERVATION = IR.VOXEL_UNITS, IR.ONE_OBSERVATION
MAX_COUNT, MAX_BLOCKS = 1 << 22, 4096
R_MIN, R_MAX = IR.R_MIN, IR.R_MAX


def _least(t):
    """(axis [M], least [M]) of tmax [M, 3]: the smallest, x before y before z on a tie (a NaN is never the smaller)"""
    axis = np.zeros(len(t), dtype=np.int64)
    least = t[:, 0]
    for a in (1, 2):
        smaller = t[:, a] < least
        axis[smaller] = a
        least = np.where(smaller, t[:, a], least)
    return axis, least


def walk(o, n, ta, tb):
    """vk_volume_integrate_rays' traversal of the cells the rays cross between ta and tb, both given: (ray [M], cell [M, 3]
    int64, leaves [M] float32), every visit of every ray in the order of the walk; `leaves` is the smallest tmax right after
    the visit, the distance at which the walk leaves the cell"""
    count = len(o)
    with np.errstate(all="ignore"):
        p = o + ta[:, None] * n
        c = np.clip(MP.to_int(np.floor(p)), -FAR, FAR)
        pos, neg = n > 0, n < 0
        face = np.where(pos, c + 1, c).astype(f32)
        tmax = np.where(pos | neg, ta[:, None] + (face - p) / n, f32(np.inf)).astype(f32)
        tdelta = np.where(pos | neg, f32(1) / np.abs(n), f32(np.inf)).astype(f32)
        step = pos.astype(np.int64) - neg.astype(np.int64)
        guard = 3 * (np.clip(MP.to_int(np.ceil(tb - ta)), 0, 1024) + 2)
        assert tmax.dtype == f32 and tdelta.dtype == f32 and p.dtype == f32
        who, cells, leaves = [], [], []
        active = np.arange(count)
        for turn in range(int(guard.max()) if count else 0):
            active = active[turn < guard[active]]
            if not len(active):
                break
            axis, least = _least(tmax[active])
            who.append(active)
            cells.append(c[active].copy())
            leaves.append(least)
            go = least <= tb[active]
            active, axis = active[go], axis[go]
            c[active, axis] += step[active, axis]
            tmax[active, axis] = tmax[active, axis] + tdelta[active, axis]
    if not who:
        return np.zeros(0, dtype=np.int64), np.zeros((0, 3), dtype=np.int64), np.zeros(0, dtype=f32)
    return np.concatenate(who), np.concatenate(cells), np.concatenate(leaves)


def block_walk(o, n, t0, te, max_blocks, branches=None):
    """the blocks the rays cross between t0 and te: (ray [M], block [M, 3] int64, t_in [M], t_out [M]) per visit in the order
    of the walk, and cut [N]: the ray's turns ran out first"""
    count = len(o)
    with np.errstate(all="ignore"):
        p = o + t0 * n
        B = np.clip(MP.to_int(np.floor(p)), -FAR, FAR) >> 3
        pos, neg = n > 0, n < 0
        face = np.where(pos, 8 * (B + 1), 8 * B).astype(f32)
        bmax = np.where(pos | neg, t0 + (face - p) / n, f32(np.inf)).astype(f32)
        bdelta = np.where(pos | neg, f32(8) / np.abs(n), f32(np.inf)).astype(f32)
        step = pos.astype(np.int64) - neg.astype(np.int64)
        assert bmax.dtype == f32 and bdelta.dtype == f32 and p.dtype == f32
        if branches is not None:
            branches["zero_component"] += int((n == 0).sum())
            branches["negative_step"] += int(neg.sum())
        t_in = np.full(count, t0, dtype=f32)
        done = np.zeros(count, dtype=bool)
        who, blocks, t_ins, t_outs = [], [], [], []
        active = np.arange(count)
        for _ in range(max_blocks):
            if not len(active):
                break
            t = bmax[active]
            axis, least = _least(t)
            if branches is not None:
                branches["ties"] += int((np.isfinite(least) & ((t == least[:, None]).sum(-1) > 1)).sum())
            who.append(active)
            blocks.append(B[active].copy())
            t_ins.append(t_in[active].copy())
            t_outs.append(np.fmin(least, te[active]))
            go = least < te[active]
            done[active[~go]] = True
            active, axis, least = active[go], axis[go], least[go]
            B[active, axis] += step[active, axis]
            bmax[active, axis] = bmax[active, axis] + bdelta[active, axis]
            t_in[active] = least
    if not who:
        return np.zeros(0, dtype=np.int64), np.zeros((0, 3), dtype=np.int64), np.zeros(0, dtype=f32), np.zeros(0, dtype=f32), ~done
    return np.concatenate(who), np.concatenate(blocks), np.concatenate(t_ins), np.concatenate(t_outs).astype(f32), ~done


class Result:
    """counts (the eight of vk.h), branches (how often each branch of the definition was taken), N (the count per pool
    voxel), and every carve: ray [M] (its index in the call), segment [M] (which visit of a block, numbered in the order of
    each ray's block walk), cell [M, 3], the cells of a segment in the order of its walk"""


def carve(hv, rays, ranges, pose=None, r_min=R_MIN, r_max=R_MAX, t_from=0.0, cap=16.0, flags=0, max_blocks=1024):
    """Mutates `hv` as the call is defined. `flags`: VOXEL_UNITS | ONE_OBSERVATION. Returns a Result."""
    voxel_units, one = bool(flags & VOXEL_UNITS), bool(flags & ONE_OBSERVATION)
    assert 1 <= max_blocks <= MAX_BLOCKS and 1 <= cap <= 32767 and 0 <= r_min < r_max and np.isfinite(r_max)
    assert np.isfinite(t_from) and t_from >= 0
    out = Result()
    out.branches = b = dict(ties=0, zero_component=0, negative_step=0, nothing_to_carve=0, outside_int16=0, absent=0, present=0,
                            outside_block=0, straddling=0, cut_short=0, shared_voxels=0, most_on_a_voxel=0, cap_reached=0)
    count = len(np.asarray(ranges).reshape(-1))
    assert count <= MAX_COUNT
    if count == 0:
        out.counts = None                                               # counts_dev is left alone
        return out
    L = f32(hv.voxel_length)
    with np.errstate(all="ignore"):
        tr = f32(hv.truncation_length) / L
        assert tr <= 64
        o, n, r, kind = IR.carried(hv, rays, ranges, pose, r_min, r_max, voxel_units)
        t0 = f32(t_from) if voxel_units else f32(t_from) / L
        te = r - tr
        assert te.dtype == f32 and t0.dtype == f32
        carves = (kind == IR.INTEGRATED) & (t0 < te)                    # false for a NaN
    nothing = (kind == IR.INTEGRATED) & ~carves
    b["nothing_to_carve"] = int(nothing.sum())
    index = np.flatnonzero(carves)
    o, n, te = o[index], n[index], te[index]
    who, blocks, t_in, t_out, cut = block_walk(o, n, t0, te, max_blocks, b)
    b["cut_short"] = int(cut.sum())
    inside = IR.in_int16(blocks)
    b["outside_int16"] = int((~inside).sum())
    slot = CR.Lookup(RR.block_table(hv)).slots(blocks) if len(blocks) else np.zeros(0, dtype=np.int64)
    held = slot >= 0
    b["absent"], b["present"] = int((inside & ~held).sum()), int(held.sum())
    who, blocks, t_in, t_out, slot = who[held], blocks[held], t_in[held], t_out[held], slot[held]

    # the cell walk of every visit of a present block
    visit, cells, leaves = walk(o[who], n[who], t_in, t_out)
    mine = ((cells >> 3) == blocks[visit]).all(-1)
    before = leaves <= te[who[visit]]
    b["outside_block"], b["straddling"] = int((~mine).sum()), int((mine & ~before).sum())
    take = mine & before
    visit, cells = visit[take], cells[take]
    out.ray, out.segment, out.cell = index[who[visit]], visit, cells
    at = slot[visit] * 512 + (cells[:, 2] & 7) * 64 + (cells[:, 1] & 7) * 8 + (cells[:, 0] & 7)
    N = np.zeros(hv.max * 512, dtype=np.int64)
    np.add.at(N, at, 1)
    out.N = N
    b["shared_voxels"], b["most_on_a_voxel"] = int((N >= 2).sum()), int(N.max()) if len(N) else 0

    # the fold: the running average goes on with an observation of exactly 1
    at = np.flatnonzero(N > 0)
    with np.errstate(all="ignore"):
        ws = np.ones(len(at), dtype=f32) if one else N[at].astype(f32)
        wd = hv.voxels["distance_weight"][at].astype(f32)
        total = wd + ws
        mean = (wd * hv.voxels["distance"][at] + ws) / total
        assert mean.dtype == f32
        b["cap_reached"] = int((total >= f32(cap)).sum())
        hv.voxels["distance"][at] = np.where(wd == 0, f32(1), mean)
        hv.voxels["distance_weight"][at] = np.minimum(f32(cap), total).astype(np.int16)
    out.counts = (int(carves.sum()), int(nothing.sum()), int((kind == IR.NO_MEASUREMENT).sum()), int((kind == IR.INVALID).sum()),
                  int(cut.sum()), len(np.unique(at // 512)), len(at), int(N.sum()) & 0xffffffff)
    return out


# ---- the ray sets the CPU and the GPU tests share ----------------------------------------------------------------------

NAMES = "abcdefgh"
_SETS = {}
BEYOND = 1.5                                                          # set (h): the ranges of the scene's hits times this


def ray_sets(orc, voxel_units):
    """integrate_rays_reference's seven sets and (h): the scene's pixel rays with cast_rays' ranges times 1.5, clipped below
    r_max — rays that pass through the fused surface and carve it"""
    if voxel_units in _SETS:
        return _SETS[voxel_units]
    L = f32(CR.volume(orc).voxel_length)
    rays, t = IR.pixel_hits(orc)
    with np.errstate(all="ignore"):
        beyond = np.minimum(t * f32(BEYOND), f32(0.98) * f32(R_MAX)).astype(f32)
        for units in (False, True):
            sets = dict(IR.ray_sets(orc, units))
            there = rays.copy()
            there[:, :3] = rays[:, :3] / L if units else rays[:, :3]
            sets["h"] = (there, beyond / L if units else beyond)
            _SETS[units] = sets
    return _SETS[voxel_units]


def spans(orc):
    sets, at, out = ray_sets(orc, False), 0, {}
    for name in NAMES:
        out[name] = slice(at, at + len(sets[name][1]))
        at += len(sets[name][1])
    return out


def all_rays(orc, voxel_units):
    """(rays [N, 6], ranges [N]): every set, one after the other"""
    sets = ray_sets(orc, voxel_units)
    return (np.ascontiguousarray(np.concatenate([sets[name][0] for name in NAMES]), dtype=f32),
            np.ascontiguousarray(np.concatenate([sets[name][1] for name in NAMES]), dtype=f32))


bounds, permuted = IR.bounds, IR.permuted


def keywords(flags, kw):
    """the statement's and the device call's keywords for one case: t_from is given in metres and converted like the bounds"""
    units = bool(flags & VOXEL_UNITS)
    r_min, r_max = bounds(units)
    kw = dict(kw)
    t_from = kw.pop("t_from", 0.0)
    kw["t_from"] = float(np.float32(t_from) / np.float32(R.VOXEL)) if units else float(np.float32(t_from))
    return r_min, r_max, kw


def state_but_voxels(hv):
    """everything of a HostVolume the call must leave as it found it, as bytes"""
    return (hv.hash_entries.tobytes(), hv.free_voxel_blocks.tobytes(), hv.block_visibility.tobytes(), hv.allocation_types.tobytes(),
            hv.allocation_blocks.tobytes(), hv.visible_blocks.tobytes(), hv.counters.tobytes())


# ---- the scenario the call exists for: a wall that is no longer there ---------------------------------------------------

FRONT, BACK = 1.0, 1.4                      # two fronto-parallel planes in metres: ten truncation lengths apart
SIZES = (4093, 2048)
REPEATS = 3
_SCENARIO = {}


def scenario_rays():
    """(rays [19 200, 6], ranges of the front plane, ranges of the back plane): the fusing camera's pixel rays, and the
    distance along each normalised ray to the plane z = FRONT, z = BACK"""
    rays = IR.pixel_rays()[0]
    d = rays[:, 3:]
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return rays, (f32(FRONT) * length).astype(f32), (f32(BACK) * length).astype(f32)


def scenario(orc, carving=True):
    """(host volume, the counts of every call in order, cast_reference.cast of the rays at the end): the front wall fused
    once, then the back wall fused and (with `carving`) carved REPEATS times, every call with ONE_OBSERVATION, in a fresh
    volume. Computed once, never changed."""
    if carving not in _SCENARIO:
        rays, front, back = scenario_rays()
        hv = M.fresh(orc, *SIZES)
        counts = [IR.integrate(hv, rays, front, r_min=0.1, flags=ONE_OBSERVATION).counts]
        for _ in range(REPEATS):
            counts.append(IR.integrate(hv, rays, back, r_min=0.1, flags=ONE_OBSERVATION).counts)
            if carving:
                counts.append(carve(hv, rays, back, r_min=0.1, flags=ONE_OBSERVATION).counts)
        _SCENARIO[carving] = (hv, counts, CR.cast(hv, rays))
    return _SCENARIO[carving]
