"""The CPU statement of vk_volume_color_rays (include/vk.h): which voxels of a volume a batch of coloured range rays visits —
the cells of existing blocks a ray crosses within `band` of its measurement — and what colour each holds afterwards, in numpy,
on an oracle.HostVolume. The ray, its range and the cell traversal are vk_volume_integrate_rays'
(tests/integrate_rays_reference.py); the test that a voxel is near the surface and the capped running average are the
reference colour integrator's (src/color_integrator.cu:121, 125-129). There is no upstream call for a colour that is no pixel
of a pinhole image, so this file is the definition.

Everything is float32 with one rounding per operation, in the order vk.h gives, and what rays that share a voxel add up are
integers: no result depends on the order of the rays, no tolerance exists and the device is held to it bit for bit
(tests/test_gpu_color_rays.py).

It is vectorised over rays with a per-ray active mask (carve_rays_reference.walk between the ends this call gives it), and it
holds the colours and the scenario the CPU and the GPU tests share."""
import numpy as np

import carve_rays_reference as CV
import cast_reference as CR
import integrate_rays_reference as IR
import merge_reference as M
import register_reference as RR
import release_reference as R

f32 = np.float32
VOXEL_UNITS, ONE_OBSERVATION = IR.VOXEL_UNITS, IR.ONE_OBSERVATION
MAX_COUNT = 1 << 21
MAX_BAND = 64                                                         # in voxels
SCALE = f32(1024.0)                                                   # 2^10: a visit adds rintf(c * 2^10)
R_MIN, R_MAX = IR.R_MIN, IR.R_MAX
COLOURED, NO_COLOUR, NO_MEASUREMENT, INVALID = 0, 1, 2, 3


def ends(r, b):
    """(ta, tb) of the walk: within b of the measurement, from the origin on"""
    with np.errstate(all="ignore"):
        return np.fmax(r - b, f32(0)), r + b


def classify(kind, colors):
    """what each ray is, by the first rule that applies: invalid, no measurement, no colour, coloured"""
    with np.errstate(all="ignore"):
        has = ((f32(0) <= colors) & (colors <= f32(1))).all(-1)                      # false for a NaN
    return np.where(kind == IR.INVALID, INVALID, np.where(kind == IR.NO_MEASUREMENT, NO_MEASUREMENT, np.where(has, COLOURED, NO_COLOUR)))


class Result:
    """counts (the eight of vk.h), branches (how often each branch of the definition was taken), S [pool voxels, 3] and N (the
    sums per pool voxel), near (the voxels with N > 0 that were updated)"""


def color(hv, rays, ranges, colors, pose=None, r_min=R_MIN, r_max=R_MAX, band=None, cap=16.0, flags=0):
    """Mutates `hv` as the call is defined. `band` None: the truncation length in the unit the form takes it in. `flags`:
    VOXEL_UNITS | ONE_OBSERVATION. Returns a Result."""
    voxel_units, one = bool(flags & VOXEL_UNITS), bool(flags & ONE_OBSERVATION)
    L = f32(hv.voxel_length)
    if band is None:
        band = f32(hv.truncation_length) / L if voxel_units else f32(hv.truncation_length)
    band = f32(band)
    with np.errstate(all="ignore"):
        b = band if voxel_units else band / L
        tr = f32(hv.truncation_length) / L
    assert 1 <= cap <= 32767 and 0 <= r_min < r_max and np.isfinite(r_max) and np.isfinite(band) and band > 0 and b <= MAX_BAND and tr <= 64
    out = Result()
    out.branches = br = dict(ta_clamped=0, visits=0, outside_int16=0, lost=0, shared_voxels=0, most_on_a_voxel=0, not_near=0,
                             first_colour=0, continued=0, cap_reached=0)
    count = len(np.asarray(ranges).reshape(-1))
    assert count <= MAX_COUNT
    if count == 0:
        out.counts = None                                               # counts_dev is left alone
        return out
    colors = np.ascontiguousarray(colors, dtype=f32).reshape(-1, 3)
    assert len(colors) == count
    o, n, r, kind = IR.carried(hv, rays, ranges, pose, r_min, r_max, voxel_units)
    what = classify(kind, colors)
    index = np.flatnonzero(what == COLOURED)
    o, n, r = o[index], n[index], r[index]
    with np.errstate(all="ignore"):
        q = np.rint(colors[index] * SCALE).astype(np.int64)                          # ties to even
        br["ta_clamped"] = int((r - b < 0).sum())
    ta, tb = ends(r, b)
    who, cells, _ = CV.walk(o, n, ta, tb)
    blocks = cells >> 3
    inside = IR.in_int16(blocks)
    br["visits"], br["outside_int16"] = len(who), int((~inside).sum())
    who, cells, blocks = who[inside], cells[inside], blocks[inside]
    slot = CR.Lookup(RR.block_table(hv)).slots(blocks) if len(blocks) else np.zeros(0, dtype=np.int64)
    held = slot >= 0
    br["lost"] = int((~held).sum())
    who, cells, slot = who[held], cells[held], slot[held]
    out.ray, out.cell = index[who], cells
    at = slot * 512 + (cells[:, 2] & 7) * 64 + (cells[:, 1] & 7) * 8 + (cells[:, 0] & 7)
    S, N = np.zeros((hv.max * 512, 3), dtype=np.int64), np.zeros(hv.max * 512, dtype=np.int64)
    np.add.at(S, at, q[who])
    np.add.at(N, at, 1)
    br["shared_voxels"], br["most_on_a_voxel"] = int((N >= 2).sum()), int(N.max()) if len(N) else 0
    heads = (len(index), int((what == NO_COLOUR).sum()), int((what == NO_MEASUREMENT).sum()), int((what == INVALID).sum()))
    return fold(hv, out, S, N, heads, br["lost"], cap, one)


def fold(hv, out, S, N, heads, lost, cap, one):
    """the fold of the sums S [pool voxels, 3] and N [pool voxels] into `hv`: a voxel near the surface continues its colour's
    running average with the mean colour and weight ws. `heads`: the four ray counts. Fills and returns `out`."""
    assert S.max(initial=0) <= 1 << 31 and N.max(initial=0) <= 1 << 21              # the four fields of the two words never meet
    out.S, out.N = S, N
    br = out.branches
    visited = np.flatnonzero(N > 0)
    with np.errstate(all="ignore"):
        near = np.abs(hv.voxels["distance"][visited]) < f32(1)                       # false for a NaN
        at = visited[near]
        m = (S[at].astype(f32) / N[at].astype(f32)[:, None]) * f32(2.0 ** -10)
        ws = np.ones(len(at), dtype=f32) if one else N[at].astype(f32)
        wc = hv.voxels["color_weight"][at].astype(f32)
        total = wc + ws
        mean = (wc[:, None] * hv.voxels["color"][at] + ws[:, None] * m) / total[:, None]
        assert m.dtype == f32 and mean.dtype == f32
        br["not_near"], br["first_colour"], br["continued"] = int((~near).sum()), int((wc == 0).sum()), int((wc != 0).sum())
        br["cap_reached"] = int((total >= f32(cap)).sum())
        hv.voxels["color"][at] = np.where((wc == 0)[:, None], m, mean)
        hv.voxels["color_weight"][at] = np.minimum(f32(cap), total).astype(np.int16)
    out.near = at
    out.counts = tuple(heads) + (len(np.unique(at // 512)), len(at), int((~near).sum()), as_int32(lost))
    return out


def as_int32(lost):
    """the visits lost as counts_dev[7] holds them: the sum wraps at 2^32 and is read as an int32"""
    lost &= 0xffffffff
    return lost - (1 << 32) if lost >= 1 << 31 else lost


# ---- the colours the CPU and the GPU tests share -----------------------------------------------------------------------

def colors_for(count, seed=83):
    """seeded random colours [count, 3] with strided bad channels: a NaN (every 97th ray, channel 0), -0.25 (every 101st,
    channel 1), 1.5 (every 103rd, channel 2); and the exact ends 0 and 1 (every 89th and 91st), which are colours"""
    colors = np.random.default_rng(seed).uniform(0, 1, (count, 3)).astype(f32)
    colors[::89] = 0
    colors[::91] = 1
    colors[5::97, 0] = np.nan
    colors[7::101, 1] = -0.25
    colors[11::103, 2] = 1.5
    return colors


def all_rays(orc, voxel_units):
    """(rays, ranges, colours): integrate_rays' seven sets, one after the other, with the seeded colours"""
    rays, ranges = IR.all_rays(orc, voxel_units)
    return rays, ranges, colors_for(len(ranges))


def keywords(flags, kw):
    """the statement's and the device call's keywords for one case: the band is given in metres (None: the truncation length)
    and converted like the bounds"""
    units = bool(flags & VOXEL_UNITS)
    r_min, r_max = IR.bounds(units)
    kw = dict(kw)
    band = np.float32(R.TRUNCATION if kw.get("band") is None else kw["band"])
    kw["band"] = float(band / np.float32(R.VOXEL)) if units else float(band)
    return r_min, r_max, kw


def permuted(rays, ranges, colors, seed=5):
    order = np.random.default_rng(seed).permutation(len(ranges))
    return np.ascontiguousarray(rays[order]), np.ascontiguousarray(ranges[order]), np.ascontiguousarray(colors[order])


# ---- the scenario the call exists for: a map built from rays has colours ------------------------------------------------

SIZES = (4093, 2048)
_SCENARIO = {}


def paint(points):
    """the colour of a point in metres [N, 3], a smooth function: float32 [N, 3] inside [0.1, 0.9]"""
    x, y = points[:, 0].astype(np.float64), points[:, 1].astype(np.float64)
    return np.stack([0.5 + 0.4 * np.sin(6 * x), 0.5 + 0.4 * np.sin(6 * y + 1), 0.5 + 0.4 * np.sin(6 * (x + y) + 2)], -1).astype(f32)


def hit_points(rays, t):
    """where the rays (origins in metres, the volume's frame) end, in metres: float64 [N, 3]"""
    d = rays[:, 3:].astype(np.float64)
    return rays[:, :3].astype(np.float64) + t.astype(np.float64)[:, None] * d / np.linalg.norm(d, axis=-1)[:, None]


def scenario_rays(orc):
    """(rays [19 200, 6], ranges, colours): the scene's pixel rays that all hit, with cast_rays' ranges, painted at the hit"""
    rays, t = IR.pixel_hits(orc)
    return rays, t, paint(hit_points(rays, t))


def scenario(orc, band=None, coloring=True):
    """(host volume, the counts of the calls in order, cast_reference.cast of the rays at the end): the rays fused into a fresh
    volume, then (with `coloring`) coloured, both with ONE_OBSERVATION. `band` in metres; None: the truncation length.
    Computed once, never changed."""
    key = (None if band is None else float(band), coloring)
    if key not in _SCENARIO:
        rays, t, colors = scenario_rays(orc)
        hv = M.fresh(orc, *SIZES)
        counts = [IR.integrate(hv, rays, t, r_min=0.1, flags=ONE_OBSERVATION).counts]
        if coloring:
            counts.append(color(hv, rays, t, colors, r_min=0.1, band=band, flags=ONE_OBSERVATION).counts)
        _SCENARIO[key] = (hv, counts, CR.cast(hv, rays))
    return _SCENARIO[key]


TWO_VOXELS = float(f32(2) * f32(R.VOXEL))
