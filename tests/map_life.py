"""The life of a map, as data: chains of volume operations in which every operation starts from the state the one before it
left. A step is a record with a name, a function that applies the CPU statement (tests/*_reference.py) to oracle.HostVolume
objects and a function that makes the same call on api.Volume objects through their methods; a chain is the volumes it starts
from and its steps. tests/test_map_life.py shows on the statements alone that the chains reach what they are for — a pool a
release has rebuilt, colour no camera wrote, carved voxels, an exhausted pool — and tests/test_gpu_map_life.py holds the device
to every step, bit for bit, with one upload at the start.

The units and bounds of every call are converted where the per-operation GPU tests convert them (the statements' keywords()
helpers and integrate_rays_reference.bounds); a merge goes on with VK_MERGE_CONTINUE on the host exactly as Volume.merge does on the device.

Two of the read steps compare the terms of a registration, which the C++ class layer does not expose: their class_host is the
statement of the loop the class makes instead, for tests/test_gpu_chain_replay.py, which runs the same chains through that layer
from the files tests/chain_files.py writes.

The chains over two lattices (two_resolutions, resampled_exhausted, random_resolution_chain) add the resampled merge, the pack
and its merge, the load of a saved map into an object of other table sizes and the clearance field; they start from the
depth-integrated view, since a map of two ray quarters gives a resampled merge next to nothing to sample. These four are not
yet calls of the class layer's replay.

The rays are integrate_rays_reference.pixel_hits: the 19 200 pixel rays with the ranges cast_rays gives them, taken in strided
quarters of 4 800; the colours are color_rays_reference.colors_for, seeded by the quarter."""
import numpy as np

import carve_rays_reference as CV
import cast_reference as CR
import color_rays_reference as CO
import distance_field_reference as DF
import extract_attributes_reference as A
import integrate_rays_reference as IR
import merge_pose_reference as MP
import merge_reference as M
import merge_resample_reference as MR
import pack_reference as P
import register_rays_reference as RY
import register_reference as RR
import release_reference as R
import sample_reference as S
import score_poses_reference as SP
import scenes
from vulcan_amd import vk_types as T

f32 = np.float32
LONG, OTHER = (509, 4096), (4093, 2048)                   # long chains; the other volume of a merge
MUTATE, FRAME, READ = "mutate", "frame", "read"
BEYOND = CV.BEYOND                                         # carving ranges: the hit's times this, through the surface
BAND = 0.75                                                # register's band, in truncation lengths
LOOP_STEPS = 3                                             # Gauss-Newton steps of the loops the class layer makes (class_host)
_RAYS, _RUNS = {}, {}


def rays_of(orc, quarter, units=False, stretch=1.0):
    """(rays [4 800, 6], ranges [4 800]) of strided quarter `quarter` of the pixel rays, in metres or (`units`) in voxels, as
    integrate_rays_reference.ray_sets converts a set; `stretch`: the ranges times this, clipped below r_max as
    carve_rays_reference's set (h) is"""
    key = (quarter, bool(units), float(stretch))
    if key not in _RAYS:
        rays, t = IR.pixel_hits(orc)
        rays, ranges = rays[quarter::4].copy(), t[quarter::4].copy()
        L = f32(R.VOXEL)
        with np.errstate(all="ignore"):
            if stretch != 1.0:
                ranges = np.minimum(ranges * f32(stretch), f32(0.98) * f32(IR.R_MAX)).astype(f32)
            if units:
                rays[:, :3] = rays[:, :3] / L
                ranges = ranges / L
        _RAYS[key] = (np.ascontiguousarray(rays, dtype=f32), np.ascontiguousarray(ranges, dtype=f32))
    return _RAYS[key]


def colors_of(quarter):
    return CO.colors_for(4800, seed=83 + quarter)


def another_pose():
    """a pose that is not generic(): yaw -7 degrees, t = (0.02, 0.01, -0.015) m"""
    return T.Transform.translate(0.02, 0.01, -0.015) * scenes.yaw(-7.0)


class DeviceSide:
    """what the device functions of the steps share: the module api, {name: api.Volume}, the rays on the device, and one
    Extractor and one Tracer per volume, kept between the steps like the volumes' own workspaces"""

    def __init__(self, api, volumes):
        self.api, self.volumes = api, volumes
        self._tensors, self._extractors, self._tracers = {}, {}, {}
        self._directory = None

    def directory(self):
        """a temporary directory of this side's own, for the map files of the load steps: gone with the side"""
        import pathlib
        import tempfile
        if self._directory is None:
            self._directory = tempfile.TemporaryDirectory(prefix="map_life_")
        return pathlib.Path(self._directory.name)

    def replace(self, name, volume):
        """another object under `name` (a load step): the Extractor and the Tracer of the one before go with it"""
        self.volumes[name] = volume
        self._extractors.pop(name, None)
        self._tracers.pop(name, None)

    def tensor(self, key, make):
        import torch
        if key not in self._tensors:
            self._tensors[key] = torch.as_tensor(np.ascontiguousarray(make(), dtype=np.float32)).cuda()
        return self._tensors[key]

    def rays(self, orc, quarter, units, stretch=1.0):
        key = (quarter, bool(units), float(stretch))
        return (self.tensor(("rays",) + key, lambda: rays_of(orc, quarter, units, stretch)[0]),
                self.tensor(("ranges",) + key, lambda: rays_of(orc, quarter, units, stretch)[1]))

    def extractor(self, name):
        if name not in self._extractors:
            ex = self._extractors[name] = self.api.Extractor(self.volumes[name])
            ex.all_allocated, ex.interpolate = True, True
        return self._extractors[name]

    def extractors(self):
        return list(self._extractors.values())

    def tracer(self, name):
        """the volume's one Tracer: the integrators prepare its raycast bounds ahead, the volume operations void them"""
        if name not in self._tracers:
            self._tracers[name] = self.api.Tracer(self.volumes[name])
        return self._tracers[name]


class Step:
    """`host(orc, volumes)` applies the statement to the HostVolume objects and returns what the call returns; `device(orc,
    side, want)` makes the call on side.volumes and returns the same, as the statement gives it; `workspace(side)` makes sure
    the workspace the call will use is the volume's cached one. `on`: the volume a mutating step changes; `reads`: the volumes
    it only reads. `work(want)`: did the step do anything. `class_host(orc, volumes)`: a second statement, for the steps whose
    call the C++ class layer does not expose (tests/chain_files.py) — what the call it makes instead returns on the same
    state; host_run evaluates it only when asked"""

    def __init__(self, name, kind, on, host, device, workspace=None, reads=(), work=None, class_host=None, **facts):
        self.name, self.kind, self.on, self.reads = name, kind, on, tuple(reads)
        self.host, self.device, self.work = host, device, work
        self.class_host = class_host
        self.workspace = workspace or (lambda side: None)
        self.facts = facts

    def __repr__(self):
        return self.name


def _workspace(side, name, operation, size, bytes_name, counts):
    dv = side.volumes[name]
    dv._workspace(operation, size, getattr(side.api.lib(), bytes_name), counts)


def _form(flags):
    return bool(flags & IR.VOXEL_UNITS), bool(flags & IR.ONE_OBSERVATION)


def _tag(pose, flags, cap):
    units, one = _form(flags)
    return "".join([", posed" if pose is not None else "", ", voxels" if units else "", ", one observation" if one else "",
                    f", cap {cap:g}" if cap != 16.0 else ""])


# ---- the steps that change a volume --------------------------------------------------------------------------------------

def integrate_rays(quarter, pose=None, flags=0, cap=16.0, on="map"):
    units, one = _form(flags)
    r_min, r_max = IR.bounds(units)

    def host(orc, volumes):
        rays, ranges = rays_of(orc, quarter, units)
        return IR.integrate(volumes[on], rays, ranges, pose=pose, r_min=r_min, r_max=r_max, cap=cap, flags=flags).counts

    def device(orc, side, want):
        rays, ranges = side.rays(orc, quarter, units)
        return side.volumes[on].integrate_rays(rays, ranges, pose=pose, r_min=r_min, r_max=r_max, max_distance_weight=cap,
                                               one_observation=one, voxel_units=units)

    def workspace(side):
        dv = side.volumes[on]
        _workspace(side, on, "integrate_rays", (dv.main, dv.excess), "vk_volume_integrate_rays_workspace_bytes", 8)

    return Step(f"integrate_rays(quarter {quarter}{_tag(pose, flags, cap)})", MUTATE, on, host, device, workspace,
                work=lambda counts: counts[6] > 0, operation="integrate_rays", allocates=True, quarter=quarter, pose=pose, flags=flags, cap=cap,
                r_min=r_min, r_max=r_max)


def color_rays(quarter, pose=None, flags=0, cap=16.0, band=None, on="map"):
    """`band` in metres (None: the truncation length), converted like the bounds by color_rays_reference.keywords"""
    units, one = _form(flags)
    r_min, r_max, kw = CO.keywords(flags, {"band": band})

    def host(orc, volumes):
        rays, ranges = rays_of(orc, quarter, units)
        return CO.color(volumes[on], rays, ranges, colors_of(quarter), pose=pose, r_min=r_min, r_max=r_max, band=kw["band"], cap=cap,
                        flags=flags).counts

    def device(orc, side, want):
        rays, ranges = side.rays(orc, quarter, units)
        colors = side.tensor(("colors", quarter), lambda: colors_of(quarter))
        return side.volumes[on].color_rays(rays, ranges, colors, pose=pose, band=kw["band"], r_min=r_min, r_max=r_max,
                                           max_color_weight=cap, one_observation=one, voxel_units=units)

    def workspace(side):
        dv = side.volumes[on]
        _workspace(side, on, "color_rays", (dv.main, dv.excess), "vk_volume_color_rays_workspace_bytes", 8)

    name = f"color_rays(quarter {quarter}{_tag(pose, flags, cap)}{'' if band is None else ', band %g m' % band})"
    return Step(name, MUTATE, on, host, device, workspace, work=lambda counts: counts[5] > 0, operation="color_rays", quarter=quarter, pose=pose,
                flags=flags, cap=cap, r_min=r_min, r_max=r_max, band=kw["band"])


def carve_rays(quarter, pose=None, flags=0, cap=16.0, stretch=BEYOND, on="map"):
    units, one = _form(flags)
    r_min, r_max, kw = CV.keywords(flags, {})

    def host(orc, volumes):
        rays, ranges = rays_of(orc, quarter, units, stretch)
        return CV.carve(volumes[on], rays, ranges, pose=pose, r_min=r_min, r_max=r_max, t_from=kw["t_from"], cap=cap, flags=flags).counts

    def device(orc, side, want):
        rays, ranges = side.rays(orc, quarter, units, stretch)
        return side.volumes[on].carve_rays(rays, ranges, pose=pose, t_from=kw["t_from"], r_min=r_min, r_max=r_max,
                                           max_distance_weight=cap, one_observation=one, voxel_units=units)

    def workspace(side):
        dv = side.volumes[on]
        _workspace(side, on, "carve_rays", (dv.main, dv.excess), "vk_volume_carve_rays_workspace_bytes", 8)

    return Step(f"carve_rays(quarter {quarter}, ranges x {stretch:g}{_tag(pose, flags, cap)})", MUTATE, on, host, device, workspace,
                work=lambda counts: counts[6] > 0, operation="carve_rays", quarter=quarter, pose=pose, flags=flags, cap=cap, r_min=r_min, r_max=r_max,
                t_from=kw["t_from"], stretch=stretch)


def release_blocks(rule, on="map", keep_box=None):
    """`rule`: a key of release_reference.RULES; `keep_box`: that rule set with this box to keep, in block coordinates"""
    keywords = R.RULES[rule] if keep_box is None else dict(R.RULES[rule], keep_box=keep_box)

    def host(orc, volumes):
        return R.release_blocks(volumes[on], *R.helper_arguments(keywords))

    def device(orc, side, want):
        return side.volumes[on].release_blocks(**keywords)

    def workspace(side):
        dv = side.volumes[on]
        _workspace(side, on, "release", (dv.main, dv.excess), "vk_volume_release_workspace_bytes", 4)

    name = f"release_blocks({rule}{'' if keep_box is None else ', keep %s .. %s' % keep_box})"
    return Step(name, MUTATE, on, host, device, workspace, work=lambda counts: counts[0] > 0,
                operation="release_blocks", rule=rule, keywords=keywords)


def merge_statement(dst, src, pose=None, max_rounds=8, calls=None):
    """Volume.merge on the host: the statement's call, then its call that continues while a call posted requests in every
    round, dropped none and still left blocks out — the later calls' counts added up as Volume._merge_rounds adds them.
    `calls`: a list that takes the counts of every call made"""
    workspace = {}
    if pose is None:
        return rounds_statement(dst, lambda flags: M.merge(dst, src, flags, max_rounds, workspace=workspace), max_rounds, False, calls)
    return rounds_statement(dst, lambda flags: MP.merge(dst, src, pose, flags, max_rounds, workspace=workspace), max_rounds, True, calls)


def rounds_statement(dst, call, max_rounds, eight, calls=None):
    """Volume._merge_rounds on the host: `call(0)`, then `call(CONTINUE)` under merge_statement's rule. `eight`: the call
    returns the eight counts of the posed and the resampled merge (left out = 4, rounds = 5, summed 2, 3, 5, 7), not the
    six of the plain and the packed one (left out = 3, rounds = 4, summed 1, 2, 4)"""
    dropped = int(dst.counters[T.VK_CTR_DROPPED])
    left_out, rounds, summed = (4, 5, (2, 3, 5, 7)) if eight else (3, 4, (1, 2, 4))
    counts = call(0)
    total = list(counts)
    made = [] if calls is None else calls
    made.append(tuple(counts))
    while counts[rounds] == max_rounds and counts[left_out] > 0 and int(dst.counters[T.VK_CTR_DROPPED]) == dropped:
        counts = call(M.CONTINUE)
        made.append(tuple(counts))
        for i in summed:
            total[i] += counts[i]
        total[left_out] = counts[left_out]
    return tuple(total)


def merge(on, source, pose=None, max_rounds=8):
    """volume `on` takes volume `source`, through `pose` (T_on_source) or on the shared lattice, in calls of `max_rounds`
    allocation rounds; the calls the statement made are the step's facts["calls"]"""
    step = None

    def host(orc, volumes):
        step.facts["calls"] = []
        return merge_statement(volumes[on], volumes[source], pose, max_rounds, step.facts["calls"])

    def device(orc, side, want):
        return side.volumes[on].merge(side.volumes[source], pose=pose, max_rounds=max_rounds)

    def workspace(side):
        dv, ds = side.volumes[on], side.volumes[source]
        if pose is None:
            _workspace(side, on, "merge", (ds.main, ds.excess), "vk_volume_merge_workspace_bytes", 6)
        else:
            _workspace(side, on, "merge_posed", (ds.main, ds.excess, dv.main, dv.excess), "vk_volume_merge_posed_workspace_bytes", 8)

    name = f"merge({on} <- {source}{', posed' if pose is not None else ''}{'' if max_rounds == 8 else ', %d round(s) a call' % max_rounds})"
    step = Step(name, MUTATE, on, host, device, workspace, reads=(source,),
                work=lambda counts: counts[1 if pose is None else 2] > 0, operation="merge", posed=pose is not None, allocates=True, source=source, pose=pose,
                max_rounds=max_rounds)
    return step


def merge_resampled(on, source, pose, supersample, max_rounds=8, skip_unobserved=False):
    """volume `on` takes volume `source` of another voxel or truncation length through `pose` (T_on_source), `supersample`^3
    samples a voxel, in calls of `max_rounds` allocation rounds: Volume.merge_resampled, with merge's rule for the calls that
    continue; the calls the statement made are the step's facts["calls"]"""
    step = None
    flags = MR.SKIP_UNOBSERVED if skip_unobserved else 0

    def host(orc, volumes):
        step.facts["calls"] = []
        dst, src, workspace = volumes[on], volumes[source], {}
        return rounds_statement(dst, lambda go_on: MR.merge(dst, src, pose, supersample, flags | go_on, max_rounds, workspace=workspace),
                                max_rounds, True, step.facts["calls"])

    def device(orc, side, want):
        return side.volumes[on].merge_resampled(side.volumes[source], pose=pose, supersample=supersample, skip_unobserved=skip_unobserved,
                                                max_rounds=max_rounds)

    def workspace(side):
        dv, ds = side.volumes[on], side.volumes[source]
        box = MR.box_blocks(f32(ds.voxel_length) / f32(dv.voxel_length))
        _workspace(side, on, "merge_resampled", (ds.main, ds.excess, dv.main, dv.excess, box), "vk_volume_merge_resampled_workspace_bytes", 8)

    name = (f"merge_resampled({on} <- {source}, n {supersample}{', skip unobserved' if skip_unobserved else ''}"
            f"{'' if max_rounds == 8 else ', %d round(s) a call' % max_rounds})")
    step = Step(name, MUTATE, on, host, device, workspace, reads=(source,), work=lambda counts: counts[2] > 0 and counts[7] > 0,
                operation="merge_resampled", allocates=True, source=source, pose=pose, supersample=supersample, max_rounds=max_rounds,
                skip_unobserved=skip_unobserved)
    return step


def _pack_rule(box, skip_unobserved):
    flags = (P.SKIP_UNOBSERVED if skip_unobserved else 0) | (P.BOX if box is not None else 0)
    lo, hi = box if box is not None else ((0, 0, 0), (0, 0, 0))
    return flags, lo, hi


def pack_merge(on, source, box=None, skip_unobserved=False, max_rounds=8):
    """volume `source` packed under the rule (`box` in block coordinates, inclusive; `skip_unobserved`), and the pack merged
    into volume `on` (which may be `source` itself: a pack is a copy): Volume.pack, then Volume.merge(pack). Returns merge's
    six counts, then the pack's origins and voxels; the pack's four counts are the step's facts["packed"]"""
    step = None

    def host(orc, volumes):
        dst, workspace = volumes[on], {}
        origins, voxels, step.facts["packed"] = P.pack(volumes[source], *_pack_rule(box, skip_unobserved))
        src = volumes[source]
        step.facts["calls"] = []
        if len(origins) == 0:                                             # Volume.merge makes no call for a pack without blocks
            return (0, 0, 0, 0, 0, 0, origins, voxels)
        counts = rounds_statement(dst, lambda go_on: P.merge_packed(dst, origins, voxels, len(origins), src.voxel_length, src.truncation_length,
                                                                    go_on, max_rounds, workspace=workspace),
                                  max_rounds, False, step.facts["calls"])
        return counts + (origins, voxels)

    def device(orc, side, want):
        pack = side.volumes[source].pack(box=box, skip_unobserved=skip_unobserved)
        counts = side.volumes[on].merge(pack, max_rounds=max_rounds)
        return tuple(counts) + pack.host()

    def workspace(side):
        ds = side.volumes[source]
        _workspace(side, source, "pack", (ds.main, ds.excess), "vk_volume_pack_workspace_bytes", 4)
        _workspace(side, on, "merge_packed", (step.facts["packed"][2],), "vk_volume_merge_packed_workspace_bytes", 6)

    rule = "".join([", box" if box is not None else "", ", skip unobserved" if skip_unobserved else ""])
    name = f"pack_merge({on} <- {source}{rule}{'' if max_rounds == 8 else ', %d round(s) a call' % max_rounds})"
    step = Step(name, MUTATE, on, host, device, workspace, reads=(source,), work=lambda want: want[1] > 0, operation="pack_merge",
                allocates=True, source=source, box=box, skip_unobserved=skip_unobserved, max_rounds=max_rounds)
    return step


def load(on, source):
    """volume `source` packed whole, saved, and the file loaded as a new volume in the place of `on` — a volume the chain
    starts fresh, of `source`'s lattice and of table sizes of its own, which nothing has touched: PackedVolume.save, then
    Volume.load with `on`'s sizes. Volume.load returns the volume and no counts (it raises where a block is left out), so
    the step returns the one number both sides can give, (blocks loaded,): on the host the blocks the merge of the load —
    both caps 32767 — fused, none left out; on the device the blocks of the pack that was saved. What holds the device to
    the statement is the state of `on` compared behind the step."""
    step = None

    def host(orc, volumes):
        dst, src = volumes[on], volumes[source]
        assert not (dst.hash_entries["data"] >= 0).any() and not (dst.voxels["distance_weight"] != 0).any(), f"{on} is not fresh"
        assert int(dst.counters[T.VK_CTR_DROPPED]) == 0, f"{on} is not fresh"
        assert (f32(dst.voxel_length), f32(dst.truncation_length)) == (f32(src.voxel_length), f32(src.truncation_length))
        origins, voxels, step.facts["packed"] = P.pack(src)
        workspace = {}
        counts = rounds_statement(dst, lambda go_on: P.merge_packed(dst, origins, voxels, len(origins), src.voxel_length, src.truncation_length,
                                                                    go_on, 8, 32767.0, 32767.0, workspace=workspace),
                                  8, False)
        assert counts[3] == 0 and counts[1] == len(origins), "the chain's sizes for the loaded volume must hold the map"
        return (counts[1],)

    def device(orc, side, want):
        api, old = side.api, side.volumes[on]
        path = side.directory() / f"{on}.vkmap"
        pack = side.volumes[source].pack()
        pack.save(path)
        new = api.Volume.load(path, old.main, old.excess)
        assert new._workspaces == {} and new._sample_pose is None, "a loaded volume has made no call of its own"
        side.replace(on, new)
        return (len(pack),)

    def workspace(side):
        ds = side.volumes[source]
        _workspace(side, source, "pack", (ds.main, ds.excess), "vk_volume_pack_workspace_bytes", 4)

    step = Step(f"load({on} <- {source})", MUTATE, on, host, device, workspace, reads=(source,), work=lambda counts: counts[0] > 0,
                operation="load", allocates=True, source=source)
    return step


def frame(yaw_deg, on="map"):
    """three SetView rounds, a depth integration and a raycast at `yaw_deg`, as gpu_support.continue_both makes them —
    but with the volume's one Tracer, attached before the integration, so that the integrate launch prepares the raycast's
    bounds ahead as in the frame loop: ((depth, colour, normals) of the raycast, whether a SetView round dropped a request)"""
    def host(orc, volumes):
        hv = volumes[on]
        hf = R.frame_at(orc, yaw_deg)
        dropped = int(hv.counters[T.VK_CTR_DROPPED])
        for _ in range(3):
            hv.set_view(hf, orc.POLICY_MAXKEY)
        ran_dry = int(hv.counters[T.VK_CTR_DROPPED]) != dropped
        orc.integrate_depth(hv, hf)
        return tuple(image.copy() for image in orc.trace(hv, hf)[:3]), ran_dry

    def device(orc, side, want):
        api, dv = side.api, side.volumes[on]
        hf = R.frame_at(orc, yaw_deg)
        df = api.Frame(hf.depth, hf.depth_projection, hf.depth_to_world)
        if want[1]:                     # vk_volume_set_view_rounds ends its rounds with the first that drops a request (vk.h)
            for _ in range(3):
                dv.set_view(df)
        else:
            dv.set_view(df, rounds=3)
        tracer = side.tracer(on)
        api.DepthIntegrator(dv).integrate(df)
        out = api.Frame(np.zeros((R.H, R.W), np.float32), hf.depth_projection, hf.depth_to_world)
        tracer.trace(out)
        return tuple(image.cpu().numpy() for image in (out.depth, out.color, out.normals)), want[1]

    return Step(f"frame(yaw {yaw_deg:g})", FRAME, on, host, device, work=lambda want: (want[0][0] > 0).sum() > 1000,
                operation="frame", allocates=True, yaw=yaw_deg)


# ---- the steps that only read --------------------------------------------------------------------------------------------

def coloured_voxels(hv, limit):
    """global voxel coordinates [<= limit, 3] of voxels with color_weight != 0, evenly strided over the pool"""
    origin = {}
    for index in M.source_blocks(hv):
        origin.setdefault(int(hv.hash_entries["data"][index]), M.origin_of(hv, index))
    at = np.flatnonzero(hv.voxels["color_weight"] != 0)
    at = at[np.isin(at // 512, list(origin))]
    at = at[::max(1, len(at) // limit)][:limit]
    origins = np.array([origin[int(slot)] for slot in at // 512], dtype=np.int64).reshape(-1, 3)
    return 8 * origins + MP.OFFSETS[at % 512]


def raycast(yaw_deg, on="map"):
    """the raycast alone, at the pose of the frame step before, with no SetView in between: (depth, colour, normals). Behind
    color_rays and carve_rays the visible list and the bounds made ahead still stand, and the image shows what they wrote;
    behind an operation that moves blocks the list is empty, what was made ahead is void, and so is the image"""
    def host(orc, volumes):
        return tuple(image.copy() for image in orc.trace(volumes[on], R.frame_at(orc, yaw_deg))[:3])

    def device(orc, side, want):
        hf = R.frame_at(orc, yaw_deg)
        out = side.api.Frame(np.zeros((R.H, R.W), np.float32), hf.depth_projection, hf.depth_to_world)
        side.tracer(on).trace(out)
        return tuple(image.cpu().numpy() for image in (out.depth, out.color, out.normals))

    return Step(f"raycast(yaw {yaw_deg:g}, {on})", READ, None, host, device, reads=(on,), work=lambda want: (want[0] > 0).sum() > 1000,
                operation="raycast", yaw=yaw_deg)


def sample(on="map", count=2000, seed=7):
    """vk_volume_sample, with gradients, in voxels: at the centres of the first `count` observed voxels, and of `count` / 2
    voxels that hold a colour, plus a seeded jitter
    that leaves each axis alone half of the time — a map made from every fourth pixel's rays is sparse, a sample along an axis
    without an offset reads no neighbour there (vk.h), and a point that is a centre reads the voxel itself, colour included.
    The points are the host state's, so they come with the statement: (points, samples, gradients)"""
    def host(orc, volumes):
        hv = volumes[on]
        centres = np.concatenate([S.weighted_voxels(hv, count)[0], coloured_voxels(hv, count // 2)])
        rng = np.random.default_rng(seed)
        jitter = rng.uniform(-0.75, 0.75, centres.shape) * rng.integers(0, 2, centres.shape)
        points = (centres + 0.5 + jitter).astype(f32)
        samples, gradients = S.sample(hv, points, voxel_units=True)
        return points, samples, gradients

    def device(orc, side, want):
        import torch
        points = torch.as_tensor(want[0]).cuda()
        got = side.volumes[on].sample(points, gradient=True, voxel_units=True)
        return want[0], np.frombuffer(got.samples.cpu().numpy().tobytes(), dtype=T.voxel_dtype), got.gradients.cpu().numpy()

    return Step(f"sample({on})", READ, None, host, device, reads=(on,), work=lambda want: (want[1]["distance_weight"] != 0).sum() > 100,
                operation="sample")


def cast_rays(quarter, on="map"):
    """vk_volume_cast_rays of a quarter of the pixel rays, with samples and gradients: (status, t, samples, gradients)"""
    def host(orc, volumes):
        want = CR.cast(volumes[on], rays_of(orc, quarter)[0])
        return want.status, want.t, want.samples, want.gradients

    def device(orc, side, want):
        got = side.volumes[on].cast_rays(side.rays(orc, quarter, False)[0], t_max=CR.T_MAX, max_steps=CR.MAX_STEPS, gradient=True)
        return (got.status.cpu().numpy(), got.t.cpu().numpy(), np.frombuffer(got.samples.cpu().numpy().tobytes(), dtype=T.voxel_dtype),
                got.gradients.cpu().numpy())

    return Step(f"cast_rays(quarter {quarter}, {on})", READ, None, host, device, reads=(on,),
                work=lambda want: (want[0] == CR.HIT).sum() > 100, operation="cast_rays", quarter=quarter)


def extract(on="map"):
    """extract(colors=True, normals=True) over every allocated block: (points, faces, colours, normals); the statement's
    statistics ride along in the step's facts"""
    step = None

    def host(orc, volumes):
        hv = volumes[on]
        points, faces, _ = orc.extract_mesh(hv, True, True)
        statistics = {}
        colors, normals = A.extract_attributes(orc, hv, True, True, statistics)
        step.facts["statistics"] = statistics
        return points, faces, colors, normals

    def device(orc, side, want):
        mesh = side.extractor(on).extract(colors=True, normals=True)
        return mesh.host() + mesh.host_attributes()

    def workspace(side):
        side.extractor(on)

    step = Step(f"extract({on})", READ, None, host, device, workspace, reads=(on,), work=lambda want: len(want[0]) > 1000,
                operation="extract")
    return step


def register_terms(on, source, pose):
    """the per-voxel terms of vk_volume_register of `source` against `on` at `pose`: (valid, residuals, jacobians)"""
    def host(orc, volumes):
        want = RR.terms(RR.Pair(volumes[on], volumes[source]), pose, BAND)
        return want.valid, want.r, want.J

    def device(orc, side, want):
        return side.volumes[on]._register_terms_call(side.volumes[source], pose, BAND)

    def workspace(side):
        ds = side.volumes[source]
        side.volumes[on]._register_setup(ds, pose, 1, BAND)

    def class_host(orc, volumes):
        return RR.register(orc, volumes[on], volumes[source], pose, iterations=LOOP_STEPS, band=BAND)

    return Step(f"register_terms({on} <- {source})", READ, None, host, device, workspace, reads=(on, source),
                work=lambda want: want[0].sum() > 1000, class_host=class_host, operation="register", source=source, pose=pose)


def _rays_form():
    """(flags, r_min, r_max) of rays in metres, as gpu_support.form gives them"""
    return (0,) + IR.bounds(False)


def score_poses(quarter, on="map"):
    """vk_volume_score_poses of a quarter of the pixel rays at score_poses_reference.eight_poses() (the identity and
    generic() among them), with the band and the bounds of tests/test_gpu_score_poses.py: the vk_pose_score array"""
    _, r_min, r_max = _rays_form()

    def host(orc, volumes):
        rays, ranges = rays_of(orc, quarter)
        return (SP.score(RY.Map(volumes[on]), rays, ranges, SP.eight_poses(), SP.BAND, r_min, r_max, False),)

    def device(orc, side, want):
        rays, ranges = side.rays(orc, quarter, False)
        scored = side.volumes[on].score_poses(rays, ranges, SP.eight_poses(), max_abs_distance=SP.BAND, r_min=r_min, r_max=r_max)
        return (scored.host(),)

    def workspace(side):
        _workspace(side, on, "score_poses", (4800, 8), "vk_volume_score_poses_workspace_bytes", 1)

    return Step(f"score_poses(quarter {quarter}, {on})", READ, None, host, device, workspace, reads=(on,),
                work=lambda want: want[0]["residuals"].max() > 100, operation="score_poses", quarter=quarter)


def register_rays_terms(quarter, pose, on="map"):
    """the per-ray terms of vk_volume_register_rays of a quarter of the pixel rays at `pose`: (valid, residuals, jacobians)"""
    flags, r_min, r_max = _rays_form()

    def host(orc, volumes):
        rays, ranges = rays_of(orc, quarter)
        want = RY.terms(RY.Map(volumes[on]), rays, ranges, pose, RY.BAND, r_min, r_max, False)
        return want.valid, want.r, want.J

    def device(orc, side, want):
        rays, ranges = side.rays(orc, quarter, False)
        valid, residuals, jacobians = side.volumes[on]._register_rays_terms_call(rays, ranges, pose, RY.BAND, flags, r_min, r_max)
        return valid.cpu().numpy(), residuals.cpu().numpy(), jacobians.cpu().numpy()

    def workspace(side):
        side.volumes[on]._register_rays_setup(4800, pose, 1, RY.BAND, flags, r_min, r_max)

    def class_host(orc, volumes):
        rays, ranges = rays_of(orc, quarter)
        return RY.register(orc, RY.Map(volumes[on]), rays, ranges, pose, iterations=LOOP_STEPS, band=RY.BAND, r_min=r_min, r_max=r_max)

    return Step(f"register_rays_terms(quarter {quarter}, {on})", READ, None, host, device, workspace, reads=(on,),
                work=lambda want: want[0].sum() > 1000, class_host=class_host, operation="register_rays", quarter=quarter, pose=pose)


def distance_field(on, stride, max_cells, signed=False, sites=DF.OCCUPIED, most=(64, 56, 48)):
    """Volume.distance_field over distance_field_reference.grid_around of the host state's blocks, at most `most` cells an
    axis — the grid comes with the statement, as sample's points do, and is the step's facts["grid"]: (the grid's origin
    and dims [6], classes, squared cells, the distance's bits as uint32)"""
    step = None

    def host(orc, volumes):
        hv = volumes[on]
        table = RR.block_table(hv)
        origin, dims = DF.grid_around(table, stride, most)
        step.facts["grid"] = (origin, dims)
        classes, d2, distance = DF.distance_field(hv, origin, dims, stride, max_cells, site_mask=sites, signed=signed, table=table)
        return np.array(origin + dims, dtype=np.int64), classes, d2, np.ascontiguousarray(distance, dtype=f32).view(np.uint32)

    def device(orc, side, want):
        origin, dims = tuple(int(c) for c in want[0][:3]), tuple(int(c) for c in want[0][3:])
        got = side.volumes[on].distance_field(origin, dims, stride=stride, max_cells=max_cells, sites=sites, signed=signed, squared=True)
        return want[0], got.classes.cpu().numpy(), got.squared_cells.cpu().numpy(), got.distance.cpu().numpy().view(np.uint32)

    def workspace(side):
        dims = step.facts["grid"][1]
        side.volumes[on]._workspace("distance_field", tuple(dims), side.api._grid_workspace_bytes, 1)

    def work(want):
        classes, d2 = want[1], want[2]
        return all((classes == c).any() for c in (DF.UNKNOWN, DF.FREE, DF.OCCUPIED)) and ((d2 > 0) & (d2 != DF.BEYOND)).any()

    name = f"distance_field({on}, stride {stride}, {max_cells} cells{', signed' if signed else ''}{'' if sites == DF.OCCUPIED else ', sites %d' % sites})"
    step = Step(name, READ, None, host, device, workspace, reads=(on,), work=work, operation="distance_field", stride=stride,
                max_cells=max_cells, signed=signed, sites=sites)
    return step


def same(got, want):
    """is what the device returned what the statement returned, bit for bit: counts as they are, arrays as bytes"""
    if isinstance(want, (tuple, list)):
        return len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))
    if isinstance(want, np.ndarray):
        got = np.ascontiguousarray(got)
        return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == np.ascontiguousarray(want).tobytes()
    return got == want


def first_difference(got, want):
    """which part of what a step returned is not the statement's, for the message of a failing step"""
    if isinstance(want, (tuple, list)) and not all(isinstance(w, (int, np.integer)) for w in want):
        for k, (g, w) in enumerate(zip(got, want)):
            if not same(g, w):
                return f"[{k}] {first_difference(g, w)}"
    if isinstance(want, np.ndarray):
        got = np.ascontiguousarray(got)
        if got.shape != want.shape or got.dtype != want.dtype:
            return f"{got.dtype}{got.shape} for {want.dtype}{want.shape}"
        if got.size == 0:
            return "nothing"
        rows = np.flatnonzero(got.reshape(len(got), -1).view(np.uint8) != np.ascontiguousarray(want).reshape(len(want), -1).view(np.uint8))
        return f"{len(rows)} bytes differ"
    return f"{got} for {want}"


# ---- the chains ----------------------------------------------------------------------------------------------------------

class Chain:
    """`start`: {volume name: function of orc that makes its HostVolume}; `steps`: the Step records in order"""

    def __init__(self, name, start, steps):
        self.name, self.start, self.steps = name, start, steps


def checkpoint(on="map", register=None, sweep=(0, None)):
    """the read-only operations: sample, cast_rays of quarter 2 (rays the map was not made from) and of quarter 0 (rays it was
    made from), the mesh with colours and normals, the scores of quarter `sweep[0]` at the eight poses and the terms of
    vk_volume_register_rays of that quarter at `sweep[1]` (the pose the chain fused it through; None: the identity), and with
    `register` = (source, pose) the terms of vk_volume_register"""
    quarter, pose = sweep
    reads = [sample(on), cast_rays(2, on), cast_rays(0, on), extract(on), score_poses(quarter, on),
             register_rays_terms(quarter, T.Transform.identity() if pose is None else pose, on)]
    if register is not None:
        reads.append(register_terms(on, *register))
    return reads


def ray_map():
    """a map built from rays alone: fused, coloured, carved, released, fused again through a pose, merged both ways, continued
    back in calls that continue, continued by a camera and repaired, with the read-only operations at four checkpoints"""
    generic = MP.generic()
    # (one quarter alone is too sparse for a trilinear sample: no endpoint finds all eight voxels observed, and the two sweep
    # reads of the checkpoint would compare nothing. A second quarter on the same lattice gives them residuals.)
    steps = [integrate_rays(0), color_rays(0), integrate_rays(3), color_rays(3)] + checkpoint()
    steps += [carve_rays(0), carve_rays(0), carve_rays(0), carve_rays(3), carve_rays(3), carve_rays(3)]
    steps += [release_blocks("unobserved+no-surface"), integrate_rays(1, generic)]
    steps += checkpoint(sweep=(1, generic))
    steps += [color_rays(1, flags=IR.VOXEL_UNITS, band=CO.TWO_VOXELS), merge("other", "map"), merge("map", "other", generic)]
    steps += checkpoint(register=("other", generic), sweep=(1, generic))
    steps += [merge("other", "map", max_rounds=1)]                        # what the posed merge added, one round a call: it continues
    steps += [frame(12), release_blocks("repair"), raycast(12)] + checkpoint(sweep=(1, generic))
    return Chain("ray_map", {"map": lambda orc: M.fresh(orc, *LONG), "other": lambda orc: M.fresh(orc, *OTHER)}, steps)


def exhausted():
    """a pool that is exhausted when the chain begins, repaired by a release in the middle of it"""
    generic = MP.generic()
    steps = [integrate_rays(0, generic), release_blocks("all-three"), integrate_rays(0, generic), color_rays(0, generic),
             release_blocks("repair"), frame(25), raycast(25)]
    return Chain("exhausted", {"map": lambda orc: R.fused_state(orc, 509, 96)}, steps)


def pose_buffer():
    """three ray operations in a row, each with another pose argument: through generic(), with none, through another_pose()"""
    steps = [integrate_rays(0, MP.generic()), color_rays(0), carve_rays(0, another_pose())]
    return Chain("pose_buffer", {"map": lambda orc: R.fused_state(orc, *LONG)}, steps)


COARSE = (0.016, 0.08)                                     # the other lattice: voxel and truncation length in metres
MIDDLE = (0.012, 0.06)                                     # a third lattice, of `coarse`'s table sizes
MID_CUT = ((-2, -2, 9), (1, 1, 11))
FINE_CUT = ((-6, -5, 13), (5, 4, 17))                      # block boxes, inclusive, that cut a source before it is sampled
COARSE_CUT = ((-3, -3, 6), (2, 2, 8))
COARSE_SMALL = ((-1, -2, 6), (1, 0, 8))
FIT_BOX = ((0, -3, 7), (3, 0, 8))                           # resampled_exhausted: 32 blocks, each present in the dry destination
PACK_BOX = ((-4, -4, 5), (1, 3, 9))                        # the box of two_resolutions' pack, on the 16 mm lattice


def field_reads(on):
    """Volume.distance_field on three grids in a row through the volume's one cached workspace: one, one of another shape,
    the first again"""
    return [distance_field(on, 1, 16), distance_field(on, 2, 12), distance_field(on, 1, 16)]


def two_resolutions():
    """a depth-integrated 8 mm map that lives (colour from rays, carved, released), resampled into a 16 mm map that then
    lives itself (a camera, carved, released), resampled back one round a call with a plain posed merge straight behind it,
    saved and loaded into other table sizes, and the loaded map — a camera and a repair later — packed under a rule
    back into the 16 mm map; the clearance field at every stage"""
    generic, identity = MP.generic(), T.Transform.identity()
    fine, coarse, back, loaded, mid = "fine", "coarse", "back", "loaded", "mid"
    steps = [color_rays(0, flags=IR.VOXEL_UNITS, band=CO.TWO_VOXELS, on=fine), carve_rays(0, on=fine), carve_rays(0, on=fine), carve_rays(0, on=fine),
             release_blocks("unobserved+no-surface", on=fine, keep_box=FINE_CUT)]
    steps += [merge_resampled(coarse, fine, generic, 2), raycast(12, on=coarse), frame(12, on=coarse)]
    steps += checkpoint(coarse)[:5] + field_reads(coarse)
    steps += [carve_rays(0, on=coarse), distance_field(coarse, 1, 16, signed=True, sites=7), distance_field(coarse, 1, 16, signed=True, sites=DF.OCCUPIED),
              release_blocks("no-surface", on=coarse, keep_box=COARSE_CUT)]
    # two ratios into one destination from sources of one table size: the cached workspace differs in the box size K alone
    # (12 mm into 8 mm: K = 4, then 16 mm into 8 mm: K = 5, the larger one second)
    steps += [merge_resampled(mid, fine, generic, 2), release_blocks("unobserved", on=mid, keep_box=MID_CUT),
              merge_resampled(back, mid, identity, 1)]
    steps += [merge_resampled(back, coarse, identity, 1, max_rounds=1), merge(back, fine, generic)]
    steps += checkpoint(back, register=(fine, generic))
    steps += [load(loaded, coarse), frame(25, on=loaded), release_blocks("repair", on=loaded)]
    steps += checkpoint(loaded)[:5] + [distance_field(loaded, 1, 16)]
    steps += [pack_merge(coarse, loaded, box=PACK_BOX, skip_unobserved=True), raycast(12, on=coarse)]
    steps += checkpoint(coarse)[:5] + [distance_field(coarse, 2, 12)]
    start = {fine: lambda orc: M.view_state(orc, "a", *LONG), coarse: lambda orc: MR.fresh(orc, 509, 1024, *COARSE),
             back: lambda orc: M.fresh(orc, *OTHER), loaded: lambda orc: MR.fresh(orc, *OTHER, *COARSE),
             mid: lambda orc: MR.fresh(orc, 509, 1024, *MIDDLE)}
    return Chain("two_resolutions", start, steps)


def resampled_exhausted():
    """a destination whose excess list a resampled merge runs dry: it drops, nothing continues; then the repair, the pack of
    the same source cut to a box that fits, a camera, the raycast alone and the clearance field. A pack keeps its lattice
    and merge(pack) refuses another, so the 8 mm source cannot be packed into the 16 mm destination: the source, cut by a
    release, is first resampled into a roomy 16 mm volume "fit", and the pack is of that, under FIT_BOX"""
    generic = MP.generic()
    steps = [color_rays(0, on="fine"), carve_rays(0, on="fine"), release_blocks("unobserved+no-surface", on="fine"),
             merge_resampled("coarse", "fine", generic, 2), release_blocks("repair", on="coarse"),
             release_blocks("unobserved", on="fine", keep_box=FINE_CUT), merge_resampled("fit", "fine", generic, 2),
             pack_merge("coarse", "fit", box=FIT_BOX), frame(12, on="coarse"), raycast(12, on="coarse"), distance_field("coarse", 1, 16)]
    start = {"fine": lambda orc: M.view_state(orc, "a", *LONG), "coarse": lambda orc: MR.fresh(orc, 509, 16, *COARSE),
             "fit": lambda orc: MR.fresh(orc, 509, 1024, *COARSE)}
    return Chain("resampled_exhausted", start, steps)


# Six seeds whose chains have no step that does nothing (tests/test_map_life.py). A release by the "repair" rule set releases
# no block by definition, so a chain that draws it cannot pass that test and its seed is not among these: the repair alone is
# a step of ray_map and of exhausted.
SEEDS = (1, 8, 9, 12, 15, 17)
RULES = list(R.RULES)
OPERATIONS = ("integrate_rays", "color_rays", "carve_rays", "release_blocks", "merge")


def random_chain(seed):
    """eight mutating steps drawn from the seed, each followed by a frame step — and, between the two, by the raycast alone
    at the frame step before — and three reads at the end (sample, cast_rays, score_poses): integrate_rays, color_rays, carve_rays,
    release_blocks by one of the five rule sets, and the merge of view "b" (through generic() at most once a chain). The ray
    quarter, pose or no pose, metres or voxels, one observation or not and a cap of 3 or 16 are drawn with the step; the chain
    starts from the fused state or from a fresh volume. Nothing a statement refuses can be drawn: every call is a valid one."""
    rng = np.random.default_rng(1000 + seed)
    generic = MP.generic()
    fused = bool(rng.integers(0, 2))
    start = {"map": (lambda orc: R.fused_state(orc, *LONG)) if fused else (lambda orc: M.fresh(orc, *LONG)),
             "b": lambda orc: M.view_state(orc, "b", *OTHER)}
    steps, posed_merge, previous = [], False, None
    for _ in range(8):
        operation = OPERATIONS[int(rng.integers(0, len(OPERATIONS)))]
        quarter = int(rng.integers(0, 4))
        pose = generic if rng.integers(0, 2) else None
        flags = (IR.VOXEL_UNITS if rng.integers(0, 2) else 0) | (IR.ONE_OBSERVATION if rng.integers(0, 2) else 0)
        cap = float((3, 16)[int(rng.integers(0, 2))])
        rule = RULES[int(rng.integers(0, len(RULES)))]
        yaw_deg = float((0, 12, 25)[int(rng.integers(0, 3))])
        if operation == "integrate_rays":
            steps.append(integrate_rays(quarter, pose, flags, cap))
        elif operation == "color_rays":
            steps.append(color_rays(quarter, pose, flags, cap))
        elif operation == "carve_rays":
            steps.append(carve_rays(quarter, pose, flags, cap))
        elif operation == "release_blocks":
            steps.append(release_blocks(rule))
        else:
            through = pose if not posed_merge else None
            posed_merge = posed_merge or through is not None
            steps.append(merge("map", "b", through))
        if previous is not None:
            steps.append(raycast(previous))
        steps.append(frame(yaw_deg))
        previous = yaw_deg
    steps += [sample(), cast_rays(2), score_poses(2)]
    return Chain(f"random_chain({seed})", start, steps)


RESOLUTION_OPERATIONS = OPERATIONS + ("merge_resampled", "pack_merge", "load")
RESOLUTION_SEEDS = (1, 2, 12, 19, 24)
_STARTS = {}


def _resolution_start(orc, which):
    """the dense starts of random_resolution_chain, made once and handed out as copies: view "a" cut to FINE_CUT, and what
    the statement of the resampled merge makes of it on the 16 mm lattice through generic() with n = 2"""
    if "fine" not in _STARTS:
        _STARTS["fine"] = MR.cut(M.view_state(orc, "a", *LONG), FINE_CUT)
        coarse = MR.fresh(orc, 509, 1024, *COARSE)
        MR.merge(coarse, _STARTS["fine"], MP.generic(), 2)
        _STARTS["coarse"] = coarse
    return R.clone(orc, _STARTS[which])


def random_resolution_chain(seed):
    """random_chain's kind over two lattices: eight mutating steps drawn from the seed, each followed by a frame step on the
    volume it changed — and, between the two, by the raycast alone at that volume's frame step before — and four reads
    of each lattice's map at the end (sample, cast_rays, score_poses, distance_field).
    The volumes: "fine" (8 mm, view "a" cut to a box) and "coarse" (16 mm, its resampled copy), view "b" for the plain
    merge into "fine", and "loaded", fresh, for the one load a chain may draw — of the lattice of the map it will take,
    which is known when the chain is drawn; from then on the loaded map lives in the place of the one it was loaded from.
    The five old operations are drawn onto either lattice (rays in metres on the coarse one: random_chain's voxel units
    are the fine lattice's); merge_resampled runs either way, n from 1 .. 3, through generic() or the identity, 1 or 8
    rounds a call, behind a release that cuts its source to a box (facts["cut"]: the statement's cost goes with the blocks
    sampled); pack_merge takes the pack of the map of its own lattice that the chain holds besides (the loaded map
    and the one it came from) or of the map itself — a pack is a copy — under the box rule, the skip rule, both or none."""
    rng = np.random.default_rng(5000 + seed)
    generic, identity = MP.generic(), T.Transform.identity()
    now = {"fine": "fine", "coarse": "coarse"}                            # lattice: the volume that lives there
    loaded_lattice = None
    steps, posed_merge, previous = [], False, {}
    for _ in range(8):
        operation = RESOLUTION_OPERATIONS[int(rng.integers(0, len(RESOLUTION_OPERATIONS)))]
        lattice = ("fine", "coarse")[int(rng.integers(0, 2))]
        quarter = int(rng.integers(0, 4))
        pose = generic if rng.integers(0, 2) else None
        flags = (IR.VOXEL_UNITS if rng.integers(0, 2) else 0) | (IR.ONE_OBSERVATION if rng.integers(0, 2) else 0)
        cap = float((3, 16)[int(rng.integers(0, 2))])
        rule = RULES[int(rng.integers(0, len(RULES)))]
        yaw_deg = float((0, 12, 25)[int(rng.integers(0, 3))])
        supersample = int(rng.integers(1, 4))
        rounds = (1, 8)[int(rng.integers(0, 2))]
        box, skip = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        if lattice == "coarse":
            flags &= ~IR.VOXEL_UNITS
        if operation == "load" and loaded_lattice is not None:
            operation = "pack_merge"                                     # one load a chain: "loaded" is fresh once
        on = now[lattice]
        if operation == "integrate_rays":
            steps.append(integrate_rays(quarter, pose, flags, cap, on=on))
        elif operation == "color_rays":
            steps.append(color_rays(quarter, pose, flags, cap, on=on))
        elif operation == "carve_rays":
            steps.append(carve_rays(quarter, pose, flags, cap, on=on))
        elif operation == "release_blocks":
            steps.append(release_blocks(rule, on=on))
        elif operation == "merge":
            on = now["fine"]
            through = pose if not posed_merge else None
            posed_merge = posed_merge or through is not None
            steps.append(merge(on, "b", through))
        elif operation == "merge_resampled":
            source = now["coarse" if lattice == "fine" else "fine"]
            # (the statement's cost goes with the candidates times n^3: the source is cut to a box first, a small one on
            # the coarse lattice, whose every block reaches a dozen fine ones)
            cut = release_blocks("unobserved", on=source, keep_box=FINE_CUT if lattice == "coarse" else COARSE_SMALL)
            cut.facts["cut"] = True
            steps += [cut, merge_resampled(on, source, generic if pose is not None else identity, supersample, max_rounds=rounds)]
        elif operation == "pack_merge":
            source = lattice if loaded_lattice == lattice and on == "loaded" else on
            steps.append(pack_merge(on, source, box=(FINE_CUT if lattice == "fine" else PACK_BOX) if box else None, skip_unobserved=skip))
        else:
            loaded_lattice, now[lattice] = lattice, "loaded"
            steps.append(load("loaded", on))
            on = "loaded"
        if on in previous:
            steps.append(raycast(previous[on], on=on))
        steps.append(frame(yaw_deg, on=on))
        previous[on] = yaw_deg
    for lattice in ("fine", "coarse"):
        on = now[lattice]
        steps += [sample(on), cast_rays(2, on), score_poses(2, on), distance_field(on, 1 if lattice == "coarse" else 2, 12)]
    start = {"fine": lambda orc: _resolution_start(orc, "fine"), "coarse": lambda orc: _resolution_start(orc, "coarse"),
             "b": lambda orc: M.view_state(orc, "b", *OTHER)}
    if loaded_lattice is not None:
        start["loaded"] = (lambda orc: M.fresh(orc, *OTHER)) if loaded_lattice == "fine" else (lambda orc: MR.fresh(orc, *OTHER, *COARSE))
    chain = Chain(f"random_resolution_chain({seed})", start, steps)
    chain.drawn = [step for step in steps if step.kind == MUTATE and not step.facts.get("cut")]
    return chain


# ---- the host side of a chain: once, then never changed ------------------------------------------------------------------

SMALL = ("hash_entries", "free_voxel_blocks", "allocation_types", "allocation_blocks", "block_visibility", "visible_blocks", "counters")


class Snapshot:
    """a HostVolume as it stood: the small arrays as copies, of the voxels the blocks that are not as vk_volume_initialize
    leaves them (a (509, 4096) pool is 47 MB, what a chain ever writes a quarter of it)"""

    def __init__(self, orc, hv):
        self.shape = (hv.main, hv.excess, hv.voxel_length, hv.truncation_length, hv.depth_range)
        self.main, self.excess, self.max = hv.main, hv.excess, hv.max
        for name in SMALL:
            setattr(self, name, getattr(hv, name).copy())
        empty = np.zeros(512, dtype=T.voxel_dtype)
        empty["distance"] = 1
        blocks = hv.voxels.view(np.uint8).reshape(hv.max, -1)
        self.written = np.flatnonzero((blocks != empty.view(np.uint8)[None]).any(1))
        self.blocks = blocks[self.written].copy()

    def restore(self, orc):
        """a new HostVolume with these contents"""
        main, excess, voxel_length, truncation_length, depth_range = self.shape
        hv = orc.HostVolume(main, excess, voxel_length=voxel_length, truncation_length=truncation_length, depth_range=depth_range)
        for name in SMALL:
            getattr(hv, name)[:] = getattr(self, name)
        hv.voxels.view(np.uint8).reshape(hv.max, -1)[self.written] = self.blocks
        return hv

    def written_voxels(self):
        """the voxels of the written blocks, [blocks * 512]"""
        return self.blocks.reshape(-1).view(T.voxel_dtype)


class Record:
    """one step on the host: `want` (what the statement returned), `after` ({name: a Snapshot of every volume after the step;
    a volume the step did not change shares the one before}), `defined` ({name: does every counter of
    gpu_support.DEFINED_COUNTERS hold the statement's value}: a frame step leaves VK_CTR_BANDED to the device alone, the
    next operation that ends on VK_CTR_BANDED = -1 defines it again)"""


class Run:
    """`start`: {name: Snapshot of the volumes the chain starts from}, `records`: a Record per step"""


def host_run(orc, chain, keep=True, class_layer=False):
    """the chain on the host. `keep`: cached under the chain's name, for the tests that share it. `class_layer`: every record
    whose step has a class_host also gets `class_want`, that statement on the state the step found — evaluated here, once,
    from the snapshots, so a run that was cached without them takes them later"""
    run = _RUNS[chain.name] if chain.name in _RUNS else _host_run(orc, chain, keep)
    if class_layer:
        for index, record in enumerate(run.records):
            if record.step.class_host is not None and not hasattr(record, "class_want"):
                volumes = {name: before(run, index)[name].restore(orc) for name in record.step.reads}
                record.class_want = record.step.class_host(orc, volumes)
    return run


def _host_run(orc, chain, keep):
    run = Run()
    run.chain, run.orc = chain, orc
    volumes = {name: make(orc) for name, make in chain.start.items()}
    run.start = after = {name: Snapshot(orc, hv) for name, hv in volumes.items()}
    defined = {name: True for name in volumes}
    run.records = []
    for step in chain.steps:
        record = Record()
        record.step, record.want = step, step.host(orc, volumes)
        if step.kind == FRAME:
            defined[step.on] = False
        elif step.kind == MUTATE and step.facts["operation"] in ("integrate_rays", "release_blocks", "merge", "merge_resampled", "pack_merge", "load"):
            defined[step.on] = True
        if step.on is not None:
            after = dict(after)
            after[step.on] = Snapshot(orc, volumes[step.on])
        record.after, record.defined = after, dict(defined)
        run.records.append(record)
    if keep:
        _RUNS[chain.name] = run
    return run


def before(run, index):
    """{name: Snapshot of the volumes as step `index` found them}"""
    return run.start if index == 0 else run.records[index - 1].after


def slots_in_use(state):
    return set(int(s) for s in state.hash_entries["data"][state.hash_entries["data"] >= 0])


def entries_in_use(state):
    """table indices of the entries that hold a block"""
    return set(int(i) for i in np.flatnonzero(state.hash_entries["data"] >= 0))
