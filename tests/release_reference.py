"""The CPU statement of vk_volume_release_blocks (include/vk.h): which blocks a call releases and the state of the
hash table, the visibility bytes, the pool and the voxels afterwards — in numpy, on an oracle.HostVolume. The device
is held to it bit for bit (tests/test_gpu_release.py); there is no upstream counterpart (src/volume.cu:304-368 never
returns a slot), so this file is the definition.

Every decision compares stored values; nothing is computed, so no tolerance exists."""
import numpy as np

from vulcan_amd import vk_types as T

UNOBSERVED, NO_SURFACE, OUTSIDE_BOX = 1, 2, 4

# the rule sets the tests and the chains (tests/map_life.py) release by, as the keywords of api.Volume.release_blocks
BOX = ((-10, -8, 14), (2, 7, 16))
RULES = {
    "repair": {},
    "unobserved": {"unobserved": True},
    "no-surface": {"min_abs_distance": 0.75},
    "unobserved+no-surface": {"unobserved": True, "min_abs_distance": 0.75},
    "all-three": {"unobserved": True, "min_abs_distance": 0.75, "keep_box": BOX},
}


def helper_arguments(rule):
    """release_blocks' arguments behind `hv` for a rule set of RULES"""
    flags = ((UNOBSERVED if rule.get("unobserved") else 0) | (NO_SURFACE if "min_abs_distance" in rule else 0) |
             (OUTSIDE_BOX if "keep_box" in rule else 0))
    lo, hi = rule.get("keep_box", ((0, 0, 0), (0, 0, 0)))
    return flags, rule.get("min_abs_distance", 0.0), lo, hi


def chain(entries, bucket, limit):
    """entry indices of main bucket `bucket`'s chain, entry `bucket` first (a `next` outside the table ends it)"""
    out, index = [], bucket
    while 0 <= index < limit and len(out) < limit:
        out.append(index)
        index = int(entries["next"][index])
    return out


def released(hv, entry, flags, min_abs_distance, keep_lo, keep_hi):
    """does an enabled rule hold for the block of `entry` (data >= 0)"""
    if flags & OUTSIDE_BOX:
        origin = entry["block"]["origin"]
        if any(int(origin[a]) < int(keep_lo[a]) or int(origin[a]) > int(keep_hi[a]) for a in range(3)):
            return True
    if flags & (UNOBSERVED | NO_SURFACE):
        slot = int(entry["data"])
        voxels = hv.voxels[slot * 512:(slot + 1) * 512]
        observed = voxels["distance_weight"] != 0
        if flags & UNOBSERVED and not observed.any():
            return True
        if flags & NO_SURFACE and observed.any():
            near = np.abs(voxels["distance"][observed]) < np.float32(min_abs_distance)       # fabsf(d) < t, in float
            if not near.any():
                return True
    return False


def release_blocks(hv, flags=0, min_abs_distance=0.0, keep_lo=(0, 0, 0), keep_hi=(0, 0, 0)):
    """Mutates `hv` as the call is defined; returns (blocks released, blocks kept, excess entries in use, free slots)."""
    main, total = hv.main, hv.max
    old = hv.hash_entries.copy()
    old_visibility = hv.block_visibility.copy()

    default = np.zeros(1, dtype=T.hash_entry_dtype)[0]
    default["data"], default["next"] = -1, -1
    hv.hash_entries[:] = default
    hv.block_visibility[:] = T.VISIBILITY_FALSE

    empty = np.zeros(1, dtype=T.voxel_dtype)[0]
    empty["distance"] = 1.0

    used = np.zeros(total, dtype=bool)
    n_released = n_kept = 0
    excess_at = main
    for bucket in range(main):
        survivors = []
        for index in chain(old, bucket, total):
            entry = old[index]
            if entry["data"] < 0:
                continue                                   # a ghost (volume.cu:344), or the empty main entry
            if released(hv, entry, flags, min_abs_distance, keep_lo, keep_hi):
                slot = int(entry["data"])
                hv.voxels[slot * 512:(slot + 1) * 512] = empty
                n_released += 1
            else:
                survivors.append(index)
        where = [bucket] + list(range(excess_at, excess_at + len(survivors) - 1))
        excess_at += max(len(survivors) - 1, 0)
        for k, index in enumerate(survivors):
            entry = old[index].copy()
            entry["next"] = where[k + 1] if k + 1 < len(survivors) else -1
            hv.hash_entries[where[k]] = entry
            hv.block_visibility[where[k]] = old_visibility[index]
            used[int(entry["data"])] = True
        n_kept += len(survivors)

    free = np.nonzero(~used)[0].astype(np.int32)
    hv.free_voxel_blocks[:] = -1
    hv.free_voxel_blocks[:len(free)] = free
    hv.counters[T.VK_CTR_EXCESS_PTR] = excess_at
    hv.counters[T.VK_CTR_VOXEL_PTR] = len(free) - 1
    hv.counters[T.VK_CTR_VISIBLE] = 0
    hv.counters[T.VK_CTR_BANDED] = -1
    return n_released, n_kept, excess_at - main, len(free)


# ---- the states the CPU and the GPU tests start from ---------------------------------------------------------------

W, H = 160, 120
VOXEL, TRUNCATION = 0.008, 0.04
_STATES = {}


def projection():
    return T.Projection.make(136, 136, 80, 60)


def frame_at(orc, yaw_deg):
    import scenes
    return orc.HostFrame(scenes.ripple(W, H), projection(), scenes.yaw(yaw_deg))


def clone(orc, hv):
    out = orc.HostVolume(hv.main, hv.excess, voxel_length=hv.voxel_length, truncation_length=hv.truncation_length,
                         depth_range=hv.depth_range)
    for name in ("voxels", "hash_entries", "free_voxel_blocks", "allocation_types", "allocation_blocks", "block_visibility",
                 "visible_blocks", "counters"):
        getattr(out, name)[:] = getattr(hv, name)
    return out


def fused_state(orc, main, excess):
    """160x120 ripple frames at yaw 0 and 25 degrees, eight SetView calls and one depth integration each, in
    HostVolume(main, excess): computed once per size, handed out as copies."""
    key = (main, excess)
    if key not in _STATES:
        hv = orc.HostVolume(main, excess, voxel_length=VOXEL, truncation_length=TRUNCATION)
        for yaw_deg in (0, 25):
            frame = frame_at(orc, yaw_deg)
            for _ in range(8):
                hv.set_view(frame, orc.POLICY_MAXKEY)
            orc.integrate_depth(hv, frame)
        _STATES[key] = hv
    return clone(orc, _STATES[key])


def ghost_state(orc):
    """fused_state(509, 4096) with one mid-chain excess entry turned into what volume.cu:344 leaves when the pool is
    empty: linked, never written. Returns (volume, bucket, index of the ghost, its former slot, origins behind it)."""
    hv = fused_state(orc, 509, 4096)
    for bucket in range(hv.main):
        links = chain(hv.hash_entries, bucket, hv.max)
        if len(links) >= 4:
            ghost = links[2]
            slot = int(hv.hash_entries["data"][ghost])
            behind = [tuple(int(c) for c in hv.hash_entries["block"]["origin"][i]) for i in links[3:]]
            hv.hash_entries["data"][ghost] = -1
            hv.hash_entries["block"]["origin"][ghost] = 0
            return hv, bucket, ghost, slot, behind
    raise AssertionError("no chain of four entries")


def continue_at(orc, hv, yaw_deg, rounds=3):
    """three SetView calls, one depth integration and a raycast at `yaw_deg`: (depth, colour, normals) of the raycast"""
    frame = frame_at(orc, yaw_deg)
    for _ in range(rounds):
        hv.set_view(frame, orc.POLICY_MAXKEY)
    orc.integrate_depth(hv, frame)
    return orc.trace(hv, frame)[:3]


def find(hv, origin):
    """pool slot of the block at `origin` by the chain walk of volume.cu:183-190, -1 when absent"""
    P1, P2, P3 = 73856093, 19349669, 83492791
    bx, by, bz = origin
    bucket = (((bx * P1) & 0xFFFFFFFF) ^ ((by * P2) & 0xFFFFFFFF) ^ ((bz * P3) & 0xFFFFFFFF)) % hv.main
    for index in chain(hv.hash_entries, bucket, hv.max):
        entry = hv.hash_entries[index]
        if entry["data"] >= 0 and tuple(int(c) for c in entry["block"]["origin"]) == tuple(origin):
            return int(entry["data"])
    return -1


def block_voxels(hv):
    """{block origin: the 512 voxels' bytes} over the blocks reachable from a main bucket"""
    out = {}
    for bucket in range(hv.main):
        for index in chain(hv.hash_entries, bucket, hv.max):
            entry = hv.hash_entries[index]
            if entry["data"] >= 0:
                slot = int(entry["data"])
                out[tuple(int(c) for c in entry["block"]["origin"])] = hv.voxels[slot * 512:(slot + 1) * 512].tobytes()
    return out
