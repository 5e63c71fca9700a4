"""The CPU statement of vk_volume_merge (include/vk.h): which blocks of a source volume a call allocates in the destination,
and the state of the destination's hash table, visibility bytes, pool, counters and voxels afterwards — in numpy, on two
oracle.HostVolume. The device is held to it bit for bit (tests/test_gpu_merge.py); there is no upstream counterpart (its
Volume is a process-wide singleton, src/volume.cu:17-21), so this file is the definition.

The allocation compares stored values only and goes through the oracle's handle pass; the fusion is the integrators'
running average (src/depth_integrator.cu:55-59, src/color_integrator.cu:109-118) with the source voxel's weight in place
of 1, in float32 with one rounding per operation: numpy's float32 arithmetic is exactly that, so no tolerance exists."""
import numpy as np

import release_reference as R
from vulcan_amd import vk_types as T

SKIP_UNOBSERVED, CONTINUE = 1, 2
P1, P2, P3 = 73856093, 19349669, 83492791


def bucket_of(origin, main):
    bx, by, bz = origin
    return (((bx * P1) & 0xFFFFFFFF) ^ ((by * P2) & 0xFFFFFFFF) ^ ((bz * P3) & 0xFFFFFFFF)) % main


def request_key(kind, origin):
    """oracle_volume.c:64-68"""
    bx, by, bz = origin
    return (kind << 48) | ((bz & 0xFFFF) << 32) | ((by & 0xFFFF) << 16) | (bx & 0xFFFF)


def origin_of(hv, index):
    return tuple(int(c) for c in hv.hash_entries["block"]["origin"][index])


def source_blocks(src):
    """entry indices of the source blocks: reachable from a main bucket along `next`, data >= 0"""
    out = []
    for bucket in range(src.main):
        for index in R.chain(src.hash_entries, bucket, src.max):
            if src.hash_entries["data"][index] >= 0:
                out.append(index)
    return out


def unobserved(src, index):
    slot = int(src.hash_entries["data"][index])
    voxels = src.voxels[slot * 512:(slot + 1) * 512]
    return not (voxels["distance_weight"] != 0).any() and not (voxels["color_weight"] != 0).any()


def fuse_block(dst, dst_slot, src, src_slot, cap_d, cap_c):
    f32 = np.float32
    d = dst.voxels[dst_slot * 512:(dst_slot + 1) * 512]               # a view: written in place
    s = src.voxels[src_slot * 512:(src_slot + 1) * 512]
    with np.errstate(invalid="ignore", divide="ignore"):
        take = s["distance_weight"] != 0
        wd, ws = d["distance_weight"].astype(f32), s["distance_weight"].astype(f32)
        total = wd + ws
        mean = (wd * d["distance"] + ws * s["distance"]) / total
        d["distance"] = np.where(take, np.where(wd == 0, s["distance"], mean), d["distance"])
        d["distance_weight"] = np.where(take, np.minimum(f32(cap_d), total).astype(np.int16), d["distance_weight"])

        take = s["color_weight"] != 0
        wd, ws = d["color_weight"].astype(f32), s["color_weight"].astype(f32)
        total = wd + ws
        mean = (wd[:, None] * d["color"] + ws[:, None] * s["color"]) / total[:, None]
        d["color"] = np.where(take[:, None], np.where((wd == 0)[:, None], s["color"], mean), d["color"])
        d["color_weight"] = np.where(take, np.minimum(f32(cap_c), total).astype(np.int16), d["color_weight"])


def merge(dst, src, flags=0, max_rounds=8, cap_d=16.0, cap_c=16.0, workspace=None):
    """Mutates `dst` as the call is defined; returns the six counts (considered, fused, allocated, left out, rounds that
    posted, skipped as unobserved). `workspace`: a dict standing for the device workspace — the call leaves the entries
    it left out there, and with CONTINUE those are what it considers."""
    assert max_rounds >= 1 and 1 <= cap_d <= 32767 and 1 <= cap_c <= 32767
    assert np.float32(dst.voxel_length) == np.float32(src.voxel_length)
    assert np.float32(dst.truncation_length) == np.float32(src.truncation_length)
    skipped = 0
    if flags & CONTINUE:
        considered = list(workspace["left_out"])
    else:
        considered = source_blocks(src)
        if flags & SKIP_UNOBSERVED:
            observed = [i for i in considered if not unobserved(src, i)]
            skipped = len(considered) - len(observed)
            considered = observed
    origins = {i: origin_of(src, i) for i in considered}

    present_before = sum(1 for i in considered if R.find(dst, origins[i]) >= 0)
    rounds = 0
    for _ in range(max_rounds):
        winners = {}
        for i in considered:
            if R.find(dst, origins[i]) >= 0:
                continue
            bucket = bucket_of(origins[i], dst.main)
            kind = T.ALLOC_MAIN if dst.hash_entries["data"][bucket] == -1 else T.ALLOC_EXCESS
            key = request_key(kind, origins[i])
            if bucket not in winners or key > winners[bucket][0]:
                winners[bucket] = (key, kind, origins[i])
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

    fused, left_out = 0, []
    for i in considered:
        slot = R.find(dst, origins[i])
        if slot < 0:
            left_out.append(i)
            continue
        fuse_block(dst, slot, src, int(src.hash_entries["data"][i]), cap_d, cap_c)
        fused += 1
    if workspace is not None:
        workspace["left_out"] = left_out
    dst.counters[T.VK_CTR_VISIBLE] = 0
    dst.counters[T.VK_CTR_BANDED] = -1
    return len(considered), fused, fused - present_before, len(left_out), rounds, skipped


# ---- the states the CPU and the GPU tests start from ---------------------------------------------------------------

W, H = R.W, R.H
VOXEL, TRUNCATION = R.VOXEL, R.TRUNCATION
VIEWS = {"a": (0, 2, 11), "b": (25, 3, 12)}        # yaw in degrees, frames fused, seed of the colour images
_STATES = {}


def frame_at(orc, yaw_deg, color=None):
    import scenes
    return orc.HostFrame(scenes.ripple(W, H), R.projection(), scenes.yaw(yaw_deg), color=color)


def view_state(orc, which, main, excess):
    """release_reference's 160x120 ripple frame at one yaw, fused `frames` times — eight SetView calls, a depth and a
    colour integration per frame, each frame with its own seeded random colour image — in HostVolume(main, excess):
    computed once per view and size, handed out as copies."""
    key = (which, main, excess)
    if key not in _STATES:
        yaw_deg, frames, seed = VIEWS[which]
        rng = np.random.default_rng(seed)
        hv = orc.HostVolume(main, excess, voxel_length=VOXEL, truncation_length=TRUNCATION)
        for k in range(frames):
            frame = frame_at(orc, yaw_deg, color=rng.random((H, W, 3), dtype=np.float32))
            for _ in range(8):
                hv.set_view(frame, orc.POLICY_MAXKEY)
            orc.integrate_depth(hv, frame)
            orc.integrate_color(hv, frame)
        _STATES[key] = hv
    return R.clone(orc, _STATES[key])


def fresh(orc, main, excess):
    return orc.HostVolume(main, excess, voxel_length=VOXEL, truncation_length=TRUNCATION)
