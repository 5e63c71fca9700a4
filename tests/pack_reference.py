"""The CPU statement of vk_volume_pack and vk_volume_merge_packed (include/vk.h), in numpy, on merge_reference's host
states (oracle.HostVolume). The device is held to it byte for byte (tests/test_gpu_pack.py); there is no upstream
counterpart (its Volume is a process-wide singleton, src/volume.cu:17-21), so this file is the definition.

pack: the source blocks are merge's (merge_reference.source_blocks); one is selected unless the box excludes its origin
or — of those the box leaves — nobody observed it (merge_reference.unobserved); the selected blocks in ascending order of
their table entry index, each as its origin (x, y, z, 0) and the 512 voxels of its pool slot.

merge_packed: vk.h defines it as vk_volume_merge with "the considered source blocks" replaced by packed blocks
0 .. count-1. PackAsSource is that sentence: a stand-in for the source volume in which packed block k is entry k of a table
of `count` main buckets, each its own chain, with pool slot k — so merge_reference.merge, unchanged, considers exactly the
packed blocks, in pack order, and no arithmetic is stated twice.

Nothing is computed here that merge does not compute; there is no tolerance."""
import numpy as np

import merge_reference as M
from vulcan_amd import vk_types as T

SKIP_UNOBSERVED, BOX = 1, 2          # vk_pack_rule.flags


def inside(origin, lo, hi):
    return all(int(lo[a]) <= origin[a] <= int(hi[a]) for a in range(3))


def select(src, flags=0, lo=(0, 0, 0), hi=(0, 0, 0)):
    """(entry indices of the selected blocks in pack order, source blocks, blocks skipped as unobserved)"""
    assert flags & ~(SKIP_UNOBSERVED | BOX) == 0 and all(lo[a] <= hi[a] for a in range(3))
    source = sorted(M.source_blocks(src))
    left = [i for i in source if not (flags & BOX) or inside(M.origin_of(src, i), lo, hi)]
    chosen = [i for i in left if not (flags & SKIP_UNOBSERVED) or not M.unobserved(src, i)]
    return chosen, len(source), len(left) - len(chosen)


def pack(src, flags=0, lo=(0, 0, 0), hi=(0, 0, 0), capacity=None, count_only=False):
    """(origins [written, 4] int16, voxels [512 * written] voxel_dtype, (source blocks, selected, written, skipped as
    unobserved)). `capacity` None: room for all; `count_only`: voxels == NULL, nothing is written."""
    chosen, source, skipped = select(src, flags, lo, hi)
    written = 0 if count_only else len(chosen) if capacity is None else min(len(chosen), capacity)
    origins = np.zeros((written, 4), dtype=np.int16)
    voxels = np.zeros(512 * written, dtype=T.voxel_dtype)
    for k, index in enumerate(chosen[:written]):
        origins[k, :3] = M.origin_of(src, index)
        slot = int(src.hash_entries["data"][index])
        voxels[512 * k:512 * (k + 1)] = src.voxels[512 * slot:512 * (slot + 1)]
    return origins, voxels, (source, len(chosen), written, skipped)


class PackAsSource:
    """packed blocks 0 .. count-1 in the place of a source volume's considered blocks (see the module's docstring)"""

    def __init__(self, origins, voxels, count, voxel_length, truncation_length):
        origins = np.asarray(origins, dtype=np.int16).reshape(-1, 4)
        assert 0 <= count <= len(origins) and len(voxels) >= 512 * count
        assert not origins[:count, 3].any() and len({tuple(o) for o in origins[:count]}) == count    # the caller's duty
        self.main, self.excess, self.max = count, 0, count
        self.hash_entries = np.zeros(count, dtype=T.hash_entry_dtype)
        self.hash_entries["block"]["origin"] = origins[:count, :3]
        self.hash_entries["data"] = np.arange(count)
        self.hash_entries["next"] = -1
        self.voxels = voxels
        self.voxel_length, self.truncation_length = voxel_length, truncation_length


def merge_packed(dst, origins, voxels, count, voxel_length, truncation_length, flags=0, max_rounds=8, cap_d=16.0, cap_c=16.0,
                 workspace=None):
    """Mutates `dst` as the call is defined; returns merge's six counts. `workspace` as merge_reference.merge's."""
    return M.merge(dst, PackAsSource(origins, voxels, count, voxel_length, truncation_length), flags, max_rounds, cap_d, cap_c,
                   workspace=workspace)


def block_set(origins, voxels):
    """{origin: the 512 voxels' bytes} of a pack: what release_reference.block_voxels gives of a volume"""
    return {tuple(int(c) for c in origins[k, :3]): voxels[512 * k:512 * (k + 1)].tobytes() for k in range(len(origins))}
