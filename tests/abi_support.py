"""What the "validates before touching a device" tests of the volume entry points share."""
from vulcan_amd import vk_types as T


def fake_volume(base=1 << 20):
    """a T.Volume of plausible sizes whose buffers are distinct addresses from `base` on that are no memory: an entry point
    given it has to return its error code before it reads or launches anything"""
    v = T.Volume()
    for k, name in enumerate(("voxels", "hash_entries", "free_voxel_blocks", "allocation_types", "allocation_blocks",
                              "block_visibility", "visible_blocks", "counters")):
        setattr(v, name, base + 4096 * k)
    v.main_block_count, v.excess_block_count, v.voxel_length, v.truncation_length = 8, 8, 0.008, 0.04
    return v
