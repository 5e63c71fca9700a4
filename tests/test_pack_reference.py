"""The definitions of vk_volume_pack and vk_volume_merge_packed (include/vk.h; tests/pack_reference.py states them in
numpy) held against merge's statement and the oracle's states: a pack made without a rule, merged, leaves what merging
the volume leaves — entries, visibility, free list, voxels, counters and counts; the pack's order is the table's; box and
skip-unobserved select what their definitions say; and the map file (vulcan_amd/io.py) keeps every byte and refuses
every malformed file. The states are merge_reference.view_state's: 888 blocks ("a") and 812 ("b")."""
import numpy as np
import pytest

import merge_reference as M
import pack_reference as P
import release_reference as R
from vulcan_amd import io, vk_types as T

SIZES = [(509, 4096), (4093, 2048)]
BOX = ((4, -6, 13), (10, 4, 16))         # in block coordinates: cuts state "b" and holds some of its 26 unobserved blocks
STATE = ("voxels", "hash_entries", "free_voxel_blocks", "allocation_types", "allocation_blocks", "block_visibility",
         "visible_blocks", "counters")


def same_state(a, b):
    for name in STATE:
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name


@pytest.mark.parametrize("sizes", SIZES)
def test_merging_the_pack_is_merging_the_volume(orc, sizes):
    hv, hs = M.view_state(orc, "a", *sizes), M.view_state(orc, "b", *sizes)
    origins, voxels, counts = P.pack(hs)
    assert counts == (812, 812, 812, 0)
    want = M.merge(hv, hs)
    got_volume = M.view_state(orc, "a", *sizes)
    got = P.merge_packed(got_volume, origins, voxels, 812, hs.voxel_length, hs.truncation_length)
    assert got == want == (812, 812, 512, 0, want[4], 0)
    same_state(got_volume, hv)
    # in two calls, the second continuing the first: the same state again
    split, workspace = M.view_state(orc, "a", *sizes), {}
    first = P.merge_packed(split, origins, voxels, 812, hs.voxel_length, hs.truncation_length, max_rounds=2, workspace=workspace)
    second = P.merge_packed(split, origins, voxels, 812, hs.voxel_length, hs.truncation_length, flags=M.CONTINUE, workspace=workspace)
    assert first[3] > 0 and second[0] == first[3] and second[3] == 0 and first[4] + second[4] == want[4]
    same_state(split, hv)
    # with SKIP_UNOBSERVED the packed voxels are classified as the source's are
    a, b = M.view_state(orc, "a", *sizes), M.view_state(orc, "a", *sizes)
    assert (P.merge_packed(a, origins, voxels, 812, hs.voxel_length, hs.truncation_length, flags=M.SKIP_UNOBSERVED) ==
            M.merge(b, hs, M.SKIP_UNOBSERVED))
    same_state(a, b)
    # a prefix of the pack is a pack: only its blocks arrive
    part = M.fresh(orc, 1021, 2048)
    assert P.merge_packed(part, origins, voxels, 100, hs.voxel_length, hs.truncation_length, cap_d=32767.0, cap_c=32767.0)[:4] == (100, 100, 100, 0)
    assert R.block_voxels(part) == P.block_set(origins[:100], voxels[:51200])


@pytest.mark.parametrize("sizes", SIZES)
def test_the_order_is_the_tables(orc, sizes):
    hs = M.view_state(orc, "b", *sizes)
    before = {name: getattr(hs, name).tobytes() for name in STATE}
    origins, voxels, counts = P.pack(hs)
    chosen, source, skipped = P.select(hs)
    assert chosen == sorted(chosen) and len(set(chosen)) == 812 and (source, skipped) == (812, 0)
    assert any(i >= hs.main for i in chosen) and any(i < hs.main for i in chosen)          # main entries first, then excess
    for k, index in enumerate(chosen):
        entry = hs.hash_entries[index]
        assert tuple(origins[k]) == tuple(entry["block"]["origin"]) + (0,)
        slot = int(entry["data"])
        assert voxels[512 * k:512 * (k + 1)].tobytes() == hs.voxels[512 * slot:512 * (slot + 1)].tobytes()
    assert P.block_set(origins, voxels) == R.block_voxels(hs)
    assert all(getattr(hs, name).tobytes() == before[name] for name in STATE)               # only read
    # a capacity below the selection keeps the first blocks of that order; a count-only call writes nothing
    o2, v2, c2 = P.pack(hs, capacity=809)
    assert c2 == (812, 812, 809, 0) and o2.tobytes() == origins[:809].tobytes() and v2.tobytes() == voxels[:809 * 512].tobytes()
    assert P.pack(hs, count_only=True)[2] == (812, 812, 0, 0)
    # an empty main entry holds origin (0, 0, 0) and data -1: it is no block
    assert P.pack(M.fresh(orc, 61, 7))[2] == (0, 0, 0, 0)


def test_box_and_skip_unobserved_select_by_their_definitions(orc):
    hs = M.view_state(orc, "b", 509, 4096)
    blocks = R.block_voxels(hs)
    lo, hi = BOX
    in_box = {o for o in blocks if all(lo[a] <= o[a] <= hi[a] for a in range(3))}
    observed = {o for o, b in blocks.items() if np.frombuffer(b, dtype=T.voxel_dtype)["distance_weight"].any() or
                np.frombuffer(b, dtype=T.voxel_dtype)["color_weight"].any()}
    assert 0 < len(in_box) < 812 and len(observed) == 812 - 26 and 0 < len(in_box - observed) < len(in_box)
    origins, voxels, counts = P.pack(hs, P.BOX, lo, hi)
    assert set(P.block_set(origins, voxels)) == in_box and counts == (812, len(in_box), len(in_box), 0)
    origins, voxels, counts = P.pack(hs, P.SKIP_UNOBSERVED)
    assert set(P.block_set(origins, voxels)) == observed and counts == (812, 786, 786, 26)
    origins, voxels, counts = P.pack(hs, P.BOX | P.SKIP_UNOBSERVED, lo, hi)
    assert set(P.block_set(origins, voxels)) == in_box & observed
    assert counts == (812, len(in_box & observed), len(in_box & observed), len(in_box - observed))   # skipped: of the box's
    assert all(P.block_set(origins, voxels)[o] == blocks[o] for o in in_box & observed)
    # a box that holds no block; and lo and hi are inclusive
    assert P.pack(hs, P.BOX, (100, 100, 100), (101, 101, 101))[2] == (812, 0, 0, 0)
    one = next(iter(in_box))
    assert P.pack(hs, P.BOX, one, one)[2] == (812, 1, 1, 0)


def test_the_file_keeps_every_byte_and_refuses_what_is_malformed(orc, tmp_path):
    hs = M.view_state(orc, "b", 509, 4096)
    origins, voxels, _ = P.pack(hs)
    path = str(tmp_path / "b.map")
    io.write_map(path, origins, voxels, hs.voxel_length, hs.truncation_length)
    data = open(path, "rb").read()
    assert len(data) == 32 + 812 * (8 + 10240)
    assert data[:8] == io.MAP_MAGIC and data[8:16] == np.array([1, 812], "<i4").tobytes() and data[24:32] == bytes(8)
    assert data[16:24] == np.array([hs.voxel_length, hs.truncation_length], "<f4").tobytes()
    assert data[32:32 + 812 * 8] == origins.tobytes() and data[32 + 812 * 8:] == voxels.tobytes()
    got_origins, got_voxels, voxel_length, truncation_length = io.read_map(path)
    assert got_origins.tobytes() == origins.tobytes() and got_voxels.tobytes() == voxels.tobytes()
    assert voxel_length == np.float32(hs.voxel_length) and truncation_length == np.float32(hs.truncation_length)
    # written again it is the same file
    again = str(tmp_path / "again.map")
    io.write_map(again, got_origins, got_voxels, voxel_length, truncation_length)
    assert open(again, "rb").read() == data
    # a map without blocks
    io.write_map(again, np.zeros((0, 4), np.int16), np.zeros(0, T.voxel_dtype), 0.008, 0.04)
    assert len(open(again, "rb").read()) == 32 and len(io.read_map(again)[0]) == 0

    def refused(changed, what):
        bad = str(tmp_path / "bad.map")
        with open(bad, "wb") as fh:
            fh.write(changed)
        with pytest.raises(ValueError, match=what):
            io.read_map(bad)

    small = data[:32 + 3 * 8] + data[32 + 812 * 8:32 + 812 * 8 + 3 * 10240]          # the first three blocks
    small = small[:12] + np.array([3], "<i4").tobytes() + small[16:]
    assert len(io.read_map(_written(tmp_path, small))[0]) == 3
    refused(b"VULCANMQ" + small[8:], "magic")
    refused(small[:8] + np.array([2], "<i4").tobytes() + small[12:], "version")
    refused(small[:12] + np.array([-1], "<i4").tobytes() + small[16:], "count")
    refused(small[:-1], "bytes")
    refused(small + b"\0", "bytes")
    refused(small[:12] + np.array([4], "<i4").tobytes() + small[16:], "bytes")
    refused(small[:10], "magic")                                                       # shorter than a header
    refused(small[:32 + 6] + b"\1\0" + small[32 + 8:], "fourth")
    refused(small[:32 + 8] + small[32:32 + 8] + small[32 + 16:], "same origin")
    with pytest.raises(ValueError):
        io.write_map(str(tmp_path / "bad.map"), origins[:3], voxels[:1000], 0.008, 0.04)


def _written(tmp_path, content):
    path = str(tmp_path / "good.map")
    with open(path, "wb") as fh:
        fh.write(content)
    return path
