"""vk_volume_pack and vk_volume_merge_packed on the device against their CPU statement (tests/pack_reference.py), byte for
byte: the device starts from uploaded oracle states (merge_reference.view_state, 888 and 812 blocks), packs, and must
hold the origins, voxel bytes, counts and order the statement gives, with every byte behind what it may write left alone
and the source untouched; a destination merged from a pack must hold the hash entries, visibility bytes, free list, voxel
bytes, public counters and counts that merge_reference.merge leaves when it merges the VOLUME — then both sides go on as
in test_gpu_merge.py. Everything is bytes and integers: there is no tolerance anywhere in this file.

Every call is handed a workspace and a counts tensor that were overwritten first (`fill`: noise by default): vk.h lets
a caller hand over a workspace that is not initialised. The one thing carried is what a VK_MERGE_CONTINUE call takes over."""
import ctypes as C

import numpy as np
import pytest

from abi_support import fake_volume
import merge_reference as M
import pack_reference as P
import release_reference as R
from gpu_support import api, assert_same_state, assert_volume_equal, continue_both, device_copy, overwrite, sync  # noqa: F401
from vulcan_amd import vk_types as T

pytestmark = pytest.mark.gpu

SIZES = [(509, 4096), (4093, 2048)]
BOX = ((4, -6, 13), (10, 4, 16))        # cuts state "b" and holds some of its 26 unobserved blocks (test_pack_reference.py)
POISON = 0xA5
BLOCK_BYTES = 10240


def dirty(dv, operation, size, workspace_bytes, counts, fill="noise"):
    """the workspace and counts tensor the next `operation` of `dv` will use, created as the call will ask for them and
    overwritten"""
    workspace, held = dv._workspace(operation, size, workspace_bytes, counts)
    overwrite(workspace, fill, 1 + workspace.numel())
    overwrite(held, fill, 2)


def rule_of(flags, lo, hi):
    if not flags:
        return None
    rule = T.PackRule()
    rule.flags = flags
    rule.lo[:], rule.hi[:] = list(lo), list(hi)
    return rule


def poisoned(dv, room):
    """device arrays of a pack with room for `room` blocks, every byte the poison"""
    import torch
    origins = torch.full((room * 8,), POISON, dtype=torch.uint8, device=dv.device).view(torch.int16).view(room, 4)
    return origins, torch.full((room * BLOCK_BYTES,), POISON, dtype=torch.uint8, device=dv.device)


def pack_raw(api, dv, flags=0, lo=(0, 0, 0), hi=(0, 0, 0), capacity=0, room=0, count_only=False, fill="noise"):
    """one vk_volume_pack into poisoned arrays with room for `room` blocks, of which the call is told `capacity`:
    (origins [room, 4] int16, voxel bytes [room * 10240] uint8, the four counts), all of the arrays read back"""
    origins, voxels = poisoned(dv, room)
    dirty(dv, "pack", (dv.main, dv.excess), api.lib().vk_volume_pack_workspace_bytes, 4, fill)
    counts = dv._pack_call(rule_of(flags, lo, hi), origins, None if count_only else voxels, capacity)
    sync()
    return origins.cpu().numpy(), voxels.cpu().numpy(), counts


def assert_pack_is(got_origins, got_voxels, want_origins, want_voxels, room):
    """the first blocks are the statement's, every byte behind them is the poison"""
    written = len(want_origins)
    assert got_origins[:written].tobytes() == want_origins.tobytes()
    assert got_voxels[:written * BLOCK_BYTES].tobytes() == want_voxels.tobytes()
    assert (got_origins[written:room].view(np.uint8) == POISON).all()
    assert (got_voxels[written * BLOCK_BYTES:] == POISON).all()


def device_pack(api, dv, **rule):
    """Volume.pack with a dirty workspace"""
    dirty(dv, "pack", (dv.main, dv.excess), api.lib().vk_volume_pack_workspace_bytes, 4)
    return dv.pack(**rule)


def merge_packed_both(api, dv, pack, hv, origins, voxels, flags=0, max_rounds=8, cap_d=16.0, cap_c=16.0, workspace=None,
                      all_counters=True, fill="noise"):
    """one vk_volume_merge_packed on the device, the statement on the host: the same six counts, the same state"""
    want = P.merge_packed(hv, origins, voxels, len(origins), hv.voxel_length, hv.truncation_length, flags, max_rounds, cap_d, cap_c,
                          workspace=workspace)
    if not flags & M.CONTINUE:
        dirty(dv, "merge_packed", (pack.count,), api.lib().vk_volume_merge_packed_workspace_bytes, 6, fill)
    got = dv._merge_packed_call(pack, flags, max_rounds, cap_d, cap_c)
    print("counts", got, want)
    assert got == want
    assert_same_state(dv, hv, all_counters)
    return want


@pytest.mark.parametrize("sizes", SIZES, ids=["long-chains", "other-bucket-count"])
def test_pack_matches_the_cpu_statement(api, orc, sizes):
    """chains up to 11 deep: main entries first, then excess entries, in table order; the source is only read"""
    hs = M.view_state(orc, "b", *sizes)
    ds = device_copy(api, hs)
    want_origins, want_voxels, want = P.pack(hs)
    assert pack_raw(api, ds, count_only=True)[2] == (812, 812, 0, 0)
    origins, voxels, counts = pack_raw(api, ds, capacity=812, room=814)
    assert counts == want == (812, 812, 812, 0)
    assert_pack_is(origins, voxels, want_origins, want_voxels, 814)
    # through the class: a count call, an exact allocation, the pack call
    pack = device_pack(api, ds)
    assert len(pack) == 812 and pack.origins.shape == (812, 4) and pack.voxels.numel() == 812 * BLOCK_BYTES
    got_origins, got_voxels = pack.host()
    assert got_origins.tobytes() == want_origins.tobytes() and got_voxels.tobytes() == want_voxels.tobytes()
    assert np.float32(pack.voxel_length) == np.float32(hs.voxel_length)
    assert_same_state(ds, hs)


def test_a_count_only_call_writes_nothing(api, orc):
    hs = M.view_state(orc, "b", 509, 4096)
    ds = device_copy(api, hs)
    origins, voxels, counts = pack_raw(api, ds, capacity=812, room=812, count_only=True)      # voxels == NULL, origins given
    assert counts == (812, 812, 0, 0)
    assert_pack_is(origins, voxels, np.zeros((0, 4), np.int16), np.zeros(0, T.voxel_dtype), 812)
    assert_same_state(ds, hs)


def test_a_capacity_below_the_selection_keeps_the_first_blocks(api, orc):
    hs = M.view_state(orc, "b", 509, 4096)
    ds = device_copy(api, hs)
    want_origins, want_voxels, want = P.pack(hs, capacity=809)
    origins, voxels, counts = pack_raw(api, ds, capacity=809, room=812)
    assert counts == want == (812, 812, 809, 0)
    assert_pack_is(origins, voxels, want_origins, want_voxels, 812)
    # and capacity 0 with arrays given
    origins, voxels, counts = pack_raw(api, ds, capacity=0, room=2)
    assert counts == (812, 812, 0, 0)
    assert_pack_is(origins, voxels, want_origins[:0], want_voxels[:0], 2)


@pytest.mark.parametrize("flags", [P.BOX, P.SKIP_UNOBSERVED, P.BOX | P.SKIP_UNOBSERVED], ids=["box", "skip-unobserved", "both"])
def test_box_and_skip_unobserved(api, orc, flags):
    hs = M.view_state(orc, "b", 509, 4096)
    ds = device_copy(api, hs)
    want_origins, want_voxels, want = P.pack(hs, flags, *BOX)
    assert 0 < want[1] < 812 and (want[3] > 0) == bool(flags & P.SKIP_UNOBSERVED)
    origins, voxels, counts = pack_raw(api, ds, flags, *BOX, capacity=want[1], room=want[1] + 1)
    assert counts == want
    assert_pack_is(origins, voxels, want_origins, want_voxels, want[1] + 1)
    pack = device_pack(api, ds, box=BOX if flags & P.BOX else None, skip_unobserved=bool(flags & P.SKIP_UNOBSERVED))
    assert pack.host()[0].tobytes() == want_origins.tobytes() and pack.host()[1].tobytes() == want_voxels.tobytes()
    assert_same_state(ds, hs)


def test_a_box_without_blocks(api, orc):
    hs = M.view_state(orc, "b", 509, 4096)
    ds = device_copy(api, hs)
    origins, voxels, counts = pack_raw(api, ds, P.BOX | P.SKIP_UNOBSERVED, (100, 100, 100), (101, 101, 101), capacity=4, room=4)
    assert counts == P.pack(hs, P.BOX | P.SKIP_UNOBSERVED, (100, 100, 100), (101, 101, 101))[2] == (812, 0, 0, 0)
    assert_pack_is(origins, voxels, np.zeros((0, 4), np.int16), np.zeros(0, T.voxel_dtype), 4)
    pack = device_pack(api, ds, box=((100, 100, 100), (101, 101, 101)))
    assert len(pack) == 0 and pack.host()[0].shape == (0, 4)
    assert_same_state(ds, hs)


@pytest.mark.parametrize("sizes", [((509, 4096), (509, 4096)), ((4093, 2048), (509, 4096))], ids=["long-chains", "other-bucket-count"])
def test_merging_the_pack_is_merging_the_volume(api, orc, sizes):
    """the statement the device is held to here is merge's own, on the volume the pack was made from"""
    hv, hs = M.view_state(orc, "a", *sizes[0]), M.view_state(orc, "b", *sizes[1])
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    pack = device_pack(api, ds)
    want = M.merge(hv, hs)
    dirty(dv, "merge_packed", (pack.count,), api.lib().vk_volume_merge_packed_workspace_bytes, 6)
    got = dv._merge_packed_call(pack, 0, 8, 16.0, 16.0)
    assert got == want == (812, 812, 512, 0, 5 if sizes[0][0] == 509 else 3, 0)
    assert_same_state(dv, hv)
    assert_same_state(ds, hs)
    continue_both(api, orc, dv, hv, 12)


def test_into_a_fresh_volume_with_caps_32767(api, orc):
    hs = M.view_state(orc, "b", 509, 4096)
    hv = M.fresh(orc, 1021, 2048)
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    pack = device_pack(api, ds)
    origins, voxels = pack.host()
    assert merge_packed_both(api, dv, pack, hv, origins, voxels, cap_d=32767.0, cap_c=32767.0) == (812, 812, 812, 0, 6, 0)
    assert R.block_voxels(hv) == R.block_voxels(hs)
    # the loaded volume packs to the same set of (origin, bytes), in its own table's order
    again = device_pack(api, dv)
    assert len(again) == 812 and P.block_set(*again.host()) == P.block_set(origins, voxels) == R.block_voxels(hs)
    assert again.host()[0].tobytes() == P.pack(hv)[0].tobytes()
    continue_both(api, orc, dv, hv, 25)


def test_skip_unobserved_is_classified_from_the_packed_voxels(api, orc):
    hv, hs = M.view_state(orc, "a", 4093, 2048), M.view_state(orc, "b", 509, 4096)
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    pack = device_pack(api, ds)
    counts = merge_packed_both(api, dv, pack, hv, *pack.host(), flags=M.SKIP_UNOBSERVED)
    assert counts[5] == 26 and counts[0] == 786 and counts[3] == 0
    want = M.view_state(orc, "a", 4093, 2048)
    assert M.merge(want, hs, M.SKIP_UNOBSERVED) == counts
    assert_same_state(dv, want)


def test_two_rounds_then_a_call_that_completes(api, orc):
    """max_rounds = 2 leaves blocks out; the call that continues fuses those and only those; the class does both"""
    hv, hs = M.view_state(orc, "a", 509, 4096), M.view_state(orc, "b", 509, 4096)
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    pack = device_pack(api, ds)
    origins, voxels = pack.host()
    workspace = {}
    first = merge_packed_both(api, dv, pack, hv, origins, voxels, max_rounds=2, workspace=workspace)
    assert first[3] > 0 and first[4] == 2
    second = merge_packed_both(api, dv, pack, hv, origins, voxels, flags=M.CONTINUE, max_rounds=8, workspace=workspace)
    assert second[0] == first[3] and second[3] == 0 and first[1] + second[1] == 812
    whole = M.view_state(orc, "a", 509, 4096)
    assert M.merge(whole, hs) == (812, 812, 512, 0, first[4] + second[4], 0)
    assert_same_state(dv, whole)                           # the state of one call, on the volume, with all the rounds
    dv2 = device_copy(api, M.view_state(orc, "a", 509, 4096))
    assert dv2.merge(pack, max_rounds=2) == (812, 812, 512, 0, 5, 0)
    assert_same_state(dv2, whole)
    continue_both(api, orc, dv2, whole, 12)


def test_exhausted_destination(api, orc):
    """the excess list, then the pool run dry in the second round: upstream's leaked slots and never-written entries included"""
    hs = M.view_state(orc, "a", 509, 4096)
    hv = M.fresh(orc, 509, 64)
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    pack = device_pack(api, ds)
    origins, voxels = pack.host()
    assert merge_packed_both(api, dv, pack, hv, origins, voxels) == (888, 457, 457, 431, 2, 0)
    assert hv.counters[T.VK_CTR_DROPPED] == 185
    whole = M.fresh(orc, 509, 64)
    assert M.merge(whole, hs) == (888, 457, 457, 431, 2, 0)
    assert_same_state(dv, whole)
    # the class does not go on after a drop
    dv2 = device_copy(api, M.fresh(orc, 509, 64))
    assert dv2.merge(pack) == (888, 457, 457, 431, 2, 0)
    assert_same_state(dv2, hv)
    # and a destination that is exhausted when the call begins
    hw, hb = M.view_state(orc, "a", 509, 64), M.view_state(orc, "b", 509, 4096)
    dw, db = device_copy(api, hw), device_copy(api, hb)
    pack_b = device_pack(api, db)
    counts = merge_packed_both(api, dw, pack_b, hw, *pack_b.host())
    assert counts[2] == 0 and counts[3] > 0 and counts[4] == 1
    continue_both(api, orc, dv, hv, 25)


def test_neither_call_depends_on_what_its_workspace_held(api, orc):
    """the same two calls from workspaces of 0xFF bytes: the statement's results again"""
    hv, hs = M.view_state(orc, "a", 509, 4096), M.view_state(orc, "b", 509, 4096)
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    want_origins, want_voxels, want = P.pack(hs, P.SKIP_UNOBSERVED)
    origins, voxels, counts = pack_raw(api, ds, P.SKIP_UNOBSERVED, capacity=786, room=787, fill="ones")
    assert counts == want
    assert_pack_is(origins, voxels, want_origins, want_voxels, 787)
    pack = device_pack(api, ds)
    merge_packed_both(api, dv, pack, hv, *pack.host(), flags=M.SKIP_UNOBSERVED, fill="ones")


def test_three_blocks_at_the_int16_edges_in_a_table_of_seven(api, orc):
    """a hand-made host state: blocks (0,0,0), (-32768,-32768,-32768) and (32767,32767,32767) in a (7, 5) table — the empty
    main entries (origin 0, data -1) do not stand in for block 0, the edges survive the trip, and 3 is no multiple of 4"""
    rng = np.random.default_rng(7)
    origins = np.array([[0, 0, 0, 0], [-32768, -32768, -32768, 0], [32767, 32767, 32767, 0]], dtype=np.int16)
    voxels = np.zeros(3 * 512, dtype=T.voxel_dtype)
    voxels["distance"] = rng.uniform(-1, 1, 3 * 512).astype(np.float32)
    voxels["color"] = rng.random((3 * 512, 3), dtype=np.float32)
    voxels["distance_weight"] = rng.integers(1, 9, 3 * 512)
    voxels["color_weight"] = rng.integers(1, 9, 3 * 512)
    hs = M.fresh(orc, 7, 5)
    assert P.merge_packed(hs, origins, voxels, 3, hs.voxel_length, hs.truncation_length, cap_d=32767.0, cap_c=32767.0)[:4] == (3, 3, 3, 0)
    assert R.block_voxels(hs) == P.block_set(origins, voxels)
    assert (hs.hash_entries["data"][:7] == -1).sum() >= 4
    ds = device_copy(api, hs)
    want_origins, want_voxels, want = P.pack(hs)
    got_origins, got_voxels, counts = pack_raw(api, ds, capacity=3, room=5)
    assert counts == want == (3, 3, 3, 0)
    assert_pack_is(got_origins, got_voxels, want_origins, want_voxels, 5)
    assert {tuple(o) for o in got_origins[:3]} == {tuple(o) for o in origins}
    pack = device_pack(api, ds)
    hv = M.fresh(orc, 7, 5)
    dv = device_copy(api, hv)
    assert merge_packed_both(api, dv, pack, hv, want_origins, want_voxels, cap_d=32767.0, cap_c=32767.0)[:4] == (3, 3, 3, 0)
    assert R.block_voxels(hv) == P.block_set(origins, voxels)
    assert device_pack(api, dv).host()[0].tobytes() == P.pack(hv)[0].tobytes()


def test_no_blocks(api, orc):
    """block_count == 0, and an empty volume: zero counts, no byte of a table or a pool changes"""
    hv, hs = M.view_state(orc, "a", 509, 4096), M.fresh(orc, 61, 7)
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    origins, voxels, counts = pack_raw(api, ds, capacity=2, room=2)
    assert counts == P.pack(hs)[2] == (0, 0, 0, 0)
    assert_pack_is(origins, voxels, np.zeros((0, 4), np.int16), np.zeros(0, T.voxel_dtype), 2)
    assert len(device_pack(api, ds)) == 0
    assert_same_state(ds, hs)
    # block_count == 0 of a pack that has room: what merging the empty volume leaves
    room = api.PackedVolume(*poisoned(dv, 2), hv.voxel_length, hv.truncation_length)
    before = dv.host_voxels().tobytes(), dv.host_entries().tobytes()
    dirty(dv, "merge_packed", (0,), api.lib().vk_volume_merge_packed_workspace_bytes, 6)
    workspace, counts = dv._workspace("merge_packed", (0,), api.lib().vk_volume_merge_packed_workspace_bytes, 6)
    params = T.MergeParams(0, 8, 16.0, 16.0)
    assert api.lib().vk_volume_merge_packed(C.byref(dv.desc()), C.byref(room.desc()), 0, room.voxel_length, room.truncation_length,
                                            C.byref(params), C.c_void_p(counts.data_ptr()), C.c_void_p(workspace.data_ptr()), api.stream()) == 0
    sync()
    assert tuple(counts.cpu().numpy()) == M.merge(hv, hs) == (0, 0, 0, 0, 0, 0)
    assert (dv.host_voxels().tobytes(), dv.host_entries().tobytes()) == before
    assert_same_state(dv, hv)
    # the class makes no call for a pack without blocks
    assert dv.merge(device_pack(api, ds)) == (0, 0, 0, 0, 0, 0)


def test_abi_validates_before_touching_a_device(api):
    lib = api.lib()
    one = C.c_void_p(16)
    v = fake_volume(1 << 20)

    def a_pack(capacity=4, origins=3 << 20, voxels=4 << 20):
        pack = T.BlockPack()
        pack.capacity, pack.origins, pack.voxels = capacity, origins, voxels
        return pack

    # ---- vk_volume_pack
    def pack_call(volume=v, rule=None, pack=None, counts=one, workspace=one):
        pack = a_pack() if pack is None else pack
        return lib.vk_volume_pack(C.byref(volume), C.byref(rule) if rule is not None else None, C.byref(pack), counts, workspace, None)

    assert lib.vk_volume_pack(None, None, None, None, None, None) == -1
    assert lib.vk_volume_pack(C.byref(v), None, None, one, one, None) == -1
    assert pack_call(counts=None) == -1 and pack_call(workspace=None) == -1
    other = fake_volume(1 << 20)
    other.hash_entries = None
    assert pack_call(volume=other) == -1
    other = fake_volume(1 << 20)
    other.main_block_count = 0
    assert pack_call(volume=other) == -1
    other = fake_volume(1 << 20)
    other.excess_block_count = -1
    assert pack_call(volume=other) == -1
    other = fake_volume(1 << 20)
    other.voxels += 8                                                             # not 16-byte aligned
    assert pack_call(volume=other) == -1
    assert pack_call(pack=a_pack(voxels=(4 << 20) + 8)) == -1
    assert pack_call(pack=a_pack(origins=(3 << 20) + 2)) == -1
    assert pack_call(pack=a_pack(origins=None)) == -1
    assert pack_call(pack=a_pack(capacity=-1)) == -1
    assert pack_call(pack=a_pack(capacity=-1, voxels=None)) == -1
    assert pack_call(rule=rule_of(4, (0, 0, 0), (0, 0, 0))) == -1                 # an unknown flag
    assert pack_call(rule=rule_of(P.BOX | 8, (0, 0, 0), (0, 0, 0))) == -1
    for axis in range(3):
        lo = [0, 0, 0]
        lo[axis] = 1
        assert pack_call(rule=rule_of(P.BOX, lo, (0, 0, 0))) == -1                # lo > hi
    assert lib.vk_volume_pack_workspace_bytes(0, 0) == 0
    assert lib.vk_volume_pack_workspace_bytes(8, -1) == 0
    assert lib.vk_volume_pack_workspace_bytes(509, 96) >= 605 * 12
    assert C.sizeof(T.BlockPack) == 24 and C.sizeof(T.PackRule) == 16

    # ---- vk_volume_merge_packed
    good = T.MergeParams(0, 8, 16.0, 16.0)

    def merge_call(dst=v, pack=None, count=4, voxel_length=0.008, truncation_length=0.04, params=good, counts=one, workspace=one):
        pack = a_pack() if pack is None else pack
        return lib.vk_volume_merge_packed(C.byref(dst), C.byref(pack), count, voxel_length, truncation_length,
                                          C.byref(params) if params is not None else None, counts, workspace, None)

    assert lib.vk_volume_merge_packed(None, None, 0, 0.008, 0.04, None, None, None, None) == -1
    assert lib.vk_volume_merge_packed(C.byref(v), None, 0, 0.008, 0.04, C.byref(good), one, one, None) == -1
    assert merge_call(params=None) == -1 and merge_call(counts=None) == -1 and merge_call(workspace=None) == -1
    for params in (T.MergeParams(4, 8, 16.0, 16.0), T.MergeParams(0, 0, 16.0, 16.0), T.MergeParams(0, 8, 0.5, 16.0),
                   T.MergeParams(0, 8, 16.0, 32768.0), T.MergeParams(0, 8, float("nan"), 16.0)):
        assert merge_call(params=params) == -1
    assert merge_call(voxel_length=0.005) == -1 and merge_call(truncation_length=0.05) == -1
    assert merge_call(count=-1) == -1 and merge_call(count=5) == -1                # outside 0 .. capacity
    assert merge_call(count=0, pack=a_pack(capacity=-1)) == -1
    assert merge_call(pack=a_pack(origins=None)) == -1 and merge_call(pack=a_pack(voxels=None)) == -1
    assert merge_call(pack=a_pack(voxels=(4 << 20) + 8)) == -1 and merge_call(pack=a_pack(origins=(3 << 20) + 4)) == -1
    assert merge_call(pack=a_pack(voxels=v.voxels)) == -1                          # into itself
    other = fake_volume(1 << 20)
    other.voxels += 8
    assert merge_call(dst=other) == -1
    other = fake_volume(1 << 20)
    other.counters = None
    assert merge_call(dst=other) == -1
    assert lib.vk_volume_merge_packed_workspace_bytes(-1) == 0
    assert lib.vk_volume_merge_packed_workspace_bytes(0) > 0
    assert lib.vk_volume_merge_packed_workspace_bytes(605) >= 605 * 5


def test_the_python_surface(api, orc, tmp_path):
    """pack -> save -> load -> merge; what the classes refuse"""
    hs = M.view_state(orc, "b", 509, 4096)
    ds = device_copy(api, hs)
    pack = ds.pack()
    path = str(tmp_path / "b.map")
    pack.save(path)
    origins, voxels, _ = P.pack(hs)
    from vulcan_amd import io
    assert io.read_map(path)[0].tobytes() == origins.tobytes() and io.read_map(path)[1].tobytes() == voxels.tobytes()
    loaded = api.PackedVolume.load(path)
    assert len(loaded) == 812 and loaded.host()[1].tobytes() == voxels.tobytes()
    assert loaded.to("cpu").voxels.device.type == "cpu" and loaded.to("cpu").to("cuda").host()[0].tobytes() == origins.tobytes()
    # Volume.load: a fresh volume of other table sizes that holds the map
    volume = api.Volume.load(path, 1021, 2048)
    sync()
    hv = M.fresh(orc, 1021, 2048)
    assert M.merge(hv, hs, cap_d=32767.0, cap_c=32767.0)[:4] == (812, 812, 812, 0)
    assert_same_state(volume, hv)
    with pytest.raises(api.VkError):
        api.Volume.load(path, 509, 64)                                          # the blocks do not fit
    # merge(pack) into a volume that has a history, as merge(volume)
    ha = M.view_state(orc, "a", 509, 4096)
    da = device_copy(api, ha)
    assert da.merge(loaded) == M.merge(ha, hs) == (812, 812, 512, 0, 5, 0)
    assert_same_state(da, ha)
    # refusals
    with pytest.raises(TypeError):
        da.merge(loaded, pose=np.eye(4))
    other = api.Volume(509, 64, voxel_length=0.005, truncation_length=hs.truncation_length)
    with pytest.raises(api.VkError):
        other.merge(loaded)
    other = api.Volume(509, 64, voxel_length=hs.voxel_length, truncation_length=0.05)
    with pytest.raises(api.VkError):
        other.merge(loaded)
    with pytest.raises(api.VkError):
        ds.pack(box=((1, 0, 0), (0, 0, 0)))
    with pytest.raises(ValueError):
        open(path, "ab").write(b"\0")
        api.PackedVolume.load(path)


def test_merge_of_a_pack_is_refused_while_a_frame_is_announced_and_pack_is_not(api, orc):
    hv, hs = M.view_state(orc, "a", 509, 4096), M.view_state(orc, "b", 509, 4096)
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    pack = ds.pack()
    hf = R.frame_at(orc, 25)
    df = api.Frame(hf.depth, hf.depth_projection, hf.depth_to_world)
    dv.set_view(df, rounds=3)
    out = api.Frame(np.zeros((R.H, R.W), np.float32), hf.depth_projection, hf.depth_to_world)
    nf = R.frame_at(orc, 12)
    api.Tracer(dv).trace(out, next_frame=api.Frame(nf.depth, nf.depth_projection, nf.depth_to_world))
    sync()
    assert dv.requests_ahead is not None and dv.requests_ahead.valid == 1
    before = (dv.host_entries(), dv.host_voxels().tobytes(), dv.read_counters(), dv.host_allocation_types())
    with pytest.raises(api.VkError):
        dv.merge(pack)
    # pack only reads: allowed, and it leaves the announced frame's requests where they are
    held = dv.pack()
    sync()
    after = (dv.host_entries(), dv.host_voxels().tobytes(), dv.read_counters(), dv.host_allocation_types())
    for a, b in zip(before, after):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    assert dv.requests_ahead.valid == 1
    entries, pool = dv.host_entries(), dv.host_voxels()
    origins, voxels = held.host()
    assert len(held) == int((entries["data"] >= 0).sum()) > 888
    index = np.nonzero(entries["data"] >= 0)[0]
    assert origins[:, :3].tobytes() == entries["block"]["origin"][index].tobytes()
    assert all(voxels[512 * k:512 * (k + 1)].tobytes() == pool[512 * s:512 * (s + 1)].tobytes()
               for k, s in enumerate(entries["data"][index]))
    dv.cancel_requests_ahead(rounds=3)
    assert dv.merge(pack)[3] == 0
