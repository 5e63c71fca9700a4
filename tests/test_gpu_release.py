"""vk_volume_release_blocks on the device against its CPU statement (tests/release_reference.py) and the oracle, bit for bit:
the device starts from an uploaded oracle state, makes the call, and must hold the same hash entries, visibility bytes, free
list, voxel bytes, public counters and counts as the helper leaves on the host; then both sides go on — three SetView calls,
a depth integration and a raycast at another pose — and must still agree, images included. Every decision of the call
compares stored values, so there is no tolerance anywhere in this file."""
import ctypes as C

import numpy as np
import pytest

import release_reference as R
from gpu_support import api, assert_same_state, assert_volume_equal, continue_both, device_copy, sync  # noqa: F401
from release_reference import RULES, helper_arguments
from vulcan_amd import vk_types as T

pytestmark = pytest.mark.gpu


def release_both(dv, hv, rule, all_counters=True):
    want = R.release_blocks(hv, *helper_arguments(rule))
    got = dv.release_blocks(**rule)
    print("counts", got, want)
    assert got == want
    assert_same_state(dv, hv, all_counters)
    return want


@pytest.mark.parametrize("rule", list(RULES))
def test_release_matches_the_cpu_statement(api, orc, rule):
    """chains 0 to 11 deep, the wave's decision over 512 AoS voxels, the clear of the released blocks"""
    hv = R.fused_state(orc, 509, 4096)
    dv = device_copy(api, hv)
    counts = release_both(dv, hv, RULES[rule])
    expected = {"repair": (0, 1398, 940, 3207), "unobserved": (52, 1346, 889, 3259), "no-surface": (209, 1189, 743, 3416),
                "unobserved+no-surface": (261, 1137, 696, 3468)}
    if rule in expected:
        assert counts == expected[rule]
    else:
        assert counts[0] > 261 and counts[1] > 0
    continue_both(api, orc, dv, hv, 25)
    continue_both(api, orc, dv, hv, 12)


def test_more_buckets_than_one_scan_trip(api, orc):
    """16 411 main buckets: the ordered scan over the buckets makes three trips of 8 192"""
    hv = R.fused_state(orc, 16411, 4096)
    assert int(hv.counters[T.VK_CTR_EXCESS_PTR]) > hv.main             # and chains exist beyond the first trip
    assert (hv.hash_entries["next"][8192:hv.main] >= 0).any()
    dv = device_copy(api, hv)
    counts = release_both(dv, hv, RULES["unobserved+no-surface"])
    assert counts[0] > 0 and counts[2] > 0
    continue_both(api, orc, dv, hv, 25)


def test_exhausted_volume_recovers(api, orc):
    """negative VK_CTR_VOXEL_PTR, VK_CTR_EXCESS_PTR past the end of the table, leaked slots"""
    hv = R.fused_state(orc, 509, 96)
    assert hv.counters[T.VK_CTR_VOXEL_PTR] == -4070 and hv.counters[T.VK_CTR_EXCESS_PTR] == 4270
    dv = device_copy(api, hv)
    assert release_both(dv, hv, RULES["all-three"]) == (218, 271, 30, 334)
    continue_both(api, orc, dv, hv, 25)
    assert int((hv.hash_entries["data"] >= 0).sum()) == 509


def test_ghost_entries_go(api, orc):
    """data = -1 inside a chain (what volume.cu:344 links when the pool is empty)"""
    hv, bucket, ghost, slot, behind = R.ghost_state(orc)
    dv = device_copy(api, hv)
    assert release_both(dv, hv, RULES["repair"]) == (0, 1397, 939, 3208)
    assert slot in set(int(s) for s in dv.free_voxel_blocks.cpu().numpy()[:3208])
    continue_both(api, orc, dv, hv, 25)


@pytest.mark.parametrize("rule", ["repair", "all-three"])
def test_fresh_volume_stays_as_initialised(api, orc, rule):
    """an empty table: the state is vk_volume_initialize's (all slots free: there is no -1 tail)"""
    dv = api.Volume(1021, 510)
    fresh = api.Volume(1021, 510)
    hv = orc.HostVolume(1021, 510)
    assert dv.release_blocks(**RULES[rule]) == R.release_blocks(hv, *helper_arguments(RULES[rule])) == (0, 0, 0, 1531)
    assert_same_state(dv, hv, all_counters=False)
    for name in ("hash_entries", "block_visibility", "free_voxel_blocks", "voxels", "allocation_types"):
        assert np.array_equal(getattr(dv, name).cpu().numpy(), getattr(fresh, name).cpu().numpy()), name
    got, want = dv.read_counters(), fresh.read_counters()
    want[T.VK_CTR_BANDED] = -1
    assert np.array_equal(got, want)


def test_the_same_call_again_changes_nothing(api, orc):
    hv = R.fused_state(orc, 509, 4096)
    dv = device_copy(api, hv)
    first = release_both(dv, hv, RULES["all-three"])
    again = release_both(dv, hv, RULES["all-three"])
    assert again == (0,) + first[1:]
    snapshot = R.clone(orc, hv)
    assert dv.release_blocks() == (0,) + first[1:]               # and a repair on top
    assert_same_state(dv, snapshot)


def test_refused_while_a_frame_is_announced_then_allowed(api, orc):
    hv = R.fused_state(orc, 509, 4096)
    dv = device_copy(api, hv)
    hf = R.frame_at(orc, 25)
    df = api.Frame(hf.depth, hf.depth_projection, hf.depth_to_world)
    dv.set_view(df, rounds=3)
    tracer = api.Tracer(dv)
    out = api.Frame(np.zeros((R.H, R.W), np.float32), hf.depth_projection, hf.depth_to_world)
    nf = R.frame_at(orc, 12)
    next_frame = api.Frame(nf.depth, nf.depth_projection, nf.depth_to_world)
    tracer.trace(out, next_frame=next_frame)
    sync()
    assert dv.requests_ahead is not None and dv.requests_ahead.valid == 1
    before = (dv.host_entries(), dv.host_visibility(), dv.free_voxel_blocks.cpu().numpy(), dv.host_voxels().tobytes(),
              dv.read_counters())
    with pytest.raises(api.VkError):
        dv.release_blocks(unobserved=True)
    sync()
    after = (dv.host_entries(), dv.host_visibility(), dv.free_voxel_blocks.cpu().numpy(), dv.host_voxels().tobytes(),
             dv.read_counters())
    assert dv.requests_ahead.valid == 1
    for a, b in zip(before, after):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    # the way out: complete the announced frame's SetView, then release
    dv.cancel_requests_ahead(rounds=3)
    assert dv.requests_ahead.valid == 0
    for hframe in (hf, nf):
        for _ in range(3):
            hv.set_view(hframe, orc.POLICY_MAXKEY)
    assert_volume_equal(dv, hv)
    release_both(dv, hv, RULES["unobserved+no-surface"], all_counters=False)
    continue_both(api, orc, dv, hv, 12)


def test_abi_validates_before_touching_a_device(api):
    lib = api.lib()
    one = C.c_void_p(16)
    assert lib.vk_volume_release_blocks(None, None, None, None, None) == -1
    v, rule = T.Volume(), T.ReleaseRule()
    assert lib.vk_volume_release_blocks(C.byref(v), None, one, one, None) == -1
    assert lib.vk_volume_release_blocks(C.byref(v), C.byref(rule), one, one, None) == -1      # no buffers, no buckets
    for name in ("voxels", "hash_entries", "free_voxel_blocks", "block_visibility", "counters"):
        setattr(v, name, 16)
    assert lib.vk_volume_release_blocks(C.byref(v), C.byref(rule), one, one, None) == -1      # main_block_count 0
    v.main_block_count = 8
    rule.flags = 8
    assert lib.vk_volume_release_blocks(C.byref(v), C.byref(rule), one, one, None) == -1      # an unknown rule
    rule.flags = 0
    assert lib.vk_volume_release_blocks(C.byref(v), C.byref(rule), None, one, None) == -1
    assert lib.vk_volume_release_blocks(C.byref(v), C.byref(rule), one, None, None) == -1
    assert lib.vk_volume_release_workspace_bytes(0, 0) == 0
    assert lib.vk_volume_release_workspace_bytes(8, -1) == 0
    assert lib.vk_volume_release_workspace_bytes(509, 96) >= 605 * (16 + 3) + 3 * 4 * 509
    assert C.sizeof(T.ReleaseRule) == 20
    assert (T.VK_RELEASE_UNOBSERVED, T.VK_RELEASE_NO_SURFACE, T.VK_RELEASE_OUTSIDE_BOX) == (1, 2, 4)
