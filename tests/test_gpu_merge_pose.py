"""vk_volume_merge_posed on the device against its CPU statement (tests/merge_pose_reference.py), bit for bit: both volumes
start from uploaded oracle states, the device makes the call, and the destination must hold the same hash entries,
visibility bytes, free list, voxel bytes, public counters and the eight counts as the statement leaves on the host, the
source what it held before. Which blocks are candidates is decided by fp32 values whose operation order is fixed, the
allocation compares stored values and the fusion is one defined sequence of float32 operations, so there is no tolerance
anywhere in this file."""
import ctypes as C

import numpy as np
import pytest

from abi_support import fake_volume
import merge_pose_reference as MP
import merge_reference as M
import release_reference as R
from gpu_support import api, assert_same_state, assert_volume_equal, continue_both, device_copy, sync  # noqa: F401
from vulcan_amd import vk_types as T

pytestmark = pytest.mark.gpu


def merge_both(dv, ds, hv, hs, pose, flags=0, max_rounds=8, cap_d=16.0, cap_c=16.0, workspace=None):
    """one call of the entry point on the device, the statement on the host: the same eight counts, the same state"""
    want = MP.merge(hv, hs, pose, flags, max_rounds, cap_d, cap_c, workspace=workspace)
    got = dv._merge_posed_call(ds, pose, flags, max_rounds, cap_d, cap_c)
    print("counts", got, want)
    assert got == want
    assert_same_state(dv, hv)
    assert_same_state(ds, hs)                              # the source is only read
    return want


@pytest.mark.parametrize("sizes", [((509, 4096), (509, 4096)), ((4093, 2048), (509, 4096))], ids=["long-chains", "other-bucket-count"])
def test_a_generic_pose_matches_the_cpu_statement(api, orc, sizes):
    hv, hs = M.view_state(orc, "a", *sizes[0]), M.view_state(orc, "b", *sizes[1])
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    counts = merge_both(dv, ds, hv, hs, MP.generic())
    assert counts[0] == 812 and counts[1] > 812 and counts[3] > 0 and counts[4] == 0 and counts[7] > 100000
    if sizes[0][0] == 509:
        continue_both(api, orc, dv, hv, 12)                # the merged volume goes on


def test_identity_is_the_plain_merge_on_the_device_too(api, orc):
    hv, hs = M.view_state(orc, "a", 509, 4096), M.view_state(orc, "b", 509, 4096)
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    plain = device_copy(api, hv)
    counts = merge_both(dv, ds, hv, hs, T.Transform.identity())
    assert counts[:7] == (812, 812, 812, 512, 0, 5, 0)
    assert plain.merge(ds) == (812, 812, 512, 0, 5, 0)
    assert_same_state(plain, hv)
    assert plain.host_voxels().tobytes() == dv.host_voxels().tobytes()
    # and through the class, from a 4x4 array
    dv2 = device_copy(api, M.view_state(orc, "a", 509, 4096))
    assert dv2.merge(ds, pose=np.eye(4)) == counts
    assert_same_state(dv2, hv)


@pytest.mark.parametrize("pose", ["quarter-turn", "block-shift"])
def test_lattice_preserving_poses(api, orc, pose):
    hv, hs = M.view_state(orc, "a", 509, 4096), M.view_state(orc, "b", 509, 4096)
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    counts = merge_both(dv, ds, hv, hs, MP.quarter_turn((3, -1, 2)) if pose == "quarter-turn" else MP.shift((8, -16, 0)))
    assert counts[:3] == (812, 812, 812) and counts[4] == 0 and counts[7] == 249718      # every voxel with a weight, once


def test_caps_of_four(api, orc):
    hv, hs = M.view_state(orc, "a", 509, 4096), M.view_state(orc, "b", 509, 4096)
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    merge_both(dv, ds, hv, hs, MP.generic(), cap_d=4.0, cap_c=4.0)
    assert int(hv.voxels["distance_weight"].max()) == 4 and int(hv.voxels["color_weight"].max()) == 4


def test_skip_unobserved(api, orc):
    hs = M.view_state(orc, "b", 509, 4096)
    hv = M.view_state(orc, "a", 4093, 2048)
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    counts = merge_both(dv, ds, hv, hs, MP.generic(), flags=MP.SKIP_UNOBSERVED)
    assert counts[6] == 26 and counts[0] == 786 and counts[4] == 0
    dv2 = device_copy(api, M.view_state(orc, "a", 4093, 2048))
    assert dv2.merge(ds, pose=MP.generic(), skip_unobserved=True) == counts
    assert_same_state(dv2, hv)


def test_two_rounds_then_a_call_that_completes(api, orc):
    """max_rounds = 2 leaves candidates out; the call that continues fuses those and only those; the class does both"""
    pose = MP.generic()
    hv, hs = M.view_state(orc, "a", 509, 4096), M.view_state(orc, "b", 509, 4096)
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    workspace = {}
    first = merge_both(dv, ds, hv, hs, pose, max_rounds=2, workspace=workspace)
    assert first[4] > 0 and first[5] == 2
    second = merge_both(dv, ds, hv, hs, pose, flags=MP.CONTINUE, max_rounds=8, workspace=workspace)
    assert second[0] == first[0] and second[1] == first[4] and second[4] == 0 and first[2] + second[2] == first[1]
    whole = M.view_state(orc, "a", 509, 4096)
    want = MP.merge(whole, hs, pose)
    assert want == (first[0], first[1], first[1], first[3] + second[3], 0, first[5] + second[5], 0, first[7] + second[7])
    assert_same_state(dv, whole)                           # the state of one call with all the rounds
    dv2 = device_copy(api, M.view_state(orc, "a", 509, 4096))
    assert dv2.merge(ds, pose=pose, max_rounds=2) == want
    assert_same_state(dv2, whole)


def test_exhausted_destination(api, orc):
    """the excess list, then the pool run dry: candidates stay absent and each is counted once"""
    hs = M.view_state(orc, "a", 509, 4096)
    hv = M.fresh(orc, 509, 64)
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    counts = merge_both(dv, ds, hv, hs, MP.generic())
    assert counts[4] > 0 and counts[2] + counts[4] == counts[1] and counts[3] == counts[2]
    assert hv.counters[T.VK_CTR_DROPPED] > 0
    # the class does not go on after a drop
    dv2 = device_copy(api, M.fresh(orc, 509, 64))
    assert dv2.merge(ds, pose=MP.generic()) == counts
    assert_same_state(dv2, hv)


def test_candidates_beyond_the_block_range_are_none(api, orc):
    """a translation of 32 760 blocks along x: the candidates whose x would pass 32 767 do not exist, the others are fused"""
    pose = T.Transform.translate(float(np.float32(32760 * 8) * np.float32(M.VOXEL)), 0.0, 0.0) * MP.generic()
    hs = M.view_state(orc, "b", 509, 4096)
    hv = M.fresh(orc, 4093, 2048)
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    counts = merge_both(dv, ds, hv, hs, pose)
    inside = MP.merge(M.fresh(orc, 4093, 2048), hs, MP.generic())
    print(counts, inside)
    assert 0 < counts[1] < inside[1] and counts[4] == 0 and counts[7] > 0
    origins = dv.host_entries()["block"]["origin"][dv.host_entries()["data"] >= 0]
    assert int(origins[:, 0].max()) == 32767


def test_refused_while_a_frame_is_announced(api, orc):
    hv, hs = M.view_state(orc, "a", 509, 4096), M.view_state(orc, "b", 509, 4096)
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    hf = R.frame_at(orc, 25)
    df = api.Frame(hf.depth, hf.depth_projection, hf.depth_to_world)
    dv.set_view(df, rounds=3)
    out = api.Frame(np.zeros((R.H, R.W), np.float32), hf.depth_projection, hf.depth_to_world)
    nf = R.frame_at(orc, 12)
    api.Tracer(dv).trace(out, next_frame=api.Frame(nf.depth, nf.depth_projection, nf.depth_to_world))
    sync()
    assert dv.requests_ahead is not None and dv.requests_ahead.valid == 1
    before = (dv.host_entries(), dv.host_voxels().tobytes(), dv.read_counters(), ds.host_voxels().tobytes())
    pose = MP.generic()
    with pytest.raises(api.VkError):
        dv.merge(ds, pose=pose)
    with pytest.raises(api.VkError):
        ds.merge(dv, pose=pose)
    with pytest.raises(api.VkError):
        ds.merge(ds, pose=pose)                             # and never into itself
    sync()
    after = (dv.host_entries(), dv.host_voxels().tobytes(), dv.read_counters(), ds.host_voxels().tobytes())
    for a, b in zip(before, after):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    dv.cancel_requests_ahead(rounds=3)
    assert dv.merge(ds, pose=pose)[4] == 0


def test_abi_validates_before_touching_a_device(api):
    lib = api.lib()
    one = C.c_void_p(16)

    def call(dst, src, params, counts=one, workspace=one):
        return lib.vk_volume_merge_posed(C.byref(dst), C.byref(src), C.byref(params), counts, workspace, None)

    def params(pose=None, merge=None):
        return T.MergePoseParams(merge or T.MergeParams(0, 8, 16.0, 16.0), pose or T.Transform.identity())

    dst, src = fake_volume(1 << 20), fake_volume(2 << 20)
    assert call(dst, src, params(), counts=None) == -1
    assert call(dst, src, params(), workspace=None) == -1
    assert call(dst, dst, params()) == -1                                         # into itself
    for at in (0, 5, 10, 12, 14):                                                 # rows 0-2 of m and of inv
        for bad in (float("nan"), float("inf")):
            pose = T.Transform.identity()
            pose.m[at] = bad
            assert call(dst, src, params(pose)) == -1
            pose = T.Transform.identity()
            pose.inv[at] = bad
            assert call(dst, src, params(pose)) == -1
    for merge in (T.MergeParams(4, 8, 16.0, 16.0), T.MergeParams(0, 0, 16.0, 16.0), T.MergeParams(0, 8, 0.5, 16.0),
                  T.MergeParams(0, 8, 16.0, float("nan"))):
        assert call(dst, src, params(merge=merge)) == -1
    other = fake_volume(2 << 20)
    other.voxel_length = 0.005
    assert call(dst, other, params()) == -1
    other = fake_volume(2 << 20)
    other.truncation_length = 0.05
    assert call(dst, other, params()) == -1
    other = fake_volume(2 << 20)
    other.voxels += 8                                                             # not 16-byte aligned
    assert call(dst, other, params()) == -1
