"""vk_volume_merge on the device against its CPU statement (tests/merge_reference.py) and the oracle, bit for bit: both
volumes start from uploaded oracle states, the device makes the call, and the destination must hold the same hash entries,
visibility bytes, free list, voxel bytes, public counters and counts as the statement leaves on the host, the source what
it held before; then both sides go on — three SetView calls, a depth integration and a raycast at another pose — and must
still agree, images and mesh included. The allocation compares stored values and the fusion is one defined sequence of
float32 operations, so there is no tolerance anywhere in this file."""
import ctypes as C

import numpy as np
import pytest

from abi_support import fake_volume
import merge_reference as M
import release_reference as R
from gpu_support import api, assert_same_state, assert_volume_equal, continue_both, device_copy, sync  # noqa: F401
from vulcan_amd import vk_types as T

pytestmark = pytest.mark.gpu


def merge_both(dv, ds, hv, hs, flags=0, max_rounds=8, cap_d=16.0, cap_c=16.0, workspace=None, all_counters=True):
    """one call of the entry point on the device, the statement on the host: the same six counts, the same state"""
    want = M.merge(hv, hs, flags, max_rounds, cap_d, cap_c, workspace=workspace)
    got = dv._merge_call(ds, flags, max_rounds, cap_d, cap_c)
    print("counts", got, want)
    assert got == want
    assert_same_state(dv, hv, all_counters)
    assert_same_state(ds, hs, all_counters)               # the source is only read
    return want


@pytest.mark.parametrize("sizes", [((509, 4096), (509, 4096)), ((4093, 2048), (509, 4096))], ids=["long-chains", "other-bucket-count"])
def test_merge_matches_the_cpu_statement(api, orc, sizes):
    """chains up to 11 deep and five rounds; a destination whose buckets are not the source's; then both sides go on"""
    hv, hs = M.view_state(orc, "a", *sizes[0]), M.view_state(orc, "b", *sizes[1])
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    counts = merge_both(dv, ds, hv, hs)
    assert counts == (812, 812, 512, 0, 5 if sizes[0][0] == 509 else 3, 0)
    continue_both(api, orc, dv, hv, 12)
    # the mesh of the merged volume
    points, faces, _ = orc.extract_mesh(hv, True, True)
    ex = api.Extractor(dv)
    ex.all_allocated = True
    got_points, got_faces = ex.extract().host()
    assert len(points) > 10000
    assert np.array_equal(got_points, points) and np.array_equal(got_faces, faces)


def test_the_other_direction_gives_the_same_map(api, orc):
    """B <- A on the device holds, per block origin, the bytes A <- B holds"""
    ha, hb = M.view_state(orc, "a", 509, 4096), M.view_state(orc, "b", 509, 4096)
    da, db = device_copy(api, ha), device_copy(api, hb)
    assert db.merge(da) == (888, 888, 588, 0, 6, 0)
    M.merge(ha, M.view_state(orc, "b", 509, 4096))
    sync()
    hb.hash_entries[:] = db.host_entries()
    hb.voxels[:] = db.host_voxels()
    assert R.block_voxels(hb) == R.block_voxels(ha)


def test_into_a_fresh_volume(api, orc):
    hs = M.view_state(orc, "b", 509, 4096)
    hv = M.fresh(orc, 1021, 2048)
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    assert merge_both(dv, ds, hv, hs) == (812, 812, 812, 0, 6, 0)
    assert R.block_voxels(hv) == R.block_voxels(hs)
    continue_both(api, orc, dv, hv, 25)


def test_a_fresh_source_changes_nothing(api, orc):
    hv, hs = M.view_state(orc, "a", 509, 4096), M.fresh(orc, 61, 7)
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    before = dv.host_voxels().tobytes()
    assert merge_both(dv, ds, hv, hs) == (0, 0, 0, 0, 0, 0)
    assert dv.host_voxels().tobytes() == before


def test_caps_of_four(api, orc):
    hv, hs = M.view_state(orc, "a", 509, 4096), M.view_state(orc, "b", 509, 4096)
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    merge_both(dv, ds, hv, hs, cap_d=4.0, cap_c=4.0)
    assert int(hv.voxels["distance_weight"].max()) == 4 and int(hv.voxels["color_weight"].max()) == 4
    # through the class: the same state
    hv2 = M.view_state(orc, "a", 509, 4096)
    dv2 = device_copy(api, hv2)
    assert dv2.merge(ds, max_distance_weight=4, max_color_weight=4) == (812, 812, 512, 0, 5, 0)
    assert_same_state(dv2, hv)


def test_skip_unobserved(api, orc):
    hs = M.view_state(orc, "b", 509, 4096)
    hv = M.view_state(orc, "a", 4093, 2048)
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    counts = merge_both(dv, ds, hv, hs, flags=M.SKIP_UNOBSERVED)
    assert counts[5] == 26 and counts[0] == 786 and counts[3] == 0
    dv2 = device_copy(api, M.view_state(orc, "a", 4093, 2048))
    assert dv2.merge(ds, skip_unobserved=True) == counts
    assert_same_state(dv2, hv)


def test_two_rounds_then_a_call_that_completes(api, orc):
    """max_rounds = 2 leaves blocks out; the call that continues fuses those and only those; the class does both"""
    hv, hs = M.view_state(orc, "a", 509, 4096), M.view_state(orc, "b", 509, 4096)
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    workspace = {}
    first = merge_both(dv, ds, hv, hs, max_rounds=2, workspace=workspace)
    assert first[3] > 0 and first[4] == 2
    second = merge_both(dv, ds, hv, hs, flags=M.CONTINUE, max_rounds=8, workspace=workspace)
    assert second[0] == first[3] and second[3] == 0 and first[1] + second[1] == 812
    whole = M.view_state(orc, "a", 509, 4096)
    assert M.merge(whole, hs) == (812, 812, 512, 0, first[4] + second[4], 0)
    assert_same_state(dv, whole)                           # the state of one call with all the rounds
    dv2 = device_copy(api, M.view_state(orc, "a", 509, 4096))
    assert dv2.merge(ds, max_rounds=2) == (812, 812, 512, 0, 5, 0)
    assert_same_state(dv2, whole)
    continue_both(api, orc, dv2, whole, 12)


def test_exhausted_destination(api, orc):
    """the excess list, then the pool run dry in the second round: upstream's leaked slots and never-written entries included"""
    hs = M.view_state(orc, "a", 509, 4096)
    hv = M.fresh(orc, 509, 64)
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    assert merge_both(dv, ds, hv, hs) == (888, 457, 457, 431, 2, 0)
    assert hv.counters[T.VK_CTR_DROPPED] == 185
    # the class does not go on after a drop
    dv2 = device_copy(api, M.fresh(orc, 509, 64))
    assert dv2.merge(ds) == (888, 457, 457, 431, 2, 0)
    assert_same_state(dv2, hv)
    # and a destination that is exhausted when the call begins
    hw, hb = M.view_state(orc, "a", 509, 64), M.view_state(orc, "b", 509, 4096)
    dw, db = device_copy(api, hw), device_copy(api, hb)
    counts = merge_both(dw, db, hw, hb)
    assert counts[2] == 0 and counts[3] > 0 and counts[4] == 1
    continue_both(api, orc, dv, hv, 25)


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
    with pytest.raises(api.VkError):
        dv.merge(ds)
    with pytest.raises(api.VkError):
        ds.merge(dv)
    with pytest.raises(api.VkError):
        ds.merge(ds)                                        # and never into itself
    sync()
    after = (dv.host_entries(), dv.host_voxels().tobytes(), dv.read_counters(), ds.host_voxels().tobytes())
    for a, b in zip(before, after):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    dv.cancel_requests_ahead(rounds=3)
    assert dv.merge(ds)[3] == 0


def test_abi_validates_before_touching_a_device(api):
    lib = api.lib()
    one = C.c_void_p(16)
    assert lib.vk_volume_merge(None, None, None, None, None, None) == -1

    def call(dst, src, params, counts=one, workspace=one):
        return lib.vk_volume_merge(C.byref(dst), C.byref(src), C.byref(params), counts, workspace, None)

    good = T.MergeParams(0, 8, 16.0, 16.0)
    dst, src = fake_volume(1 << 20), fake_volume(2 << 20)
    assert call(dst, src, good, counts=None) == -1
    assert call(dst, src, good, workspace=None) == -1
    assert lib.vk_volume_merge(C.byref(dst), C.byref(src), None, one, one, None) == -1
    assert call(dst, dst, good) == -1                                             # into itself
    for params in (T.MergeParams(4, 8, 16.0, 16.0), T.MergeParams(0, 0, 16.0, 16.0), T.MergeParams(0, 8, 0.5, 16.0),
                   T.MergeParams(0, 8, 16.0, 32768.0), T.MergeParams(0, 8, float("nan"), 16.0)):
        assert call(dst, src, params) == -1
    other = fake_volume(2 << 20)
    other.voxel_length = 0.005
    assert call(dst, other, good) == -1
    other = fake_volume(2 << 20)
    other.truncation_length = 0.05
    assert call(dst, other, good) == -1
    other = fake_volume(2 << 20)
    other.voxels += 8                                                             # not 16-byte aligned
    assert call(dst, other, good) == -1
    other = fake_volume(2 << 20)
    other.main_block_count = 0
    assert call(dst, other, good) == -1
    other = fake_volume(2 << 20)
    other.hash_entries = None
    assert call(dst, other, good) == -1
    assert lib.vk_volume_merge_workspace_bytes(0, 0) == 0
    assert lib.vk_volume_merge_workspace_bytes(8, -1) == 0
    assert lib.vk_volume_merge_workspace_bytes(509, 96) >= 605 * 5
    assert C.sizeof(T.MergeParams) == 16
