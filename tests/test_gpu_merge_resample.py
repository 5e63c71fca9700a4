"""vk_volume_merge_resampled on the device against its CPU statement (tests/merge_resample_reference.py), bit for bit: both
volumes start from uploaded oracle states, the device makes the call, and the destination must hold the same hash entries,
visibility bytes, free list, voxel bytes, public counters and the eight counts as the statement leaves on the host, the
source what it held before. Which blocks are candidates is decided by fp32 values whose operation order is fixed, the
allocation compares stored values and the fusion is one defined sequence of float32 operations, so there is no tolerance
anywhere in this file but the two conditions on what a user sees, which are stated where they are asserted.

The statement costs seconds per thousand sampled blocks, so where a case does not need the whole 812-block view the source
is cut to a box of blocks first (merge_resample_reference.cut), on the host, before it is uploaded."""
import ctypes as C

import numpy as np
import pytest

from abi_support import fake_volume
import cast_reference as CR
import merge_pose_reference as MP
import merge_reference as M
import merge_resample_reference as MR
import release_reference as R
from gpu_support import OTHER, SAME, api, assert_same_state, continue_both, device_copy, on_device, overwrite, sync  # noqa: F401
from vulcan_amd import vk_types as T

pytestmark = pytest.mark.gpu

B200, B114, B18 = ((3, -4, 9), (10, 3, 18)), ((4, -3, 9), (9, 2, 18)), ((6, -1, 9), (7, 1, 18))     # of view "b": blocks kept


def dirty(api, dv, ds, fill):
    """the workspace and counts tensor the next merge_resampled of `dv` from `ds` will use, created as the call will ask
    for them and overwritten"""
    size = (ds.main, ds.excess, dv.main, dv.excess, dv._resample_ratios(ds)[2])
    workspace, counts = dv._workspace("merge_resampled", size, api.lib().vk_volume_merge_resampled_workspace_bytes, 8)
    overwrite(workspace, fill, 1 + workspace.numel())
    overwrite(counts, fill, 2)


def merge_both(api, dv, ds, hv, hs, pose, n, flags=0, max_rounds=8, cap_d=16.0, cap_c=16.0, workspace=None, fill="noise"):
    """one call of the entry point on the device, the statement on the host: the same eight counts, the same state"""
    want = MR.merge(hv, hs, pose, n, flags, max_rounds, cap_d, cap_c, workspace=workspace)
    if not flags & MR.CONTINUE:
        dirty(api, dv, ds, fill)
    got = dv._merge_resampled_call(ds, pose, n, flags, max_rounds, cap_d, cap_c)
    print("counts", got, want)
    assert got == want
    assert_same_state(dv, hv)
    assert_same_state(ds, hs)                              # the source is only read
    return want


def fresh_pair(api, orc, main, excess, voxel_length, truncation_length):
    hv = MR.fresh(orc, main, excess, voxel_length, truncation_length)
    return hv, device_copy(api, hv)


def test_equal_lengths_and_one_point_is_the_posed_merge_on_the_device_too(api, orc):
    hv, hs = M.view_state(orc, "a", 509, 4096), M.view_state(orc, "b", 509, 4096)
    dv, ds, posed = device_copy(api, hv), device_copy(api, hs), device_copy(api, hv)
    counts = merge_both(api, dv, ds, hv, hs, MP.generic(), 1)
    assert posed._merge_posed_call(ds, MP.generic(), 0, 8, 16.0, 16.0) == counts
    assert_same_state(posed, hv)
    assert posed.host_voxels().tobytes() == dv.host_voxels().tobytes()
    assert counts[0] == 812 and counts[1] > 812 and counts[4] == 0 and counts[7] > 100000


@pytest.mark.parametrize("sizes", [SAME, OTHER], ids=["long-chains", "other-bucket-count"])
def test_eight_into_sixteen_millimetres_and_half_the_truncation_scale(api, orc, sizes):
    """8 mm / 0.04 into a fresh 16 mm / 0.08 volume (k = 0.5), n = 2, a generic pose; then the merged volume goes on"""
    hs = M.view_state(orc, "a", *sizes[1])
    hv, dv = fresh_pair(api, orc, sizes[0][0], sizes[0][1], 0.016, 0.08)
    ds = device_copy(api, hs)
    counts = merge_both(api, dv, ds, hv, hs, MP.generic(), 2, fill="ones" if sizes is SAME else "noise")
    assert counts[0] == 888 and 100 < counts[1] < 888 and counts[4] == 0 and counts[7] > 10000
    assert (np.abs(hv.voxels["distance"][hv.voxels["distance_weight"] != 0]) < 0.5).all()
    continue_both(api, orc, dv, hv, 12)


@pytest.mark.parametrize("truncation", [0.04, 0.02], ids=["k=1", "k=2"])
def test_eight_into_five_millimetres(api, orc, truncation):
    """ratio 1.6: no sample point is a lattice point, K = 4 and D = 3 (200 blocks of view "b")"""
    hs = MR.cut(M.view_state(orc, "b", 509, 4096), B200)
    hv, dv = fresh_pair(api, orc, 4093, 4096, 0.005, truncation)
    ds = device_copy(api, hs)
    assert MR.box_blocks(MR.ratios(hv, hs)[0]) == 4 and MR.ratios(hv, hs)[2] == np.float32(0.04 / truncation)
    counts = merge_both(api, dv, ds, hv, hs, MP.generic(), 1)
    assert counts[0] == 200 and counts[1] > 800 and counts[4] == 0 and counts[7] > 100000


def test_eight_into_four_millimetres(api, orc):
    """ratio 1/2: K = 5 (114 blocks of view "b")"""
    hs = MR.cut(M.view_state(orc, "b", 509, 4096), B114)
    hv, dv = fresh_pair(api, orc, 4093, 2048, 0.004, 0.04)
    ds = device_copy(api, hs)
    assert MR.box_blocks(MR.ratios(hv, hs)[0]) == 5
    counts = merge_both(api, dv, ds, hv, hs, MP.generic(), 1, fill="ones")
    assert counts[0] == 114 and counts[1] > 1000 and counts[4] == 0


@pytest.mark.parametrize("voxel_length, n", [(0.002, 1), (0.032, 4)], ids=["ratio-4", "ratio-1/4"])
def test_the_largest_box_and_the_largest_directory(api, orc, voxel_length, n):
    """K = 8 into 2 mm, D = 9 into 32 mm (18 blocks of view "b"): a box or a directory too small shows in the candidates
    and in the voxels that took a sample, here and nowhere else"""
    hs = MR.cut(M.view_state(orc, "b", 509, 4096), B18)
    hv, dv = fresh_pair(api, orc, 4093, 4096, voxel_length, 0.04)
    ds = device_copy(api, hs)
    r_fwd, r_back, _ = MR.ratios(hv, hs)
    assert (MR.box_blocks(r_fwd), MR.directory_blocks(r_back)) == ((8, 2) if n == 1 else (2, 9))
    want = MR.merge(R.clone(orc, hv), hs, MP.generic(), n)
    counts = merge_both(api, dv, ds, hv, hs, MP.generic(), n)
    assert counts[1] == want[1] and counts[7] == want[7] and counts[0] == 18 and counts[4] == 0 and counts[7] > 50


def test_two_to_one_at_the_identity_is_the_ordered_mean_on_the_device(api, orc):
    """test_merge_resample_reference's exact case: the device leaves the statement's bytes, which that test holds to the
    mean of the stored 2x2x2 voxels computed by slicing"""
    hs = M.view_state(orc, "a", 509, 4096)
    hv, dv = fresh_pair(api, orc, 509, 1024, 0.016, M.TRUNCATION)
    ds = device_copy(api, hs)
    counts = merge_both(api, dv, ds, hv, hs, T.Transform.identity(), 2)
    assert counts[0] == 888 and counts[4] == 0 and counts[7] > 20000
    # the device's voxels are the host's (merge_both); those against the slicing, with no pose, lattice or table between
    coords, voxels = MP.cloud(hv)
    want, short = MR.ordered_mean_of_eight(hs, coords)
    assert voxels.tobytes() == want.tobytes() and dv.host_voxels().tobytes() == hv.voxels.tobytes()
    assert short["distance"] > 100 and short["color"] > 100


def test_three_points_per_axis(api, orc):
    """n = 3 is the one n whose offsets (1/6, 1/2, 5/6 less 1/2) are not exact"""
    hs = MR.cut(M.view_state(orc, "b", 509, 4096), B18)
    hv = M.view_state(orc, "a", 509, 4096)
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    counts = merge_both(api, dv, ds, hv, hs, MP.generic(), 3)
    assert counts[0] == 18 and counts[4] == 0 and counts[7] > 1000


def test_skip_unobserved(api, orc):
    hs = M.view_state(orc, "b", 509, 4096)
    hv, dv = fresh_pair(api, orc, 4093, 2048, 0.016, 0.04)
    ds = device_copy(api, hs)
    counts = merge_both(api, dv, ds, hv, hs, MP.generic(), 2, flags=MR.SKIP_UNOBSERVED)
    assert counts[6] == 26 and counts[0] == 786 and counts[4] == 0
    dv2 = fresh_pair(api, orc, 4093, 2048, 0.016, 0.04)[1]
    assert dv2.merge_resampled(ds, pose=MP.generic(), supersample=2, skip_unobserved=True) == counts
    assert_same_state(dv2, hv)


def test_two_rounds_then_a_call_that_completes(api, orc):
    """max_rounds = 2 leaves candidates out; the call that continues fuses those and only those; the class does both"""
    pose = MP.generic()
    hs = M.view_state(orc, "b", 509, 4096)
    hv, dv = fresh_pair(api, orc, 31, 1024, 0.016, 0.04)
    ds = device_copy(api, hs)
    workspace = {}
    first = merge_both(api, dv, ds, hv, hs, pose, 2, max_rounds=2, workspace=workspace)
    assert first[4] > 0 and first[5] == 2
    second = merge_both(api, dv, ds, hv, hs, pose, 2, flags=MR.CONTINUE, max_rounds=16, workspace=workspace)
    assert second[0] == first[0] and second[1] == first[4] and second[4] == 0 and first[2] + second[2] == first[1]
    whole = MR.fresh(orc, 31, 1024, 0.016, 0.04)
    want = MR.merge(whole, hs, pose, 2, max_rounds=32)
    assert want == (first[0], first[1], first[1], first[3] + second[3], 0, first[5] + second[5], 0, first[7] + second[7])
    assert_same_state(dv, whole)                           # the state of one call with all the rounds
    dv2 = fresh_pair(api, orc, 31, 1024, 0.016, 0.04)[1]
    assert dv2.merge_resampled(ds, pose=pose, supersample=2, max_rounds=2) == want
    assert_same_state(dv2, whole)


def test_exhausted_destination(api, orc):
    """the excess list runs dry: candidates stay absent and each is counted once. (At 16 mm the 888 blocks of view "a" reach
    252 candidates, 53 of them behind another in one of the 509 buckets: an excess list of 64 holds them all and drops
    nothing, so the list here has 16 entries.)"""
    hs = M.view_state(orc, "a", 509, 4096)
    hv, dv = fresh_pair(api, orc, 509, 16, 0.016, 0.04)
    ds = device_copy(api, hs)
    counts = merge_both(api, dv, ds, hv, hs, MP.generic(), 2)
    assert counts[4] > 0 and counts[2] + counts[4] == counts[1] and counts[3] == counts[2]
    assert hv.counters[T.VK_CTR_DROPPED] > 0
    # the class does not go on after a drop
    dv2 = fresh_pair(api, orc, 509, 16, 0.016, 0.04)[1]
    assert dv2.merge_resampled(ds, pose=MP.generic(), supersample=2) == counts
    assert_same_state(dv2, hv)


def test_refused_while_a_frame_is_announced_into_itself_and_from_a_pack(api, orc):
    hv, hs = M.view_state(orc, "a", 509, 4096), M.view_state(orc, "b", 509, 4096)
    dv, ds = device_copy(api, hv), device_copy(api, hs)
    coarse = fresh_pair(api, orc, 509, 1024, 0.016, 0.04)[1]
    hf = R.frame_at(orc, 25)
    df = api.Frame(hf.depth, hf.depth_projection, hf.depth_to_world)
    dv.set_view(df, rounds=3)
    out = api.Frame(np.zeros((R.H, R.W), np.float32), hf.depth_projection, hf.depth_to_world)
    nf = R.frame_at(orc, 12)
    api.Tracer(dv).trace(out, next_frame=api.Frame(nf.depth, nf.depth_projection, nf.depth_to_world))
    sync()
    assert dv.requests_ahead is not None and dv.requests_ahead.valid == 1
    pack = ds.pack()
    volumes = (dv, ds, coarse)
    before = [(v.host_entries(), v.host_voxels().tobytes(), v.read_counters()) for v in volumes]
    pose = MP.generic()
    with pytest.raises(api.VkError):
        dv.merge_resampled(ds, pose=pose)
    with pytest.raises(api.VkError):
        coarse.merge_resampled(dv, pose=pose)              # the source has the frame announced
    with pytest.raises(api.VkError):
        ds.merge_resampled(ds, pose=pose)                  # never into itself
    with pytest.raises(TypeError):
        coarse.merge_resampled(pack)
    sync()
    after = [(v.host_entries(), v.host_voxels().tobytes(), v.read_counters()) for v in volumes]
    for was, now in zip(before, after):
        for a, b in zip(was, now):
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    dv.cancel_requests_ahead(rounds=3)
    assert coarse.merge_resampled(dv, pose=pose)[4] == 0


def test_abi_validates_before_touching_a_device(api):
    lib = api.lib()
    one = C.c_void_p(16)

    def call(dst, src, params, counts=one, workspace=one):
        return lib.vk_volume_merge_resampled(C.byref(dst), C.byref(src), C.byref(params), counts, workspace, None)

    def params(pose=None, merge=None, supersample=1, reserved=0):
        return T.MergeResampleParams(merge or T.MergeParams(0, 8, 16.0, 16.0), pose or T.Transform.identity(), supersample, reserved)

    def other_lengths(voxel_length=None, truncation_length=None):
        other = fake_volume(2 << 20)
        if voxel_length is not None:
            other.voxel_length = voxel_length
        if truncation_length is not None:
            other.truncation_length = truncation_length
        return other

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
    other.voxels += 8                                                             # not 16-byte aligned
    assert call(dst, other, params()) == -1
    # what this call adds: the ratio of the voxel lengths, the ratio of the truncation lengths, n, the reserved word
    length = float(dst.voxel_length)
    for ratio in (0.2, 4.5):
        assert call(dst, other_lengths(voxel_length=length * ratio), params()) == -1
        assert call(other_lengths(voxel_length=length * ratio), src, params()) == -1
    for bad in (float("nan"), 0.0, float("inf"), -0.04):
        assert call(dst, other_lengths(truncation_length=bad), params()) == -1
    for supersample in (0, 5, -1):
        assert call(dst, src, params(supersample=supersample)) == -1
    assert call(dst, src, params(reserved=1)) == -1


def test_a_coarse_copy_shows_a_ray_the_same_surface(api, orc):
    """What a user sees: view "a" resampled to 16 mm through the class, and the same interior pixel rays cast through both
    maps (test_merge_resample_reference.interior_rays' choice, which the statement alone meets). Of the rays that hit in
    the 8 mm map at most 10 % may miss in the 16 mm map, and where both hit the two distances differ by at most one
    voxel of the coarse map, 16 mm."""
    rays, xs, ys = CR.pixel_rays()
    rays = rays[(xs >= 40) & (xs < 120) & (ys >= 30) & (ys < 90)]
    fine = device_copy(api, M.view_state(orc, "a", 509, 4096))
    coarse = fine.resampled(0.016, M.TRUNCATION, 509, 1024, supersample=2)
    assert coarse.voxel_length == 0.016 and coarse.read_counters()[T.VK_CTR_DROPPED] == 0
    through_fine = fine.cast_rays(on_device(rays), t_max=CR.T_MAX, max_steps=CR.MAX_STEPS)
    through_coarse = coarse.cast_rays(on_device(rays), t_max=CR.T_MAX, max_steps=CR.MAX_STEPS)
    status_fine, status_coarse = through_fine.status.cpu().numpy(), through_coarse.status.cpu().numpy()
    t_fine, t_coarse = through_fine.t.cpu().numpy().astype(np.float64), through_coarse.t.cpu().numpy().astype(np.float64)
    hit_fine, hit_coarse = status_fine == CR.HIT, status_coarse == CR.HIT
    lost = float((hit_fine & ~hit_coarse).sum()) / float(hit_fine.sum())
    worst = float(np.abs(t_fine - t_coarse)[hit_fine & hit_coarse].max())
    print("rays", len(rays), "hit in the fine map", int(hit_fine.sum()), "lost in the coarse map", lost, "worst |dt|", worst)
    assert hit_fine.sum() > 1000
    assert lost <= 0.10
    assert worst <= 0.016
