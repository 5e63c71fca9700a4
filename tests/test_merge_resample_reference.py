"""The definition of vk_volume_merge_resampled (include/vk.h; tests/merge_resample_reference.py states it in numpy) held
against what it must mean: at equal lengths with one sample point it is vk_volume_merge_posed; a 2:1 copy at the identity
is the ordered mean of 2x2x2 stored voxels; a 1:2 copy of an affine field is that field; a stored distance is carried into
the destination's truncation length and stays inside the band; the blocks that own a candidate lie where the way back
looks for them; and a coarse copy of a fused map shows a ray the same surface. The volumes are merge_reference.view_state's."""
import numpy as np

import cast_reference as CR
import merge_pose_reference as MP
import merge_reference as M
import merge_resample_reference as MR
import release_reference as R
from vulcan_amd import vk_types as T

STATE = ("voxels", "hash_entries", "free_voxel_blocks", "block_visibility", "allocation_types", "counters")
f32 = np.float32


def test_equal_lengths_and_one_point_is_the_posed_merge(orc):
    for pose in (T.Transform.identity(), MP.generic(), MP.quarter_turn((3, -1, 2))):
        posed, resampled = M.view_state(orc, "a", 509, 4096), M.view_state(orc, "a", 509, 4096)
        source = MR.cut(M.view_state(orc, "b", 509, 4096), ((3, -4, 9), (10, 3, 18)))      # 200 blocks: seconds, not tens
        want = MP.merge(posed, source, pose)
        got = MR.merge(resampled, source, pose, 1)
        print(want, got)
        assert got == want and want[0] == 200 and want[7] > 10000
        for name in STATE:
            assert getattr(resampled, name).tobytes() == getattr(posed, name).tobytes(), name


def test_two_to_one_at_the_identity_is_the_ordered_mean_of_eight_voxels(orc):
    """8 mm into a fresh 16 mm volume, n = 2: every sample point is a source voxel centre (0.016f / 0.008f == 2.0f and the
    offsets are +-0.25f: exact), so a dst voxel is the mean, in point order, of the stored 2x2x2 source voxels that carry a
    weight where at least 5 do, with the smallest of their weights — computed here by slicing a dense copy of the source"""
    assert f32(0.016) / f32(0.008) == f32(2) and f32(0.008) / f32(0.016) == f32(0.5)
    source = M.view_state(orc, "a", 509, 4096)
    fresh = MR.fresh(orc, 509, 1024, 0.016, M.TRUNCATION)
    counts = MR.merge(fresh, source, T.Transform.identity(), 2)
    print(counts)
    assert counts[0] == 888 and counts[4] == 0 and counts[2] == counts[1] == counts[3] and counts[7] > 20000
    coords, voxels = MP.cloud(fresh)
    want, short = MR.ordered_mean_of_eight(source, coords)
    print("voxels with a distance", int((want["distance_weight"] != 0).sum()), "a colour", int((want["color_weight"] != 0).sum()),
          "with some but fewer than 5 of 8", short)
    assert voxels.tobytes() == want.tobytes()
    assert (want["distance_weight"] != 0).sum() > 20000 and (want["color_weight"] != 0).sum() > 15000
    assert short["distance"] > 100 and short["color"] > 100
    assert counts[7] == int((voxels["distance_weight"] != 0).sum())


def affine_source(orc, gradient):
    """a few whole blocks of view "b" (a box of 3 x 3 x 2 blocks), every voxel gradient . (centre - middle), weights 3 and 2"""
    source = M.view_state(orc, "b", 509, 4096)
    origins = np.array([M.origin_of(source, i) for i in M.source_blocks(source)])
    centre = np.round(origins.mean(0)).astype(int)
    MR.cut(source, (tuple(centre - (1, 1, 1)), tuple(centre + (1, 1, 0))))
    blocks = M.source_blocks(source)
    middle = 8.0 * np.array([M.origin_of(source, i) for i in blocks]).mean(0)
    for i in blocks:
        slot = int(source.hash_entries["data"][i])
        voxels = source.voxels[slot * 512:(slot + 1) * 512]
        at = 8.0 * np.asarray(M.origin_of(source, i)) + MP.OFFSETS + 0.5
        voxels["distance"] = ((at - middle) @ gradient).astype(f32)
        voxels["distance_weight"] = 3
        voxels["color_weight"] = 2
    return source, middle, len(blocks)


def test_one_to_two_of_an_affine_field_is_the_field(orc):
    """8 mm into a fresh 4 mm volume at the identity, n = 1: a trilinear sample of an affine field is the field. A dst voxel
    that took a sample holds gradient . (centre / 2 - middle) within 1e-4, the project's TSDF tolerance (README.md): the
    carried centre is exact (a product with 0.5f), the stored values carry one rounding of at most 2^-25 each and the seven
    lerps three roundings each of values below 1. Measured: the worst case printed below, 7.7e-8."""
    gradient = np.array([0.03, -0.025, 0.031])
    source, middle, blocks = affine_source(orc, gradient)
    assert 4 <= blocks <= 18
    fresh = MR.fresh(orc, 509, 1024, 0.004, M.TRUNCATION)
    counts = MR.merge(fresh, source, T.Transform.identity(), 1)
    print(counts)
    assert counts[0] == blocks and counts[4] == 0 and counts[1] >= 8 * blocks
    coords, voxels = MP.cloud(fresh)
    taken = voxels["distance_weight"] != 0
    assert int(taken.sum()) == counts[7] and counts[7] > 3000 * blocks
    assert (voxels["distance_weight"][taken] == 3).all() and (voxels["color_weight"][taken] == 2).all()
    want = ((coords[taken] + 0.5) * 0.5 - middle) @ gradient
    error = np.abs(voxels["distance"][taken].astype(np.float64) - want)
    print("largest error", error.max(), "largest |field|", np.abs(want).max())
    assert error.max() < 1e-4


def test_a_stored_distance_is_carried_into_the_destination_truncation_length(orc):
    """equal voxel lengths at the identity with n = 1: dst voxel x takes source voxel x. k = 2 (truncation 0.04 into 0.02)
    clamps at 1.0 and takes nothing at or behind -1; k = 0.5 (0.04 into 0.08) takes nothing from a saturated voxel, and
    every distance it writes lies in (-0.5, 0.5)"""
    source = M.view_state(orc, "a", 509, 4096)
    coords_s, voxels_s = MP.cloud(source)
    observed = voxels_s["distance_weight"] != 0
    d = voxels_s["distance"]
    assert (observed & (d >= 1)).sum() > 100 and (observed & (d <= f32(-0.5))).sum() > 100 and (d[observed] > -1).all()
    for truncation, k in ((0.02, 2.0), (0.08, 0.5)):
        fresh = MR.fresh(orc, 4093, 2048, M.VOXEL, truncation)
        assert MR.ratios(fresh, source)[2] == f32(k)
        counts = MR.merge(fresh, source, T.Transform.identity(), 1)
        coords, voxels = MP.cloud(fresh)
        assert counts[:5] == (888, 888, 888, 888, 0) and np.array_equal(coords, coords_s)
        scaled = f32(k) * d
        if k > 1:
            taken = observed & ~(scaled <= -1)
            want = np.where(scaled >= 1, f32(1), scaled)
            assert (taken & (scaled >= 1)).sum() > 100 and (observed & ~taken).sum() > 100
        else:
            taken = observed & ~(d >= 1)
            want = scaled
            assert (np.abs(voxels["distance"][voxels["distance_weight"] != 0]) < 0.5).all()
        print(k, counts, int(taken.sum()))
        assert counts[7] == int(taken.sum())
        assert np.array_equal(voxels["distance_weight"] != 0, taken)
        assert voxels["distance"][taken].tobytes() == want[taken].astype(f32).tobytes()
        assert (voxels["distance"][~taken] == 1).all()
        # the colour is not rescaled, and is decided apart
        colored = voxels_s["color_weight"] != 0
        assert np.array_equal(voxels["color_weight"] != 0, colored)
        assert voxels["color"][colored].tobytes() == voxels_s["color"][colored].tobytes()


def test_the_blocks_that_own_a_candidate_lie_in_its_box_on_the_way_back(orc):
    """A <- B under T at ratio r and B <- A under the inverse at 1 / r do not give the same voxels (one averages, the other
    interpolates). What holds on both ways, and what the count of the absent candidates rests on: every candidate's owners
    — the source blocks that reach it — lie in the box of K(1 / r)^3 blocks that the candidate's own corners reach back to."""
    pose = MP.generic()
    a = MR.cut(M.view_state(orc, "a", 509, 4096), ((-3, -2, 14), (2, 2, 16)))
    coarse = MR.fresh(orc, 509, 1024, 0.016, M.TRUNCATION)
    MR.merge(coarse, a, pose, 2)
    for dst, src, way, n in ((coarse, a, pose, 2), (a, coarse, pose.inverse(), 1)):
        r_fwd, r_back, _ = MR.ratios(dst, src)
        fwd, back = MR.rows(way.m, r_fwd, dst.voxel_length), MR.rows(way.inv, r_back, src.voxel_length)
        span, owners = MR.box_blocks(r_back), 0
        considered = M.source_blocks(src)
        assert len(considered) > 20
        for i in considered:
            origin = M.origin_of(src, i)
            for candidate in MR.candidates_of(origin, fwd, back, n, MR.box_blocks(r_fwd)):
                q = MP.apply(back, (8 * np.asarray(candidate, dtype=np.int64) + 8 * MP.CORNERS).astype(f32))
                lo = MP.to_int(np.floor(q.min(0) * f32(0.125)))
                hi = np.minimum(MP.to_int(np.floor(q.max(0) * f32(0.125))), lo + span - 1)
                assert (lo <= origin).all() and (origin <= hi).all(), (candidate, origin, lo, hi)
                owners += 1
        print("ratio", r_fwd, "owners checked", owners)
        assert owners > len(considered)


# ---- what a user sees: the same rays through the map and through its coarse copy -------------------------------------

def interior_rays():
    """the pixel rays of view "a"'s camera (the identity pose) over the middle half of the image, every second pixel: the
    ripple has no depth discontinuity there and every ray meets the fused surface well inside the map"""
    rays, xs, ys = CR.pixel_rays()
    inside = (xs >= 40) & (xs < 120) & (ys >= 30) & (ys < 90)
    return rays[inside]


def same_surface(fine, coarse, voxel_length):
    """(share of the rays that hit in `fine` and not in `coarse`, the largest |t_fine - t_coarse| over the rays that hit in
    both) and the two conditions on them: at most 10 %, at most one voxel of the coarse map"""
    hit_fine, hit_coarse = fine.status == CR.HIT, coarse.status == CR.HIT
    assert hit_fine.sum() > 1000
    lost = float((hit_fine & ~hit_coarse).sum()) / float(hit_fine.sum())
    both = hit_fine & hit_coarse
    worst = float(np.abs(fine.t[both].astype(np.float64) - coarse.t[both]).max())
    print("rays", len(hit_fine), "hit in the fine map", int(hit_fine.sum()), "lost in the coarse map", lost, "worst |dt|", worst)
    assert lost <= 0.10
    assert worst <= voxel_length
    return lost, worst


def test_a_coarse_copy_shows_a_ray_the_same_surface(orc):
    """view "a" at 8 mm resampled to 16 mm (n = 2, the same truncation length, both caps 32767 as Volume.resampled has them):
    the statement alone meets the two conditions the device test asserts. Measured: none of the 1200 rays lost, worst |dt| 3.11 mm."""
    source = M.view_state(orc, "a", 509, 4096)
    coarse = MR.fresh(orc, 509, 1024, 0.016, M.TRUNCATION)
    counts = MR.merge(coarse, source, T.Transform.identity(), 2, cap_d=32767.0, cap_c=32767.0)
    assert counts[4] == 0
    rays = interior_rays()
    same_surface(CR.cast(source, rays), CR.cast(coarse, rays), 0.016)


def test_entry_points_validate_their_arguments_without_a_device():
    import ctypes as C
    from vulcan_amd import api
    lib = api.lib()
    assert lib.vk_volume_merge_resampled(None, None, None, None, None, None) == -1
    assert lib.vk_volume_merge_resampled_workspace_bytes(0, 0, 8, 8, 3) == 0
    assert lib.vk_volume_merge_resampled_workspace_bytes(8, 8, 8, -1, 3) == 0
    assert lib.vk_volume_merge_resampled_workspace_bytes(8, 8, 8, 8, 1) == 0 and lib.vk_volume_merge_resampled_workspace_bytes(8, 8, 8, 8, 9) == 0
    small, large = (lib.vk_volume_merge_resampled_workspace_bytes(509, 96, 61, 7, k) for k in (3, 8))
    assert small >= 605 * (1 + 12 + 16 + 4) + 68 * 4 and large >= small + 605 * 60
    assert C.sizeof(T.MergeResampleParams) == 16 + 128 + 8
    assert [MR.box_blocks(r) for r in (0.25, 0.5, 1.0, 1.6, 2.0, 4.0)] == [2, 2, 3, 4, 5, 8]
    assert [MR.directory_blocks(r) for r in (0.25, 0.5, 1.0, 2.0, 4.0)] == [2, 2, 3, 5, 9]
