"""The definition of vk_volume_merge_posed (include/vk.h; tests/merge_pose_reference.py states it in numpy) held against what
it must mean: at the identity pose it is vk_volume_merge, a lattice-preserving pose into a fresh volume copies or permutes
the voxels exactly, either volume may be the destination, an affine field comes out as the same field, and a generic pose
samples and allocates. The volumes are merge_reference.view_state's."""
import numpy as np

import merge_pose_reference as MP
import merge_reference as M
import release_reference as R
from vulcan_amd import vk_types as T

SIZES = [((509, 4096), (509, 4096)), ((4093, 2048), (509, 4096))]
STATE = ("voxels", "hash_entries", "free_voxel_blocks", "block_visibility", "allocation_types", "counters")
f32 = np.float32


def test_identity_is_the_plain_merge(orc):
    for dst_size, src_size in SIZES:
        plain, posed = M.view_state(orc, "a", *dst_size), M.view_state(orc, "a", *dst_size)
        source = M.view_state(orc, "b", *src_size)
        want = M.merge(plain, source)
        got = MP.merge(posed, source, T.Transform.identity())
        print(dst_size, want, got)
        # the candidates are exactly the source blocks, and every voxel with a weight is a sample
        assert got[:7] == (want[0], want[0], want[1], want[2], want[3], want[4], want[5])
        assert got[7] == int((source.voxels["distance_weight"] != 0).sum())
        for name in STATE:
            assert getattr(posed, name).tobytes() == getattr(plain, name).tobytes(), name


def test_a_block_shift_into_a_fresh_volume_is_a_shifted_copy(orc):
    for k in (8.0, 16.0):
        assert f32(f32(k) * f32(M.VOXEL)) / f32(M.VOXEL) == f32(k)             # the translation is whole voxels in fp32 too
    source = M.view_state(orc, "b", 509, 4096)
    fresh = M.fresh(orc, 1021, 2048)
    counts = MP.merge(fresh, source, MP.shift((8, -16, 0)))
    assert counts[:5] == (812, 812, 812, 812, 0) and counts[6] == 0
    want = {(x + 1, y - 2, z): voxels for (x, y, z), voxels in R.block_voxels(source).items()}
    assert R.block_voxels(fresh) == want


def test_a_quarter_turn_into_a_fresh_volume_permutes_the_voxels(orc):
    source = M.view_state(orc, "b", 509, 4096)
    fresh = M.fresh(orc, 1021, 2048)
    counts = MP.merge(fresh, source, MP.quarter_turn((3, -1, 2)))
    assert counts[:5] == (812, 812, 812, 812, 0)
    coords, voxels = MP.cloud(source)
    # centre (x + .5, y + .5, z + .5) goes to (-(y + .5) + 24, (x + .5) - 8, (z + .5) + 16)
    moved = np.stack([-coords[:, 1] - 1 + 24, coords[:, 0] - 8, coords[:, 2] + 16], -1)
    order = np.lexsort(moved.T)
    got_coords, got_voxels = MP.cloud(fresh)
    assert np.array_equal(got_coords, moved[order])
    assert got_voxels.tobytes() == voxels[order].tobytes()


def test_either_volume_may_be_the_destination(orc):
    """A <- B under T and B <- A under the inverse of T hold bit-equal voxels at corresponding places"""
    for pose, place in ((MP.shift((8, -16, 0)), lambda c: c - np.array([8, -16, 0])),
                        (MP.quarter_turn((3, -1, 2)), lambda c: np.stack([c[:, 1] + 8, -c[:, 0] - 1 + 24, c[:, 2] - 16], -1))):
        a, b = M.view_state(orc, "a", 509, 4096), M.view_state(orc, "b", 509, 4096)
        counts_ab = MP.merge(a, R.clone(orc, b), pose)
        counts_ba = MP.merge(b, M.view_state(orc, "a", 509, 4096), pose.inverse())
        print(counts_ab, counts_ba)
        assert counts_ab[4] == 0 and counts_ba[4] == 0 and counts_ab[1] == 812 and counts_ba[1] == 888
        coords_a, voxels_a = MP.cloud(a)
        coords_b, voxels_b = MP.cloud(b)
        back = place(coords_a)                               # where a voxel of A's frame lies in B's
        order = np.lexsort(back.T)
        assert np.array_equal(back[order], coords_b)
        assert voxels_a[order].tobytes() == voxels_b.tobytes()
        assert int(voxels_a["distance_weight"].max()) == 5   # some voxels carry both histories


def test_an_affine_field_stays_the_same_field(orc):
    """every source voxel holds gradient . (centre - middle), every weight is set: under a generic pose a sampled voxel
    holds the same function of its own centre carried back, within 1e-4 — at most 4 roundings of at most 2^-16 voxel per
    component of the carried-back centre (|coordinates| < 256 voxels), times sqrt(3), times a gradient of 0.2 per voxel:
    about 2e-5; the seven lerps' roundings are smaller still."""
    source = M.view_state(orc, "b", 509, 4096)
    gradient = np.array([0.12, -0.1, 0.124])
    assert 0.19 < np.linalg.norm(gradient) < 0.2
    origins = np.array([M.origin_of(source, i) for i in M.source_blocks(source)])
    assert np.abs(8 * origins).max() + 8 < 256
    middle = 8.0 * origins.mean(0)
    for i in M.source_blocks(source):
        slot = int(source.hash_entries["data"][i])
        voxels = source.voxels[slot * 512:(slot + 1) * 512]
        centre = 8.0 * np.asarray(M.origin_of(source, i)) + MP.OFFSETS + 0.5
        voxels["distance"] = ((centre - middle) @ gradient).astype(f32)
        voxels["distance_weight"] = 1
        voxels["color_weight"] = 1
    pose = MP.generic()
    fresh = M.fresh(orc, 4093, 8192)
    counts = MP.merge(fresh, source, pose)
    print(counts)
    assert counts[4] == 0 and counts[7] > 100000
    coords, voxels = MP.cloud(fresh)
    assert np.abs(coords).max() < 256
    taken = voxels["distance_weight"] != 0
    assert int(taken.sum()) == counts[7]
    inverse = np.array(pose.inv[:], dtype=np.float64).reshape(4, 4).T
    inverse[:3, 3] /= float(f32(M.VOXEL))
    back = (coords[taken] + 0.5) @ inverse[:3, :3].T + inverse[:3, 3]
    error = np.abs(voxels["distance"][taken] - (back - middle) @ gradient)
    print("largest error", error.max())
    assert error.max() < 1e-4


def test_a_generic_pose_samples_and_allocates(orc):
    a, b = M.view_state(orc, "a", 509, 4096), M.view_state(orc, "b", 509, 4096)
    counts = MP.merge(a, b, MP.generic())
    print(counts)
    assert counts[0] == 812 and counts[1] > 812 and counts[3] >= 1 and counts[4] == 0 and counts[7] > 0
    assert a.counters[T.VK_CTR_VISIBLE] == 0 and a.counters[T.VK_CTR_BANDED] == -1 and not a.allocation_types.any()


def test_entry_points_validate_their_arguments_without_a_device():
    import ctypes as C
    from vulcan_amd import api
    lib = api.lib()
    assert lib.vk_volume_merge_posed(None, None, None, None, None, None) == -1
    assert lib.vk_volume_merge_posed_workspace_bytes(0, 0, 8, 8) == 0
    assert lib.vk_volume_merge_posed_workspace_bytes(8, 8, 8, -1) == 0
    assert lib.vk_volume_merge_posed_workspace_bytes(509, 96, 61, 7) >= 605 * 17 + 68 * 4
    assert C.sizeof(T.MergePoseParams) == 16 + 128
