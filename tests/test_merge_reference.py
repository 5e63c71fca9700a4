"""The definition of vk_volume_merge (include/vk.h; tests/merge_reference.py states it in numpy) held against the oracle:
the merge does not depend on which of two volumes is the destination, a merge into a fresh volume is a copy, a fresh
source changes nothing, the caps engage, an exhausted destination reports what it left out, unobserved blocks can stay
behind, and the merged volume raycasts. The states the tests share — merge_reference.view_state: 160x120 ripple frames,
volume "a" two frames at yaw 0, volume "b" three frames at yaw 25 degrees, depth plus a seeded random colour image each —
hold 888 and 812 blocks, 300 of them in common."""
import numpy as np

import merge_reference as M
import release_reference as R
from vulcan_amd import vk_types as T

SIZES = [(509, 4096), (4093, 2048)]


def test_the_shared_states_are_the_ones_the_numbers_are_for(orc):
    a, b = M.view_state(orc, "a", 509, 4096), M.view_state(orc, "b", 509, 4096)
    blocks_a, blocks_b = R.block_voxels(a), R.block_voxels(b)
    assert (len(blocks_a), len(blocks_b), len(set(blocks_a) & set(blocks_b))) == (888, 812, 300)
    assert a.counters[T.VK_CTR_DROPPED] == 0 and b.counters[T.VK_CTR_DROPPED] == 0
    assert int(a.voxels["distance_weight"].max()) == 2 and int(b.voxels["color_weight"].max()) == 3
    assert max(len(R.chain(b.hash_entries, bucket, b.max)) for bucket in range(b.main)) >= 5


def test_either_volume_may_be_the_destination(orc):
    for main, excess in SIZES:
        a, b = M.view_state(orc, "a", main, excess), M.view_state(orc, "b", main, excess)
        source_b, source_a = R.clone(orc, b), R.clone(orc, a)
        counts_ab = M.merge(a, source_b)
        counts_ba = M.merge(b, source_a)
        print(main, excess, counts_ab, counts_ba)
        assert counts_ab[:4] == (812, 812, 512, 0) and counts_ba[:4] == (888, 888, 588, 0)
        assert counts_ab[4] >= 2 and counts_ba[4] >= 2 and counts_ab[5] == counts_ba[5] == 0
        merged_ab, merged_ba = R.block_voxels(a), R.block_voxels(b)
        assert len(merged_ab) == 1400 and set(merged_ab) == set(merged_ba)
        assert all(merged_ab[origin] == merged_ba[origin] for origin in merged_ab)     # bit-equal: a + b == b + a in fp32
        # the sources were only read
        assert source_b.voxels.tobytes() == M.view_state(orc, "b", main, excess).voxels.tobytes()
        assert source_b.hash_entries.tobytes() == M.view_state(orc, "b", main, excess).hash_entries.tobytes()
        # the blocks the two have in common carry both histories
        both = np.frombuffer(merged_ab[next(iter(set(R.block_voxels(source_a)) & set(R.block_voxels(source_b))))], dtype=T.voxel_dtype)
        assert int(both["distance_weight"].max()) == 5
        assert a.counters[T.VK_CTR_VISIBLE] == 0 and a.counters[T.VK_CTR_BANDED] == -1
        assert not a.allocation_types.any() and a.counters[T.VK_CTR_DROPPED] == 0
        # and the same rounds in two calls leave the same state: what the first call fused is not fused again
        a2, workspace = M.view_state(orc, "a", main, excess), {}
        first = M.merge(a2, source_b, 0, 2, workspace=workspace)
        assert first[3] > 0 and first[4] == 2 and first[1] + first[3] == 812
        second = M.merge(a2, source_b, M.CONTINUE, 8, workspace=workspace)
        assert second[0] == first[3] and second[3] == 0 and first[4] + second[4] == counts_ab[4]
        assert first[1] + second[1] == 812 and first[2] + second[2] == 512
        for name in ("voxels", "hash_entries", "free_voxel_blocks", "block_visibility", "counters"):
            assert getattr(a2, name).tobytes() == getattr(a, name).tobytes(), name


def test_a_merge_into_a_fresh_volume_is_a_copy(orc):
    for main, excess in SIZES:
        b = M.view_state(orc, "b", main, excess)
        fresh = M.fresh(orc, 1021, 2048)
        counts = M.merge(fresh, b)
        assert counts[:4] == (812, 812, 812, 0) and counts[4] >= 2
        assert R.block_voxels(fresh) == R.block_voxels(b)
        assert fresh.counters[T.VK_CTR_VOXEL_PTR] == fresh.max - 1 - 812


def test_a_fresh_source_changes_nothing(orc):
    a = M.view_state(orc, "a", 509, 4096)
    before = R.clone(orc, a)
    assert M.merge(a, M.fresh(orc, 61, 7)) == (0, 0, 0, 0, 0, 0)
    before.counters[T.VK_CTR_VISIBLE], before.counters[T.VK_CTR_BANDED] = 0, -1       # what every call defines
    for name in ("voxels", "hash_entries", "free_voxel_blocks", "block_visibility", "allocation_types", "counters"):
        assert getattr(a, name).tobytes() == getattr(before, name).tobytes(), name


def test_the_caps_engage(orc):
    a, b = M.view_state(orc, "a", 509, 4096), M.view_state(orc, "b", 509, 4096)
    M.merge(a, b, 0, 8, 4.0, 4.0)
    assert int(a.voxels["distance_weight"].max()) == 4 and int(a.voxels["color_weight"].max()) == 4
    uncapped = M.view_state(orc, "a", 509, 4096)
    M.merge(uncapped, b)
    assert int(uncapped.voxels["distance_weight"].max()) == 5 and int(uncapped.voxels["color_weight"].max()) == 5
    reached = uncapped.voxels["distance_weight"] == 5
    assert reached.any() and np.all(a.voxels["distance_weight"][reached] == 4)
    # the cap bounds the weight, not the average
    assert np.array_equal(a.voxels["distance"], uncapped.voxels["distance"])
    assert np.array_equal(a.voxels["color"], uncapped.voxels["color"])


def test_an_exhausted_destination_reports_what_it_left_out(orc):
    a = M.view_state(orc, "a", 509, 4096)
    small = M.fresh(orc, 509, 64)
    counts = M.merge(small, a)
    print(counts, small.counters[:T.VK_CTR_PUBLIC])
    # the first round fills main entries, the second runs the excess list and then the pool dry and is the last
    assert counts == (888, 457, 457, 431, 2, 0)
    assert small.counters[T.VK_CTR_DROPPED] == 185 and small.counters[T.VK_CTR_VOXEL_PTR] < -1
    assert small.counters[T.VK_CTR_EXCESS_PTR] > small.max              # upstream's pointer runs on (volume.cu:337)
    after, full = R.block_voxels(small), R.block_voxels(a)
    assert len(after) == 457 and all(after[origin] == full[origin] for origin in after)
    assert not small.allocation_types.any()
    # a destination that is exhausted already takes what it has blocks for and reports the rest
    b = M.view_state(orc, "b", 509, 4096)
    worn = M.view_state(orc, "a", 509, 64)
    held, dropped_before = R.block_voxels(worn), int(worn.counters[T.VK_CTR_DROPPED])
    considered, fused, allocated, left_out, rounds, _ = M.merge(worn, b)
    assert (considered, allocated, rounds) == (812, 0, 1) and fused + left_out == 812 and fused > 0 and left_out > 0
    assert int(worn.counters[T.VK_CTR_DROPPED]) > dropped_before
    assert set(R.block_voxels(worn)) == set(held)
    assert sum(1 for origin in R.block_voxels(b) if origin in held) == fused


def test_unobserved_blocks_can_stay_behind(orc):
    b = M.view_state(orc, "b", 509, 4096)
    unobserved = [i for i in M.source_blocks(b) if M.unobserved(b, i)]
    assert len(unobserved) >= 1
    everything, observed_only = M.fresh(orc, 1021, 2048), M.fresh(orc, 1021, 2048)
    all_counts = M.merge(everything, b)
    counts = M.merge(observed_only, b, M.SKIP_UNOBSERVED)
    assert counts[5] == len(unobserved) and counts[0] == 812 - len(unobserved) and counts[3] == 0
    assert counts[2] < all_counts[2]
    kept, full = R.block_voxels(observed_only), R.block_voxels(b)
    assert set(full) - set(kept) == {M.origin_of(b, i) for i in unobserved}
    assert all(kept[origin] == full[origin] for origin in kept)


def test_the_merged_volume_raycasts(orc):
    a, b = M.view_state(orc, "a", 509, 4096), M.view_state(orc, "b", 509, 4096)
    M.merge(a, b)
    depth, color, normals = R.continue_at(orc, a, 12)
    assert (depth > 0).sum() > 1000
    assert (color[depth > 0] > 0).any()


def test_entry_points_validate_their_arguments_without_a_device():
    import ctypes as C
    from vulcan_amd import api
    lib = api.lib()
    assert lib.vk_volume_merge(None, None, None, None, None, None) == -1
    assert lib.vk_volume_merge_workspace_bytes(0, 0) == 0
    assert lib.vk_volume_merge_workspace_bytes(509, 96) >= 605 * 5
    assert C.sizeof(T.MergeParams) == 16
    assert (T.VK_MERGE_SKIP_UNOBSERVED, T.VK_MERGE_CONTINUE) == (M.SKIP_UNOBSERVED, M.CONTINUE)
