"""The chains of tests/map_life.py on the CPU statements alone: they reach what they exist for. tests/test_gpu_map_life.py holds
the device to every step of them, so a chain that never pops a rebuilt free list, never reads a colour that color_rays wrote or
never runs its pool dry would make that file green for nothing. Every number below is a lower bound on what the statements
give (the measured value stands beside it), never the digits themselves."""
import pytest

import cast_reference as CR
import map_life as ML
from vulcan_amd import vk_types as T

_SUMMARIES = {}


def changing(run):
    """the records of the steps that change a volume, frame steps included, in order: [(index in the chain, record)]"""
    return [(i, record) for i, record in enumerate(run.records) if record.step.kind != ML.READ]


def reads_after(run, index):
    """{operation: [record]} of the read-only steps between step `index` and the next step that changes a volume"""
    out = {}
    for record in run.records[index + 1:]:
        if record.step.kind != ML.READ:
            break
        out.setdefault(record.step.facts["operation"], []).append(record)
    return out


def coloured(state):
    return int((state.written_voxels()["color_weight"] > 0).sum())


def test_ray_map_reaches_what_it_is_for(orc):
    run = ML.host_run(orc, ML.ray_map())
    steps = changing(run)
    names = [record.step.facts["operation"] for _, record in steps]
    assert names == ["integrate_rays", "color_rays", "integrate_rays", "color_rays"] + ["carve_rays"] * 6 + ["release_blocks", "integrate_rays",
                     "color_rays", "merge", "merge", "merge", "frame", "release_blocks"]
    for _, record in steps[:-1]:                                          # the last step is the repair alone: it releases nothing
        assert record.step.work(record.want), record.step

    # the release frees blocks that three carves of each fused quarter pushed to distance 1 (measured: 94), and chains
    # survive it
    at, release = steps[10]
    was, now = ML.before(run, at)["map"], release.after["map"]
    print("release", release.want)
    assert release.want[0] >= 50
    for k in (6, 9):
        assert steps[k][1].want[6] > 10000                                # voxels the third carve of a quarter updated
    freed = ML.slots_in_use(was) - ML.slots_in_use(now)
    assert len(freed) == release.want[0]
    entries = now.hash_entries
    heads = int(((entries["data"][:now.main] >= 0) & (entries["next"][:now.main] >= 0)).sum())
    print("main buckets that head a chain", heads)
    assert heads >= 100
    assert now.counters[T.VK_CTR_EXCESS_PTR] < was.counters[T.VK_CTR_EXCESS_PTR]
    assert now.counters[T.VK_CTR_VISIBLE] == 0 and now.counters[T.VK_CTR_BANDED] == -1

    # integrate_rays pops the rebuilt free list and appends behind the compacted chains (measured: 369 blocks)
    _, fused = steps[11]
    then = fused.after["map"]
    print("integrate_rays after the release", fused.want)
    assert fused.want[3] >= 100
    taken = ML.slots_in_use(then) - ML.slots_in_use(now)
    assert len(taken) == fused.want[3] and freed <= taken
    placed = ML.entries_in_use(then) - ML.entries_in_use(now)
    assert any(now.main <= index < was.counters[T.VK_CTR_EXCESS_PTR] for index in placed)

    # colour no camera wrote crosses both merges (measured: 46 933 voxels)
    at, merged = steps[13]
    source, target = ML.before(run, at)["map"], merged.after["other"]
    print("voxels with a colour", coloured(source), coloured(target))
    assert coloured(target) == coloured(source) > 10000 and coloured(ML.before(run, at)["other"]) == 0
    _, posed = steps[14]
    print("posed merge", posed.want)
    assert posed.want[3] > 100 and posed.want[5] >= 2 and posed.want[4] == 0           # measured: 819 blocks in 7 rounds
    assert coloured(posed.after["map"]) > coloured(source)

    # the camera goes on (measured: 17 231 pixels) and the mesh has colours (19 431 vertices)
    # the merge back takes one allocation round a call and more calls than one: VK_MERGE_CONTINUE is carried (measured: 3 calls)
    _, back = steps[15]
    calls = back.step.facts["calls"]
    print("merge back", back.want, "calls", calls)
    assert back.step.facts["max_rounds"] == 1 and len(calls) >= 2 and back.want[2] > 100
    assert all(call[4] == 1 and call[3] > 0 for call in calls[:-1]) and back.want[3] == 0
    assert back.want[4] == sum(call[4] for call in calls) and back.want[2] == sum(call[2] for call in calls)

    _, camera = steps[16]
    assert int((camera.want[0][0] > 0).sum()) > 10000 and not camera.want[1]
    last = reads_after(run, steps[17][0])
    statistics = last["extract"][0].step.facts["statistics"]
    print("mesh", statistics)
    assert statistics["color_both"] + statistics["color_one"] > 10000

    # every checkpoint reads something: colour at sampled points each time, hits and register terms where the map is dense
    assert not last["raycast"][0].want[0].any()                            # behind the release the visible list is empty
    for k in (3, 11, 14, 17):
        reads = reads_after(run, steps[k][0])
        assert set(reads) >= {"sample", "cast_rays", "extract", "score_poses", "register_rays"}
        scores, terms = reads["score_poses"][0], reads["register_rays"][0]
        print("residuals per pose", scores.want[0]["residuals"], "terms of register_rays", int(terms.want[0].sum()))
        assert scores.step.work(scores.want) and terms.step.work(terms.want)
        points, samples, gradients = reads["sample"][0].want
        print("checkpoint after", steps[k][1].step, "samples with a distance", int((samples["distance_weight"] != 0).sum()),
              "with a colour", int((samples["color_weight"] != 0).sum()), "hits",
              [int((record.want[0] == CR.HIT).sum()) for record in reads["cast_rays"]])
        assert (samples["distance_weight"] != 0).sum() > 500 and (samples["color_weight"] != 0).sum() > 100
        assert len(reads["extract"][0].want[0]) > 1000
    assert (last["sample"][0].want[2][:, 3] != 0).sum() > 1000
    assert max(int((record.want[0] == CR.HIT).sum()) for record in last["cast_rays"]) > 1000
    assert reads_after(run, steps[14][0])["register"][0].want[0].sum() > 1000


def test_exhausted_runs_dry_and_recovers(orc):
    run = ML.host_run(orc, ML.exhausted())
    steps = changing(run)
    assert run.start["map"].counters[T.VK_CTR_VOXEL_PTR] < 0
    first, release, again, colour = (record for _, record in steps[:4])
    print("first", first.want, "release", release.want, "again", again.want, "colour", colour.want)
    assert first.want[3] == 0 and first.want[7] > 10000                    # every request is dropped
    assert first.after["map"].counters[T.VK_CTR_DROPPED] > run.start["map"].counters[T.VK_CTR_DROPPED]
    assert release.want[0] > 100 and release.after["map"].counters[T.VK_CTR_VOXEL_PTR] > 0
    assert again.want[3] > 100                                              # measured: 217
    assert again.after["map"].counters[T.VK_CTR_DROPPED] > release.after["map"].counters[T.VK_CTR_DROPPED]    # and ends on a drop
    assert again.want[7] > 0 and colour.want[5] > 10000
    assert steps[5][1].step.work(steps[5][1].want)
    assert (run.records[-1].want[0] > 0).sum() > 1000                       # the raycast alone, with the bounds the frame step made


def test_the_pose_buffer_chain_does_something_with_every_pose(orc):
    run = ML.host_run(orc, ML.pose_buffer())
    for record in run.records:
        print(record.step, record.want)
        assert record.step.work(record.want), record.step
    fused, coloured_, carved = (record.want for record in run.records)
    assert fused[6] > 10000 and coloured_[5] > 1000 and carved[6] > 1000


def summary(orc, seed):
    """[(step, what the statement returned)] of the changing steps of random_chain(seed): the snapshots are not kept"""
    if seed not in _SUMMARIES:
        run = ML.host_run(orc, ML.random_chain(seed), keep=False)
        _SUMMARIES[seed] = [(record.step, record.want) for record in run.records]
    return [(step, want) for step, want in _SUMMARIES[seed] if step.kind != ML.READ]


def raycasts(orc, seed):
    """[(the operation before it, pixels with a depth)] of the raycasts alone of random_chain(seed)"""
    summary(orc, seed)
    steps = _SUMMARIES[seed]
    return [(steps[k - 1][0].facts["operation"], int((want[0] > 0).sum())) for k, (step, want) in enumerate(steps)
            if step.facts["operation"] == "raycast"]


def drawn(orc, seed):
    """the operations of the chain in order, the frame step each carries left out"""
    return [step for step, _ in summary(orc, seed) if step.kind == ML.MUTATE]


@pytest.mark.parametrize("seed", ML.SEEDS)
def test_no_step_of_a_random_chain_is_a_no_op(orc, seed):
    steps = summary(orc, seed)
    assert len(steps) == 16 and [step.kind for step, _ in steps] == [ML.MUTATE, ML.FRAME] * 8
    assert sum(1 for step, _ in steps if step.facts.get("posed")) <= 1
    for step, want in steps:
        print(step, want if step.kind == ML.MUTATE else int((want[0][0] > 0).sum()))
        assert step.work(want), step


def test_the_random_chains_cover_the_operations_and_their_orders(orc):
    assert len(ML.SEEDS) == 6
    chains = [drawn(orc, seed) for seed in ML.SEEDS]
    names = [[step.facts["operation"] for step in chain] for chain in chains]
    for operation in ML.OPERATIONS:
        count = sum(chain.count(operation) for chain in names)
        print(operation, count)
        assert count >= 3
    pairs = set()
    for chain in chains:
        for a, b in zip(chain, chain[1:]):
            pairs.add((a.facts["operation"], "allocates" if b.facts.get("allocates") else b.facts["operation"]))
            pairs.add((a.facts["operation"], b.facts["operation"]))
    print(sorted(pairs))
    assert ("release_blocks", "allocates") in pairs and ("color_rays", "merge") in pairs and ("carve_rays", "release_blocks") in pairs
    assert any(step.facts.get("posed") for chain in chains for step in chain)
    # the raycast alone: an image behind the operations that leave the visible list alone, none behind those that void it
    seen = [pair for seed in ML.SEEDS for pair in raycasts(orc, seed)]
    print(seen)
    for operation in ("color_rays", "carve_rays"):
        assert any(before == operation and pixels > 10000 for before, pixels in seen)
    for operation in ("integrate_rays", "release_blocks", "merge"):
        assert any(before == operation for before, _ in seen)
        assert all(pixels == 0 for before, pixels in seen if before == operation)


@pytest.mark.parametrize("seed", ML.SEEDS)
def test_a_random_chain_ends_on_scores_with_residuals(orc, seed):
    """the last read of a random chain: at one of the eight poses at least, more than 100 rays of quarter 2 are residuals"""
    summary(orc, seed)
    step, want = _SUMMARIES[seed][-1]
    print(step, want[0]["residuals"])
    assert step.facts["operation"] == "score_poses" and step.work(want)


def test_the_loops_of_the_class_layer_move_the_pose(orc):
    """the second statements of the two terms steps (Step.class_host): three Gauss-Newton steps each, on residuals"""
    run = ML.host_run(orc, ML.ray_map(), class_layer=True)
    loops = [record for record in run.records if record.step.class_host is not None]
    assert sorted(set(record.step.facts["operation"] for record in loops)) == ["register", "register_rays"]
    for record in loops:
        want = record.class_want
        print(record.step, want.steps, want.code, want.counts)
        assert want.steps == ML.LOOP_STEPS and want.counts[2] > 100       # the bar of the scores: more than 100 residuals
        assert bytes(want.pose) != bytes(record.step.facts["pose"]) or want.code == 1
