"""The chains of tests/map_life.py on the CPU statements alone: they reach what they exist for. tests/test_gpu_map_life.py holds
the device to every step of them, so a chain that never pops a rebuilt free list, never reads a colour that color_rays wrote or
never runs its pool dry would make that file green for nothing. Every number below is a lower bound on what the statements
give (the measured value stands beside it), never the digits themselves."""
import numpy as np
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


# ---- the chains over two lattices ----------------------------------------------------------------------------------------

def steps_of(run, operation):
    return [(index, record) for index, record in enumerate(run.records) if record.step.facts["operation"] == operation]


def carved(state):
    """voxels that carve_rays pushed to distance 1 and that keep a weight"""
    voxels = state.written_voxels()
    return int(((voxels["distance"] == 1) & (voxels["distance_weight"] > 0)).sum())


def assert_fields_have_all_classes(run):
    fields = steps_of(run, "distance_field")
    for _, record in fields:
        classes = record.want[1]
        print(record.step, [int((classes == c).sum()) for c in (ML.DF.UNKNOWN, ML.DF.FREE, ML.DF.OCCUPIED)])
        assert all((classes == c).any() for c in (ML.DF.UNKNOWN, ML.DF.FREE, ML.DF.OCCUPIED)), record.step
        # (with every class a site no cell has a distance to measure: the one read that is all zeros and -inf by definition)
        assert record.step.work(record.want) or record.step.facts["sites"] == 7, record.step
    return fields


def test_two_resolutions_reaches_what_it_is_for(orc):
    run = ML.host_run(orc, ML.two_resolutions())
    for index, record in changing(run):
        if record.step.facts.get("rule") != "repair":
            assert record.step.work(record.want), record.step

    # the resampled merge samples a source that has lived: carved voxels (measured: 56 529), colour that color_rays wrote
    # where the camera wrote none, a table a release compacted — and the colour arrives
    (at, down), _, (second_at, second), (up_at, up) = steps_of(run, "merge_resampled")
    fine, was, coarse = ML.before(run, at)["fine"], ML.before(run, at)["coarse"], down.after["coarse"]
    release = run.records[at - 1]
    rays = run.records[0]
    print("fine: carved", carved(fine), "coloured", coloured(fine), "by color_rays", rays.want, "release", release.want)
    assert release.step.facts["operation"] == "release_blocks" and release.want[0] > 100
    # colour from rays, in a band of two voxels and not the truncation band the camera's colour lies in
    assert rays.step.facts["operation"] == "color_rays" and rays.step.facts["band"] == 2.0 and rays.want[5] > 5000       # voxels (measured: 19 758)
    assert rays.after["fine"].written_voxels()["color"].tobytes() != run.start["fine"].written_voxels()["color"].tobytes()
    assert carved(fine) > 10000 and coloured(fine) > 10000
    print("down", down.want, "coloured", coloured(coarse))
    assert not ML.entries_in_use(was) and down.want[7] > 5000 and coloured(coarse) > 1000
    assert coarse.counters[T.VK_CTR_VISIBLE] == 0 and coarse.counters[T.VK_CTR_BANDED] == -1
    assert run.records[at + 1].step.facts["operation"] == "raycast" and not run.records[at + 1].want[0].any()
    camera = run.records[at + 2]
    assert camera.step.kind == ML.FRAME and int((camera.want[0][0] > 0).sum()) > 10000

    # two ratios into one destination, from sources of one table size: the workspaces differ in K alone, the larger K second
    a, b, into = ML.before(run, second_at)["mid"], ML.before(run, up_at)["coarse"], second.after["back"]
    boxes = [ML.MR.box_blocks(np.float32(source.shape[2]) / np.float32(into.shape[2])) for source in (a, b)]
    print("into back", second.want, "K", boxes)
    assert second.step.on == up.step.on == "back" and (a.main, a.excess) == (b.main, b.excess) and boxes[0] < boxes[1]
    assert second.want[3] > 50 and up.want[2] - up.want[3] > 50          # the second merge also fuses into blocks the first made

    # back, one round a call: more calls than one (measured: 3), from a source that was carved and released on its lattice
    calls = up.step.facts["calls"]
    source = ML.before(run, up_at)["coarse"]
    print("up", up.want, "calls", calls, "coarse: carved", carved(source))
    assert up.step.facts["max_rounds"] == 1 and len(calls) >= 2 and carved(source) > 1000
    assert all(call[5] == 1 and call[4] > 0 for call in calls[:-1]) and up.want[4] == 0
    assert up.want[2] == sum(call[2] for call in calls) and up.want[7] == sum(call[7] for call in calls)
    posed = run.records[up_at + 1]
    assert posed.step.facts["operation"] == "merge" and posed.step.facts["posed"] and posed.want[3] > 100     # measured: 210 new blocks

    # the pack of the released map is smaller than the pool's high-water mark, the loaded map is the map, and it goes on living
    (at, loaded), = steps_of(run, "load")
    source = ML.before(run, at)["coarse"]
    high_water = max(len(ML.slots_in_use(record.after["coarse"])) for record in run.records[:at])
    print("load", loaded.want, loaded.step.facts["packed"], "high-water mark", high_water)
    assert loaded.step.facts["packed"][2] == len(ML.slots_in_use(source)) < high_water
    a, b = ML.MP.cloud(loaded.after["loaded"].restore(orc)), ML.MP.cloud(source.restore(orc))
    order_a, order_b = (np.lexsort(c[0].T) for c in (a, b))
    assert (a[0][order_a] == b[0][order_b]).all() and a[1][order_a].tobytes() == b[1][order_b].tobytes()
    assert (loaded.after["loaded"].main, loaded.after["loaded"].excess) != (source.main, source.excess)
    assert run.records[at + 1].step.kind == ML.FRAME and run.records[at + 1].step.work(run.records[at + 1].want)

    # the pack under a rule leaves blocks out (measured: 86 of 226) and lands in a destination that has lived
    (at, packed), = steps_of(run, "pack_merge")
    counts = packed.step.facts["packed"]
    print("pack_merge", packed.want[:6], counts)
    assert 0 < counts[1] < counts[0] and packed.want[1] == counts[2] and packed.want[2] > 0 and 0 < packed.want[1] - packed.want[2]
    assert len(packed.want[6]) == counts[2] and len(packed.want[7]) == 512 * counts[2]

    # the clearance field: three grids in a row (one, another shape, the first again), then behind a carve, a frame step, a load
    fields = assert_fields_have_all_classes(run)
    shapes = [record.want[1].shape for _, record in fields]
    assert len(fields) == 7 and shapes[0] == shapes[2] != shapes[1]
    assert [record.step.facts["sites"] for _, record in fields[3:5]] == [7, ML.DF.OCCUPIED]
    assert all(record.step.facts["signed"] for _, record in fields[3:5])
    assert not np.isfinite(fields[3][1].want[3].view(np.float32)).any()


def test_resampled_exhausted_drops_then_recovers(orc):
    run = ML.host_run(orc, ML.resampled_exhausted())
    (at, dry), (_, fits) = steps_of(run, "merge_resampled")
    was, now = ML.before(run, at)["coarse"], dry.after["coarse"]
    calls = dry.step.facts["calls"]
    print("dry", dry.want, "calls", calls)
    assert (was.main, was.excess) == (509, 16)
    assert dry.want[4] > 10 and len(calls) == 1                              # measured: 38 left out; a call that dropped is not continued
    assert now.counters[T.VK_CTR_DROPPED] > was.counters[T.VK_CTR_DROPPED]
    repair = run.records[at + 1]
    assert repair.step.facts["rule"] == "repair" and repair.want[0] == 0
    (_, packed), = steps_of(run, "pack_merge")
    print("pack_merge", packed.want[:6], packed.step.facts["packed"])
    assert packed.want[1] == packed.step.facts["packed"][2] >= 20 and packed.want[3] == 0        # the box fits: none left out
    for record in run.records[-3:]:
        assert record.step.work(record.want), record.step
    assert [record.step.facts["operation"] for record in run.records[-3:]] == ["frame", "raycast", "distance_field"]
    assert_fields_have_all_classes(run)


NEW = ("merge_resampled", "pack_merge", "load")


def resolution_summary(orc, seed):
    """[(step, what the statement returned)] of random_resolution_chain(seed), every step; the snapshots are not kept"""
    key = ("resolution", seed)
    if key not in _SUMMARIES:
        run = ML.host_run(orc, ML.random_resolution_chain(seed), keep=False)
        _SUMMARIES[key] = [(record.step, record.want) for record in run.records]
    return _SUMMARIES[key]


def behind(steps):
    """{(new operation, "release" | "frame")}: the operation ran on a volume — the one it changes or the one it reads —
    whose last changing step was a frame step, or whose last drawn operation, the frame step behind it aside, was a release.
    The release that cuts a resampled merge's source (facts["cut"]) stands in front of every one of them by construction
    and does not count"""
    last_mutate, last_change, out = {}, {}, set()
    for step in steps:
        if step.kind == ML.READ:
            continue
        operation = step.facts["operation"]
        if operation in NEW:
            for name in (step.on,) + step.reads:
                if last_mutate.get(name) == "release_blocks":
                    out.add((operation, "release"))
                if last_change.get(name) == "frame":
                    out.add((operation, "frame"))
        if step.facts.get("cut"):
            continue
        if step.kind == ML.MUTATE:
            last_mutate[step.on] = operation
        last_change[step.on] = operation
    return out


@pytest.mark.parametrize("seed", ML.RESOLUTION_SEEDS)
def test_no_step_of_a_random_resolution_chain_is_a_no_op(orc, seed):
    steps = resolution_summary(orc, seed)
    drawn = [(step, want) for step, want in steps if step.kind != ML.READ and not step.facts.get("cut")]
    assert len(drawn) == 16 and [step.kind for step, _ in drawn] == [ML.MUTATE, ML.FRAME] * 8
    assert all(frame.on == step.on for (step, _), (frame, _) in zip(drawn[0::2], drawn[1::2]))
    for step, want in steps:
        if step.kind == ML.MUTATE:
            print(step, tuple(part for part in want if not isinstance(part, np.ndarray)))
        if step.facts["operation"] != "raycast":
            assert step.work(want), step
    # the raycast alone: behind the new operations, which move blocks, what was made ahead is void and the image is empty
    alone = [(steps[k - 1][0].facts["operation"], int((want[0] > 0).sum())) for k, (step, want) in enumerate(steps)
             if step.facts["operation"] == "raycast"]
    print(alone)
    assert all(pixels == 0 for operation, pixels in alone if operation in NEW + ("integrate_rays", "release_blocks", "merge"))
    assert [step.facts["operation"] for step, _ in steps[-4:]] == ["sample", "cast_rays", "score_poses", "distance_field"]


def test_the_random_resolution_chains_cover_the_new_operations(orc):
    assert len(ML.RESOLUTION_SEEDS) >= 4
    seen = set()
    for seed in ML.RESOLUTION_SEEDS:
        chain = ML.random_resolution_chain(seed)
        seen |= behind(chain.steps)
    print(sorted(seen))
    assert seen == {(operation, what) for operation in NEW for what in ("release", "frame")}
    # and a raycast alone stands behind each of them, on a volume whose Tracer holds bounds an earlier frame step made ahead
    # (behind a load the volume is a new object: there the bounds are its predecessor's, which the step lets go)
    behind_new = set()
    for seed in ML.RESOLUTION_SEEDS:
        steps = ML.random_resolution_chain(seed).steps
        behind_new |= {a.facts["operation"] for a, b in zip(steps, steps[1:]) if b.facts["operation"] == "raycast"}
    print(sorted(behind_new))
    assert behind_new >= {"merge_resampled", "pack_merge"}


def test_the_old_random_chains_draw_what_they_drew(orc):
    """random_resolution_chain stands beside random_chain: the old generator's operations and seeds are as they were"""
    assert ML.OPERATIONS == ("integrate_rays", "color_rays", "carve_rays", "release_blocks", "merge") and ML.SEEDS == (1, 8, 9, 12, 15, 17)
    assert ML.RESOLUTION_OPERATIONS[:5] == ML.OPERATIONS and set(ML.RESOLUTION_OPERATIONS[5:]) == set(NEW)
