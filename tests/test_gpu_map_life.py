"""The chains of tests/map_life.py on the device: one api.Volume per volume of a chain, uploaded once, then every operation
starts from what the operation before it left there — the pool a release rebuilt, colour that color_rays wrote, voxels that
carve_rays pushed to distance 1, VK_CTR_VISIBLE = 0 and VK_CTR_BANDED = -1, an exhausted pool, and whatever api.Volume keeps
between calls. After every step that changes a volume the device holds the counts and the state the CPU statements leave
(tests/test_map_life.py shows what the chains reach); at every checkpoint the read-only operations return the statements'
bytes and leave the volumes alone. Every comparison is bit for bit, as in the per-operation files the statements come from.

`workspaces`: vk.h lets a caller hand every volume operation a workspace that is not initialised, and the Python layer does
(torch.empty). A new process mostly gets zeroed pages, so "ones" and "noise" overwrite every workspace, counts tensor and pose
buffer the objects hold before every call — the call's own workspace included, created first as the call will ask for it.
Between a merge call and the VK_MERGE_CONTINUE call that follows it the workspace is carried state (vk.h); Volume.merge makes
both calls itself, so nothing is overwritten in between."""
import numpy as np
import pytest

import map_life as ML
from gpu_support import api, assert_arrays_state, device_copy, state_arrays, sync  # noqa: F401

pytestmark = pytest.mark.gpu

WORKSPACES = ["as-allocated", "ones", "noise"]
SENTINEL = 0x5A5A5A5A
NEW_OPERATIONS = ("merge_resampled", "pack_merge", "load", "distance_field")
NEW_WORKSPACES = {"merge_resampled", "pack", "merge_packed", "distance_field"}      # their keys of Volume._workspaces
BUFFERS = ("voxels", "hash_entries", "free_voxel_blocks", "allocation_types", "allocation_blocks", "block_visibility", "visible_blocks",
           "counters")


def held_tensors(side):
    """(every workspace and buffer the objects keep between calls, every cached counts tensor)"""
    workspaces, counts = [], []
    for dv in side.volumes.values():
        for _, workspace, count in dv._workspaces.values():
            workspaces.append(workspace)
            counts.append(count)
        if dv._sample_pose is not None:
            workspaces.append(dv._sample_pose)
        # (the workspaces and counts of register_rays and score_poses are among dv._workspaces; the scores are a new tensor
        # every call)
        for buffers in (dv._register_buffers, dv._register_rays_buffers):
            if buffers is not None:
                workspaces += [buffers[name] for name in ("pose", "system", "state", "update")]
    for ex in side.extractors():
        workspaces.append(ex.workspace)
        counts.append(ex.counts)
    return workspaces, counts


def overwrite_held(side, how, generator):
    import torch
    workspaces, counts = held_tensors(side)
    for tensor in workspaces:
        raw = tensor.view(torch.uint8)
        if how == "ones":
            raw.fill_(0xFF)
        else:
            raw.random_(0, 256, generator=generator)
    for tensor in counts:
        tensor.fill_(SENTINEL)


def assert_state(dv, hv, defined):
    """the device holds the host's state (assert_arrays_state)"""
    sync()
    assert_arrays_state(state_arrays(dv), hv, defined)


def run_on_device(api, orc, chain, workspaces="as-allocated", keep=True):
    """the whole chain once: (the device side as the chain leaves it, the host run)"""
    import torch
    run = ML.host_run(orc, chain, keep)
    side = ML.DeviceSide(api, {name: device_copy(api, state.restore(orc)) for name, state in run.start.items()})
    generator = torch.Generator(device="cuda")
    generator.manual_seed(20)
    restored, read = {}, set()

    def host(name, state):
        if restored.get(name, (None, None))[0] is not state:
            restored[name] = (state, state.restore(orc))
        return restored[name][1]

    for index, record in enumerate(run.records):
        step = record.step
        try:
            if workspaces != "as-allocated" and step.kind != ML.FRAME:
                step.workspace(side)
                overwrite_held(side, workspaces, generator)
            held = {name: (dv, dict(dv._workspaces)) for name, dv in side.volumes.items()}
            got = step.device(orc, side, record.want)
            sync()
            if workspaces != "as-allocated" and step.facts["operation"] in NEW_OPERATIONS:
                # the call used the workspaces step.workspace() made and overwrite_held dirtied: it allocated none of them again
                for name, (dv, before) in held.items():
                    for operation in NEW_WORKSPACES & set(before):
                        assert dv._workspaces[operation] is before[operation], f"{name}: a new {operation} workspace"
            assert ML.same(got, record.want), ML.first_difference(got, record.want)
            if workspaces != "as-allocated" and step.kind == ML.MUTATE:          # the counts came from the call, not from the sentinel
                assert SENTINEL not in [part for part in got if not isinstance(part, np.ndarray)]
            # the state: behind every step that changes a volume, and behind the last read of a checkpoint
            read |= set(step.reads)
            last_read = step.kind == ML.READ and (index + 1 == len(run.records) or run.records[index + 1].step.kind != ML.READ)
            if step.kind != ML.READ or last_read:
                for name in sorted(read | ({step.on} if step.on else set())):
                    assert_state(side.volumes[name], host(name, record.after[name]), record.defined[name])
                read = set()
        except AssertionError as error:
            raise AssertionError(f"step {index} of {chain.name}, {step.name}: {error}") from error
    return side, run


@pytest.mark.parametrize("workspaces", WORKSPACES)
def test_ray_map_chain(api, orc, workspaces):
    run_on_device(api, orc, ML.ray_map(), workspaces)


@pytest.mark.parametrize("workspaces", WORKSPACES)
def test_exhausted_chain(api, orc, workspaces):
    run_on_device(api, orc, ML.exhausted(), workspaces)


@pytest.mark.parametrize("seed", ML.SEEDS)
def test_random_chain(api, orc, seed):
    run_on_device(api, orc, ML.random_chain(seed), "noise", keep=False)


def cached_workspaces(side):
    """the operations whose workspace some volume of the side holds: held_tensors overwrites exactly these"""
    return set(operation for dv in side.volumes.values() for operation in dv._workspaces)


@pytest.mark.parametrize("workspaces", WORKSPACES)
def test_two_resolutions_chain(api, orc, workspaces):
    side, _ = run_on_device(api, orc, ML.two_resolutions(), workspaces)
    assert cached_workspaces(side) >= NEW_WORKSPACES


@pytest.mark.parametrize("workspaces", WORKSPACES)
def test_resampled_exhausted_chain(api, orc, workspaces):
    side, _ = run_on_device(api, orc, ML.resampled_exhausted(), workspaces)
    assert cached_workspaces(side) >= NEW_WORKSPACES


@pytest.mark.parametrize("seed", ML.RESOLUTION_SEEDS)
def test_random_resolution_chain(api, orc, seed):
    run_on_device(api, orc, ML.random_resolution_chain(seed), "noise", keep=False)


def second_object_sees_the_same_map(api, orc, chain, name):
    """after `chain` its volume `name` is downloaded and uploaded into a new api.Volume: the last checkpoint again, from an
    object that has made no call — nothing the operations need lives only in the first object's caches"""
    side, run = run_on_device(api, orc, chain)
    sync()
    first = side.volumes[name]
    hv = run.records[-1].after[name].restore(orc)
    for buffer in BUFFERS:
        array = getattr(first, buffer).cpu().numpy()
        getattr(hv, buffer)[:] = np.frombuffer(array.tobytes(), dtype=getattr(hv, buffer).dtype)
    second = device_copy(api, hv)
    assert second._workspaces == {} and second._sample_pose is None and second._register_buffers is None
    again = ML.DeviceSide(api, dict(side.volumes, **{name: second}))
    at = max(index for index, record in enumerate(run.records) if record.step.kind != ML.READ)
    assert len(run.records) - at - 1 >= 3
    for record in run.records[at + 1:]:
        got = record.step.device(orc, again, record.want)
        sync()
        assert ML.same(got, record.want), f"{record.step.name}: {ML.first_difference(got, record.want)}"
    for buffer in BUFFERS:
        assert getattr(second, buffer).cpu().numpy().tobytes() == getattr(first, buffer).cpu().numpy().tobytes(), buffer
    assert_state(second, run.records[-1].after[name].restore(orc), run.records[-1].defined[name])


def test_a_second_volume_object_sees_the_same_map(api, orc):
    """ray_map's map (second_object_sees_the_same_map)"""
    second_object_sees_the_same_map(api, orc, ML.ray_map(), "map")


def test_a_second_volume_object_sees_the_same_coarse_map(api, orc):
    """two_resolutions' 16 mm map, which a resampled merge made and a pack went into: its last checkpoint, the clearance
    field included, from an object with no cached workspace"""
    second_object_sees_the_same_map(api, orc, ML.two_resolutions(), "coarse")


@pytest.mark.parametrize("workspaces", ["as-allocated", "noise"])
def test_the_device_pose_buffer_is_not_shared_across_a_call(api, orc, workspaces):
    """integrate_rays through generic(), at once color_rays with no pose, then carve_rays through another pose, on one
    volume: the Python layer uploads every host pose into the one buffer Volume._sample_pose"""
    side, run = run_on_device(api, orc, ML.pose_buffer(), workspaces)
    assert side.volumes["map"]._sample_pose is not None
    assert [record.step.facts["operation"] for record in run.records] == ["integrate_rays", "color_rays", "carve_rays"]
