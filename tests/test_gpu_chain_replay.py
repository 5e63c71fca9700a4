"""The chains of tests/map_life.py through the C++ class layer (vulcan_amd/host, libvulcan.so): what a Vulcan user links. The
class layer keeps its own copy of the caller's side of every volume operation — fourteen cached buffers, one pose buffer,
VoidMadeAhead / EmptyVisibleList around the operations that move blocks, the VK_MERGE_CONTINUE loop, the Extractor's workspace,
a Tracer whose bounds the integrators make ahead — and its scenario programs start from a fresh volume and make a call or two.

A test takes the host run of a chain (map_life.host_run), writes it as files (tests/chain_files.py), starts ONE
vulcan_amd/host/bin/chain_replay on them, and compares what the program wrote with the CPU statements step by step: the counts
of every step that changes a volume, the images of the frame steps and of the raycasts alone, every array of sample, cast_rays,
extract and score_poses, bit for bit; behind every changing step and every checkpoint the state of the volumes, with the
comparisons tests/test_gpu_map_life.py makes on its device volumes; and Volume::GetVisibleBlocks().GetSize(). The two steps that
compare the terms of a registration stand for the loops the class exposes (Register, RegisterRays, three steps): steps, end
code and counts are the statement's (Step.class_host), the pose and its inverse are within 2e-5 per entry of it, the bound
tests/test_gpu_register.py and tests/test_gpu_register_rays.py hold the Python layer's loops to — the device adds the normal
system in float32 in its own order. "ones" and "noise": the program overwrites every workspace the objects hold before every
call (chain_replay.cpp)."""
import os
import subprocess
import time

import numpy as np
import pytest

import chain_files as CF
import map_life as ML
from gpu_support import assert_arrays_state
from vulcan_amd import vk_types as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "vulcan_amd", "host", "bin", "chain_replay")
POSE_BOUND = 2e-5
EMPTIES_THE_VISIBLE_LIST = ("integrate_rays", "release_blocks", "merge", "merge_posed", "merge_resampled", "pack_merge", "load")


def replay(directory, fill, exe=EXE, env=None):
    """one chain_replay on the files of `directory`: (exit status, what it printed); a timeout is an exit status of its own"""
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    try:
        done = subprocess.run([exe, directory, fill], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env)
    except subprocess.TimeoutExpired as expired:
        return "timeout", str(expired.stdout)
    return done.returncode, done.stdout


def as_bytes_of(got, want):
    """`got` read as the statement's dtype and shape where the bytes allow it: the comparison is of bytes"""
    want = np.ascontiguousarray(want)
    got = np.ascontiguousarray(got)
    if got.nbytes == want.nbytes and got.dtype != want.dtype:
        got = np.frombuffer(got.tobytes(), dtype=want.dtype)
    if got.size == want.size:
        got = got.reshape(want.shape)
    return got


def assert_returns(got, want):
    got = tuple(as_bytes_of(g, w) for g, w in zip(got, want))
    assert len(got) == len(want) and ML.same(got, tuple(want)), ML.first_difference(got, tuple(want))


def assert_loop(got, want):
    """Register / RegisterRays against the statement's loop"""
    print("loop", got["steps"], got["code"], got["counts"], "statement", want.steps, want.code, want.counts,
          "worst entry", float(np.abs(got["pose"].matrix() - want.pose.matrix()).max()))
    assert (got["steps"], got["code"]) == (want.steps, want.code)
    assert got["counts"] == tuple(want.counts)
    assert got["result"] == (want.steps, int(want.code == 1), int(want.code != T.VK_REGISTER_NO_OVERLAP), want.counts[2])
    assert np.abs(got["pose"].matrix() - want.pose.matrix()).max() <= POSE_BOUND
    assert np.abs(got["pose"].inverse_matrix() - want.pose.inverse_matrix()).max() <= POSE_BOUND


def assert_step(operation, record, got, fill):
    """what one line of the script returned against the record of the step it stands for"""
    step, want = record.step, record.want
    if step.kind == ML.MUTATE:
        counts = tuple(int(c) for c in got["counts"])
        expected = tuple(int(c) for c in want if not isinstance(c, np.ndarray))
        assert counts == expected, f"counts {counts} for {expected}"
        assert CF.SENTINEL not in counts
        if operation == "pack_merge":                                    # the pack itself, behind the six counts
            assert_returns(got["returns"], want[6:])
    elif operation == "frame":
        assert_returns(got["returns"], want[0])
    elif operation in ("sample", "distance_field"):                      # the points and the grid are the statement's own
        assert_returns(got["returns"], want[1:])
    elif operation in CF.LOOPS:
        assert_loop(got["loop"], record.class_want)
    else:
        assert operation in CF.RETURNS, operation
        assert_returns(got["returns"], want)


def compare(orc, run, directory, fill, again=None):
    """everything chain_replay wrote into `directory`/out against the run, step by step"""
    script = CF.parse(directory)
    written = CF.read(directory)
    restored = {}

    def host(name, state):
        if restored.get(name, (None, None))[0] is not state:
            restored[name] = (state, state.restore(orc))
        return restored[name][1]

    for index, operation, arguments in script:
        if operation == "second_volume":
            continue
        record = run.records[int(arguments.get("of", index))]
        try:
            assert_step(operation, record, written[index], fill)
            after = run.records[-1] if "of" in arguments else record
            for name, state in written[index]["states"].items():
                hv = host(name, after.after[name])
                assert_arrays_state(state, hv, after.defined[name])
                if operation in EMPTIES_THE_VISIBLE_LIST and name == record.step.on:
                    assert state["visible_size"] == 0, f"GetVisibleBlocks().GetSize() is {state['visible_size']}"
                if operation == "frame":
                    assert state["visible_size"] == hv.counters[T.VK_CTR_VISIBLE] > 0
            if "state" in arguments and arguments["state"] != "-":
                assert set(written[index]["states"]) == set(arguments["state"].split(","))
        except AssertionError as error:
            raise AssertionError(f"step {index} of {run.chain.name}, {record.step.name}{' (again)' if 'of' in arguments else ''}: {error}") from error


def directory_bytes(directory):
    return sum(os.path.getsize(os.path.join(folder, name)) for folder, _, names in os.walk(directory) for name in names)


def run_through_the_classes(orc, chain, fill, tmp_path, keep=True, again=None):
    began = time.time()
    run = ML.host_run(orc, chain, keep, class_layer=True)
    directory = str(tmp_path / "chain")
    CF.write(run, directory, fill, again=again)
    wrote = time.time()
    status, output = replay(directory, fill)
    replayed = time.time()
    assert status == 0, f"chain_replay ended with {status}:\n{output[-4000:]}"
    compare(orc, run, directory, fill, again)
    print(f"{chain.name}, {fill}: statements and files {wrote - began:.1f} s, chain_replay {replayed - wrote:.1f} s, "
          f"comparison {time.time() - replayed:.1f} s, directory {directory_bytes(directory) / 1e6:.0f} MB")
    return run


@pytest.mark.parametrize("fill", CF.FILLS)
def test_ray_map_through_the_classes(orc, tmp_path, fill):
    """... and behind the chain a second Volume object takes the map's eight buffers, device to device, and the last
    checkpoint is made again from it: an object that has made no call gives the statements' bytes too"""
    run = run_through_the_classes(orc, ML.ray_map(), fill, tmp_path, again="map")
    assert len(CF.last_checkpoint(run)) >= 3


def test_exhausted_through_the_classes(orc, tmp_path):
    run_through_the_classes(orc, ML.exhausted(), "noise", tmp_path)


def test_the_pose_buffer_through_the_classes(orc, tmp_path):
    """IntegrateRays through generic(), at once ColorRays with no pose, then CarveRays through another pose: PoseOnDevice
    uploads every host pose into the one buffer sample_pose_"""
    run_through_the_classes(orc, ML.pose_buffer(), "noise", tmp_path)


@pytest.mark.parametrize("seed", ML.SEEDS)
def test_random_chain_through_the_classes(orc, tmp_path, seed):
    run_through_the_classes(orc, ML.random_chain(seed), "noise", tmp_path, keep=False)


@pytest.mark.parametrize("fill", CF.FILLS)
def test_two_resolutions_through_the_classes(orc, tmp_path, fill):
    """MergeResampled, Pack + Merge(pack), PackedVolume::Save + Volume::Load and DistanceField as steps: the 16 mm map a
    resampled merge made lives on through the classes, DistanceField (const) resizes field_workspace_ for three grids in a
    row, and the object Volume::Load hands out takes the place of the fresh one and goes on: frame, repair, reads"""
    run_through_the_classes(orc, ML.two_resolutions(), fill, tmp_path)


def test_resampled_exhausted_through_the_classes(orc, tmp_path):
    run_through_the_classes(orc, ML.resampled_exhausted(), "noise", tmp_path)


@pytest.mark.parametrize("seed", ML.RESOLUTION_SEEDS)
def test_random_resolution_chain_through_the_classes(orc, tmp_path, seed):
    run_through_the_classes(orc, ML.random_resolution_chain(seed), "noise", tmp_path, keep=False)
