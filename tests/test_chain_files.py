"""tests/chain_files.py on the CPU: every chain of tests/map_life.py writes as files and parses back, every operation a script
names is one the class layer has a call for, the same run writes the same bytes twice, and the files of a start volume restore
the HostVolume the chain starts from."""
import hashlib
import os

import numpy as np
import pytest

import chain_files as CF
import map_life as ML

CHAINS = [ML.ray_map, ML.exhausted, ML.pose_buffer] + [lambda seed=seed: ML.random_chain(seed) for seed in ML.SEEDS]
IDS = ["ray_map", "exhausted", "pose_buffer"] + [f"random_chain({seed})" for seed in ML.SEEDS]
CHAINS += [ML.two_resolutions, ML.resampled_exhausted] + [lambda seed=seed: ML.random_resolution_chain(seed) for seed in ML.RESOLUTION_SEEDS]
IDS += ["two_resolutions", "resampled_exhausted"] + [f"random_resolution_chain({seed})" for seed in ML.RESOLUTION_SEEDS]


def digest(directory):
    out = hashlib.sha256()
    for name in sorted(os.listdir(directory)):
        out.update(name.encode())
        with open(os.path.join(directory, name), "rb") as data:
            out.update(data.read())
    return out.hexdigest()


@pytest.mark.parametrize("make", CHAINS, ids=IDS)
def test_a_chain_writes_and_parses_back(orc, tmp_path, make):
    chain = make()
    run = ML.host_run(orc, chain, keep=not chain.name.startswith("random"))
    again = "map" if chain.name == "ray_map" else None
    CF.write(run, str(tmp_path / "a"), "noise", again=again)
    script = CF.parse(str(tmp_path / "a"))
    assert [index for index, _, _ in script] == list(range(len(script)))
    assert len(script) == len(run.records) + (1 + len(CF.last_checkpoint(run)) if again else 0)
    for (index, operation, arguments), record in zip(script, run.records):
        assert operation in CF.CALLS and operation == CF.operation_of(record.step), (index, operation)
        assert arguments["on"] in run.start
        for key, value in arguments.items():
            if value.endswith(".bin"):
                assert os.path.getsize(tmp_path / "a" / value) > 0, (index, key, value)
        if record.step.kind == ML.MUTATE:
            assert arguments["on"] == record.step.on and record.step.on in arguments["state"].split(",")
    for index, operation, arguments in script[len(run.records):]:
        assert operation in CF.CALLS
    # the floats are the statements' bytes
    for index, operation, arguments in script:
        if operation == "integrate_rays":
            facts = run.records[index].step.facts
            assert CF.from_hex32(arguments["r_max"]).tobytes() == np.float32(facts["r_max"]).tobytes()
            assert CF.from_hex32(arguments["cap"]) == np.float32(facts["cap"])
            assert (arguments["pose"] == "-") == (facts["pose"] is None)
            if facts["pose"] is not None:
                assert open(tmp_path / "a" / arguments["pose"], "rb").read() == bytes(facts["pose"])
        if operation == "merge_resampled":
            facts = run.records[index].step.facts
            assert int(arguments["supersample"]) == facts["supersample"] and int(arguments["max_rounds"]) == facts["max_rounds"]
            assert open(tmp_path / "a" / arguments["pose"], "rb").read() == bytes(facts["pose"])
        if operation == "distance_field":
            origin, dims = run.records[index].step.facts["grid"]
            assert tuple(int(v) for v in arguments["origin"].split(",")) == origin and tuple(int(v) for v in arguments["dims"].split(",")) == dims
            assert all(o % int(arguments["stride"]) == 0 for o in origin)
        if operation == "pack_merge":
            assert int(arguments["packed"]) == len(run.records[index].want[6]) > 0
    # twice: the same bytes
    CF.write(run, str(tmp_path / "b"), "noise", again=again)
    assert digest(str(tmp_path / "a")) == digest(str(tmp_path / "b"))
    # the start volumes come back
    restored = CF.start_volumes(str(tmp_path / "a"), orc)
    assert sorted(restored) == sorted(run.start)
    for name, state in run.start.items():
        want, got = state.restore(orc), restored[name]
        assert (got.main, got.excess) == (want.main, want.excess)
        assert np.float32(got.voxel_length) == np.float32(want.voxel_length)
        assert np.float32(got.truncation_length) == np.float32(want.truncation_length)
        assert tuple(np.float32(got.depth_range)) == tuple(np.float32(want.depth_range))
        for buffer in CF.BUFFERS:
            assert getattr(got, buffer).tobytes() == getattr(want, buffer).tobytes(), (name, buffer)
        again_state = ML.Snapshot(orc, got)
        assert np.array_equal(again_state.written, state.written) and again_state.blocks.tobytes() == state.blocks.tobytes()


def test_the_states_written_are_those_the_python_chain_compares(orc):
    run = ML.host_run(orc, ML.ray_map())
    states = CF.states_after(run)
    for record, names in zip(run.records, states):
        if record.step.kind != ML.READ:
            assert record.step.on in names
    assert sum(1 for names in states if names) == sum(1 for r in run.records if r.step.kind != ML.READ) + 4      # four checkpoints
    assert any("other" in names and "map" in names for names in states)                                           # register_terms reads both
