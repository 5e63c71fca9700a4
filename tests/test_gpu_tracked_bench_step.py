"""bench.FrameLoop("rgbd-icp") — the step `bench.py --workload rgbd-icp` times, in the forms it times by default — against
the CPU oracle. The step composes vk_icp_pyramid_track_frame (the frame's normals and the key frame's deferred normals ride
in the pyramid launch), vk_volume_set_view_at_device_pose (enqueued behind the Track, at the pose the tracker leaves in
device memory, before the host has it), vk_integrate_ahead, vk_trace_ahead(normals = NULL) and vk_track_wait. Every pair
of its call forms has an equality test (tests/test_gpu_round6.py); tests/test_gpu_closed_loop.py holds the api.* wrapper
calls to the oracle's loop. This module holds the composed step itself to the oracle: nothing here is compared with another
device run.

Four frames at 640x480, the motion of test_closed_loop_at_the_benchmark_size (room poses 30, 32, 34, 36):
  * the oracle led through the DEVICE's tracked poses (each given as its 128 bytes) reproduces every raycast image, the
    key frame's normals, the raycast bounds, the frame's normal image and the visible count of every frame, and at the
    end the hash table and every voxel byte — bit for bit;
  * every Track, made again by the oracle from that same state (the oracle's raycast at the device's previous pose, which
    the first item has shown to be the device's key frame), lands within 2e-5 per entry of the device's pose;
  * the oracle's own closed loop, its tracked pose fed forward, stays within 2e-5 of FrameLoop's at every frame.
2e-5 is the bound of tests/test_gpu_closed_loop.py for these two comparisons (measured there: 3e-7)."""
import numpy as np
import pytest

import scenes
from closed_loop_oracle import POSE_ATOL, oracle_loop
from gpu_support import api, assert_volume_equal, pin_bench_defaults, sync  # noqa: F401
from vulcan_amd import vk_types as T

pytestmark = pytest.mark.gpu

def pose_distance(a, b):
    """largest |a - b| over the entries of the matrix and of the inverse matrix"""
    return float(max(np.abs(a.matrix() - b.matrix()).max(), np.abs(a.inverse_matrix() - b.inverse_matrix()).max()))


def test_tracked_bench_step_matches_the_oracle(api, orc, monkeypatch):
    """Key-frame normals: there is ONE key buffer and the raycast of frame i leaves its normal image to Track i + 1, so the
    normals of raycast i are read behind begin(i + 1) — the Track and the early SetView enqueued, by a copy on the same
    stream, no host synchronisation — and before finish(i + 1), whose raycast writes the depth they belong to anew (and, in
    the last frame, the normals as well: that raycast has no Track behind it and writes its own, which are read directly).
    step(i) is begin(i) + finish(i)."""
    import torch
    bench = pin_bench_defaults(monkeypatch)
    count = 4
    k = T.Projection.make(*scenes.APP_INTRINSICS)
    truth = [scenes.room_pose(30 + 2 * i) for i in range(count)]
    inputs = [scenes.room_frame(k, p, bench.W, bench.H, light=bench.LIGHT) for p in truth]
    light = T.Light.make(*bench.LIGHT)
    seq = bench.RoomSequence.__new__(bench.RoomSequence)
    seq.truth = truth
    seq.depth = [torch.from_numpy(d).cuda() for d, _ in inputs]
    seq.color = [torch.from_numpy(c).cuda() for _, c in inputs]
    sync()

    # ---- the device: the bench's own step
    loop = bench.FrameLoop("rgbd-icp", seq.truth, sequence=seq)
    assert loop.set_view_early and loop.built is None and loop.early is None
    vol, tracer = loop.vols[0]["vol"], loop.vols[0]["tracer"]
    device = []
    for i in range(count):
        loop.begin(i)
        if i > 0:
            assert loop.set_view_done, "SetView was not enqueued behind the Track"
            device[i - 1]["key_normals"] = loop.key.normals.clone()
        loop.finish(i)
        sync()
        assert loop.key_normals_pending == (i + 1 < count)
        ctr = vol.read_counters()
        device.append(dict(pose=bytes(loop.tracked_poses[i]), depth=loop.key.depth.clone(), color=loop.key.color.clone(),
                           frame_normals=loop.frame.normals.clone(), bounds=tracer.bounds.clone(),
                           visible=int(ctr[T.VK_CTR_VISIBLE]), voxel_pointer=int(ctr[T.VK_CTR_VOXEL_PTR]),
                           dropped=int(ctr[T.VK_CTR_DROPPED]), state=int(loop.tracker.tracker.state.cpu()[1])))
    device[-1]["key_normals"] = loop.key.normals.clone()
    sync()
    gn_steps = list(loop.gn_steps)
    assert len(loop.tracked_poses) == count and len(gn_steps) == count - 1
    assert all(len(d["pose"]) == 128 for d in device)
    poses = [T.Transform.from_buffer_copy(d["pose"]) for d in device]
    assert device[0]["pose"] == bytes(truth[0])                      # the first frame defines the map

    # ---- the oracle, led through the device's poses: bit for bit
    orc.set_threads(16)
    hv, led = oracle_loop(orc, k, inputs, light, poses[0], poses=poses,
                          volume=(bench.MAIN, bench.EXCESS, bench.VOXEL, bench.TRUNC))
    for i, (got, want) in enumerate(zip(device, led)):
        assert bytes(want["pose"]) == got["pose"]
        assert np.array_equal(got["depth"].cpu().numpy(), want["depth"]), f"frame {i}: raycast depth"
        assert np.array_equal(got["color"].cpu().numpy(), want["color"]), f"frame {i}: raycast colour"
        assert np.array_equal(got["key_normals"].cpu().numpy(), want["normals"], equal_nan=True), f"frame {i}: key normals"
        assert np.array_equal(got["bounds"].cpu().numpy(), want["bounds"]), f"frame {i}: raycast bounds"
        assert np.array_equal(got["frame_normals"].cpu().numpy(), want["frame_normals"], equal_nan=True), f"frame {i}: frame normals"
        assert got["visible"] == want["visible"] > 3000, f"frame {i}: visible count"
        assert got["dropped"] == 0, f"frame {i}: dropped requests"
        assert (want["depth"] > 0).sum() > 100000, f"frame {i}: the raycast hit nothing"
    assert device[-1]["voxel_pointer"] == int(hv.counters[T.VK_CTR_VOXEL_PTR])
    assert_volume_equal(vol, hv)

    # ---- every Track again, by the oracle, from the same state: the key frame is the oracle's raycast at the device's
    # previous pose (just shown to be the device's), the frame starts at that pose
    single = [pose_distance(poses[0], truth[0])]                      # (frame 0 is not tracked: its pose is given)
    for i in range(1, count):
        hf = orc.HostFrame(inputs[i][0], k, poses[i - 1], color=inputs[i][1])
        hf.compute_normals()
        want, _ = orc.pyramid_track(led[i - 1]["key"], hf)
        single.append(pose_distance(poses[i], want))
    print("   one Track from the same state, max |device - oracle| per frame (matrix and inverse): "
          + ", ".join(f"{d:.1e}" for d in single))

    # ---- the free-running loops: the oracle's own closed loop on the same inputs
    _, free = oracle_loop(orc, k, inputs, light, truth[0], track=lambda key, hf: orc.pyramid_track(key, hf)[0],
                          volume=(bench.MAIN, bench.EXCESS, bench.VOXEL, bench.TRUNC))
    orc.set_threads(1)
    running = [pose_distance(poses[i], free[i]["pose"]) for i in range(count)]
    print("   free-running loops, max |device - oracle| per frame (matrix and inverse): " + ", ".join(f"{d:.1e}" for d in running))
    assert max(single) <= POSE_ATOL
    for i in range(count):
        np.testing.assert_allclose(poses[i].matrix(), free[i]["pose"].matrix(), atol=POSE_ATOL, rtol=0)
        np.testing.assert_allclose(poses[i].inverse_matrix(), free[i]["pose"].inverse_matrix(), atol=POSE_ATOL, rtol=0)

    # ---- and none of it vacuously: the camera moved, the tracker worked and followed it
    moved = bench.pose_error(truth[-1], truth[0])
    errors = [bench.pose_error(p, t) for p, t in zip(poses, truth)]
    print(f"   camera moved {moved[0] * 1e3:.1f} mm / {moved[1]:.2f} deg; Gauss-Newton steps at full size {gn_steps}; "
          "tracking error per frame " + ", ".join(f"{e[0] * 1e3:.2f} mm / {e[1]:.3f} deg" for e in errors))
    assert moved[0] > 0.005 and moved[1] > 0.5
    assert all(n >= 1 for n in gn_steps)
    assert all(d["state"] in (0, 1) for d in device), "a Track aborted"
    assert max(e[0] for e in errors) < 0.1 * moved[0] + 0.002
    assert max(e[1] for e in errors) < 0.1 * moved[1] + 0.02
    del loop, vol, tracer
    torch.cuda.empty_cache()
