#!/usr/bin/env python3
"""tools/score_poses_bench.py — what vk_volume_score_poses costs: the steady-state volume and view of tools/cast_bench.py
(bench.py's depth workload, 40 frames of the orbit fused at 5 mm, the pose after the last fused frame), every 64th of the
640 x 480 pixel rays of that view as world rays with the ranges Volume.cast_rays gives them (4 800 rays; a range of 0 where
nothing is hit, "no measurement"), and 4 096 candidate poses around the generic pose (yaw 10 degrees, pitch 5 degrees,
t = (13, -21, 8) mm): four offsets each of yaw, pitch and roll (-6, -2, 2, 6 degrees) and of x, y and z (-30, -10, 10, 30 mm),
in grid order and in a seeded shuffle.

The volume is only read, so nothing is restored between repetitions; a 1 GiB fill in front of every repetition takes the pool
out of the 256 MB Infinity Cache. HIP events on the stream around the enqueue, two warm-up repetitions, median of --reps.
Timed in one run, per order of the candidates:
  score      vk_volume_score_poses: the pass over poses x rays and the sum of the ray tiles
  sample     yardstick 1, existing code with the same gather in one launch: vk_volume_sample with VK_SAMPLE_DISTANCE_ONLY,
             gradients only, at the poses x rays endpoints computed on the host (pose-major, in the candidates' order). It
             reads 12 bytes and writes 16 bytes per pair, which the score does not
  system     yardstick 2, what a user does today: vk_transform_upload and vk_volume_register_rays_system once per candidate,
             for the first 64 candidates in one enqueue, scaled to all of them
One JSON line to --out (profiles/score_poses_bench.json). No time is fixed for the call: it is reported against the
yardsticks and yardstick 1's own spread over the repetitions.

--localize adds the time of Volume.localize_rays' whole enqueue (score, best, 20 steps of register_rays) on the scenario of
tests/test_gpu_score_poses.py: the oracle's scene, 1 200 rays, 2 625 candidates.

The kernels, from one kernel trace of the same run (counters go in a run of their own):
  rocprofv3 --kernel-trace --output-format csv -d <dir> -o p -- python tools/score_poses_bench.py --order grid_order --out <dir>/run.json
  python tools/score_poses_bench.py --kernels <dir>   calls, median, min, max (us) per kernel

ref: src/tracker.cpp:124-163 (the loop whose start the call finds), apps/vulcan/vulcan.cu:283-325 (the workload)."""
import argparse
import ctypes as C
import itertools
import json
import os

import numpy as np

import volume_bench_support as S
from volume_bench_support import ROOT


def kernel_summary(directory):
    """per kernel of a rocprofv3 --kernel-trace run: calls and the median / min / max duration in us"""
    durations = S.kernel_durations(directory)
    print(S.KERNEL_HEADER)
    for name in sorted(durations):
        if any(word in name for word in ("score_poses_", "register_rays_", "sample_kernel")):
            print(S.kernel_row(name, durations[name]))


def candidates():
    """4^6 poses around merge_pose_reference.generic(), in grid order"""
    import scenes
    from vulcan_amd import vk_types as T

    def about(axis, degrees):
        a = np.deg2rad(degrees) / 2.0
        return T.Transform.rotate(np.cos(a), *(np.sin(a) * np.eye(3)[axis]))

    angles, shifts = (-6.0, -2.0, 2.0, 6.0), (-0.03, -0.01, 0.01, 0.03)
    out = []
    for yaw, pitch, roll in itertools.product(angles, angles, angles):
        rotation = scenes.yaw(10.0 + yaw) * about(0, 5.0 + pitch) * about(2, roll)
        for x, y, z in itertools.product(shifts, shifts, shifts):
            out.append(T.Transform.translate(0.013 + x, -0.021 + y, 0.008 + z) * rotation)
    return out


def localize_time(reps, flush):
    """the whole enqueue of Volume.localize_rays on the test's scenario, between HIP events; the result is read afterwards"""
    import torch
    from oracle import oracle
    import register_rays_reference as RY
    import score_poses_reference as SP
    from vulcan_amd import api
    oracle.build()
    oracle.lib()
    hv = RY.world(oracle).hv
    rays, ranges, truth = RY.displaced_sweep(oracle, SP.far_truth())
    rays, ranges = np.ascontiguousarray(rays[::SP.EVERY]), np.ascontiguousarray(ranges[::SP.EVERY])
    dv = api.Volume(hv.main, hv.excess, voxel_length=hv.voxel_length, truncation_length=hv.truncation_length)
    dv.upload(hv)
    d_rays, d_ranges = torch.as_tensor(rays).cuda(), torch.as_tensor(ranges).cuda()
    poses, pose_count = dv._poses_on_device(SP.grid()[1], "bench")
    found = []

    def call():
        found.append(dv.localize_rays(d_rays, d_ranges, poses, min_residuals=600, r_min=SP.R_MIN, r_max=SP.R_MAX))

    # localize_rays reads its result at the end: the events bracket enqueue, execution and that read
    result = S.timed(call, reps, flush)
    last = found[-1]
    result.update(rays=len(ranges), candidates=pose_count, best_index=int(last.best_index), steps=int(last.steps), converged=bool(last.converged),
                  iterations_enqueued=20, what="score, best and 20 enqueued steps of register_rays, and the blocking read of the result")
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--band", type=float, default=0.75)
    ap.add_argument("--every", type=int, default=64, help="every n-th pixel ray")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_poses_bench.json"))
    ap.add_argument("--order", choices=("both", "grid_order", "shuffled"), default="both")
    ap.add_argument("--localize", action="store_true", help="also time localize_rays on the test's scenario")
    ap.add_argument("--kernels", help="summarise the kernel trace in this directory instead of running")
    args = ap.parse_args()
    if args.kernels:
        return kernel_summary(args.kernels)

    import torch
    import bench
    from cast_bench import pixel_rays
    from vulcan_amd import api, vk_types as T
    torch.cuda.set_device(0)
    lib = api.lib()

    k, vol, frame, out, integ, tracer, view = S.steady_state(args.frames)
    rays = np.ascontiguousarray(pixel_rays(k, view, bench.W, bench.H)[::args.every])
    count = len(rays)
    r_min, r_max = vol.depth_range
    rays_dev = torch.as_tensor(rays).cuda()
    t, _, _, _ = vol._cast_call(rays_dev, None, T.VK_CAST_DISTANCE_ONLY, r_min, r_max, 500, samples=True, gradients=False)
    torch.cuda.synchronize()
    ranges = t.cpu().numpy().copy()
    ranges_dev = torch.as_tensor(ranges).cuda()
    grid = candidates()
    pose_count = len(grid)
    order = np.random.default_rng(29).permutation(pose_count)
    orders = {"grid_order": grid, "shuffled": [grid[i] for i in order]}
    orders = {name: value for name, value in orders.items() if args.order in ("both", name)}
    # the endpoints in the rays' frame, for yardstick 1: carried through each candidate on the host
    length = np.linalg.norm(rays[:, 3:].astype(np.float64), axis=1, keepdims=True)
    ends = rays[:, :3].astype(np.float64) + ranges[:, None].astype(np.float64) * rays[:, 3:] / length

    desc = vol.desc()
    flush = S.flush_buffer()
    pairs = count * pose_count
    gradients = torch.empty((pairs, 4), dtype=torch.float32, device="cuda")
    sample_params = T.SampleParams(T.VK_SAMPLE_DISTANCE_ONLY, 0)
    params = T.ScorePosesParams(0, 1, r_min, r_max, float(args.band), 0)
    one = 64                                    # candidates of yardstick 2
    results = {}
    for name, poses in orders.items():
        poses_dev, _ = vol._poses_on_device(poses, "bench")
        matrices = np.stack([p.matrix().astype(np.float64) for p in poses])
        points = (np.einsum("kab,nb->kna", matrices[:, :3, :3], ends) + matrices[:, None, :3, 3]).astype(np.float32).reshape(-1, 3)
        points_dev = torch.as_tensor(np.ascontiguousarray(points)).cuda()
        del points
        workspace, _ = vol._workspace("score_poses", (count, pose_count), lib.vk_volume_score_poses_workspace_bytes, 1)
        scores = torch.empty(pose_count * C.sizeof(T.PoseScore), dtype=torch.uint8, device="cuda")
        b, system_params = vol._register_rays_setup(count, poses[0], 1, args.band, 0, r_min, r_max)

        def score():
            api.check(lib.vk_volume_score_poses(C.byref(desc), api._ptr(rays_dev), api._ptr(ranges_dev), count, api._ptr(poses_dev), pose_count,
                                                C.byref(params), api._ptr(scores), api._ptr(workspace), api.stream()), "vk_volume_score_poses")

        def sample():
            api.check(lib.vk_volume_sample(C.byref(desc), api._ptr(points_dev), pairs, None, C.byref(sample_params), None,
                                           api._ptr(gradients), api.stream()), "vk_volume_sample")

        def systems():
            for pose in poses[:one]:
                api.check(lib.vk_transform_upload(api._ptr(b["pose"]), C.byref(pose), api.stream()), "vk_transform_upload")
                api.check(lib.vk_volume_register_rays_system(C.byref(desc), api._ptr(rays_dev), api._ptr(ranges_dev), count, api._ptr(b["pose"]),
                                                             C.byref(system_params), api._ptr(b["system"]), api._ptr(b["counts"]),
                                                             api._ptr(b["workspace"]), api.stream()), "vk_volume_register_rays_system")

        result = {"score": S.timed(score, args.reps, flush)}
        host = api.to_numpy(scores, T.pose_score_dtype)
        best = int(np.lexsort((np.arange(pose_count), host["sum_abs"], -host["residuals"].astype(np.int64)))[0])
        result["score"].update(best=best, best_score=[int(x) for x in host[best]], residuals_median=float(np.median(host["residuals"])),
                               sampled_median=float(np.median(host["sampled"])), measured=int(host["measured"][0]),
                               ns_per_pair=result["score"]["median_us"] * 1e3 / pairs)
        # the last of yardstick 2's candidates has to give the score's counts: the same test
        result["sample"] = S.timed(sample, args.reps, flush)
        result["sample"]["with_a_gradient"] = int((gradients[:, 3] != 0).sum().item())
        result["system"] = S.timed(systems, args.reps, flush)
        counts = [int(c) for c in b["counts"].cpu().numpy()]
        result["system"].update(candidates=one, counts_of_the_last=counts,
                                agrees_with_the_score=counts == [int(x) for x in host[one - 1]][:4],
                                scaled_median_us=result["system"]["median_us"] * pose_count / one)
        spread = result["sample"]["max_us"] - result["sample"]["min_us"]
        result["against_the_yardsticks"] = {
            "score_over_sample": result["score"]["median_us"] / result["sample"]["median_us"],
            "score_minus_sample_us": result["score"]["median_us"] - result["sample"]["median_us"],
            "sample_spread_us": spread,
            "at_or_below_sample_within_its_spread": result["score"]["median_us"] - result["sample"]["median_us"] <= spread,
            "system_scaled_over_score": result["system"]["scaled_median_us"] / result["score"]["median_us"]}
        results[name] = result
        del points_dev

    doc = {"tool": "tools/score_poses_bench.py", "device": torch.cuda.get_device_name(0),
           "volume": {"main_blocks": vol.main, "excess_blocks": vol.excess, "voxel_length": bench.VOXEL, "truncation_length": bench.TRUNC,
                      "frames_fused": args.frames},
           "rays": count, "rays_with_a_range": int((ranges > 0).sum()), "candidates": pose_count, "pairs": pairs, "r_min": r_min, "r_max": r_max,
           "band": args.band, "workspace_bytes": int(lib.vk_volume_score_poses_workspace_bytes(count, pose_count)),
           "workgroups": {"pass": [(count + 255) // 256, (pose_count + 7) // 8], "sum": (pose_count + 31) // 32},
           "method": f"HIP events around the enqueue on the stream, the Infinity Cache flushed in front of every repetition, 2 warm-up + "
                     f"{args.reps} timed, median; the score is two launches (pass, sum), yardstick 1 one, yardstick 2 an upload and two "
                     f"launches per candidate",
           "score_poses_us": results}
    if args.localize:
        del gradients
        doc["localize_rays_us"] = localize_time(args.reps, flush)
    S.write(doc, args.out)


if __name__ == "__main__":
    main()
