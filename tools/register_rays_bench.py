#!/usr/bin/env python3
"""tools/register_rays_bench.py — what vk_volume_register_rays costs: the steady-state volume and view of tools/cast_bench.py
(bench.py's depth workload, 40 frames of the orbit fused at 5 mm, the pose after the last fused frame) and the 640 x 480 pixel
rays of that view as world rays with the ranges Volume.cast_rays gives them — a range of 0 where nothing is hit, "no
measurement" — in pixel order and in a seeded shuffle. The rays are in the volume's frame, so the true pose is the identity;
the start is the generic pose (yaw 10 degrees, pitch 5 degrees, t = (13, -21, 8) mm).

The volume is only read, so nothing is restored between repetitions; a 1 GiB fill in front of every repetition takes the pool
out of the 256 MB Infinity Cache. HIP events on the stream around the enqueue, two warm-up repetitions, median of --reps.
Timed in one run, per order:
  system     vk_volume_register_rays_system at the start: one residual pass and the sum
  register   vk_volume_register_rays from the start, as many steps as the loop needs to converge (found by a call with 64;
             --iterations steps when that call does not converge): per step the residual pass, the sum and the solve —
             three launch boundaries, as vk_volume_register's step (profiles/register_bench.json's us per step is quoted
             beside it when that profile is there). bench.py's room is a sphere seen from its centre: every rotation about
             the centre leaves every return on the surface, so this view fixes the sensor's position and not its
             orientation — the loop finds the position and then wanders along the three free directions without ever taking
             a step shorter than 1e-6. The tool reports that as it is: steps_to_converge null, and the error from the truth
  sample     the yardstick, existing code with the same gather: vk_volume_sample with VK_SAMPLE_DISTANCE_ONLY, gradients
             only, at the endpoints of the same rays at the start pose (a ray without a range: at its origin). It writes 16
             bytes per point where the pass writes one row per 512 rays
One JSON line to --out (profiles/register_rays_bench.json). No time is fixed for the pass: it is reported against the
yardstick and the yardstick's own spread over the repetitions.

The residual pass against the yardstick's kernel, from one kernel trace of the same run (counters go in a run of their own):
  rocprofv3 --kernel-trace --output-format csv -d <dir> -o p -- python tools/register_rays_bench.py --skip-loop --order pixel_order --out <dir>/run.json
  python tools/register_rays_bench.py --kernels <dir>   calls, median, min, max (us) per kernel, and the ratio of the two

ref: src/tracker.cpp:124-163 (the loop), apps/vulcan/vulcan.cu:283-325 (the workload)."""
import argparse
import ctypes as C
import json
import os

import numpy as np

import volume_bench_support as S
from volume_bench_support import ROOT


def kernel_summary(directory):
    """per kernel of a rocprofv3 --kernel-trace run: calls and the median / min / max duration in us"""
    durations = S.kernel_durations(directory)
    print(S.KERNEL_HEADER)
    medians = {}
    for name in sorted(durations):
        if any(word in name for word in ("register_", "sample_kernel")):
            medians[name.replace(" ", "")] = float(np.median(durations[name]))
            print(S.kernel_row(name, durations[name]))
    yardstick = [v for k, v in medians.items() if k.startswith("sample_kernel<false,true>")]
    passes = [v for k, v in medians.items() if k.startswith("register_rays_pass_kernel<false>")]
    if yardstick and passes:
        print(f"residual pass / sample kernel: {passes[0] / yardstick[0]:.2f}")


def pose_error(pose):
    """(metres, degrees) of a Transform from the identity"""
    m = pose.matrix().astype(np.float64)
    skew = (m[:3, :3] - m[:3, :3].T) / 2.0
    sine, cosine = np.linalg.norm([skew[2, 1], skew[0, 2], skew[1, 0]]), (np.trace(m[:3, :3]) - 1.0) / 2.0
    return float(np.linalg.norm(m[:3, 3])), float(np.degrees(np.arctan2(sine, cosine)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--band", type=float, default=0.75)
    ap.add_argument("--iterations", type=int, default=8, help="steps of the timed loop when 64 steps do not converge")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "register_rays_bench.json"))
    ap.add_argument("--order", choices=("both", "pixel_order", "shuffled"), default="both")
    ap.add_argument("--skip-loop", action="store_true", help="time the system and the yardstick only: what a kernel trace compares")
    ap.add_argument("--kernels", help="summarise the kernel trace in this directory instead of running")
    args = ap.parse_args()
    if args.kernels:
        return kernel_summary(args.kernels)

    import torch
    import bench
    import merge_pose_reference as MP
    from cast_bench import pixel_rays
    from vulcan_amd import api, vk_types as T
    torch.cuda.set_device(0)
    lib = api.lib()

    k, vol, frame, out, integ, tracer, view = S.steady_state(args.frames)
    ordered = pixel_rays(k, view, bench.W, bench.H)
    count = len(ordered)
    r_min, r_max = vol.depth_range
    t, _, _, _ = vol._cast_call(torch.as_tensor(ordered).cuda(), None, T.VK_CAST_DISTANCE_ONLY, r_min, r_max, 500, samples=True, gradients=False)
    torch.cuda.synchronize()
    ranges = t.cpu().numpy().copy()
    start = MP.generic()
    # the endpoints the pass samples at, for the yardstick: in the rays' frame, carried by the same pose on the device
    length = np.linalg.norm(ordered[:, 3:].astype(np.float64), axis=1, keepdims=True)
    ends = (ordered[:, :3].astype(np.float64) + ranges[:, None].astype(np.float64) * ordered[:, 3:] / length).astype(np.float32)
    order = np.random.default_rng(23).permutation(count)
    inputs = {"pixel_order": (ordered, ranges, ends), "shuffled": (ordered[order], ranges[order], ends[order])}
    inputs = {name: value for name, value in inputs.items() if args.order in ("both", name)}

    desc = vol.desc()
    flush = S.flush_buffer()
    gradients = torch.empty((count, 4), dtype=torch.float32, device="cuda")
    sample_params = T.SampleParams(T.VK_SAMPLE_DISTANCE_ONLY, 0)
    results = {}
    for name, (rays, rng, points) in inputs.items():
        rays_dev, ranges_dev = torch.as_tensor(np.ascontiguousarray(rays)).cuda(), torch.as_tensor(np.ascontiguousarray(rng)).cuda()
        points_dev = torch.as_tensor(np.ascontiguousarray(points)).cuda()
        b, one = vol._register_rays_setup(count, start, 1, args.band, 0, r_min, r_max)

        def system():
            api.check(lib.vk_volume_register_rays_system(C.byref(desc), api._ptr(rays_dev), api._ptr(ranges_dev), count, api._ptr(b["pose"]),
                                                         C.byref(one), api._ptr(b["system"]), api._ptr(b["counts"]), api._ptr(b["workspace"]),
                                                         api.stream()), "vk_volume_register_rays_system")

        def register(params):
            api.check(lib.vk_volume_register_rays(C.byref(desc), api._ptr(rays_dev), api._ptr(ranges_dev), count, api._ptr(b["pose"]),
                                                  C.byref(params), api._ptr(b["system"]), api._ptr(b["state"]), api._ptr(b["counts"]),
                                                  api._ptr(b["update"]), api._ptr(b["workspace"]), api.stream()), "vk_volume_register_rays")

        def sample():
            api.check(lib.vk_volume_sample(C.byref(desc), api._ptr(points_dev), count, api._ptr(b["pose"]), C.byref(sample_params), None,
                                           api._ptr(gradients), api.stream()), "vk_volume_sample")

        def before_each():
            api.check(lib.vk_transform_upload(api._ptr(b["pose"]), C.byref(start), api.stream()), "vk_transform_upload")
            b["state"].zero_()

        result = {"system": S.timed(system, args.reps, flush, before_each)}
        result["system"]["counts"] = [int(c) for c in b["counts"].cpu().numpy()]
        if not args.skip_loop:
            # how many steps the loop needs: one call with the most it may take
            before_each()
            register(T.RegisterRaysParams(0, 64, r_min, r_max, float(args.band), 0))
            torch.cuda.synchronize()
            steps, code = (int(c) for c in b["state"].cpu().numpy())
            found = T.Transform.from_buffer_copy(b["pose"].cpu().numpy().tobytes())
            metres, degrees = pose_error(found)
            converged = code == 1
            needed = T.RegisterRaysParams(0, steps if converged else args.iterations, r_min, r_max, float(args.band), 0)
            result["register"] = S.timed(lambda: register(needed), args.reps, flush, before_each)
            state = [int(c) for c in b["state"].cpu().numpy()]
            counts = [int(c) for c in b["counts"].cpu().numpy()]
            system_sums = b["system"].cpu().numpy()
            result["register"].update(steps_to_converge=steps if converged else None, code_after_64_steps=code, steps=state[0], counts=counts,
                                      rms=float(np.sqrt(system_sums[42] / counts[2])) if counts[2] else 0.0,
                                      us_per_step=result["register"]["median_us"] / max(state[0], 1),
                                      error_from_the_truth_after_64_steps={"metres": metres, "degrees": degrees})
        result["sample"] = S.timed(sample, args.reps, flush, before_each)
        result["sample"]["with_a_gradient"] = int((gradients[:, 3] != 0).sum().item())
        spread = result["sample"]["max_us"] - result["sample"]["min_us"]
        result["against_the_yardstick"] = {"system_over_sample": result["system"]["median_us"] / result["sample"]["median_us"],
                                           "system_minus_sample_us": result["system"]["median_us"] - result["sample"]["median_us"],
                                           "yardstick_spread_us": spread,
                                           "within_the_spread": result["system"]["median_us"] - result["sample"]["median_us"] <= spread}
        results[name] = result

    scale = {"launches_per_step": 3, "what": "residual pass, sum, one-wave solve: as vk_volume_register's step"}
    other = os.path.join(ROOT, "profiles", "register_bench.json")
    if os.path.exists(other):
        scale["vk_volume_register_us_per_step"] = json.loads(open(other).readline())["register_us"]["register"]["us_per_step"]
    start_metres, start_degrees = pose_error(start)
    doc = {"tool": "tools/register_rays_bench.py", "device": torch.cuda.get_device_name(0),
           "volume": {"main_blocks": vol.main, "excess_blocks": vol.excess, "voxel_length": bench.VOXEL, "truncation_length": bench.TRUNC,
                      "frames_fused": args.frames},
           "rays": count, "rays_with_a_range": int((ranges > 0).sum()), "r_min": r_min, "r_max": r_max, "band": args.band,
           "start": {"metres": start_metres, "degrees": start_degrees},
           "workspace_bytes": int(lib.vk_volume_register_rays_workspace_bytes(count)), "rows_of_partials": (count + 511) // 512,
           "method": f"HIP events around the enqueue on the stream, the Infinity Cache flushed in front of every repetition, 2 warm-up + "
                     f"{args.reps} timed, median; the system is two launches (pass, sum), the yardstick one",
           "scene": "a sphere seen from its centre: the view fixes the sensor's position, not its orientation",
           "step_for_scale": scale, "register_rays_us": results}
    S.write(doc, args.out)


if __name__ == "__main__":
    main()
