#!/usr/bin/env python3
"""tools/carve_rays_bench.py — what vk_volume_carve_rays costs: the steady-state volume and view of tools/cast_bench.py
(bench.py's depth workload, 40 frames of the orbit fused at 5 mm, the pose after the last fused frame) and the 640 x 480
pixel rays of that view as world rays, with the ranges Volume.cast_rays gives them — 0 where nothing is hit, "no
measurement". Two scenes:

  static   the ranges as they are: the rays end at the surface they were cast at, carving finds almost nothing to do and
           the cost is the walk through the absent blocks in front of it — the common case;
  moved    the ranges times 1.5, clipped below r_max: the rays pass through the fused surface and carve it,

each in pixel order (neighbouring lanes walk neighbouring rays and add to neighbouring voxels) and in a seeded shuffle.
Every timed call starts from the same state: the voxels are restored from a device copy in front of it, outside the timed
stretch. Per case: the time of the call (HIP events around it, median of --reps with min and max), its eight counts and the
carves per second. Beside them, from the same process: the memset the call begins with, alone; one cast_rays call and one
integrate_rays call on the static rays. One JSON line to --out (profiles/carve_rays_bench.json). No threshold is set on
these numbers.

  rocprofv3 --kernel-trace --output-format csv -d <dir> -o p -- python tools/carve_rays_bench.py --reps 5 --out <dir>/run.json
  python tools/carve_rays_bench.py --kernels <dir> [--out <json>]   the launches of that run per case and kernel: calls, median, min, max (us)

ref: src/depth_integrator.cu:54-74 (the "free" the integrator writes in front of a surface), apps/vulcan/vulcan.cu:283-325
(the workload)."""
import argparse
import ctypes as C
import os

import numpy as np

import volume_bench_support as S
from volume_bench_support import ROOT

CASES = ("static.pixel_order", "static.shuffled", "moved.pixel_order", "moved.shuffled")
BEYOND, BELOW = 1.5, 0.98


def spread(samples):
    return {"median_us": float(np.median(samples)), "min_us": float(min(samples)), "max_us": float(max(samples))}


def kernel_summary(directory, out):
    """per case and kernel of a rocprofv3 --kernel-trace run: calls and the median / min / max duration in us. Every case
    makes the same number of calls, one after the other, so a kernel's launches split into four equal runs."""
    durations = S.kernel_durations(directory)
    doc = {"tool": "tools/carve_rays_bench.py --kernels", "kernels_us": {}}
    print(S.KERNEL_HEADER)
    for name in sorted(durations):
        if "carve_" not in name:
            continue
        t = durations[name]
        assert len(t) % len(CASES) == 0, (name, len(t))
        for which, case in enumerate(CASES):
            part = t[which * len(t) // len(CASES):(which + 1) * len(t) // len(CASES)]
            print(S.kernel_row(f"{name} {case}", part))
            doc["kernels_us"].setdefault(case, {})[name] = dict(calls=len(part), **spread(part))
    if out:
        S.write(doc, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", help="summarise the kernel trace in this directory instead of running")
    args = ap.parse_args()
    if args.kernels:
        return kernel_summary(args.kernels, args.out)
    args.out = args.out or os.path.join(ROOT, "profiles", "carve_rays_bench.json")

    import torch
    import bench
    from cast_bench import pixel_rays
    from vulcan_amd import api, vk_types as T
    torch.cuda.set_device(0)
    lib = api.lib()

    k, vol, frame, out, integ, tracer, view = S.steady_state(args.frames)
    flush = S.flush_buffer()

    ordered = pixel_rays(k, view, bench.W, bench.H)
    count = len(ordered)
    rays_dev = torch.as_tensor(ordered).cuda()
    r_min, r_max = vol.depth_range
    t, status, _, _ = vol._cast_call(rays_dev, None, T.VK_CAST_DISTANCE_ONLY, r_min, r_max, 500, samples=False, gradients=False)
    torch.cuda.synchronize()
    static = t.cpu().numpy().copy()
    moved = np.minimum(static * np.float32(BEYOND), np.float32(BELOW) * np.float32(r_max)).astype(np.float32)
    order = np.random.default_rng(23).permutation(count)
    inputs = {}
    for scene, ranges in (("static", static), ("moved", moved)):
        inputs[f"{scene}.pixel_order"] = (rays_dev, torch.as_tensor(ranges).cuda())
        inputs[f"{scene}.shuffled"] = (torch.as_tensor(ordered[order]).cuda(), torch.as_tensor(ranges[order]).cuda())

    saved = S.save(vol, ("voxels",))
    everything = S.save(vol, S.STATE + ("voxels", "allocation_types", "allocation_blocks", "visible_blocks"))

    def restore():
        S.restore(vol, saved)

    results = {}
    for name in CASES:
        rays, ranges = inputs[name]
        restore()
        counts = vol._carve_rays_call(rays, ranges, None, T.VK_RAYS_ONE_OBSERVATION, 1024, r_min, r_max, 0.0, 16.0)
        workspace, counts_dev = vol._workspace("carve_rays", (vol.main, vol.excess), lib.vk_volume_carve_rays_workspace_bytes, 8)
        params = T.CarveRaysParams(T.VK_RAYS_ONE_OBSERVATION, 1024, r_min, r_max, 0.0, 16.0)
        desc = vol.desc()

        def call():                                                        # the library call alone: nothing is read back
            api.check(lib.vk_volume_carve_rays(C.byref(desc), C.c_void_p(rays.data_ptr()), C.c_void_p(ranges.data_ptr()), count, None,
                                               C.byref(params), C.c_void_p(counts_dev.data_ptr()), C.c_void_p(workspace.data_ptr()),
                                               api.stream()), "vk_volume_carve_rays")

        result = {"counts": counts, "call": S.timed(call, args.reps, flush, restore)}
        result["carves_per_second"] = counts[7] / (result["call"]["median_us"] * 1e-6)
        result["rays_per_second"] = (counts[0] + counts[1]) / (result["call"]["median_us"] * 1e-6)
        results[name] = result
    restore()

    # the memset the call begins with, alone: the counts, the touched bytes and the control words
    workspace, _ = vol._workspace("carve_rays", (vol.main, vol.excess), lib.vk_volume_carve_rays_workspace_bytes, 8)
    zeroed = int(workspace.numel())
    memset = S.timed(lambda: api.check(lib.vk_memset(C.c_void_p(workspace.data_ptr()), 0, zeroed, api.stream()), "vk_memset"),
                     args.reps, flush)

    # for scale, from the same process and on the static rays: one cast_rays call, one integrate_rays call
    rays, ranges = inputs["static.pixel_order"]
    scale = {"cast_rays": S.timed(lambda: vol._cast_call(rays, None, T.VK_CAST_DISTANCE_ONLY, r_min, r_max, 500, samples=False,
                                                         gradients=False, out=(t, status, None, None)), args.reps, flush),
             "integrate_rays": S.timed(lambda: vol._integrate_rays_call(rays, ranges, None, T.VK_RAYS_ONE_OBSERVATION, 8, r_min, r_max, 16.0),
                                       args.reps, flush, lambda: S.restore(vol, everything))}
    S.restore(vol, everything)

    doc = {"tool": "tools/carve_rays_bench.py", "device": torch.cuda.get_device_name(0),
           "volume": {"main_blocks": vol.main, "excess_blocks": vol.excess, "voxel_length": bench.VOXEL, "truncation_length": bench.TRUNC,
                      "frames_fused": args.frames},
           "rays": count, "rays_with_a_range": int((static > 0).sum()), "r_min": r_min, "r_max": r_max, "t_from": 0.0,
           "flags": "VK_RAYS_ONE_OBSERVATION", "max_blocks": 1024, "moved": f"ranges x {BEYOND}, at most {BELOW} r_max",
           "workspace_bytes": zeroed,
           "method": f"HIP events; median of {args.reps} calls behind a 1 GiB flush, the voxels restored from a device copy in front of each",
           "for_scale": "cast_rays: the library call alone; integrate_rays: with the blocking read of its counts, as "
                        "tools/integrate_rays_bench.py times it",
           "memset_us": memset, "for_scale_us": scale, "carve_rays_us": results}
    S.write(doc, args.out)


if __name__ == "__main__":
    main()
