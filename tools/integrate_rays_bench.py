#!/usr/bin/env python3
"""tools/integrate_rays_bench.py — what vk_volume_integrate_rays costs: the steady-state volume and view of
tools/cast_bench.py (bench.py's depth workload, 40 frames of the orbit fused at 5 mm, the pose after the last fused frame)
and the 640 x 480 pixel rays of that view as world rays, with the ranges Volume.cast_rays gives them — 0 where nothing is
hit, "no measurement". The rays are fused as one observation

  into the populated volume they were cast in (all but a handful of the blocks exist already), and
  into a fresh volume of the same size (every block is allocated by the call),

each in pixel order (neighbouring lanes walk neighbouring rays and add to neighbouring voxels) and in a seeded shuffle (every
lane of a wave its own part of the image). Every timed call starts from the same state: the volume's buffers are restored
from a device copy in front of it, outside the timed stretch. Per case: the time of the call (HIP events around it, median of
--reps), and the time of each pass from the events the call itself records between its passes
(vk_volume_integrate_rays_time_next): allocation rounds, mark, zero, add, fold. The add pass issues one 64-bit integer atomic
per update at this number of rays (below 2^21 a voxel's count and sum share a word); their number is the sum of the counts
N, which the call's eight counts do not carry, so it is recounted here from the weights of a cap-less call into a fresh
volume. Beside them, for scale, this process's vk_integrate_depth stage (DepthIntegrator.integrate of the same
view) and one cast_rays call, timed as tools/cast_bench.py times them. One JSON line to --out
(profiles/integrate_rays_bench.json). No threshold is set on these numbers.

ref: src/depth_integrator.cu:54-115 (the integrator the rays stand in for), apps/vulcan/vulcan.cu:283-325 (the workload)."""
import argparse
import ctypes as C
import os

import numpy as np

import volume_bench_support as S
from volume_bench_support import ROOT

PASSES = ("rounds", "mark", "zero", "add", "fold")
BUFFERS = ("voxels", "hash_entries", "free_voxel_blocks", "allocation_types", "allocation_blocks", "block_visibility",
           "visible_blocks", "counters")


def spread(samples):
    return {"median_us": float(np.median(samples)), "min_us": float(min(samples)), "max_us": float(max(samples))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "integrate_rays_bench.json"))
    args = ap.parse_args()

    import torch
    import bench
    from cast_bench import pixel_rays
    from vulcan_amd import api, vk_types as T
    torch.cuda.set_device(0)
    lib = api.lib()

    k, vol, frame, out, integ, tracer, view = S.steady_state(args.frames)

    def events(n):
        made = []
        for _ in range(n):
            e = C.c_void_p()
            api.check(lib.vk_event_create(C.byref(e)), "vk_event_create")
            made.append(e)
        return made

    def elapsed_us(e0, e1):
        ms = C.c_float()
        api.check(lib.vk_event_elapsed_ms(e0, e1, C.byref(ms)), "vk_event_elapsed_ms")
        return ms.value * 1e3

    def bracketed(call, before=lambda: None):
        e0, e1 = events(2)
        times = []
        for _ in range(args.reps + 1):
            before()
            lib.vk_event_record(e0, api.stream())
            call()
            lib.vk_event_record(e1, api.stream())
            torch.cuda.synchronize()
            times.append(elapsed_us(e0, e1))
        return spread(times[1:])                                           # the first call warms up

    ordered = pixel_rays(k, view, bench.W, bench.H)
    count = len(ordered)
    rays_dev = torch.as_tensor(ordered).cuda()
    r_min, r_max = vol.depth_range
    t, status, _, _ = vol._cast_call(rays_dev, None, T.VK_CAST_DISTANCE_ONLY, r_min, r_max, 500, samples=False, gradients=False)
    torch.cuda.synchronize()
    scale = {"integrate_depth": bracketed(lambda: integ.integrate(frame)),
             "cast_rays": bracketed(lambda: vol._cast_call(rays_dev, None, T.VK_CAST_DISTANCE_ONLY, r_min, r_max, 500, samples=False,
                                                           gradients=False, out=(t, status, None, None)))}
    ranges = t.cpu().numpy().copy()
    order = np.random.default_rng(23).permutation(count)
    inputs = {"pixel_order": (rays_dev, torch.as_tensor(ranges).cuda()),
              "shuffled": (torch.as_tensor(ordered[order]).cuda(), torch.as_tensor(ranges[order]).cuda())}

    fresh = api.Volume(bench.MAIN, bench.EXCESS, voxel_length=bench.VOXEL, truncation_length=bench.TRUNC)
    torch.cuda.synchronize()
    # the atomics a call issues: with no cap, into a fresh volume and counting every ray, a voxel's weight is its N
    uncapped = fresh._integrate_rays_call(*inputs["pixel_order"], None, 0, 8, r_min, r_max, 32767.0)
    weights = fresh.host_voxels()["distance_weight"].astype(np.int64)
    updates = int(weights.sum())
    assert int((weights != 0).sum()) == uncapped[6] and int(weights.max()) < 32767
    fresh = api.Volume(bench.MAIN, bench.EXCESS, voxel_length=bench.VOXEL, truncation_length=bench.TRUNC)
    torch.cuda.synchronize()

    per_update = 1 if count < (1 << 21) else 2
    results = {}
    for target, volume in (("populated", vol), ("fresh", fresh)):
        saved = S.save(volume, BUFFERS)

        def restore():
            S.restore(volume, saved)

        for name, (rays, rng) in inputs.items():
            call = lambda: volume._integrate_rays_call(rays, rng, None, T.VK_RAYS_ONE_OBSERVATION, 8, r_min, r_max, 16.0)   # noqa: E731
            restore()
            counts = call()
            result = {"counts": counts, "call": bracketed(call, restore)}
            marks = events(6)
            pointers = (C.c_void_p * 6)(*marks)
            per_pass = {p: [] for p in PASSES}
            for _ in range(args.reps + 1):
                restore()
                api.check(lib.vk_volume_integrate_rays_time_next(pointers, 6), "vk_volume_integrate_rays_time_next")
                call()
                torch.cuda.synchronize()
                for which, p in enumerate(PASSES):
                    per_pass[p].append(elapsed_us(marks[which], marks[which + 1]))
            result["passes"] = {p: spread(v[1:]) for p, v in per_pass.items()}
            if counts[7] == 0 and counts[6] == uncapped[6]:
                # no visit was lost and the same voxels took an update: the updates are those counted above
                result["atomics_issued"] = per_update * updates
                result["atomics_per_second"] = per_update * updates / (result["passes"]["add"]["median_us"] * 1e-6)
            result["rays_per_second"] = counts[0] / (result["call"]["median_us"] * 1e-6)
            results[f"{target}.{name}"] = result
        restore()

    doc = {"tool": "tools/integrate_rays_bench.py", "device": torch.cuda.get_device_name(0),
           "volume": {"main_blocks": vol.main, "excess_blocks": vol.excess, "voxel_length": bench.VOXEL, "truncation_length": bench.TRUNC,
                      "frames_fused": args.frames},
           "rays": count, "rays_with_a_range": int((ranges > 0).sum()), "r_min": r_min, "r_max": r_max, "flags": "VK_RAYS_ONE_OBSERVATION",
           "max_rounds": 8, "voxel_updates_fresh": updates, "voxels_updated_fresh": uncapped[6],
           "workspace_bytes": int(lib.vk_volume_integrate_rays_workspace_bytes(vol.main, vol.excess)),
           "method": f"HIP events; median of {args.reps} calls, the volume's buffers restored from a device copy in front of each; the "
                     "passes from the events the call records between them (vk_volume_integrate_rays_time_next)",
           "for_scale_us": scale, "integrate_rays_us": results}
    S.write(doc, args.out)


if __name__ == "__main__":
    main()
