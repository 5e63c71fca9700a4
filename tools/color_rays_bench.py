#!/usr/bin/env python3
"""tools/color_rays_bench.py — what vk_volume_color_rays costs: the steady-state volume and view of tools/cast_bench.py
(bench.py's depth workload, 40 frames of the orbit fused at 5 mm, the pose after the last fused frame) and the 640 x 480 pixel
rays of that view as world rays, with the ranges and the colours Volume.cast_rays gives them — a range of 0 where nothing is
hit, "no measurement"; the depth workload fuses no colour, so every colour is (0, 0, 0), which is a colour like any other to
the call. The rays are coloured as one observation, in four cases:

  band     the truncation length (8 voxels: the stretch integrate_rays fuses), and 2 voxels
  order    pixel order (neighbouring lanes walk neighbouring rays and add to neighbouring voxels), and a seeded shuffle

Every timed call starts from the same state: the voxels are restored from a device copy in front of it, outside the timed
stretch. Per case: the time of the call (HIP events around it, median of --reps) and the time of each pass from the events
the call itself records between its passes (vk_volume_color_rays_time_next): mark, zero, add, fold. The add pass issues two
64-bit integer atomics per visit of a present block; the eight counts do not carry the visits, so they are recounted here by
the CPU statement's walk (tests/color_rays_reference.py) against the table read back from the device, and checked against
the visits the call reports lost. Beside them, from the same process and on the same rays: vk_volume_integrate_rays with its
passes (vk_volume_integrate_rays_time_next; one atomic per update at this number of rays) and one cast_rays call. One JSON
line to --out (profiles/color_rays_bench.json). No threshold is set on these numbers.

ref: src/color_integrator.cu:110-148 (the integrator the rays stand in for), apps/vulcan/vulcan.cu:283-325 (the workload)."""
import argparse
import ctypes as C
import os

import numpy as np

import volume_bench_support as S
from volume_bench_support import ROOT

PASSES = ("mark", "zero", "add", "fold")
RAYS_PASSES = ("rounds", "mark", "zero", "add", "fold")
EVERYTHING = ("voxels", "hash_entries", "free_voxel_blocks", "allocation_types", "allocation_blocks", "block_visibility",
              "visible_blocks", "counters")


def spread(samples):
    return {"median_us": float(np.median(samples)), "min_us": float(min(samples)), "max_us": float(max(samples))}


def visits(vol, rays, ranges, band, r_min, r_max):
    """(visits of present blocks, visits lost) of the coloured rays, by the statement's walk against the device's table"""
    import carve_rays_reference as CV
    import color_rays_reference as CO
    import integrate_rays_reference as IR

    class Lengths:
        voxel_length = vol.voxel_length

    o, n, r, kind = IR.carried(Lengths, rays, ranges, None, r_min, r_max, False)
    walks = kind == IR.INTEGRATED
    with np.errstate(all="ignore"):
        b = np.float32(band) / np.float32(vol.voxel_length)
    who, cells, _ = CV.walk(o[walks], n[walks], *CO.ends(r[walks], b))
    blocks = cells >> 3
    blocks = blocks[IR.in_int16(blocks)] + 32768
    entries = vol.host_entries()
    held = entries["block"]["origin"][entries["data"] >= 0].astype(np.int64) + 32768
    pack = lambda a: (a[:, 0] << 32) | (a[:, 1] << 16) | a[:, 2]   # noqa: E731
    present = np.isin(pack(blocks), pack(held))
    return int(present.sum()), int((~present).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "color_rays_bench.json"))
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

    def passes(arm, names, call, before):
        marks = events(len(names) + 1)
        pointers = (C.c_void_p * len(marks))(*marks)
        per_pass = {p: [] for p in names}
        for _ in range(args.reps + 1):
            before()
            api.check(arm(pointers, len(marks)), "time_next")
            call()
            torch.cuda.synchronize()
            for which, p in enumerate(names):
                per_pass[p].append(elapsed_us(marks[which], marks[which + 1]))
        return {p: spread(v[1:]) for p, v in per_pass.items()}

    ordered = pixel_rays(k, view, bench.W, bench.H)
    count = len(ordered)
    rays_dev = torch.as_tensor(ordered).cuda()
    r_min, r_max = vol.depth_range
    t, status, samples, _ = vol._cast_call(rays_dev, None, 0, r_min, r_max, 500, samples=True, gradients=False)
    torch.cuda.synchronize()
    ranges = t.cpu().numpy().copy()
    colors = np.ascontiguousarray(samples.cpu().numpy().view(np.float32).reshape(count, 5)[:, 1:4])
    assert ((colors >= 0) & (colors <= 1)).all()
    order = np.random.default_rng(23).permutation(count)
    inputs = {"pixel_order": (rays_dev, torch.as_tensor(ranges).cuda(), torch.as_tensor(colors).cuda()),
              "shuffled": (torch.as_tensor(ordered[order]).cuda(), torch.as_tensor(ranges[order]).cuda(),
                           torch.as_tensor(np.ascontiguousarray(colors[order])).cuda())}
    bands = {"truncation_length": float(np.float32(bench.TRUNC)), "two_voxels": float(np.float32(2) * np.float32(bench.VOXEL))}

    saved = S.save(vol, ("voxels",))
    everything = S.save(vol, EVERYTHING)

    def restore():
        S.restore(vol, saved)

    results = {}
    for band_name, band in bands.items():
        present, lost = visits(vol, ordered, ranges, band, r_min, r_max)
        for name, (rays, rng, cols) in inputs.items():
            call = lambda: vol._color_rays_call(rays, rng, cols, None, T.VK_RAYS_ONE_OBSERVATION, r_min, r_max, band, 16.0)   # noqa: E731
            restore()
            counts = call()
            assert counts[7] == lost, (counts, lost)
            result = {"counts": counts, "call": bracketed(call, restore),
                      "passes": passes(lib.vk_volume_color_rays_time_next, PASSES, call, restore)}
            result["visits"] = present
            result["atomics_issued"] = 2 * present
            result["atomics_per_second"] = 2 * present / (result["passes"]["add"]["median_us"] * 1e-6)
            result["rays_per_second"] = counts[0] / (result["call"]["median_us"] * 1e-6)
            results[f"{band_name}.{name}"] = result
    restore()

    # beside them, on the same rays: integrate_rays with its passes (one atomic per update), and one cast_rays call
    scale = {"cast_rays": bracketed(lambda: vol._cast_call(rays_dev, None, 0, r_min, r_max, 500, samples=True, gradients=False,
                                                           out=(t, status, samples, None)))}
    for name, (rays, rng, _) in inputs.items():
        call = lambda: vol._integrate_rays_call(rays, rng, None, T.VK_RAYS_ONE_OBSERVATION, 8, r_min, r_max, 16.0)   # noqa: E731
        back = lambda: S.restore(vol, everything)   # noqa: E731
        back()
        scale[f"integrate_rays.{name}"] = {"counts": call(), "call": bracketed(call, back),
                                           "passes": passes(lib.vk_volume_integrate_rays_time_next, RAYS_PASSES, call, back)}
    S.restore(vol, everything)

    doc = {"tool": "tools/color_rays_bench.py", "device": torch.cuda.get_device_name(0),
           "volume": {"main_blocks": vol.main, "excess_blocks": vol.excess, "voxel_length": bench.VOXEL, "truncation_length": bench.TRUNC,
                      "frames_fused": args.frames},
           "rays": count, "rays_with_a_range": int((ranges > 0).sum()), "r_min": r_min, "r_max": r_max, "bands": bands,
           "flags": "VK_RAYS_ONE_OBSERVATION", "workspace_bytes": int(lib.vk_volume_color_rays_workspace_bytes(vol.main, vol.excess)),
           "method": f"HIP events; median of {args.reps} calls with the blocking read of the counts, the voxels restored from a device "
                     "copy in front of each; the passes from the events the call records between them "
                     "(vk_volume_color_rays_time_next, vk_volume_integrate_rays_time_next)",
           "for_scale_us": scale, "color_rays_us": results}
    S.write(doc, args.out)


if __name__ == "__main__":
    main()
