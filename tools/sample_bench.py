#!/usr/bin/env python3
"""tools/sample_bench.py — what vk_volume_sample costs on the bench's volume: the first replica of tools/register_bench.py
(Volume(65024, 8192) at 5 mm, fused from the first half of bench.py's depth workload), sampled at 2^20 points on four
axis-aligned slices through the fused room: 512 x 512 points each over the box of the allocated blocks, two planes of
constant z, one of constant x and one of constant y.

Four runs: the points in slice order (neighbouring lanes sample neighbouring voxels) and in a seeded shuffle (every lane its
own block), each distance-only (samples alone, VK_SAMPLE_DISTANCE_ONLY: 8 of a voxel's 20 bytes) and full (samples with
colour, and gradients). The volume is only read, so nothing is restored between repetitions; a 1 GiB fill in front of every
repetition takes the pool out of the 256 MB Infinity Cache. HIP events on the stream around the enqueue, two warm-up
repetitions, median of --reps. Reported per run: points per second and the bytes that must move — per point 12 in and 20
and/or 16 out, plus 8 or 20 bytes per distinct voxel touched (counted on the host from the statement's lattice). The
second replica is registered against the first once per repetition (vk_volume_register_system at the generic pose), so that
a kernel trace of the run holds register_pass_kernel, the existing code with the same gather shape, next to sample_kernel.
One JSON line to --out (profiles/sample_bench.json). No threshold is set on these numbers.

  rocprofv3 --kernel-trace --output-format csv -d <dir> -o p -- python tools/sample_bench.py --reps 5 --out <dir>/run.json
  python tools/sample_bench.py --kernels <dir>      per kernel: calls, median, min, max (us); ns per point and per in-band voxel

ref: src/tracer.cu:238-299 (the trilinear sample of a ray), apps/vulcan/vulcan.cu:283-325 (the workload)."""
import argparse
import ctypes as C
import json
import os

import numpy as np

import volume_bench_support as S
from volume_bench_support import ROOT

SIDE = 512                       # 4 slices of SIDE x SIDE points = 2^20


def kernel_summary(directory):
    """per kernel of a rocprofv3 --kernel-trace run: calls and the median / min / max duration in us; the sample kernels per
    point and the residual pass per in-band voxel, from the run's own JSON. A form's launches come in the run's order: the
    first half in slice order, the second shuffled."""
    run = json.loads(open(os.path.join(directory, "run.json")).read())
    durations = S.kernel_durations(directory)
    rows = []
    for name in sorted(durations):
        t = durations[name]
        if "sample_kernel" in name:
            rows.append((name + " slice order", t[:len(t) // 2], run["points"]))
            rows.append((name + " shuffled", t[len(t) // 2:], run["points"]))
        elif "register_pass" in name:
            rows.append((name, t, run["register_system"]["counts"][1]))
    print(f"{S.KERNEL_HEADER}{'ns / item':>11}")
    for name, t, items in rows:
        print(f"{S.kernel_row(name, t)}{1e3 * np.median(t) / max(items, 1):>11.4f}")
    print(f"(an item: one of the {run['points']} points of sample_kernel, {run['points_with_a_distance_sample']} of which have a sample; "
          f"one of the {run['register_system']['counts'][1]} in-band source voxels of register_pass_kernel, "
          f"{run['register_system']['counts'][2]} of which give a residual)")


def slices(volume):
    """[4 * SIDE * SIDE, 3] float32 metres: four planes over the box of the allocated blocks"""
    entries = volume.host_entries()
    origins = entries["block"]["origin"][entries["data"] >= 0].astype(np.float64)
    lo, hi = origins.min(0) * 8 * volume.voxel_length, (origins.max(0) + 1) * 8 * volume.voxel_length
    axis = [np.linspace(lo[a], hi[a], SIDE) for a in range(3)]
    out = []
    for fixed, where in ((2, 0.4), (2, 0.6), (0, 0.5), (1, 0.5)):
        u, v = [a for a in range(3) if a != fixed]
        grid = np.empty((SIDE, SIDE, 3))
        grid[..., u], grid[..., v] = np.meshgrid(axis[u], axis[v], indexing="ij")
        grid[..., fixed] = lo[fixed] + where * (hi[fixed] - lo[fixed])
        out.append(grid.reshape(-1, 3))
    return np.concatenate(out).astype(np.float32)


def voxels_touched(volume, points):
    """(distinct stored voxels the USED lattice points of `points` name, distinct voxels all eight name): what a distance-only
    run and a run with gradients read at least once"""
    f32 = np.float32
    entries = volume.host_entries()
    held = entries["block"]["origin"][entries["data"] >= 0].astype(np.int64)
    key = lambda b: (b[..., 0] + (1 << 19)) + ((b[..., 1] + (1 << 19)) << 20) + ((b[..., 2] + (1 << 19)) << 40)   # noqa: E731
    blocks = np.unique(key(held))
    g = points / f32(volume.voxel_length) - f32(0.5)
    b = np.floor(g)
    far = (g - b) != 0
    base = b.astype(np.int64)
    used_keys, all_keys = [], []
    for s in range(8):
        corner = np.array([s & 1, (s >> 1) & 1, s >> 2])
        n = base + corner
        there = np.isin(key(n >> 3), blocks)
        used = ((corner == 0) | far).all(-1)
        all_keys.append(key(n)[there])
        used_keys.append(key(n)[there & used])
    return int(len(np.unique(np.concatenate(used_keys)))), int(len(np.unique(np.concatenate(all_keys))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20, help="frames fused into each replica")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--band", type=float, default=0.75)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_bench.json"))
    ap.add_argument("--kernels", help="summarise the kernel trace in this directory instead of running")
    args = ap.parse_args()
    if args.kernels:
        return kernel_summary(args.kernels)

    import torch
    import bench
    import merge_pose_reference as MP
    from vulcan_amd import api, vk_types as T
    torch.cuda.set_device(0)
    lib = api.lib()

    dst, src = S.replicas(args.frames)
    ordered = slices(dst)
    count = len(ordered)
    shuffled = ordered[np.random.default_rng(17).permutation(count)]
    used, eight = voxels_touched(dst, ordered)
    points = {"slice_order": torch.as_tensor(ordered).cuda(), "shuffled": torch.as_tensor(shuffled).cuda()}
    samples = torch.empty((count, 20), dtype=torch.uint8, device="cuda")
    gradients = torch.empty((count, 4), dtype=torch.float32, device="cuda")
    flush = S.flush_buffer()
    b, one = dst._register_setup(src, MP.generic(), 1, args.band)
    ddesc, sdesc = dst.desc(), src.desc()

    forms = {"distance_only": (T.VK_SAMPLE_DISTANCE_ONLY, (samples, None), 12 + 20, used * 8),
             "full": (0, (samples, gradients), 12 + 20 + 16, eight * 20)}
    results = {}
    for order, tensor in points.items():
        for form, (flags, out, per_point, voxel_bytes) in forms.items():
            r = S.timed(lambda: dst._sample_call(tensor, None, flags, count=count, out=out), args.reps, flush)
            r["points_per_second"] = count / (r["median_us"] * 1e-6)
            r["bytes"] = count * per_point + voxel_bytes
            r["gigabytes_per_second"] = r["bytes"] / (r["median_us"] * 1e-6) * 1e-9
            results[f"{order}.{form}"] = r
    with_weight = int((samples.view(torch.int16)[:, 8] != 0).sum())
    with_gradient = int((gradients[:, 3] != 0).sum())

    def system():
        api.check(lib.vk_volume_register_system(C.byref(ddesc), C.byref(sdesc), api._ptr(b["pose"]), C.byref(one), api._ptr(b["system"]),
                                                api._ptr(b["counts"]), api._ptr(b["workspace"]), api.stream()), "vk_volume_register_system")

    register = S.timed(system, args.reps, flush)
    register["counts"] = [int(c) for c in b["counts"].cpu().numpy()]

    doc = {"tool": "tools/sample_bench.py", "device": torch.cuda.get_device_name(0),
           "volume": {"main_blocks": dst.main, "excess_blocks": dst.excess, "voxel_length": bench.VOXEL, "frames_fused": args.frames,
                      "blocks": int((dst.host_entries()["data"] >= 0).sum())},
           "points": count, "points_with_a_distance_sample": with_weight, "points_with_a_gradient": with_gradient,
           "distinct_voxels": {"used_points": used, "all_eight": eight},
           "method": f"HIP events around the enqueue on the stream, the Infinity Cache flushed in front of every repetition, 2 warm-up + {args.reps} timed, median",
           "bytes_what": "points x (12 in + 20 for a sample, + 16 for a gradient) + distinct voxels touched x 8 (distance only: the USED points) or 20 (full: all eight)",
           "sample_us": results, "register_system": register}
    S.write(doc, args.out)


if __name__ == "__main__":
    main()
