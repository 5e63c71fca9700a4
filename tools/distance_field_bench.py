#!/usr/bin/env python3
"""tools/distance_field_bench.py — what vk_volume_distance_field costs on the bench's steady-state volume (tools/kbench.py's:
Volume(65024, 8192) at 5 mm after --frames frames of bench.py's depth workload), over two planner grids centred on the
median block of the map: 256^3 cells at stride 4 (5.12 m a side at 2 cm) and 512 x 512 x 128 cells at stride 2, each with
max_cells 16 and 64.

The volume is only read, so nothing is restored between repetitions; a 1 GiB fill in front of every repetition takes the
pool and the grids out of the 256 MB Infinity Cache. HIP events on the stream around the enqueue, two warm-up repetitions,
median of --reps with min and max. Timed per grid and cap:
  field       the whole enqueue of vk_volume_distance_field (classes and floats out, no int32 grid)
  signed      the same with VK_FIELD_SIGNED: a second transform with the complement mask
  classify    vk_volume_classify_cells alone
  transform   vk_grid_distance_transform alone, on those classes
and next to them, once per grid, the obvious composition from existing parts and the statement on the device:
  sample      vk_volume_sample with VK_SAMPLE_DISTANCE_ONLY at every cell centre: what a caller had to start from before
              this call existed — one stored voxel per cell, not the cell's class, and no transform yet
  torch       the statement's three passes (tests/distance_field_reference.py) as torch tensor operations on the device,
              from the device's own class grid; its d2 has to equal the library's
One JSON line to --out (profiles/distance_field_bench.json). No threshold is set on these numbers.

  rocprofv3 --kernel-trace --output-format csv -d <dir> -o p -- python tools/distance_field_bench.py --reps 5 --out <dir>/run.json
  python tools/distance_field_bench.py --kernels <dir>      the launches of that run per kernel: calls, median, min, max (us)

ref: src/volume.cu:168-191 (the chain walk), apps/vulcan/vulcan.cu:283-325 (the workload)."""
import argparse
import ctypes as C
import os

import numpy as np

import volume_bench_support as S
from volume_bench_support import ROOT

GRIDS = {"256x256x256_stride4": ((256, 256, 256), 4), "512x512x128_stride2": ((512, 512, 128), 2)}
CAPS = (16, 64)
NONE = 1 << 29


def kernel_summary(directory):
    """per kernel of a rocprofv3 --kernel-trace run: calls and the median / min / max duration in us, then the launches of
    the library's own kernels in stream order"""
    durations = S.kernel_durations(directory)
    mine = ("fill_kernel", "classify_kernel", "x_pass_kernel", "axis_pass_kernel", "sample_kernel")
    print(S.KERNEL_HEADER)
    for name in sorted(durations):
        if any(word in name for word in mine):
            print(S.kernel_row(name, durations[name]))
    for name in sorted(durations):
        if any(word in name for word in mine[:4]):
            print(name, "in launch order:", " ".join(f"{d:.1f}" for d in durations[name]))


def torch_transform(classes, site_mask, max_cells):
    """distance_field_reference.transform in torch: three windowed passes, x, then y, then z, then the threshold"""
    import torch
    values = torch.where((classes & site_mask) != 0, 0, NONE).to(torch.int32)
    for axis in (2, 1, 0):
        length = values.shape[axis]
        best = values.clone()
        for k in range(1, min(max_cells, length - 1) + 1):
            here, there = best.narrow(axis, 0, length - k), best.narrow(axis, k, length - k)
            torch.minimum(here, values.narrow(axis, k, length - k) + k * k, out=here)
            torch.minimum(there, values.narrow(axis, 0, length - k) + k * k, out=there)
        values = torch.clamp(best, max=NONE)
    return torch.where(values > max_cells * max_cells, 2147483647, values).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20, help="frames fused before the grids are taken")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance_field_bench.json"))
    ap.add_argument("--kernels", help="summarise the kernel trace in this directory instead of running")
    args = ap.parse_args()
    if args.kernels:
        return kernel_summary(args.kernels)

    import torch
    import bench
    from vulcan_amd import api, vk_types as T
    torch.cuda.set_device(0)
    lib = api.lib()
    vol = S.steady_state(args.frames)[1]
    desc = vol.desc()
    flush = S.flush_buffer()
    entries = vol.host_entries()
    origins = entries["block"]["origin"][entries["data"] >= 0].astype(np.int64)
    middle = 8 * np.median(origins, 0).astype(np.int64)

    results = {}
    for name, (dims, stride) in GRIDS.items():
        origin = tuple(int(c) for c in (middle - np.array(dims) * stride // 2) // stride * stride)
        grid = T.CellGrid.make(origin, dims, stride)
        shape = dims[::-1]
        cells = int(np.prod(dims))
        classes = torch.empty(shape, dtype=torch.uint8, device="cuda")
        distance = torch.empty(shape, dtype=torch.float32, device="cuda")
        d2 = torch.empty(shape, dtype=torch.int32, device="cuda")
        workspace = api._dev_bytes(lib.vk_grid_distance_transform_workspace_bytes(grid.dims), "cuda")
        out = results[name] = {"origin": origin, "cells": cells}

        def classify():
            api.check(lib.vk_volume_classify_cells(C.byref(desc), C.byref(grid), 0.0, api._ptr(classes), api.stream()), "classify")
        out["classify"] = S.timed(classify, args.reps, flush)
        torch.cuda.synchronize()
        host = classes.cpu().numpy()
        out["classes"] = {"unknown": int((host == 1).sum()), "free": int((host == 2).sum()), "occupied": int((host == 4).sum())}
        # what has to move at the least: the fill, the blocks' 8 of 20 bytes, and per pass a grid in and a grid out
        blocks = int((np.abs(8 * origins + 4 - (middle)) <= np.array(dims) * stride // 2 + 4).all(1).sum())
        out["blocks_in_grid"] = blocks
        out["bytes_at_least"] = cells * (1 + 1 + 2 + 2 + 4 + 4 + 4) + blocks * 10240

        for cap in CAPS:
            def field(flags=0):
                params = T.DistanceFieldParams(flags, T.CELL_OCCUPIED, cap, 0.0)
                api.check(lib.vk_volume_distance_field(C.byref(desc), C.byref(grid), C.byref(params), api._ptr(classes), None,
                                                       api._ptr(distance), api._ptr(workspace), api.stream()), "distance_field")

            def transform():
                api.check(lib.vk_grid_distance_transform(api._ptr(classes), grid.dims, T.CELL_OCCUPIED, cap, api._ptr(d2),
                                                         api._ptr(workspace), api.stream()), "transform")
            run = out[f"max_cells_{cap}"] = {"field": S.timed(field, args.reps, flush),
                                             "signed": S.timed(lambda: field(T.VK_FIELD_SIGNED), args.reps, flush),
                                             "transform": S.timed(transform, args.reps, flush)}
            run["field_ns_per_cell"] = run["field"]["median_us"] * 1e3 / cells
            run["field_over_bytes_at_least_TBps"] = out["bytes_at_least"] / run["field"]["median_us"] * 1e-6
            torch.cuda.synchronize()
            finite = d2 != T.VK_FIELD_BEYOND
            run["finite_cells"] = int(finite.sum())
            # the statement in torch, from the same classes: a few repetitions, it is slow
            got = {}

            def statement():
                got["d2"] = torch_transform(classes, T.CELL_OCCUPIED, cap)
            run["torch"] = S.timed(statement, min(args.reps, 3), flush)
            assert torch.equal(got["d2"], d2), "the torch passes differ from the library's d2"
            del got

        # the composition a caller had before: a distance-only sample at every cell centre
        axes = [torch.arange(n, dtype=torch.float32, device="cuda") for n in shape]
        k, j, i = torch.meshgrid(*axes, indexing="ij")
        points = torch.stack([(o + stride * (a + 0.5)) for o, a in zip(origin, (i, j, k))], dim=-1).reshape(-1, 3).contiguous()
        del k, j, i
        samples = torch.empty((cells, 20), dtype=torch.uint8, device="cuda")
        params = T.SampleParams(T.VK_SAMPLE_VOXEL_UNITS | T.VK_SAMPLE_DISTANCE_ONLY, 0)

        def sample():
            api.check(lib.vk_volume_sample(C.byref(desc), api._ptr(points), cells, None, C.byref(params), api._ptr(samples), None,
                                           api.stream()), "sample")
        out["sample"] = S.timed(sample, args.reps, flush)
        del points, samples, classes, distance, d2, workspace

    doc = {"tool": "tools/distance_field_bench.py", "device": torch.cuda.get_device_name(0),
           "volume": {"main_blocks": vol.main, "excess_blocks": vol.excess, "voxel_length": bench.VOXEL, "frames_fused": args.frames,
                      "blocks": int(len(origins))},
           "method": f"HIP events around the enqueue on the stream, the Infinity Cache flushed in front of every repetition, 2 warm-up + {args.reps} timed (torch: {min(args.reps, 3)}), median with min and max; site mask OCCUPIED, occupied_below 0",
           "bytes_at_least": "per cell 1 (fill) + 1 (classes read) + 2 + 2 (|dx| out, in) + 4 + 4 (y pass out, in) + 4 (floats), and 10 240 B per block that meets the grid (its cache lines hold all 20 bytes of a voxel)",
           "distance_field_us": results}
    S.write(doc, args.out)


if __name__ == "__main__":
    main()
