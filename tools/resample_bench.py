#!/usr/bin/env python3
"""tools/resample_bench.py — what vk_volume_merge_resampled costs on the bench's volume, next to vk_volume_merge_posed: the
two replicas of tools/merge_pose_bench.py (Volume(65024, 8192) at 5 mm, each fused from a different half of bench.py's depth
workload), the second merged into a destination.

As there: the call changes the destination, so its table, visibility bytes, free list, counters and voxels are copied back in
front of every repetition and a 1 GiB fill behind the copy takes both pools out of the 256 MB Infinity Cache; HIP events on
the stream around the enqueue, two warm-up repetitions, median of --reps, max_rounds = 8. Timed in one run, at yaw 10 degrees,
pitch 5 degrees, t = (13, -21, 8) mm:
  posed      vk_volume_merge_posed of the pair: the yardstick (profiles/merge_pose_bench.json's `generic`)
  equal      vk_volume_merge_resampled of the same pair, n = 1: the same loads and the same bytes through the new passes
  to_10mm    the second replica into a fresh 10 mm volume, n = 2
  to_20mm    ... into a fresh 20 mm volume, n = 4
  to_2.5mm   ... into a fresh 2.5 mm volume, n = 1: only the source blocks of a box around the middle of the map, so many that
             the destination's pool holds what they reach
Per set-up the bytes the fuse pass must move, and next to the whole call the time torch's device-to-device copy takes to move
as many (flushed the same way). One JSON line to --out (profiles/resample_bench.json).

  rocprofv3 --kernel-trace --output-format csv -d <dir> -o p -- python tools/resample_bench.py --reps 5 --out <dir>/run.json
  python tools/resample_bench.py --kernels <dir>      the launches of that run per kernel: calls, median, min, max (us)

ref: src/volume.cu:304-368 (the allocator the rounds go through), apps/vulcan/vulcan.cu:283-325 (the workload)."""
import argparse
import ctypes as C
import os

import numpy as np

import volume_bench_support as S
from volume_bench_support import ROOT

BLOCK_BYTES = 10240
SETUPS = ("posed", "equal", "to_10mm", "to_20mm", "to_2.5mm")


def kernel_summary(directory):
    """per kernel of a rocprofv3 --kernel-trace run: calls and the median / min / max duration in us"""
    durations = S.kernel_durations(directory)
    print(S.KERNEL_HEADER)
    for name in sorted(durations):
        if any(word in name for word in ("resample_", "pose_", "handle", "round_end", "compact", "scan")):
            print(S.kernel_row(name, durations[name]))
    # the fuse passes by set-up: their launches in stream order, --reps + 2 per set-up
    for name in ("pose_fuse_kernel", "resample_fuse_kernel", "resample_geometry_kernel"):
        t = [d for key, values in durations.items() if name in key for d in values]
        print(name, "in launch order:", " ".join(f"{d:.1f}" for d in t))


def middle_box(volume, most):
    """the largest cube of blocks around the median block origin of `volume` that holds at most `most` of its blocks"""
    entries = volume.host_entries()
    origins = entries["block"]["origin"][entries["data"] >= 0].astype(np.int64)
    middle = np.median(origins, 0).astype(np.int64)
    half = 0
    while (np.abs(origins - middle).max(1) <= half + 1).sum() <= most and half < 4096:
        half += 1
    return tuple(int(c) for c in middle - half), tuple(int(c) for c in middle + half)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20, help="frames fused into each replica")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.json"))
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
    pose = MP.generic()
    flush = S.flush_buffer()
    counts = torch.zeros(8, dtype=torch.int32, device="cuda")

    def blocks_of(volume):
        return int((volume.host_entries()["data"] >= 0).sum())

    def fresh(voxel_length):
        return api.Volume(bench.MAIN, bench.EXCESS, voxel_length=voxel_length, truncation_length=bench.TRUNC)

    def timed(into, source, n):
        """one set-up: `source` into `into` (restored in front of every repetition); n None: vk_volume_merge_posed"""
        before = S.save(into)
        merge = T.MergeParams(0, 8, 16.0, 16.0)
        ddesc, sdesc = into.desc(), source.desc()
        if n is None:
            params, entry, name = T.MergePoseParams(merge, pose), lib.vk_volume_merge_posed, "vk_volume_merge_posed"
            size = lib.vk_volume_merge_posed_workspace_bytes(source.main, source.excess, into.main, into.excess)
        else:
            params, entry, name = T.MergeResampleParams(merge, pose, n, 0), lib.vk_volume_merge_resampled, "vk_volume_merge_resampled"
            size = lib.vk_volume_merge_resampled_workspace_bytes(source.main, source.excess, into.main, into.excess,
                                                                 into._resample_ratios(source)[2])
        workspace = api._dev_bytes(size, "cuda")

        def before_each():
            S.restore(into, before)
            counts.zero_()

        def call():
            api.check(entry(C.byref(ddesc), C.byref(sdesc), C.byref(params), api._ptr(counts), api._ptr(workspace), api.stream()), name)
        out = dict(S.timed(call, args.reps, flush, before_each), counts=[int(c) for c in counts.cpu().numpy()])
        # what the fuse pass must move: every fused dst block read and written once, every considered source block read once
        out["fuse_pass_bytes"] = (2 * out["counts"][2] + out["counts"][0]) * BLOCK_BYTES
        half = torch.empty(out["fuse_pass_bytes"] // 2, dtype=torch.uint8, device="cuda")
        other = torch.empty_like(half)
        copy = S.timed(lambda: other.copy_(half), args.reps, flush)
        out["copy_of_as_many_bytes_us"] = copy["median_us"]
        out["call_over_copy"] = out["median_us"] / copy["median_us"]
        out["workspace_bytes"] = int(size)
        S.restore(into, before)
        return out

    results = {"posed": timed(dst, src, None), "equal": timed(dst, src, 1)}
    assert results["posed"]["counts"] == results["equal"]["counts"]
    results["to_10mm"] = timed(fresh(2 * bench.VOXEL), src, 2)
    results["to_20mm"] = timed(fresh(4 * bench.VOXEL), src, 4)
    # a fine copy: a source block reaches about a dozen blocks at half the voxel length
    part = api.Volume(src.main, src.excess, voxel_length=src.voxel_length, truncation_length=src.truncation_length)
    S.restore(part, S.save(src))
    box = middle_box(src, (bench.MAIN + bench.EXCESS) // 24)
    part.release_blocks(keep_box=box)
    results["to_2.5mm"] = timed(fresh(0.5 * bench.VOXEL), part, 1)
    for name in SETUPS:
        assert results[name]["counts"][4] == 0, (name, results[name]["counts"])

    doc = {"tool": "tools/resample_bench.py", "device": torch.cuda.get_device_name(0),
           "volumes": {"main_blocks": dst.main, "excess_blocks": dst.excess, "voxel_length": bench.VOXEL,
                       "frames_fused_each": args.frames, "blocks_dst": blocks_of(dst), "blocks_src": blocks_of(src),
                       "blocks_src_in_box": blocks_of(part), "box": box},
           "method": f"HIP events around the enqueue on the stream, destination restored and the Infinity Cache flushed in front of every repetition, 2 warm-up + {args.reps} timed, median; max_rounds = 8; the copy is torch's device-to-device copy of fuse_pass_bytes / 2 (read and written), flushed the same way",
           "fuse_pass_bytes": "2 x 10 240 B per fused dst block (read, write) + 10 240 B per considered source block (each read once at least)",
           "merge_us": results}
    S.write(doc, args.out)


if __name__ == "__main__":
    main()
