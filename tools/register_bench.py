#!/usr/bin/env python3
"""tools/register_bench.py — what vk_volume_register costs on the bench's volume: the two replicas of
tools/merge_pose_bench.py (Volume(65024, 8192) at 5 mm, each fused from a different half of bench.py's depth workload), the
second registered against the first from the generic pose (yaw 10 degrees, pitch 5 degrees, t = (13, -21, 8) mm).

Both volumes are only read, so nothing is restored between repetitions; a 1 GiB fill in front of every repetition takes both
pools out of the 256 MB Infinity Cache. HIP events on the stream around the enqueue, two warm-up repetitions, median of
--reps. Timed in one run:
  system     vk_volume_register_system at the pose: the source-block list, one residual pass, the sum
  register   vk_volume_register, --iterations steps from the pose: per step a residual pass, the sum and the solve
             (us per step = the call over the steps it ran; stages behind a converged step return at once)
  merge      vk_volume_merge_posed of the same pair at the same pose into a restored destination: the yardstick's call
and, from the volumes on the host, what the residual pass must move: every considered source block once, plus the dst
blocks its directories name (each once at least). One JSON line to --out (profiles/register_bench.json).

The residual pass against the yardstick's fuse pass, kernel by kernel, comes from a trace of the same run:
  rocprofv3 --kernel-trace --output-format csv -d <dir> -o p -- python tools/register_bench.py --reps 5 --out <dir>/run.json
  python tools/register_bench.py --kernels <dir>      calls, median, min, max (us) per kernel, and the ratio of the two passes

ref: src/tracker.cpp:124-163 (the loop), apps/vulcan/vulcan.cu:283-325 (the workload)."""
import argparse
import ctypes as C
import os

import numpy as np

import volume_bench_support as S
from volume_bench_support import ROOT

BLOCK_BYTES = 10240


def kernel_summary(directory):
    """per kernel of a rocprofv3 --kernel-trace run: calls and the median / min / max duration in us"""
    durations = S.kernel_durations(directory)
    print(S.KERNEL_HEADER)
    medians = {}
    for name in sorted(durations):
        if any(word in name for word in ("register_", "pose_fuse")):
            medians[name.split("<")[0]] = float(np.median(durations[name]))
            print(S.kernel_row(name, durations[name]))
    if "register_pass_kernel" in medians and "pose_fuse_kernel" in medians:
        print(f"residual pass / fuse pass: {medians['register_pass_kernel'] / medians['pose_fuse_kernel']:.2f}")


def pass_bytes(dst, src, pose, band):
    """what the residual pass must move, from the volumes on the host: (source blocks with a voxel in band, dst blocks their
    4x4x4 directories name)"""
    import merge_pose_reference as MP
    f32 = np.float32
    entries, voxels = src.host_entries(), src.host_voxels()
    held = entries[entries["data"] >= 0]
    distance = voxels["distance"].reshape(-1, 512)[held["data"]]
    weight = voxels["distance_weight"].reshape(-1, 512)[held["data"]]
    with np.errstate(invalid="ignore"):
        banded = ((weight != 0) & (np.abs(distance) < f32(band))).any(1)
    origins = held["block"]["origin"][banded].astype(np.int64)
    fwd = MP.rows(pose.m, src.voxel_length)
    least = np.full((len(origins), 3), 1 << 40, dtype=np.int64)
    for i in range(512):                                                       # one voxel of every block at a time
        centre = (8 * origins + MP.OFFSETS[i]).astype(f32) + f32(0.5)
        least = np.minimum(least, np.floor(MP.apply(fwd, centre) - f32(0.5)).astype(np.int64) >> 3)
    cells = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    named = (least[:, None, :] + cells[None]).reshape(-1, 3)
    there = dst.host_entries()
    there = there["block"]["origin"][there["data"] >= 0].astype(np.int64)
    key = lambda b: (b[:, 0] + 32768) + ((b[:, 1] + 32768) << 17) + ((b[:, 2] + 32768) << 34)   # noqa: E731
    return int(banded.sum()), int(np.isin(np.unique(key(named)), key(there)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20, help="frames fused into each replica")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--band", type=float, default=0.75)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "register_bench.json"))
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

    dst, src = vols = S.replicas(args.frames)
    blocks = [int((v.host_entries()["data"] >= 0).sum()) for v in vols]
    pose = MP.generic()
    before = S.save(dst)
    posed_workspace = api._dev_bytes(lib.vk_volume_merge_posed_workspace_bytes(src.main, src.excess, dst.main, dst.excess), "cuda")
    merge_counts = torch.zeros(8, dtype=torch.int32, device="cuda")
    ddesc, sdesc = dst.desc(), src.desc()
    flush = S.flush_buffer()
    b, one = dst._register_setup(src, pose, 1, args.band)
    many = T.RegisterParams(0, args.iterations, float(args.band), 0)
    posed = T.MergePoseParams(T.MergeParams(0, 8, 16.0, 16.0), pose)

    def system():
        api.check(lib.vk_volume_register_system(C.byref(ddesc), C.byref(sdesc), api._ptr(b["pose"]), C.byref(one), api._ptr(b["system"]),
                                                api._ptr(b["counts"]), api._ptr(b["workspace"]), api.stream()), "vk_volume_register_system")

    def register():
        api.check(lib.vk_volume_register(C.byref(ddesc), C.byref(sdesc), api._ptr(b["pose"]), C.byref(many), api._ptr(b["system"]),
                                         api._ptr(b["state"]), api._ptr(b["counts"]), api._ptr(b["update"]), api._ptr(b["workspace"]),
                                         api.stream()), "vk_volume_register")

    def merge():
        api.check(lib.vk_volume_merge_posed(C.byref(ddesc), C.byref(sdesc), C.byref(posed), api._ptr(merge_counts),
                                            api._ptr(posed_workspace), api.stream()), "vk_volume_merge_posed")

    def timed(call, restore=False):
        def before_each():
            if restore:
                S.restore(dst, before)
            api.check(lib.vk_transform_upload(api._ptr(b["pose"]), C.byref(pose), api.stream()), "vk_transform_upload")
            b["state"].zero_()
        return S.timed(call, args.reps, flush, before_each)

    results = {"system": timed(system)}
    results["system"]["counts"] = [int(c) for c in b["counts"].cpu().numpy()]
    results["register"] = timed(register)
    state = [int(c) for c in b["state"].cpu().numpy()]
    results["register"].update(iterations=args.iterations, steps=state[0], code=state[1], counts=[int(c) for c in b["counts"].cpu().numpy()],
                               us_per_step=results["register"]["median_us"] / max(state[0], 1))
    banded_blocks, named = pass_bytes(dst, src, pose, args.band)           # (before the merge changes dst for good)
    results["merge"] = timed(merge, restore=True)
    results["merge"]["counts"] = [int(c) for c in merge_counts.cpu().numpy()]
    S.restore(dst, before)

    counts = results["system"]["counts"]
    doc = {"tool": "tools/register_bench.py", "device": torch.cuda.get_device_name(0),
           "volumes": {"main_blocks": dst.main, "excess_blocks": dst.excess, "voxel_length": bench.VOXEL,
                       "frames_fused_each": args.frames, "blocks_dst": blocks[0], "blocks_src": blocks[1]},
           "method": f"HIP events around the enqueue on the stream, the Infinity Cache flushed in front of every repetition, 2 warm-up + {args.reps} timed, median; band {args.band}",
           "register_us": results,
           "residuals_per_source_block": counts[2] / max(counts[0], 1),
           "residual_pass_bytes": {"what": "10 240 B per considered source block (each read once) + 10 240 B per dst block a directory names (each read once at least; 8 of its 20 bytes per voxel are used)",
                                   "source_blocks": counts[0], "source_blocks_with_a_voxel_in_band": banded_blocks, "dst_blocks_named": named,
                                   "bytes": (counts[0] + named) * BLOCK_BYTES},
           "fuse_pass_bytes": {"what": "the yardstick: 2 x 10 240 B per fused dst block (read, write) + 10 240 B per source block",
                               "bytes": (2 * results["merge"]["counts"][2] + blocks[1]) * BLOCK_BYTES}}
    S.write(doc, args.out)


if __name__ == "__main__":
    main()
