#!/usr/bin/env python3
"""tools/merge_pose_bench.py — what vk_volume_merge_posed costs on the bench's volume, next to vk_volume_merge: the two
replicas of tools/merge_bench.py (Volume(65024, 8192) at 5 mm, each fused from a different half of bench.py's depth
workload), the second merged into the first.

As there: the call changes the destination, so its table, visibility bytes, free list, counters and voxels are copied back in
front of every repetition and a 1 GiB fill behind the copy takes both pools out of the 256 MB Infinity Cache; HIP events on
the stream around the enqueue, two warm-up repetitions, median of --reps. Timed in one run, each from the restored and
flushed destination as its own frames left it, max_rounds = 8:
  plain      vk_volume_merge of the pair: the yardstick (profiles/merge_bench.json's `call`)
  identity   vk_volume_merge_posed at the identity pose: the same blocks and the same values through the gather path
  generic    vk_volume_merge_posed at yaw 10 degrees, pitch 5 degrees, t = (13, -21, 8) mm
One JSON line to --out (profiles/merge_pose_bench.json).

  rocprofv3 --kernel-trace --output-format csv -d <dir> -o p -- python tools/merge_pose_bench.py --reps 5 --out <dir>/run.json
  python tools/merge_pose_bench.py --kernels <dir>      the launches of that run per kernel: calls, median, min, max (us)

ref: src/volume.cu:304-368 (the allocator the rounds go through), apps/vulcan/vulcan.cu:283-325 (the workload)."""
import argparse
import ctypes as C
import os

import volume_bench_support as S
from volume_bench_support import ROOT

BLOCK_BYTES = 10240


def kernel_summary(directory):
    """per kernel of a rocprofv3 --kernel-trace run: calls and the median / min / max duration in us"""
    durations = S.kernel_durations(directory)
    print(S.KERNEL_HEADER)
    for name in sorted(durations):
        if any(word in name for word in ("pose_", "merge_", "handle")):
            print(S.kernel_row(name, durations[name]))
    # the fuse pass by set-up: its launches in stream order, --reps + 2 per set-up
    for name in ("merge_fuse_kernel", "pose_fuse_kernel"):
        t = [d for key, values in durations.items() if name in key for d in values]
        print(name, "in launch order:", " ".join(f"{d:.1f}" for d in t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20, help="frames fused into each replica")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_pose_bench.json"))
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

    vols = S.replicas(args.frames)
    dst, src = vols
    blocks = [int((v.host_entries()["data"] >= 0).sum()) for v in vols]
    before = S.save(dst)
    plain_workspace = api._dev_bytes(lib.vk_volume_merge_workspace_bytes(src.main, src.excess), "cuda")
    posed_workspace = api._dev_bytes(lib.vk_volume_merge_posed_workspace_bytes(src.main, src.excess, dst.main, dst.excess), "cuda")
    counts = torch.zeros(8, dtype=torch.int32, device="cuda")
    ddesc, sdesc = dst.desc(), src.desc()
    flush = S.flush_buffer()

    def timed(pose):
        merge = T.MergeParams(0, 8, 16.0, 16.0)
        posed = T.MergePoseParams(merge, pose) if pose is not None else None

        def before_each():
            S.restore(dst, before)
            counts.zero_()

        def call():
            if posed is None:
                api.check(lib.vk_volume_merge(C.byref(ddesc), C.byref(sdesc), C.byref(merge), api._ptr(counts),
                                              api._ptr(plain_workspace), api.stream()), "vk_volume_merge")
            else:
                api.check(lib.vk_volume_merge_posed(C.byref(ddesc), C.byref(sdesc), C.byref(posed), api._ptr(counts),
                                                    api._ptr(posed_workspace), api.stream()), "vk_volume_merge_posed")
        out = dict(S.timed(call, args.reps, flush, before_each), counts=[int(c) for c in counts.cpu().numpy()][:8 if posed else 6])
        if posed:
            # blocks a candidate took no sample into: allocated by the call and still Voxel::Empty()
            entries, voxels = dst.host_entries(), dst.host_voxels()
            slots = entries["data"][entries["data"] >= 0]
            observed = (voxels["distance_weight"].reshape(-1, 512)[slots] != 0).any(1) | (voxels["color_weight"].reshape(-1, 512)[slots] != 0).any(1)
            out["blocks_after"] = int(len(slots))
            out["blocks_empty_after"] = int((~observed).sum())
        return out

    results = {"plain": timed(None), "identity": timed(T.Transform.identity()), "generic": timed(MP.generic())}
    assert results["plain"]["counts"][:4] == [blocks[1], blocks[1], results["identity"]["counts"][3], 0]
    assert results["identity"]["counts"][:3] == [blocks[1]] * 3 and results["identity"]["counts"][4] == 0

    def fuse_bytes(r):
        # what the fuse pass must move: every fused dst block read and written once, every source block read once
        return (2 * r["counts"][2] + blocks[1]) * BLOCK_BYTES

    doc = {"tool": "tools/merge_pose_bench.py", "device": torch.cuda.get_device_name(0),
           "volumes": {"main_blocks": dst.main, "excess_blocks": dst.excess, "voxel_length": bench.VOXEL,
                       "frames_fused_each": args.frames, "blocks_dst": blocks[0], "blocks_src": blocks[1]},
           "method": f"HIP events around the enqueue on the stream, destination restored and the Infinity Cache flushed in front of every repetition, 2 warm-up + {args.reps} timed, median; max_rounds = 8",
           "merge_us": results,
           "candidates_per_source_block": {k: results[k]["counts"][1] / max(results[k]["counts"][0], 1) for k in ("identity", "generic")},
           "fuse_pass_bytes": {"what": "2 x 10 240 B per fused dst block (read, write) + 10 240 B per source block (each read once at least)",
                               "identity": fuse_bytes(results["identity"]), "generic": fuse_bytes(results["generic"])}}
    S.write(doc, args.out)


if __name__ == "__main__":
    main()
