#!/usr/bin/env python3
"""tools/merge_bench.py — what vk_volume_merge costs on the bench's volume: two replicas Volume(65024, 8192) at 5 mm, each
fused from a different half of bench.py's depth workload (the sphere room, orbit poses: frames 0 .. n - 1 and n .. 2 n - 1),
and the second merged into the first.

The call changes the destination, so its table, visibility bytes, free list, counters and voxels are copied back in front of
every repetition, and a 1 GiB fill behind the copy takes both pools out of the 256 MB Infinity Cache: what the call reads
comes from HBM. HIP events on the stream around the enqueue (no readback inside the timed region), two warm-up repetitions,
median of --reps. Timed, each from a restored and flushed state:
  call        the merge as Volume.merge makes it (max_rounds = 8) from the destination as its own frames left it
  settled     the same call on the destination AFTER a merge (every source block present, its voxels restored to that state):
              one request pass that posts nothing, idle rounds, and the fuse pass over every source block
  settled_1   ... with max_rounds = 1: (settled - settled_1) / 7 is an idle round (four short launches)
  idle_1      max_rounds = 1 with a fresh source volume of the same size: every launch of the call, no block to fuse;
              settled_1 - idle_1 bounds the fuse pass from above (it reads 10 240 B of each pool and writes 10 240 B per
              fused block): the difference also holds what the mark and the two request passes cost more on a full table,
              walked cold after the flush, than on an empty one; `rocprofv3 --kernel-trace --stats -- python
              tools/merge_bench.py` gives merge_fuse_kernel alone
  (call - settled) / rounds that posted is what a round that allocates costs over an idle one
and, in the same run, torch's device-to-device copy of half the fuse pass's bytes (read + write = the same bytes moved),
flushed the same way. One JSON line to --out (profiles/merge_bench.json).

ref: src/volume.cu:304-368 (the allocator the rounds go through), apps/vulcan/vulcan.cu:283-325 (the workload)."""
import argparse
import ctypes as C
import os

import volume_bench_support as S
from volume_bench_support import ROOT

BYTES_PER_FUSED_BLOCK = 3 * 10240


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20, help="frames fused into each replica")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_bench.json"))
    args = ap.parse_args()

    import torch
    import bench
    from vulcan_amd import api, vk_types as T
    torch.cuda.set_device(0)
    lib = api.lib()

    vols = S.replicas(args.frames)
    dst, src = vols
    fresh = api.Volume(src.main, src.excess, voxel_length=bench.VOXEL, truncation_length=bench.TRUNC)
    blocks = [int((v.host_entries()["data"] >= 0).sum()) for v in vols]

    before = S.save(dst)
    workspace = api._dev_bytes(lib.vk_volume_merge_workspace_bytes(src.main, src.excess), "cuda")
    counts = torch.zeros(6, dtype=torch.int32, device="cuda")
    ddesc, sdesc, fdesc = dst.desc(), src.desc(), fresh.desc()
    flush = S.flush_buffer()

    def timed(state, source, max_rounds):
        params = T.MergeParams(0, max_rounds, 16.0, 16.0)

        def call():
            api.check(lib.vk_volume_merge(C.byref(ddesc), C.byref(source), C.byref(params), api._ptr(counts), api._ptr(workspace),
                                          api.stream()), "vk_volume_merge")
        return dict(S.timed(call, args.reps, flush, lambda: S.restore(dst, state)), counts=[int(c) for c in counts.cpu().numpy()])

    results = {"call": timed(before, sdesc, 8)}
    merged = S.save(dst)                                   # the destination after a merge: every source block is present
    results["settled"] = timed(merged, sdesc, 8)
    results["settled_1"] = timed(merged, sdesc, 1)
    results["idle_1"] = timed(merged, fdesc, 1)
    considered, fused, allocated, left_out, rounds, _ = results["call"]["counts"]
    assert considered == fused == blocks[1] and left_out == 0 and results["settled"]["counts"][1:5] == [fused, 0, 0, 0]
    assert results["idle_1"]["counts"] == [0, 0, 0, 0, 0, 0]

    fuse_us = results["settled_1"]["median_us"] - results["idle_1"]["median_us"]
    idle_round_us = (results["settled"]["median_us"] - results["settled_1"]["median_us"]) / 7
    active_round_us = idle_round_us + (results["call"]["median_us"] - results["settled"]["median_us"]) / max(rounds, 1)
    fuse_bytes = fused * BYTES_PER_FUSED_BLOCK

    # the same bytes moved by a device-to-device copy, flushed the same way
    half = torch.empty(fuse_bytes // 2, dtype=torch.uint8, device="cuda")
    other = torch.empty_like(half)
    copy_us = S.timed(lambda: other.copy_(half), args.reps, flush)["median_us"]

    def rate(us):
        return fuse_bytes / (us * 1e-6) / 1e12 if us > 0 else None

    doc = {"tool": "tools/merge_bench.py", "device": torch.cuda.get_device_name(0),
           "volumes": {"main_blocks": dst.main, "excess_blocks": dst.excess, "voxel_length": bench.VOXEL,
                       "frames_fused_each": args.frames, "blocks_dst": blocks[0], "blocks_src": blocks[1],
                       "blocks_in_common": fused - allocated},
           "method": f"HIP events around the enqueue on the stream, destination restored and the Infinity Cache flushed in front of every repetition, 2 warm-up + {args.reps} timed, median",
           "merge_us": results,
           "call_us": results["call"]["median_us"], "rounds_that_posted": rounds,
           "round_us": {"idle": idle_round_us, "allocating": active_round_us,
                        "what": "idle: (settled - settled_1) / 7; allocating: idle + (call - settled) / rounds that posted"},
           "fuse_pass": {"what": "settled_1 - idle_1, an upper bound (the mark and request passes' cold chain walks over the full source are in it): every source block fused, both pools read from HBM",
                         "us": fuse_us, "blocks": fused, "bytes": fuse_bytes, "TB_per_s": rate(fuse_us)},
           "device_to_device_copy": {"what": "torch copy_ of bytes / 2 (read + write = the same bytes moved), same flush, same run",
                                     "us": copy_us, "bytes_moved": fuse_bytes, "TB_per_s": rate(copy_us)},
           "skip_unobserved": "not timed: the classification is one more read of the source's allocated blocks (10 240 B each)"}
    S.write(doc, args.out)


if __name__ == "__main__":
    main()
