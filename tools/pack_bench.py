#!/usr/bin/env python3
"""tools/pack_bench.py — what vk_volume_pack and vk_volume_merge_packed cost on the bench's volume: two replicas
Volume(65024, 8192) at 5 mm, each fused from a different half of bench.py's depth workload (tools/merge_bench.py's pair);
the second is packed, and its pack merged into the first next to the merge of the volume itself.

A 1 GiB fill in front of every repetition takes the pools out of the 256 MB Infinity Cache: what a call reads comes from
HBM. HIP events on the stream around the enqueue (no readback inside the timed region), two warm-up repetitions, median of
--reps. Timed:
  pack         the whole enqueue of a pack call into arrays of exactly the selected size: listing, scan, list, gather
  count_only   the same call with voxels == NULL: listing and scan, nothing gathered (what Volume.pack pays to size the pack)
  gather       pack - count_only: one wave per block, 10 240 B read and 10 240 B written each — an upper bound, the list pass
               is in it
  copy         vk_memcpy_d2d of the pack's voxel bytes, same flush, same run: the yardstick of DESIGN.md §10
  merge_volume vk_volume_merge(dst, src) as tools/merge_bench.py's `call`, the destination restored in front of every repetition
  merge_pack   vk_volume_merge_packed(dst, pack of src), likewise: the same rounds, the same fuse pass, no mark pass, and
               one lane per block instead of one per table entry
One JSON line to --out (profiles/pack_bench.json). Moving a pack to another GPU is two plain copies and is not measured here.

ref: src/volume.cu:183-190 (the chain walk that names the blocks), apps/vulcan/vulcan.cu:283-325 (the workload)."""
import argparse
import ctypes as C
import os

import volume_bench_support as S
from volume_bench_support import ROOT

BLOCK_BYTES = 10240


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20, help="frames fused into each replica")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_bench.json"))
    args = ap.parse_args()

    import torch
    import bench
    from vulcan_amd import api, vk_types as T
    torch.cuda.set_device(0)
    lib = api.lib()

    dst, src = S.replicas(args.frames)
    blocks = [int((v.host_entries()["data"] >= 0).sum()) for v in (dst, src)]
    pack = src.pack()
    assert len(pack) == blocks[1]
    flush = S.flush_buffer()
    ddesc, sdesc = dst.desc(), src.desc()

    # ---- pack
    workspace = api._dev_bytes(lib.vk_volume_pack_workspace_bytes(src.main, src.excess), "cuda")
    counts = torch.zeros(4, dtype=torch.int32, device="cuda")
    full, none = pack.desc(), T.BlockPack()

    def pack_call(into):
        def call():
            api.check(lib.vk_volume_pack(C.byref(sdesc), None, C.byref(into), api._ptr(counts), api._ptr(workspace), api.stream()),
                      "vk_volume_pack")
        return call

    results = {"pack": S.timed(pack_call(full), args.reps, flush)}
    assert [int(c) for c in counts.cpu().numpy()] == [blocks[1], blocks[1], blocks[1], 0]
    results["count_only"] = S.timed(pack_call(none), args.reps, flush)
    assert [int(c) for c in counts.cpu().numpy()] == [blocks[1], blocks[1], 0, 0]
    copy_bytes = blocks[1] * BLOCK_BYTES
    other = torch.empty_like(pack.voxels)
    results["copy"] = S.timed(lambda: api.check(lib.vk_memcpy_d2d(api._ptr(other), api._ptr(pack.voxels), copy_bytes, api.stream()),
                                                "vk_memcpy_d2d"), args.reps, flush)
    assert torch.equal(other, pack.voxels)
    gather_us = results["pack"]["median_us"] - results["count_only"]["median_us"]

    # ---- merge: the volume, then its pack, into the same destination
    before = S.save(dst)
    params = T.MergeParams(0, 8, 16.0, 16.0)
    merge_workspace = api._dev_bytes(lib.vk_volume_merge_workspace_bytes(src.main, src.excess), "cuda")
    packed_workspace = api._dev_bytes(lib.vk_volume_merge_packed_workspace_bytes(len(pack)), "cuda")
    six = torch.zeros(6, dtype=torch.int32, device="cuda")

    def merge_volume():
        api.check(lib.vk_volume_merge(C.byref(ddesc), C.byref(sdesc), C.byref(params), api._ptr(six), api._ptr(merge_workspace),
                                      api.stream()), "vk_volume_merge")

    def merge_pack():
        api.check(lib.vk_volume_merge_packed(C.byref(ddesc), C.byref(full), len(pack), pack.voxel_length, pack.truncation_length,
                                             C.byref(params), api._ptr(six), api._ptr(packed_workspace), api.stream()),
                  "vk_volume_merge_packed")

    states = {}
    for name, call in (("merge_volume", merge_volume), ("merge_pack", merge_pack)):
        results[name] = dict(S.timed(call, args.reps, flush, lambda: S.restore(dst, before)), counts=[int(c) for c in six.cpu().numpy()])
        states[name] = S.save(dst)
    assert results["merge_volume"]["counts"] == results["merge_pack"]["counts"] and results["merge_pack"]["counts"][3] == 0
    for name in states["merge_volume"]:
        assert torch.equal(states["merge_volume"][name], states["merge_pack"][name]), name      # bit for bit, here too

    def rate(nbytes, us):
        return nbytes / (us * 1e-6) / 1e12 if us > 0 else None

    doc = {"tool": "tools/pack_bench.py", "device": torch.cuda.get_device_name(0),
           "volumes": {"main_blocks": dst.main, "excess_blocks": dst.excess, "voxel_length": bench.VOXEL,
                       "frames_fused_each": args.frames, "blocks_dst": blocks[0], "blocks_src": blocks[1],
                       "pool_bytes": src.max * BLOCK_BYTES, "pack_bytes": copy_bytes + 8 * blocks[1]},
           "method": f"HIP events around the enqueue on the stream, the Infinity Cache flushed (and for the merges the destination restored) in front of every repetition, 2 warm-up + {args.reps} timed, median",
           "us": results,
           "pack_us": results["pack"]["median_us"], "count_only_us": results["count_only"]["median_us"],
           "gather_pass": {"what": "pack - count_only, an upper bound (the list pass is in it): 10 240 B read and 10 240 B written per block",
                           "us": gather_us, "blocks": blocks[1], "bytes_moved": 2 * copy_bytes, "TB_per_s": rate(2 * copy_bytes, gather_us)},
           "device_to_device_copy": {"what": "vk_memcpy_d2d of the pack's voxel bytes, same flush, same run",
                                     "us": results["copy"]["median_us"], "bytes_moved": 2 * copy_bytes,
                                     "TB_per_s": rate(2 * copy_bytes, results["copy"]["median_us"])},
           "gather_over_copy": results["copy"]["median_us"] / gather_us if gather_us > 0 else None,
           "pack_over_copy": results["copy"]["median_us"] / results["pack"]["median_us"],
           "merge_volume_us": results["merge_volume"]["median_us"], "merge_pack_us": results["merge_pack"]["median_us"],
           "merge_pack_over_merge_volume": results["merge_pack"]["median_us"] / results["merge_volume"]["median_us"],
           "multi_gpu": "not measured: one GPU; moving a pack between devices is two plain copies of origins and voxels"}
    S.write(doc, args.out)


if __name__ == "__main__":
    main()
