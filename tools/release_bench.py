#!/usr/bin/env python3
"""tools/release_bench.py — what vk_volume_release_blocks costs on the bench's volume: Volume(65024, 8192) at 5 mm after the
first 20 frames of bench.py's workload (the sphere room, orbit poses).

Three calls are timed, each from the same restored state: the call changes the volume, so the table, visibility bytes, free
list, counters and voxels are copied back in front of every repetition, and a 1 GiB fill behind the copy takes the pool out of
the 256 MB Infinity Cache (the allocator hands out the highest slots first, the very ones the copy wrote last), so what the
call reads comes from HBM:
  repair      flags 0: no voxel is read or written — the launches of the call itself
  read-all    NO_SURFACE with a threshold no stored distance reaches (|d| <= 1 < 2): every allocated block is streamed once and
              none is released; (read-all - repair) is the classify kernel's streaming time, blocks * 10 240 B its bytes
  box         OUTSIDE_BOX keeping the half space x >= 0: about half the blocks go; they are cleared, not read
HIP events on the stream around the enqueue (no readback inside the timed region), warm-up, median of --reps repetitions.
Next to it the depth integrate launch on the same pool, from `python tools/kbench.py --only integrate`, which this tool starts as
a process of its own when it is done (back-to-back launches on a warm pool: bench.BYTES_PER_BLOCK per visible block + the depth
image). One JSON line to --out (profiles/release_bench.json).

ref: src/volume.cu:304-368 (the allocator that never returns a slot), apps/vulcan/vulcan.cu:283-325 (the workload)."""
import argparse
import ctypes as C
import os
import re
import subprocess
import sys

import volume_bench_support as S
from volume_bench_support import ROOT


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "release_bench.json"))
    args = ap.parse_args()

    import torch
    import bench
    from vulcan_amd import api, vk_types as T
    torch.cuda.set_device(0)
    lib = api.lib()

    vol, = S.replicas(args.frames, 1)
    counters = vol.read_counters()
    visible = int(counters[T.VK_CTR_VISIBLE])
    allocated = int((vol.host_entries()["data"] >= 0).sum())

    saved = S.save(vol)
    workspace = api._dev_bytes(lib.vk_volume_release_workspace_bytes(vol.main, vol.excess), "cuda")
    counts = torch.zeros(4, dtype=torch.int32, device="cuda")
    vdesc = vol.desc()
    flush = S.flush_buffer()

    def timed(rule):
        def call():
            api.check(lib.vk_volume_release_blocks(C.byref(vdesc), C.byref(rule), api._ptr(counts), api._ptr(workspace), api.stream()),
                      "vk_volume_release_blocks")
        return dict(S.timed(call, args.reps, flush, lambda: S.restore(vol, saved)), counts=[int(c) for c in counts.cpu().numpy()])

    repair = T.ReleaseRule()
    read_all = T.ReleaseRule()
    read_all.flags, read_all.min_abs_distance = T.VK_RELEASE_NO_SURFACE, 2.0
    box = T.ReleaseRule()
    box.flags = T.VK_RELEASE_OUTSIDE_BOX
    box.keep_lo[:] = [0, -32768, -32768]
    box.keep_hi[:] = [32767, 32767, 32767]
    results = {"repair": timed(repair), "read_all": timed(read_all), "box_keeps_x_ge_0": timed(box)}
    assert results["read_all"]["counts"][0] == 0 and results["repair"]["counts"][1] == allocated
    stream_us = results["read_all"]["median_us"] - results["repair"]["median_us"]
    classify_gbs = allocated * 10240 / (stream_us * 1e-6) / 1e9 if stream_us > 0 else None
    released = results["box_keeps_x_ge_0"]["counts"][0]
    clear_us = results["box_keeps_x_ge_0"]["median_us"] - results["repair"]["median_us"]

    volume = {"main_blocks": vol.main, "excess_blocks": vol.excess, "voxel_length": bench.VOXEL, "frames_fused": args.frames,
              "allocated_blocks": allocated, "visible_blocks": visible, "excess_pointer": int(counters[T.VK_CTR_EXCESS_PTR])}
    # the depth integrate launch on the same pool: tools/kbench.py's own figure, from a process of its own
    del saved, flush, vol
    torch.cuda.empty_cache()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kbench.py"), "--frames", str(args.frames), "--only", "integrate"],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300).stdout
    m = re.search(r"^integrate\s+median\s+([\d.]+) us.*?([\d.]+) GB/s algorithmic", out, re.M)
    nv = re.search(r"(\d+) visible blocks", out)
    assert m and nv, out
    integrate_us, integrate_gbs, nvis = float(m.group(1)), float(m.group(2)), int(nv.group(1))

    doc = {"tool": "tools/release_bench.py", "device": torch.cuda.get_device_name(0),
           "volume": volume,
           "method": f"HIP events around the enqueue on the stream, state restored and the Infinity Cache flushed in front of every repetition, 2 warm-up + {args.reps} timed, median",
           "release_blocks_us": results,
           "classify_streaming": {"what": "read_all - repair: every allocated block read once, from HBM",
                                  "us": stream_us, "bytes": allocated * 10240, "GB_per_s": classify_gbs},
           "clear_of_released_blocks": {"what": "box - repair: the released blocks overwritten with Voxel::Empty(), none read",
                                        "us": clear_us, "bytes": released * 10240,
                                        "GB_per_s": released * 10240 / (clear_us * 1e-6) / 1e9 if clear_us > 0 else None},
           "depth_integrate": {"what": "python tools/kbench.py --only integrate, same run: vk_integrate_depth after the same frames, back-to-back "
                                       "launches (warm: each re-reads what the one before wrote; read + write of every visible block)",
                               "us": integrate_us, "visible_blocks": nvis, "GB_per_s_algorithmic": integrate_gbs}}
    S.write(doc, args.out)


if __name__ == "__main__":
    main()
