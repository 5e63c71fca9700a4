#!/usr/bin/env python3
"""tools/release_soak.py — the long run that shows what Volume.release_blocks is for. Round 6's soak (docs/rounds/r06.md §4,
tools/soak.py) found that the shipped app's Volume(65024, 8192) has a full excess list at about frame 4 000 of the tracked
loop, drops requests from then on and has an empty pool at frame 6 000. Two legs of tools/soak.py's tracked loop (bench's
`rgbd-icp` step on the looped room sequence: PyramidTracker<DepthTracker> against the previous raycast, fusion and raycast at
the tracked pose) on that volume:

  plain     the loop as it is, until VK_CTR_DROPPED is no longer 0 (looked at every --look frames): the frame of the first drop
  released  the same loop, calling release_blocks(unobserved=True, min_abs_distance=--threshold) every --interval frames,
            for --frames frames: dropped requests, blocks in use, excess entries in use and the pose error at every call,
            and the time of every call (HIP events around it)

--threshold and --interval are choices of this run, not constants of the library. One JSON document to --out.
ref: src/volume.cu:304-368 (the allocator), apps/vulcan/vulcan.cu:297-325 (the loop)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20000)
    ap.add_argument("--interval", type=int, default=500, help="frames between two release_blocks calls")
    ap.add_argument("--threshold", type=float, default=0.75, help="min_abs_distance, in units of the stored (normalised) distance")
    ap.add_argument("--look", type=int, default=250, help="plain leg: frames between two looks at VK_CTR_DROPPED")
    ap.add_argument("--plain-frames", type=int, default=8000, help="plain leg: give up looking for a drop after this many frames")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "release_soak.json"))
    args = ap.parse_args()

    import torch
    import bench
    import make_fixtures as mf
    from soak import Looped
    from vulcan_amd import api, vk_types as T
    torch.cuda.set_device(0)
    api.lib()
    torch.cuda.set_stream(torch.cuda.Stream())

    k, inputs = mf.soak_inputs(mf.SOAK_CYCLE)
    truth = [p for _, _, p in inputs]
    depth = [torch.from_numpy(d).cuda() for d, _, _ in inputs]
    color = [torch.from_numpy(c).cuda() for _, c, _ in inputs]
    torch.cuda.synchronize()

    def looped(n):
        seq = bench.RoomSequence.__new__(bench.RoomSequence)
        seq.truth, seq.depth, seq.color = Looped(truth, n), Looped(depth, n), Looped(color, n)
        return seq

    def state(vol):
        ctr = vol.read_counters()
        return {"dropped_requests": int(ctr[T.VK_CTR_DROPPED]), "voxel_pointer": int(ctr[T.VK_CTR_VOXEL_PTR]),
                "excess_entries_in_use": int(ctr[T.VK_CTR_EXCESS_PTR]) - vol.main, "visible_blocks": int(ctr[T.VK_CTR_VISIBLE])}

    doc = {"tool": "tools/release_soak.py", "device": torch.cuda.get_device_name(0), "cycle_frames": mf.SOAK_CYCLE,
           "volume": {"main_blocks": bench.MAIN, "excess_blocks": bench.EXCESS, "voxel_length": bench.VOXEL},
           "choices_of_this_run": {"interval_frames": args.interval, "min_abs_distance": args.threshold, "unobserved": True}}

    # ---- plain: where the unmodified loop first drops a request
    n = args.plain_frames
    seq = looped(n + 1)
    loop = bench.FrameLoop("rgbd-icp", seq.truth, sequence=seq)
    vol = loop.vols[0]["vol"]
    first_drop, looks = None, []
    for i in range(n):
        loop.step(i)
        if (i + 1) % args.look == 0:
            torch.cuda.synchronize()
            looks.append(dict(frame=i + 1, **state(vol)))
            if looks[-1]["dropped_requests"] > 0:
                first_drop = i + 1
                break
    doc["plain_leg"] = {"frames_run": looks[-1]["frame"] if looks else 0, "first_look_with_a_dropped_request": first_drop,
                        "looked_every": args.look, "last_looks": looks[-4:]}
    print(json.dumps(doc["plain_leg"]), flush=True)
    del loop, vol
    torch.cuda.empty_cache()

    # ---- released: the same loop with a release every --interval frames
    n = args.frames
    seq = looped(n + 1)
    loop = bench.FrameLoop("rgbd-icp", seq.truth, sequence=seq)
    vol = loop.vols[0]["vol"]
    calls, call_us, window_from = [], [], 0
    t0 = time.time()
    for i in range(n):
        loop.step(i)
        if (i + 1) % args.interval == 0:
            before = state(vol)            # (synchronises: the loop is between SetView calls here)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            counts = vol.release_blocks(unobserved=True, min_abs_distance=args.threshold)
            e1.record()
            e1.synchronize()
            if loop.prep is not None:
                loop.prep.valid = 0        # the loop's own light preparation record (the volume has none attached)
            call_us.append(e0.elapsed_time(e1) * 1e3)
            errs = [bench.pose_error(loop.tracked_poses[j], seq.truth[j]) for j in range(window_from, i + 1)]
            calls.append({"frame": i + 1, "released": counts[0], "kept": counts[1], "excess_entries_in_use": counts[2],
                          "free_slots": counts[3], "excess_entries_before": before["excess_entries_in_use"],
                          "dropped_requests": before["dropped_requests"], "call_us": call_us[-1],
                          "pose_error_max_mm": 1e3 * max(e[0] for e in errs)})
            window_from = i + 1
            loop.tracked_poses[:i + 1] = [None] * (i + 1)
            if len(calls) % 8 == 0:
                print(json.dumps(calls[-1]), flush=True)
    torch.cuda.synchronize()
    end = state(vol)
    t = np.array(call_us)
    # the first call at or behind the frame at which the plain loop had dropped a request still finds none dropped
    behind = [c for c in calls if first_drop is not None and c["frame"] >= first_drop]
    passed = bool(behind and behind[0]["dropped_requests"] == 0)
    doc["released_leg"] = {"frames": n, "seconds": time.time() - t0, "frames_per_s": n / (time.time() - t0), "calls": len(calls),
                           "dropped_requests_at_the_end": end["dropped_requests"], "end": end,
                           "passed_the_plain_legs_first_drop_without_dropping": passed,
                           "last_call_that_found_no_dropped_request": max((c["frame"] for c in calls if c["dropped_requests"] == 0), default=None),
                           "first_call_that_found_a_dropped_request": next((c["frame"] for c in calls if c["dropped_requests"] > 0), None),
                           "call_us": {"median": float(np.median(t)), "min": float(t.min()), "max": float(t.max())} if len(t) else None,
                           "largest_excess_entries_in_use": max(c["excess_entries_before"] for c in calls) if calls else None,
                           "largest_pose_error_mm": max(c["pose_error_max_mm"] for c in calls) if calls else None,
                           "per_call": calls}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    summary = {key: value for key, value in doc["released_leg"].items() if key != "per_call"}
    print(json.dumps(summary))
    return 0 if doc["released_leg"]["passed_the_plain_legs_first_drop_without_dropping"] else 1


if __name__ == "__main__":
    sys.exit(main())
