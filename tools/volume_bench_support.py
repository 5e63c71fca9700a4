"""tools/volume_bench_support.py — what the bench tools of the volume operations share ({release, merge, merge_pose, register,
sample, cast, integrate_rays}_bench.py): the volumes they measure on, the state a call changes and its way back, the flushed
event loop, the kernels of a trace, and the JSON line. Importing it puts the repository and tests/ on sys.path."""
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# what release and the merges change next to the voxels: table, visibility bytes, free list, counters
STATE = ("hash_entries", "block_visibility", "free_voxel_blocks", "counters")


def replicas(frames, count=2):
    """`count` volumes of bench.py's size, replica h fused from frames h * frames .. (h + 1) * frames - 1 of its depth workload
    (the sphere room, orbit poses)"""
    import torch
    import bench
    import scenes
    vols = []
    for half in range(count):
        poses = [scenes.orbit_pose(half * frames + i, bench.YAW_STEP) for i in range(frames)]
        loop = bench.FrameLoop("depth", poses)
        for i in range(frames):
            loop.step(i)          # (the last step announces no further frame: the volume is between SetView calls)
        torch.cuda.synchronize()
        vols.append(loop.vols[0]["vol"])
        del loop
    return vols


def steady_state(frames):
    """tools/kbench.py's steady state: `frames` frames of bench.py's depth workload fused and raycast, then SetView at the
    pose after the last: (projection, volume, frame and raycast frame at that view, integrator, tracer, the view's pose)"""
    import torch
    import bench
    import scenes
    from vulcan_amd import api, vk_types as T
    k = T.Projection.make(*scenes.APP_INTRINSICS)
    depth = bench.sphere_room_depth(k)
    poses = [scenes.orbit_pose(i, bench.YAW_STEP) for i in range(frames + 1)]
    vol = api.Volume(bench.MAIN, bench.EXCESS, voxel_length=bench.VOXEL, truncation_length=bench.TRUNC)
    frame = api.Frame(depth, k, poses[0])
    out = api.Frame(torch.zeros((bench.H, bench.W), dtype=torch.float32, device="cuda"), k, poses[0])
    integ = api.DepthIntegrator(vol)
    tracer = api.Tracer(vol)
    for i in range(frames):
        frame.depth_to_world = poses[i]
        out.depth_to_world = poses[i]
        vol.set_view(frame)
        integ.integrate(frame)
        tracer.trace(out)
    view = poses[frames]
    frame.depth_to_world = view
    out.depth_to_world = view
    vol.set_view(frame)
    torch.cuda.synchronize()
    return k, vol, frame, out, integ, tracer, view


def save(volume, names=STATE + ("voxels",)):
    """device copies of the buffers `names` of `volume`"""
    return {name: getattr(volume, name).clone() for name in names}


def restore(volume, saved):
    for name, tensor in saved.items():
        getattr(volume, name).copy_(tensor)


def flush_buffer():
    """1 GiB whose fill takes everything before it out of the 256 MB Infinity Cache"""
    import torch
    return torch.empty(1 << 30, dtype=torch.uint8, device="cuda")


def timed(call, reps, flush, before=lambda: None):
    """median / min / max in us of `call` between HIP events on the stream (no readback in between): `before()` and the
    flush in front of each of 2 warm-up + `reps` repetitions"""
    import torch
    times = []
    for rep in range(reps + 2):
        before()
        flush.fill_(1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        if rep >= 2:                                   # two warm-up repetitions
            times.append(e0.elapsed_time(e1) * 1e3)
    t = np.array(times)
    return {"median_us": float(np.median(t)), "min_us": float(t.min()), "max_us": float(t.max())}


def kernel_durations(directory):
    """{kernel: durations in us, in stream order} of the rocprofv3 --kernel-trace run under `directory`; a kernel's name
    without its namespace, return type and arguments"""
    path = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)[0]
    durations = {}
    for row in sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"])):
        name = row["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        durations.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
    return {name: np.array(t) for name, t in durations.items()}


def kernel_row(name, t):
    """a kernel's line of a --kernels table: calls, median, min, max (us)"""
    return f"{name:<44}{len(t):>6}{np.median(t):>9.2f}{t.min():>9.2f}{t.max():>9.2f}"


KERNEL_HEADER = f"{'kernel':<44}{'calls':>6}{'median':>9}{'min':>9}{'max':>9}"


def write(doc, path):
    """the tool's one JSON line: to `path` and to stdout"""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(doc) + "\n")
    print(json.dumps(doc))
