"""usage: tools/extract_bench.py [--attributes] [--calls N] [--rounds R] — time of one mesh extraction on the bench volume
(the 2 m sphere room of bench.py, 30 fused RGB-D frames, about 7.3 k blocks), between two events on the stream.
--attributes times vk_extract_mesh_attributes (colours and normals) beside vk_extract_mesh, alternating the two R times,
and prints what the attribute launch adds."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import bench, scenes
from vulcan_amd import api, vk_types as T

parser = argparse.ArgumentParser()
parser.add_argument("--attributes", action="store_true")
parser.add_argument("--calls", type=int, default=20)
parser.add_argument("--rounds", type=int, default=5)
args = parser.parse_args()

k = T.Projection.make(*scenes.APP_INTRINSICS)
depth = bench.sphere_room_depth(k)
vol = api.Volume(bench.MAIN, bench.EXCESS, voxel_length=bench.VOXEL, truncation_length=bench.TRUNC)
frame = api.Frame(depth, k, T.Transform.identity(), color=scenes.checker_color(bench.W, bench.H, 0.1, 0.9))
integ = api.ColorIntegrator(vol)
for i in range(30):
    frame.depth_to_world = scenes.orbit_pose(i, bench.YAW_STEP)
    vol.set_view(frame); integ.integrate(frame)
torch.cuda.synchronize()


def timed(ex, **what):
    """microseconds per extraction over args.calls calls"""
    m = ex.extract(**what); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s = torch.cuda.current_stream()
    e0.record(s)
    for _ in range(args.calls): m = ex.extract(**what)
    e1.record(s); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.calls * 1e3, m


for all_alloc in (False, True):
    ex = api.Extractor(vol); ex.all_allocated = all_alloc
    us, m = timed(ex)
    p, f = m.host()
    print(f"all_allocated={all_alloc}: {us:.1f} us per extraction, {len(p)} points, {len(f)} faces, blocks {vol.visible_count if not all_alloc else 'all'}")
    if args.attributes:
        plain, full, colors_only, normals_only = [], [], [], []
        for _ in range(args.rounds):
            plain.append(timed(ex)[0])
            full.append(timed(ex, colors=True, normals=True)[0])
            colors_only.append(timed(ex, colors=True)[0])
            normals_only.append(timed(ex, normals=True)[0])
        row = lambda name, v: f"  {name:34s} median {np.median(v):7.1f} us  (min {min(v):.1f}, max {max(v):.1f} over {len(v)} rounds of {args.calls} calls)"
        print(row("vk_extract_mesh", plain))
        print(row("vk_extract_mesh_attributes, both", full))
        print(row("vk_extract_mesh_attributes, colours", colors_only))
        print(row("vk_extract_mesh_attributes, normals", normals_only))
        print(f"  the attribute launch adds {np.median(full) - np.median(plain):.1f} us ({ex.blocks} blocks listed)")
