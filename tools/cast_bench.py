#!/usr/bin/env python3
"""tools/cast_bench.py — what vk_volume_cast_rays costs next to the raycast it generalises: the steady-state volume of
tools/kbench.py (bench.py's depth workload, 40 frames of the orbit fused at 5 mm) and the 640 x 480 pixel rays of the view
kbench.py times its stages at (the pose after the last fused frame), given to the call as world rays: the camera's centre
and the rotated unprojection of every pixel's centre, searched over the raycast's depth range with its 500 steps.

Four runs: the rays in pixel order (neighbouring lanes march neighbouring rays, a wave holds a 64-pixel stretch of a row) and
in a seeded shuffle (every lane of a wave its own part of the image: the wave takes as many turns as its longest ray, and no
two lanes share a block), each distance-only without a gradient and with colour and gradient. Beside them the `trace` stage
of tools/kbench.py at the same view — Tracer.trace: block bounds, the march, normals — and its `points` stage, the march
alone, both timed here by kbench.py's method (HIP events around --inner back-to-back calls, median of --reps): vk_trace.hip
is the parent commit's file byte for byte, so the stage is the parent's. The cast is timed the same way. One JSON line to
--out (profiles/cast_bench.json). No threshold is set on these numbers.

ref: src/tracer.cu:317-451 (the march), apps/vulcan/vulcan.cu:283-325 (the workload)."""
import argparse
import os

import numpy as np

import volume_bench_support as S
from volume_bench_support import ROOT


def pixel_rays(k, pose, w, h):
    """[h * w, 6] float32: the world rays of the camera at `pose` (a Transform, depth_to_world) through the pixel centres"""
    m = pose.matrix().astype(np.float64)
    ys, xs = np.mgrid[0:h, 0:w]
    d = np.stack([(xs + 0.5 - k.cx) / k.fx, (ys + 0.5 - k.cy) / k.fy, np.ones((h, w))], -1).reshape(-1, 3)
    rays = np.empty((h * w, 6), dtype=np.float32)
    rays[:, :3] = m[:3, 3]
    rays[:, 3:] = d @ m[:3, :3].T
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--inner", type=int, default=10, help="back-to-back launches per timed repetition")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cast_bench.json"))
    ap.add_argument("--variant", help="another build of the library (tools/build_variant.sh): its vk_volume_cast_rays is timed beside "
                                      "the product's, the two alternating per repetition, and must write the same bytes")
    args = ap.parse_args()

    import torch
    import bench
    from vulcan_amd import api, vk_types as T
    torch.cuda.set_device(0)

    k, vol, frame, out, integ, tracer, view = S.steady_state(args.frames)
    depths = torch.zeros((bench.H, bench.W), dtype=torch.float32, device="cuda")
    colors = torch.zeros((bench.H, bench.W, 3), dtype=torch.float32, device="cuda")

    def timed(*calls):
        """the calls alternate per repetition; one result per call"""
        for call in calls:
            call()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = [[] for _ in calls]
        for _ in range(args.reps):
            for which, call in enumerate(calls):
                e0.record()
                for _ in range(args.inner):
                    call()
                e1.record()
                e1.synchronize()
                times[which].append(e0.elapsed_time(e1) * 1e3 / args.inner)
        out = [{"median_us": float(np.median(t)), "min_us": float(min(t)), "max_us": float(max(t))} for t in times]
        return out[0] if len(out) == 1 else out

    raycast = dict(zip(("trace", "points"), timed(lambda: tracer.trace(out), lambda: tracer.compute_points(frame, depths, colors))))
    torch.cuda.synchronize()
    seen = depths > 0

    ordered = pixel_rays(k, view, bench.W, bench.H)
    count = len(ordered)
    order = np.random.default_rng(23).permutation(count)
    rays = {"pixel_order": torch.as_tensor(ordered).cuda(), "shuffled": torch.as_tensor(ordered[order]).cuda()}
    buffers = (torch.empty(count, dtype=torch.float32, device="cuda"), torch.empty(count, dtype=torch.int32, device="cuda"),
               torch.empty((count, 20), dtype=torch.uint8, device="cuda"), torch.empty((count, 4), dtype=torch.float32, device="cuda"))
    forms = {"distance_only": (T.VK_CAST_DISTANCE_ONLY, buffers[:3] + (None,)), "color_and_gradient": (0, buffers)}
    t_min, t_max = vol.depth_range
    results, variant = {}, {}
    other = None
    if args.variant:
        import ctypes as C
        other = C.CDLL(os.path.abspath(args.variant))
        other.vk_volume_cast_rays.argtypes, other.vk_volume_cast_rays.restype = api.lib().vk_volume_cast_rays.argtypes, C.c_int
        shadow = tuple(torch.zeros_like(b) for b in buffers)

    def other_call(tensor, flags, into):
        params = T.CastParams(flags, 500, t_min, t_max)
        api.check(other.vk_volume_cast_rays(api._ref(vol.desc()), api._ptr(tensor), count, None, api._ref(params), api._ptr(into[0]),
                                            api._ptr(into[1]), api._ptr(into[2]), api._ptr(into[3]), api.stream()), "variant")

    for name, tensor in rays.items():
        for form, (flags, into) in forms.items():
            product = lambda: vol._cast_call(tensor, None, flags, t_min, t_max, 500, count=count, out=into)   # noqa: E731
            if other is None:
                r = timed(product)
            else:
                beside = shadow[:3] + ((None,) if into[3] is None else (shadow[3],))
                r, v = timed(product, lambda: other_call(tensor, flags, beside))
                torch.cuda.synchronize()
                v["same_bytes"] = all(bool(torch.equal(a, b)) for a, b in zip(into, beside) if a is not None)
                variant[f"{name}.{form}"] = v
            r["rays_per_second"] = count / (r["median_us"] * 1e-6)
            r["over_trace"] = r["median_us"] / raycast["trace"]["median_us"]
            r["over_points"] = r["median_us"] / raycast["points"]["median_us"]
            results[f"{name}.{form}"] = r
    # the last run was shuffled: undo it, then compare with the raycast's depth image along the optical axis
    torch.cuda.synchronize()
    back = torch.as_tensor(np.argsort(order)).cuda()
    status, t = buffers[1][back].reshape(bench.H, bench.W), buffers[0][back].reshape(bench.H, bench.W)
    hit = status == T.VK_RAY_HIT
    d = torch.as_tensor(ordered[:, 3:]).cuda()
    cosine = (torch.as_tensor(np.ascontiguousarray(view.matrix()[:3, 2], dtype=np.float32)).cuda() * d).sum(-1) / d.norm(dim=-1)
    both = hit & seen
    error = (t * cosine.reshape(bench.H, bench.W) - depths).abs()[both]

    doc = {"tool": "tools/cast_bench.py", "device": torch.cuda.get_device_name(0),
           "volume": {"main_blocks": vol.main, "excess_blocks": vol.excess, "voxel_length": bench.VOXEL, "frames_fused": args.frames,
                      "visible_blocks": int(vol.visible_count)},
           "rays": count, "t_min": t_min, "t_max": t_max, "max_steps": 500,
           "outcomes": {name: int((status == code).sum()) for name, code in (("miss", T.VK_RAY_MISS), ("hit", T.VK_RAY_HIT),
                                                                              ("steps", T.VK_RAY_STEPS), ("invalid", T.VK_RAY_INVALID))},
           "raycast_pixels_with_depth": int(seen.sum()), "both_hit": int(both.sum()),
           "depth_difference_m": {"max": float(error.max()), "p99": float(error.quantile(0.99)), "median": float(error.median())},
           "method": f"HIP events around {args.inner} back-to-back calls, median of {args.reps} (tools/kbench.py's method, for the cast and the raycast alike)",
           "raycast_us": raycast, "cast_us": results}
    if other is not None:
        doc["variant"] = {"library": os.path.basename(args.variant), "cast_us": variant}
    S.write(doc, args.out)


if __name__ == "__main__":
    main()
