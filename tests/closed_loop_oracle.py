"""The oracle's side of the reference app's frame loop (apps/vulcan/vulcan.cu:297-325), shared by the tests that hold a
device loop to it (tests/test_gpu_closed_loop.py, tests/test_gpu_tracked_bench_step.py): per frame ComputeNormals ->
(a Track against the previous raycast, from the previous pose) -> SetView x3 -> depth + frame mask + shaded colour ->
Trace at the frame's pose. No GPU, nothing of the device in here."""
from vulcan_amd import vk_types as T

VOLUME = (65024, 8192, 0.005, 0.04)          # apps/vulcan/vulcan.cu:12-13: main, excess, voxel length, truncation length
POSE_ATOL = 2e-5                             # per entry, matrix and inverse: the project's bound for a tracked pose against the oracle's


def oracle_loop(orc, k, inputs, light, first_pose, track=None, poses=None, params=None, volume=VOLUME):
    """`inputs`: [(depth, colour)] per frame. The pose of frame 0 is `first_pose`. Frame i > 0 is fused and raycast
      * at `poses[i]` when `poses` is given (a loop led through given poses: nothing is tracked), else
      * at `track(key, frame)`: the previous raycast as the key frame, the frame started at the previous pose — the
        closed loop, the tracked pose fed forward.
    Returns the volume and per frame a dict: pose, the frame's normal image, the raycast (depth, color, normals, bounds),
    the visible count behind SetView, and `key` — the raycast as the HostFrame the next Track is made against."""
    main, excess, voxel, trunc = volume
    params = T.Integrator.default() if params is None else params
    hv = orc.HostVolume(main, excess, voxel_length=voxel, truncation_length=trunc)
    pose, hkey, out = first_pose, None, []
    for i, (depth, color) in enumerate(inputs):
        hf = orc.HostFrame(depth, k, pose, color=color)
        hf.compute_normals()
        if i > 0:
            if poses is not None:
                pose = poses[i]
            else:
                pose = track(hkey, hf)
        hf.depth_to_world = pose
        for _ in range(3):
            hv.set_view(hf, orc.POLICY_MAXKEY)
        orc.integrate_depth(hv, hf, params)
        orc.integrate_light_color(hv, hf, light, orc.light_frame_mask(hf, 0.2), params)
        odepth, ocolor, onormals, obounds = orc.trace(hv, hf)
        hkey = orc.HostFrame(odepth, k, pose, color=ocolor, normals=onormals)
        out.append(dict(pose=pose, frame_normals=hf.normals, depth=odepth, color=ocolor, normals=onormals, bounds=obounds,
                        visible=hv.visible_count, key=hkey))
    return hv, out
