#!/usr/bin/env python3
"""bench.py — throughput of the fusion + raycast hot path on MI355X.

Headline workload (`--workload rgbd`, the default): BASELINE.json's metric is "RGB-D
frames/sec (integrate+raycast), 640x480 @ 5 mm voxels", so one step = one 640x480 RGB-D
frame = Frame::ComputeNormals -> Volume::SetView x3 -> LightIntegrator::Integrate (frame
mask, depth, shaded colour: configs[2]'s integrators) -> Tracer::Trace — the calls of the
reference's frame loop (apps/vulcan/vulcan.cu:297,316-325) — through the C ABI
(include/vk.h), into Volume(65024, 8192) (vulcan.cu:12-13). The three SetView calls are ONE
vk_volume_set_view_rounds(.., 3): same state, the later rounds run on the device and only
when the round before lost a request; in `rgbd` (no tracker reads the normals first) that
call also computes the frame's normals, in its request pass (vk_light_prep.normals_out: the
same normal image, written to the frame). The camera sits at the centre of a 2 m sphere and yaws
0.5 deg per frame: the depth image (resident in HBM) is the same closed form every frame
while new blocks are allocated every frame.

  --workload depth      BASELINE configs[1]: depth-only sequence, DepthIntegrator + Tracer
  --workload rgbd-icp   configs[2] in full, closed loop: a camera moving through a box room
                        with spheres (tests/scenes.py: every pose parameter observable), each
                        frame tracked by PyramidTracker<DepthTracker> against the previous
                        raycast from the previous TRACKED pose, then fused and raycast at the
                        tracked pose; the ground truth only scores the result

A plain run sets up, runs W untimed and K timed steps and prints ONE JSON line: `value` (frames/s
of the K timed steps) and `ms_per_step`. `--full` adds everything else the line can carry: for
`rgbd` the other two workloads under "other_workloads" (same loop, same sizes, fewer steps), the
spread over further windows of K steps, the roofline and the probes, the CPU baseline, and at
N > 1 the rig step below. `--dump-outputs DIR` writes what the last timed step computed (the
raycast images, the frame's normals, the pose) as DIR/<name>.npy; the inputs are closed forms, the
same in every run with the same arguments.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]

N > 1: `python bench.py --gpus N` starts its own N ranks (fresh child processes, one per
GPU, before anything touches the GPU); under an external launcher (torchrun: RANK /
WORLD_SIZE set) it joins that job instead. Every rank owns a replica volume and its own
frames (weak scaling, no data-path collective: SURVEY.md §8e); value = frames of all ranks
/ max-over-ranks time. After the timed loop the ranks run the one step of the path that
does exchange data — the rigid multi-camera rig of configs[4]: per rank the ICP normal
system of its own view, one 48-float all-reduce over RCCL per Gauss-Newton iteration, the
same solve on every rank — and report it under "collective" (--full).

`roofline`: the dominant kernel of the workload (the fused integrate kernel), timed with HIP
events on the launch stream inside the timed region; `cpu_baseline`: the CPU oracle on a
bounded sample of the same frames plus BASELINE configs[0] (dense 128^3, 1 and all cores).
"""
import argparse
import ctypes as C
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 640, 480
VOXEL, TRUNC = 0.005, 0.04
MAIN, EXCESS = 65024, 8192
RADIUS, YAW_STEP = 2.0, 0.5
HBM_PEAK_GBS = 8000.0            # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
HBM_COPY_GBS = 6290.0            # same guide: what a float4 copy sustains (79 % of spec)
L3_BYTES = 256 << 20             # Infinity Cache
BYTES_PER_BLOCK = 4 + 16 + 2 * 512 * 20   # index + entry + voxel read + write
IMAGE_BYTES = {"depth": W * H * 4,                          # depth
               "rgbd": W * H * (4 + 12 + 12 + 4)}           # + colour + normals + mask (light integrator)
METRIC = "RGB-D frames/sec (integrate+raycast), 640x480 @ 5 mm voxels"
LIGHT = (2.0, (0.025, 0.08, 0.0))                           # apps/vulcan/vulcan.cu:87-88
EXTRA_NORMALS = int(os.environ.get("VK_BENCH_EXTRA_NORMALS", "0"))   # experiment only; 0 in every reported run
NORMALS_IN_SET_VIEW = os.environ.get("VK_BENCH_NORMALS_LAUNCH", "0") != "1"   # "1": ComputeNormals as a launch of its own (A/B)
RIG_TIMEOUT_S = 180                                         # N > 1: the rig step (reported next to the headline) may take this long
# N > 1: also time the rig's in-launch exchange (peer-mapped areas over xGMI, vk_icp_track_rig). Off unless asked
# for: the path has never run on more than one GPU (this pool has single-GPU boxes), and a fault in it would take
# the run's headline with it
RIG_IN_LAUNCH_EXCHANGE = os.environ.get("VK_BENCH_RIG_EXCHANGE", "0") == "1"
SET_VIEW_ROUNDS = 3                                         # apps/vulcan/vulcan.cu:316-318
# VK_BENCH_SPLIT_STREAMS=1: the request pass of SetView on a stream of its own, beside the previous frame's raycast
# (vk_volume_set_view_rounds_split), for the workloads that fuse at given poses. Off in every reported run: measured
# 98.1 -> 96.8 us per frame only — the two cross-queue dependencies it puts on the frame's critical cycle cost ~10 us each
# on this runtime (tools/debug/cross_stream_latency_probe.hip) — so the headline stays on one stream
SPLIT_STREAMS = os.environ.get("VK_BENCH_SPLIT_STREAMS", "0") == "1"
# VK_BENCH_REQUESTS_AHEAD (default 1; "0" = A/B): fusion at GIVEN poses knows frame i + 1 while it raycasts frame i, so the
# request pass of SetView(i + 1) rides behind the raycast's workgroups in the same launch (vk_trace_ahead_requests) and
# SetView(i + 1) is left with its handle + visibility launch. Same work, same results (tests/test_gpu_configs.py); one
# launch boundary less per frame. Not for rgbd-icp: its next pose comes out of this raycast.
REQUESTS_AHEAD = os.environ.get("VK_BENCH_REQUESTS_AHEAD", "1") != "0"
# rgbd-icp: the raycast leaves its normal image to the NEXT frame's pyramid launch (vk_trace_ahead(.., normals = NULL) +
# vk_icp_pyramid_track_frame(.., frame_normals_due = 1 | 2)): nobody reads the key frame's normals before that Track, the
# bits are the same, and the frame has one launch less. "0": Tracer::Trace's own normals launch (A/B).
KEY_NORMALS_WITH_PYRAMID = os.environ.get("VK_BENCH_KEY_NORMALS_WITH_PYRAMID", "1") != "0"
# rgbd-icp (round 6): the NEXT frame's pyramid — its normal image and half-resolution level, the raycast's
# normal image and half-resolution level — made by trailing workgroups of THIS frame's raycast launch (vk_trace_ahead_pyramid),
# so that the next Track is its two loop launches only (vk_icp_pyramid_track_built). Built, bit-exact (tests/test_gpu_round6.py),
# and measured to LOSE (profiles/r06_pyramid_ahead.txt): the frame loses its 7.3 us pyramid launch and the raycast launch grows
# by 9.9 us (65.0 -> 74.9: the key side's groups wait for the raycast's last rows, then do their work behind them) — 287.6
# against 284.3 us per frame; with the frame side alone riding (nothing waits) the raycast launch still grows by 3.3 us and
# the frame takes 286.2 against 282.3. Off in every reported run; "1": on (A/B).
PYRAMID_AHEAD = os.environ.get("VK_BENCH_PYRAMID_AHEAD", "0") == "1"
# rgbd-icp (round 6): SetView(i) enqueued right behind Track(i), at the pose the tracker leaves ON THE DEVICE, BEFORE the host
# waits for that pose: VK_BENCH_SET_VIEW_AT_DEVICE_POSE = "2" (default) the whole SetView (vk_volume_set_view_at_device_pose:
# request pass + handle / visibility), "1" its request pass only (vk_volume_requests_at_device_pose; SetView(i) then launches its
# handle + visibility pass once the host has the pose), "0" neither — the host's round trip for the pose in front of SetView, as
# until round 5 (Tracker::EndSolve, then calls that need the pose as launch arguments: ~15 us with the device idle in every
# tracked frame). Same state, bit for bit, in all three (tests/test_gpu_round6.py).
SET_VIEW_AT_DEVICE_POSE = int(os.environ.get("VK_BENCH_SET_VIEW_AT_DEVICE_POSE", "2"))
# experiment only (profiles/r05_integrate_ring.txt): the integrate launch WITHOUT the raycast bounds riding in it (the tracer then
# makes them with launches of its own); never set in a reported run
NO_BOUNDS_AHEAD = os.environ.get("VK_BENCH_NO_BOUNDS_AHEAD", "0") == "1"
# How the roofline sample times an integrate launch. Default: the dispatch's own begin and end (vk_integrate_time_next ->
# hipExtLaunchKernelGGL's start / stop events) — the duration rocprofv3's kernel trace reports. "0": two vk_event_record
# around the call, as until round 5 — that bracket also holds the events' own processing and the launch latency behind
# the first of them (1.7 - 3.5 us of a 34 us launch: 0.555 where the trace says 0.58)
TIME_BY_DISPATCH = os.environ.get("VK_BENCH_TIME_BY_DISPATCH", "1") != "0"
ROOFLINE_SAMPLE_FRAMES = 100                                # untimed frames behind the timed region whose integrate launches are bracketed
# The headline's spread: WINDOWS consecutive windows of --steps frames (the sequence continues; `value` is the first window's).
# The camera yaws 0.5 deg per frame and allocates ~62 new blocks every frame; the app's Volume(65024, 8192) takes that for
# 307 frames — at frame 308 its EXCESS list (8 192 chained entries; the sphere's blocks cluster in the 65 024 buckets) is full
# at 26 k blocks, requests are dropped and upstream's allocator drains the pool (profiles/r06_soak.json, finding 1; the
# default --steps 200 run of rounds 4 and 5 crossed that line in its roofline sample: 20 233 dropped, unnoticed) — so the
# windows and the roofline sample stay inside SEQUENCE_FRAMES: a run with --steps 20 --warmup 5 (the driver's) has all nine
# windows (285 frames), the default --steps 150 has one (270 frames). A run that does cross the line says so: `error`.
WINDOWS = int(os.environ.get("VK_BENCH_WINDOWS", "9"))
SEQUENCE_FRAMES = 300


def sphere_room_depth(k):
    """Depth seen from the centre of a sphere of radius RADIUS: z = R / |unproject(u,v)|
    (identical for every camera rotation about the centre)."""
    y, x = np.mgrid[0:H, 0:W]
    rx = (x + 0.5 - k.cx) / k.fx
    ry = (y + 0.5 - k.cy) / k.fy
    return (RADIUS / np.sqrt(rx * rx + ry * ry + 1.0)).astype(np.float32)


_REAL_STDOUT = None


def emit(result):
    """The one JSON line, on the process's original stdout."""
    line = (json.dumps(result) + "\n").encode()
    sys.stdout.flush()
    os.write(_REAL_STDOUT if _REAL_STDOUT is not None else 1, line)


# --------------------------------------------------------------------- launching ----

def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_ranks(args, argv):
    """`python bench.py --gpus N` without a launcher: N fresh children, one per GPU, started
    BEFORE this process imports torch or touches the GPU (a process that has initialised the
    GPU must never be re-executed). The parent only waits and propagates failure."""
    port = free_port()
    procs = []
    for rank in range(args.gpus):
        env = dict(os.environ)
        env.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(args.gpus),
                   LOCAL_WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env))
    rc = 0
    deadline = None
    ranks = {p.pid: r for r, p in enumerate(procs)}
    while procs:
        for p in list(procs):
            code = p.poll()
            if code is None:
                continue
            procs.remove(p)
            if code != 0:
                print(f"bench.py: rank {ranks[p.pid]} exited {code}", file=sys.stderr)
            if code != 0 and rc == 0:
                rc = code
                deadline = time.time() + 30          # one rank died: the others cannot finish
        if deadline is not None and time.time() > deadline:
            for p in procs:
                print(f"bench.py: rank {ranks[p.pid]} killed (still running 30 s after another rank failed)", file=sys.stderr)
                p.kill()                              # exact children, by handle
            break
        time.sleep(0.05)
    return rc


def launch_selftest(args):
    """What a rank does between being started and touching the GPU, on CPU: join the job
    described by RANK / WORLD_SIZE / MASTER_*, check it is the job --gpus asked for, run the
    rig's collective once over gloo, and let rank 0 print one JSON line."""
    os.environ.setdefault("VK_DIST_BACKEND", "gloo")
    import torch
    from vulcan_amd import dist as vd
    rank, local_rank, world = vd.init(backend="gloo")
    if world != max(1, args.gpus):
        print(f"--gpus {args.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        return 2
    if rank == args.selftest_fail_rank:
        return 3                                   # rehearses a dying rank: the launcher must report it
    system = torch.full((48,), float(rank + 1))
    vd.allreduce_system(system)
    slowest = vd.max_over_ranks(1.0 + rank)
    frames = vd.sum_over_ranks(args.steps)
    per_rank = vd.gather_over_ranks(1.0 + rank)
    vd.barrier()
    result = {"launch_selftest": True, "n_gpus": world, "system_sum": float(system[0]),
              "max_over_ranks": slowest, "frames_all_ranks": frames, "per_rank_ms_per_step": per_rank,
              "local_rank_env": int(os.environ.get("LOCAL_RANK", "-1"))}
    # the rig step's failure protocol, rehearsed with the functions the GPU run uses (vd.agreed_step, rig_failed, the
    # exit code): a step that raises on ONE rank must end EVERY rank non-zero, with the line printed
    collective = {"ok": True, "vk_comm": {"ok": True, "vk_comm_count": world}, "vk_comm_count": world,
                  "update_identical_on_all_ranks": True}
    try:
        def rig_step():
            if rank == args.selftest_rig_fail_rank:
                raise RuntimeError("rehearsed failure inside the rig step")
            return world
        vd.agreed_step("the rehearsed rig step", rig_step)
    except vd.StepFailed as e:
        collective["vk_comm"] = {"ok": False, "error": str(e)}
    result["collective"] = collective
    if rank == 0:
        emit(result)
    vd.shutdown()
    return RIG_FAILED_EXIT if rig_failed(collective) else 0


# ------------------------------------------------------------------- frame loops ----

class RoomSequence:
    """The tracking workload's input, resident in HBM before the timed region: depth + colour of
    every frame of the room sequence (tests/scenes.py) and the true poses, which only score."""

    def __init__(self, count, k):
        import torch
        import scenes
        from concurrent.futures import ThreadPoolExecutor
        self.truth = [scenes.room_pose(i) for i in range(count)]
        with ThreadPoolExecutor(max_workers=8) as pool:
            frames = list(pool.map(lambda p: scenes.room_frame(k, p, W, H, light=LIGHT), self.truth))
        self.depth = [torch.from_numpy(d).cuda() for d, _ in frames]
        self.color = [torch.from_numpy(c).cuda() for _, c in frames]

    def view(self, start, count):
        """frames start .. start + count - 1 as a sequence of its own (the same resident images): another camera's run through
        the same room, a quarter of the swing later — what a second replica volume on the same GPU is fed (MultiLoop)"""
        assert start + count <= len(self.truth)
        other = RoomSequence.__new__(RoomSequence)
        other.truth, other.depth, other.color = (lst[start:start + count] for lst in (self.truth, self.depth, self.color))
        return other


def pose_error(got, truth):
    """(translation error in metres, rotation error in degrees) of a tracked pose."""
    d = got.matrix().astype(np.float64) @ truth.inverse_matrix().astype(np.float64)
    angle = np.degrees(np.arccos(np.clip((np.trace(d[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))
    return float(np.linalg.norm(got.matrix()[:3, 3].astype(np.float64) - truth.matrix()[:3, 3])), float(angle)


class FrameLoop:
    """One rank's replica volume and frame loop, calling the C ABI with descriptors built
    once, the way a C++ caller would (the api.* wrappers rebuild ctypes structs per call)."""

    def __init__(self, workload, poses, volumes=1, sequence=None, stream_input=False, requests_ahead=None):
        import torch
        from vulcan_amd import api, vk_types as T
        import scenes
        self.api, self.T, self.torch = api, T, torch
        self.workload, self.poses, self.sequence = workload, poses, sequence
        self.lib, self.stream = api.lib(), api.stream()
        k = T.Projection.make(*scenes.APP_INTRINSICS)
        self.k = k
        if sequence is None:
            self.depth_np = sphere_room_depth(k)
            self.color_np = scenes.checker_color(W, H, 0.1, 0.9) if workload != "depth" else None
            self.frame = api.Frame(self.depth_np, k, poses[0], color=self.color_np)
        else:
            self.frame = api.Frame(sequence.depth[0], k, sequence.truth[0], color=sequence.color[0])
        if workload != "depth":
            # Frame::ComputeNormals runs every frame, inside the timed step (vulcan.cu:297)
            self.frame.normals = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        self.key = api.Frame(torch.zeros((H, W), dtype=torch.float32, device="cuda"), k, poses[0],
                             color=torch.zeros((H, W, 3), dtype=torch.float32, device="cuda"),
                             normals=torch.zeros((H, W, 3), dtype=torch.float32, device="cuda"))
        self.fdesc, self.kdesc = self.frame.desc(), self.key.desc()
        self.fref, self.kref = C.byref(self.fdesc), C.byref(self.kdesc)
        self.kproj = C.byref(self.k)
        self.n_ptr = None if workload == "depth" else C.c_void_p(self.frame.normals.data_ptr())
        self.out_ptrs = tuple(C.c_void_p(t.data_ptr()) for t in (self.key.depth, self.key.color, self.key.normals))
        self.mode = 0 if workload == "depth" else 2
        # `volumes` > 1: the same sequence applied to several replica volumes in lock step, so
        # that consecutive integrate launches touch different voxels (the past-L3 measurement)
        self.vols = []
        for _ in range(volumes):
            vol = api.Volume(MAIN, EXCESS, voxel_length=VOXEL, truncation_length=TRUNC)
            integ = api.DepthIntegrator(vol) if workload == "depth" else api.LightIntegrator(vol)
            if workload != "depth":
                integ.light = T.Light.make(*LIGHT)
            tracer = api.Tracer(vol)
            vdesc = vol.desc()
            self.vols.append(dict(vol=vol, integ=integ, tracer=tracer, vdesc=vdesc, vref=C.byref(vdesc),
                                  pref=C.byref(integ.params), bref=C.byref(tracer.view_bounds),
                                  lref=C.byref(integ.light) if workload != "depth" else None))
        self.mask = self.records = None
        if workload != "depth":
            self.mask = torch.empty((H, W), dtype=torch.float32, device="cuda")
            self.records = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
        self.m_ptr = None if self.mask is None else C.c_void_p(self.mask.data_ptr())
        self.r_ptr = None if self.records is None else C.c_void_p(self.records.data_ptr())
        self.depth_threshold = 0.2                                  # light_integrator.cu:256
        # Volume::SetView prepares the light integrator's mask and records in its own request pass
        # (vk_light_prep), as the class layer does; one record for all replica volumes
        self.prep = None
        if workload != "depth":
            self.prep = T.LightPrep()
            self.prep.depth_threshold = self.depth_threshold
            self.prep.mask, self.prep.records = self.mask.data_ptr(), self.records.data_ptr()
            self.prep.capacity = W * H
        self.pprep = None if self.prep is None else C.byref(self.prep)
        # --stream-input: the frame's depth and colour images are UPLOADED every frame (upstream: Image::Load's blocking
        # copy, image.h:100-123, vulcan.cu:220,232) — from two pinned staging buffers, on a copy stream of its own, into
        # two slots of device images, frame i + 1 crossing the bus while frame i is fused (vk.h "the input side of a frame")
        # two streams (vk_volume_set_view_rounds_split): the request pass of frame i runs beside the raycast of frame i - 1
        self.split = None
        if SPLIT_STREAMS and workload != "rgbd-icp" and volumes == 1 and (workload == "depth" or NORMALS_IN_SET_VIEW):
            side, requested, integrated = C.c_void_p(), C.c_void_p(), C.c_void_p()
            api.check(self.lib.vk_stream_create(C.byref(side)), "vk_stream_create")
            api.check(self.lib.vk_event_create_ordering(C.byref(requested), 1), "vk_event_create_ordering")   # the pass writes what the waiter reads
            api.check(self.lib.vk_event_create_ordering(C.byref(integrated), 0), "vk_event_create_ordering")
            self.split = {"stream": side, "requested": requested, "integrated": integrated, "frames": 0}
        self.upload = None
        if stream_input:
            assert sequence is None and workload != "rgbd-icp"
            self.upload = self.Upload(self, self.depth_np, self.color_np)
        # the request pass of the NEXT frame behind this frame's raycast (REQUESTS_AHEAD): a second frame descriptor
        # (frame i + 1: the same resident images, the next pose, the next content id) and the record SetView checks
        self.ahead = None
        if ((REQUESTS_AHEAD if requests_ahead is None else requests_ahead) and self.split is None and workload != "rgbd-icp" and volumes == 1
                and (workload == "depth" or NORMALS_IN_SET_VIEW)):
            self.ahead = T.RequestsAhead()
            self.ndesc = T.Frame.from_buffer_copy(bytes(self.fdesc))
            self.nref, self.aref = C.byref(self.ndesc), C.byref(self.ahead)
        self.tracker = None
        self.key_normals_pending = False
        self.tracked_poses, self.gn_steps = [], []
        if workload == "rgbd-icp":
            # PyramidTracker<DepthTracker>::Track through its one C entry point, descriptors built once
            self.tracker = api.PyramidTracker()
            t = self.tracker.tracker
            self.key_view, self.frame_view = t._view(self.key), t._view(self.frame)
            n = int(self.lib.vk_icp_pyramid_floats(W, H, W, H))
            self.pyramid = torch.empty(n, dtype=torch.float32, device="cuda")
            self.track_args = (C.byref(self.key_view), None, C.byref(self.frame_view), C.c_void_p(t.pose.data_ptr()),
                               C.c_void_p(self.pyramid.data_ptr()), C.c_void_p(t._workspace(self.frame).data_ptr()),
                               C.c_void_p(t.system.data_ptr()), C.c_void_p(t.state.data_ptr()),
                               C.c_void_p(t.update.data_ptr()), None, None, t._poll())
            self.pose_dev = C.c_void_p(t.pose.data_ptr())
            self.poll_words = (C.c_int32 * 4).from_address(t._poll_host.value)
            self.built = T.PyramidAhead() if PYRAMID_AHEAD else None
            self.early = T.RequestsAhead() if SET_VIEW_AT_DEVICE_POSE == 1 else None
            self.set_view_early = SET_VIEW_AT_DEVICE_POSE == 2
            self.set_view_done = False
            self._pose_host = t._pose_host
            self._fpose_at = C.addressof(self.fdesc) + T.Frame.depth_to_world.offset
            self._kpose_at = C.addressof(self.kdesc) + T.Frame.depth_to_world.offset
            self.next_view = t._view(self.frame)
            self.pose_on_device = False
            self.current = T.Transform.from_buffer_copy(bytes(sequence.truth[0]))   # the first frame defines the map

    class Upload:
        """SLOTS slots of {pinned staging, device images, `uploaded` event (copy stream), `consumed` event (compute stream)}.
        The copy stream never waits for the compute stream on the device: with such a wait in front of it the runtime
        serialised the copy with the frame's kernels (357 us per frame instead of 114, tools/stream_input_probe.py).
        The HOST waits instead — for the readers of the slot it is about to overwrite, SLOTS frames back, long done."""
        SLOTS = 4

        def __init__(self, loop, depth_np, color_np):
            import torch
            api, lib = loop.api, loop.lib
            self.loop, self.count = loop, 0
            self.copy_stream = C.c_void_p()
            api.check(lib.vk_stream_create(C.byref(self.copy_stream)), "vk_stream_create")
            self.slots = []
            for _ in range(self.SLOTS):
                slot = {"images": [], "events": []}
                for host in (depth_np, color_np):
                    if host is None:
                        continue
                    pinned = C.c_void_p()
                    api.check(lib.vk_malloc_host(C.byref(pinned), host.nbytes), "vk_malloc_host")
                    C.memmove(pinned, host.ctypes.data, host.nbytes)          # the camera's frame, written once: a driver would DMA it
                    dev = torch.empty(host.shape, dtype=torch.float32, device="cuda")
                    slot["images"].append((pinned, dev, host.nbytes))
                for publishes in (1, 0):               # uploaded (the copy wrote the images), consumed (the kernels only read them)
                    e = C.c_void_p()
                    api.check(lib.vk_event_create_ordering(C.byref(e), publishes), "vk_event_create_ordering")
                    slot["events"].append(e)
                slot["consumed_recorded"] = False
                self.slots.append(slot)
            self.bytes_per_frame = sum(n for _, _, n in self.slots[0]["images"])
            self.submit()                                                       # frame 0 on its way

        def submit(self):
            lib, slot = self.loop.lib, self.slots[self.count % self.SLOTS]
            if slot["consumed_recorded"]:
                lib.vk_event_synchronize(slot["events"][1])                     # the slot's last readers (the host waits)
            for pinned, dev, nbytes in slot["images"]:
                lib.vk_memcpy_h2d_async(C.c_void_p(dev.data_ptr()), pinned, nbytes, self.copy_stream)
            lib.vk_event_record(slot["events"][0], self.copy_stream)
            self.count += 1

        def acquire(self, n):
            """frame n's images; the compute stream waits for their upload"""
            slot = self.slots[n % self.SLOTS]
            self.loop.lib.vk_stream_wait_event(self.loop.stream, slot["events"][0])
            return [dev for _, dev, _ in slot["images"]]

        def release(self, n):
            slot = self.slots[n % self.SLOTS]
            self.loop.lib.vk_event_record(slot["events"][1], self.loop.stream)
            slot["consumed_recorded"] = True

        def h2d_rate_GBps(self, reps=40):
            """what the copy stream sustains for this frame's images alone (nothing else running)"""
            import torch
            lib = self.loop.lib
            torch.cuda.synchronize()
            lib.vk_stream_synchronize(self.copy_stream)
            t0 = time.perf_counter()
            for _ in range(reps):
                for pinned, dev, nbytes in self.slots[0]["images"]:
                    lib.vk_memcpy_h2d_async(C.c_void_p(dev.data_ptr()), pinned, nbytes, self.copy_stream)
            lib.vk_stream_synchronize(self.copy_stream)
            return reps * self.bytes_per_frame / (time.perf_counter() - t0) / 1e9

    def step(self, i, ev=None, v=0, by_dispatch=None):
        """one frame: begin (the frame's inputs; a tracked frame: the Track, enqueued) + finish (a tracked frame: the pose,
        waited for; then SetView, Integrate, Trace). Several sequences on one GPU (MultiLoop) call begin for all of them
        before they call finish for any: the host then waits for one sequence's pose while the others' Tracks are queued."""
        self.begin(i)
        self.finish(i, ev, v, by_dispatch)

    def begin(self, i):
        lib, s = self.lib, self.stream
        seq = self.sequence
        n = None
        if self.upload is not None:
            n = self.upload.count - 1                  # the frame this step fuses (its upload was submitted one step ago)
            self.upload.submit()                       # frame n + 1 crosses the bus while frame n is fused
            images = self.upload.acquire(n)
            self.fdesc.depth = images[0].data_ptr()
            if len(images) > 1:
                self.fdesc.color = images[1].data_ptr()
        if seq is not None:
            # the next camera frame: images that are already resident in HBM
            self.fdesc.depth = seq.depth[i].data_ptr()
            self.fdesc.color = seq.color[i].data_ptr()
        rc = 0
        # Frame::ComputeNormals of the input frame (vulcan.cu:297): the tracker needs the normals at once;
        # without one their first consumer is SetView's request pass, which then computes them on the way
        # (vk_light_prep.normals_out: same image, one launch less)
        normals_in_set_view = self.mode == 2 and self.tracker is None and NORMALS_IN_SET_VIEW
        # (a tracked frame: the normals are computed by the launch that builds the tracker's pyramid, vk_icp_pyramid_track_frame)
        normals_with_pyramid = self.tracker is not None and i > 0
        if self.mode == 2 and not normals_in_set_view and not normals_with_pyramid:
            rc = lib.vk_frame_compute_normals(C.c_void_p(self.fdesc.depth), self.kproj, self.n_ptr, W, H, s)   # vulcan.cu:297
        if self.tracker is not None:
            pose = self.current
            if i > 0:
                # tracker -> SetView -> Integrate -> Trace (apps/vulcan/vulcan.cu:300-325): the frame starts
                # from the previous tracked pose and is tracked against the previous raycast, which was
                # made from that pose; the tracked pose is read back, as Tracker::EndSolve does
                a = self.track_args
                self.frame_view.depths = self.fdesc.depth
                # frame.ComputeNormals() + Tracker::BeginSolve's pose upload + PyramidTracker::Track (vulcan.cu:297-311), one call:
                # the start pose and the frame's normal image travel with the pyramid's launch
                due = 1 | (2 if self.key_normals_pending else 0)       # the frame's normals, and the key frame's when the raycast left them out
                self.key_normals_pending = False
                if self.built is not None:
                    # (the level was built behind the previous raycast: no pyramid launch; the start pose is the one the last
                    # Track left on the device — uploaded only in front of the first Track)
                    start = None if (self.pose_on_device and self.built.valid == 1) else C.byref(pose)
                    rc |= lib.vk_icp_pyramid_track_built(a[0], C.byref(pose), a[2], a[3], start, due, C.byref(self.built), *a[4:], s)
                    self.pose_on_device = True
                else:
                    rc |= lib.vk_icp_pyramid_track_frame(a[0], C.byref(pose), a[2], a[3], C.byref(pose), due, *a[4:], s)
                if self.early is not None or self.set_view_early:
                    # SetView(i) — or its request pass — at the pose Track(i) leaves on the device: enqueued now, behind the
                    # Track, before the host waits for the pose (finish). The frame's content is named here, not in finish.
                    self.fdesc.content_id += 2
                    self.fdesc.depth_to_world = pose                   # the start pose: what a cancel would complete
                    if self.mode == 2:
                        self.prep.normals_out = None
                    if self.set_view_early:
                        self.vols[0]["tracer"].view_bounds.valid = 0   # Volume::SetView: new visible list
                        rc |= lib.vk_volume_set_view_at_device_pose(self.vols[0]["vref"], self.fref, a[3], self.pprep, SET_VIEW_ROUNDS, s)
                        self.set_view_done = True
                    else:
                        rc |= lib.vk_volume_requests_at_device_pose(self.vols[0]["vref"], self.fref, a[3], self.pprep, C.byref(self.early), s)
        self._begun = (i, n, rc, normals_in_set_view)

    def finish(self, i, ev=None, v=0, by_dispatch=None):
        lib, s, vv = self.lib, self.stream, self.vols[v]
        by_dispatch = TIME_BY_DISPATCH if by_dispatch is None else by_dispatch
        begun, n, rc, normals_in_set_view = self._begun
        assert begun == i, "finish(i) follows begin(i)"
        tracked = self.tracker is not None and i > 0
        if tracked:
            # Tracker::EndSolve: the pose, from pinned memory — straight into the two descriptors; the host is on the frame's
            # critical path from here to the SetView call below (the request pass enqueued in begin covers 16 us of it), so
            # the loop's own book-keeping (tracked_poses, gn_steps) waits until the frame's launches are out
            rc |= lib.vk_track_wait(self.track_args[-1], s)
            if rc:
                raise self.api.VkError(f"frame {i}: tracking returned {rc}")
            C.memmove(self._fpose_at, self._pose_host, 128)
            C.memmove(self._kpose_at, self._pose_host, 128)
        else:
            pose = self.current if self.tracker is not None else self.poses[i]
            self.fdesc.depth_to_world = pose
            self.kdesc.depth_to_world = pose
        early = self.tracker is not None and self.early is not None and self.early.valid == 1
        done = self.tracker is not None and self.set_view_done      # the whole SetView was enqueued in begin
        if self.tracker is not None:
            self.set_view_done = False
        if not early and not done:
            self.fdesc.content_id += 2             # this step's normals (and images): new content, odd ids
        if not done:
            vv["tracer"].view_bounds.valid = 0                                      # Volume::SetView: new visible list
        # volume.cu:430-437, three times (vulcan.cu:316-318), + light_integrator.cu:277-293
        if normals_in_set_view:
            self.prep.normals_out = self.n_ptr.value
        if self.split is not None:
            sp = self.split
            if sp["frames"] > 0:
                rc |= lib.vk_stream_wait_event(sp["stream"], sp["integrated"])      # the previous Integrate has read lists, mask, records
            if self.upload is not None:
                rc |= lib.vk_stream_wait_event(sp["stream"], self.upload.slots[n % self.upload.SLOTS]["events"][0])   # the frame's images
            rc |= lib.vk_volume_set_view_rounds_split(vv["vref"], self.fref, self.pprep, SET_VIEW_ROUNDS, sp["stream"], sp["requested"], s)
            sp["frames"] += 1
        elif done:
            pass
        elif early:
            rc |= lib.vk_volume_set_view_rounds_ahead(vv["vref"], self.fref, self.pprep, SET_VIEW_ROUNDS, C.byref(self.early), s)
        elif self.ahead is not None:
            rc |= lib.vk_volume_set_view_rounds_ahead(vv["vref"], self.fref, self.pprep, SET_VIEW_ROUNDS, self.aref, s)
        else:
            rc |= lib.vk_volume_set_view_rounds(vv["vref"], self.fref, self.pprep, SET_VIEW_ROUNDS, s)
        if self.mode == 2:
            if lib.vk_light_prepared(self.pprep, self.fref, C.c_float(self.depth_threshold)):
                self.prep.valid = 0
            else:
                rc |= lib.vk_light_prepare(self.fref, self.depth_threshold, self.m_ptr, self.r_ptr, s)
        if ev:
            if by_dispatch:
                rc |= lib.vk_integrate_time_next(ev[0], ev[1])      # the launch records them as its own begin and end
            else:
                lib.vk_event_record(ev[0], s)
        rc |= lib.vk_integrate_ahead(vv["vref"], vv["pref"], self.fref, self.mode, vv["lref"], self.m_ptr, self.r_ptr,
                                     None if NO_BOUNDS_AHEAD else vv["bref"], s)    # *_integrator.cu Integrate
        if ev and not by_dispatch:
            lib.vk_event_record(ev[1], s)
        if self.split is not None:
            lib.vk_event_record(self.split["integrated"], s)
        if self.upload is not None:
            self.upload.release(n)                     # the input images have no reader after Integrate
        if ev and len(ev) > 2:
            lib.vk_event_record(ev[2], s)
        if self.ahead is not None and i + 1 < len(self.poses):
            # Trace(i) + the request pass of SetView(i + 1), one launch
            self.ndesc.depth, self.ndesc.color = self.fdesc.depth, self.fdesc.color
            if self.sequence is not None:          # a sequence of resident camera frames: the NEXT frame's own images
                self.ndesc.depth, self.ndesc.color = self.sequence.depth[i + 1].data_ptr(), self.sequence.color[i + 1].data_ptr()
            if self.upload is not None:
                # the next frame's images: submitted at the top of this step, on the device by now or soon (the launch waits)
                images = self.upload.acquire(n + 1)
                self.ndesc.depth = images[0].data_ptr()
                if len(images) > 1:
                    self.ndesc.color = images[1].data_ptr()
            self.ndesc.depth_to_world = self.poses[i + 1]
            self.ndesc.content_id = self.fdesc.content_id + 2
            if normals_in_set_view:
                self.prep.normals_out = self.n_ptr.value
            rc |= lib.vk_trace_ahead_requests(vv["vref"], self.kref, vv["bref"], *self.out_ptrs, self.nref, self.pprep,
                                              self.aref, s)
        elif self.tracker is not None and self.built is not None and i + 1 < len(self.poses):
            # tracer.cpp:41-100 + the next Track's pyramid (pyramid_tracker.cpp:58-62, frame.cpp:21-58) in the same launch
            self.next_view.depths = self.sequence.depth[i + 1].data_ptr()
            rc |= lib.vk_trace_ahead_pyramid(vv["vref"], self.kref, vv["bref"], *self.out_ptrs, C.byref(self.next_view),
                                             self.track_args[4], C.byref(self.built), s)
            self.key_normals_pending = False
        elif self.tracker is not None and KEY_NORMALS_WITH_PYRAMID and i + 1 < len(self.poses):
            # tracer.cpp:41-95; its normals (:97-100) come with the next frame's pyramid launch
            rc |= lib.vk_trace_ahead(vv["vref"], self.kref, vv["bref"], self.out_ptrs[0], self.out_ptrs[1], None, s)
            self.key_normals_pending = True
        else:
            rc |= lib.vk_trace_ahead(vv["vref"], self.kref, vv["bref"], *self.out_ptrs, s)   # tracer.cpp:41-47
        if ev and len(ev) > 2:
            lib.vk_event_record(ev[3], s)
        for _ in range(EXTRA_NORMALS):      # experiment: what one more launch-floor kernel costs the frame
            rc |= lib.vk_frame_compute_normals(self.out_ptrs[0], self.kproj, self.n_ptr, W, H, s)
        if self.tracker is not None:
            if tracked:
                self.current = self.T.Transform.from_buffer_copy(bytes(self.fdesc.depth_to_world))
                self.gn_steps.append(int(self.poll_words[0]))
            self.tracked_poses.append(self.current)
        if rc:
            raise self.api.VkError(f"frame {i}: C ABI returned {rc}")

    def make_event(self):
        e = C.c_void_p()
        self.api.check(self.lib.vk_event_create(C.byref(e)), "vk_event_create")
        return e

    def elapsed_ms(self, e0, e1):
        ms = C.c_float()
        self.api.check(self.lib.vk_event_elapsed_ms(e0, e1, C.byref(ms)), "vk_event_elapsed_ms")
        return ms.value


class MultiLoop:
    """S independent sequences on ONE GPU (north_star: replica volumes, sharded by frame / camera): S
    replica volumes — 750 MB each of 288 GB —, S FrameLoops, each on a stream of its own, issued by one host thread in lock
    step: begin(i) for every sequence (a tracked frame: its Track enqueued), then finish(i) for every sequence (the pose
    waited for; SetView, Integrate, Trace enqueued). A tracked frame is a strict chain with the device idle in every tail
    (Gauss-Newton steps with 2 us of pixels in 9.4, a raycast whose last third idles, a launch-floor visibility pass): this
    offers the idle device another sequence's INDEPENDENT work. Loop launches stay chained across streams by the library
    (vk_loop_launch_begin / _end: a loop kernel needs all its workgroups resident). Each sequence's volume, images and
    poses are bit-equal to the same sequence run alone (tests/test_gpu_round6.py)."""

    def __init__(self, workload, pose_lists, sequences=None):
        import torch
        self.streams = [torch.cuda.Stream() for _ in pose_lists]
        self.loops = []
        for j, (st, poses) in enumerate(zip(self.streams, pose_lists)):
            with torch.cuda.stream(st):
                self.loops.append(FrameLoop(workload, poses, sequence=None if sequences is None else sequences[j]))
            st.synchronize()

    def step(self, i):
        for loop in self.loops:
            loop.begin(i)
        for loop in self.loops:
            loop.finish(i)


def run_sequences(workload, count, warmup, steps, room=None, stride=60):
    """`count` sequences of `workload` on this GPU (MultiLoop): aggregate frames/s over `steps` frames of every sequence."""
    import torch
    import scenes
    if workload == "rgbd-icp":
        sequences = [room.view(j * stride, warmup + steps) for j in range(count)]
        pose_lists = [seq.truth for seq in sequences]
    else:
        sequences = None
        pose_lists = [[scenes.orbit_pose(i + 7 * j, YAW_STEP) for i in range(warmup + steps)] for j in range(count)]
    torch.cuda.synchronize()             # (the resident input images were written on another stream)
    multi = MultiLoop(workload, pose_lists, sequences)
    # experiment (VK_BENCH_LOOP_GRID_CAP, docs/rounds/r06.md): a Gauss-Newton loop launch holds 4 800 waves on the device for
    # its whole life and squeezes the other sequence's raycast out of its registers; a capped grid (vk_test_hooks.loop_grid_cap:
    # every workgroup takes several pixel groups) leaves room — and makes every step longer. 0 in every reported run.
    from vulcan_amd import api as _api
    cap = int(os.environ.get("VK_BENCH_LOOP_GRID_CAP", "0"))
    with _api.test_hooks(loop_grid_cap=cap):
        for i in range(warmup):
            multi.step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            multi.step(warmup + i)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    from vulcan_amd import vk_types as T
    out = {"sequences": count, "value": count * steps / dt, "unit": "frames/s (all sequences)", "steps": steps, "warmup": warmup,
           "ms_per_frame_of_one_sequence": 1e3 * dt / steps, "frames_per_s_per_sequence": steps / dt,
           "how": f"{count} replica volumes on one GPU, each with its own frames and its own stream; one host thread issues them in "
                  "lock step (begin for all, then finish for all)"}
    dropped = [int(loop.vols[0]["vol"].read_counters()[T.VK_CTR_DROPPED]) for loop in multi.loops]
    out["dropped_requests"] = dropped
    if any(dropped):
        out["error"] = f"allocation requests were dropped ({dropped}): a pool ran dry, the figure is not the configured workload's"
    if workload == "rgbd-icp":
        errs = []
        for loop, seq in zip(multi.loops, sequences):
            e = [pose_error(p, seq.truth[i]) for i, p in enumerate(loop.tracked_poses)][warmup:]
            errs.append({"translation_m": max(x[0] for x in e), "rotation_deg": max(x[1] for x in e)})
        out["pose_error_max_per_sequence"] = errs
    return out, multi


def loop_outputs(loop):
    """What a caller of the timed step holds after the loop's last step, on the host: the raycast (Tracer::Trace's depth,
    and for the colour workloads its shaded colour; its normals unless they are left to the next frame's pyramid launch),
    the input frame's normals (Frame::ComputeNormals) and the pose the frame was fused and raycast at (rgbd-icp: the
    tracked pose)."""
    images = {"raycast_depth": loop.key.depth}
    if loop.workload != "depth":
        images["raycast_color"] = loop.key.color
        images["frame_normals"] = loop.frame.normals
    if not loop.key_normals_pending:
        images["raycast_normals"] = loop.key.normals
    out = {name: t.float().cpu().numpy() for name, t in images.items()}
    out["pose"] = loop.T.Transform.from_buffer_copy(bytes(loop.kdesc.depth_to_world)).matrix().astype(np.float64)
    return out


def write_outputs(path, arrays, cap=64 << 20):
    """DIR/<name>.npy for every array; past `cap` bytes in all, each array is replaced by the same fixed, seeded sample of
    its elements (flattened), in proportion to its size."""
    os.makedirs(path, exist_ok=True)
    total = sum(a.nbytes for a in arrays.values())
    for name, a in arrays.items():
        if total > cap:
            keep = max(1, int(a.size * (cap - 4096 * len(arrays)) / total))
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, keep, replace=False))]
        np.save(os.path.join(path, name + ".npy"), a)


def visible_counts(poses, depths=None):
    """Allocation depends only on the depth image and the pose and is deterministic, so an
    untimed replay of SetView over the same poses gives the visible-block count every
    integrate launch of the timed run saw. Also returns how many SetView rounds ran in all."""
    from vulcan_amd import api, vk_types as T
    import scenes
    k = T.Projection.make(*scenes.APP_INTRINSICS)
    vol = api.Volume(MAIN, EXCESS, voxel_length=VOXEL, truncation_length=TRUNC)
    frame = api.Frame(sphere_room_depth(k) if depths is None else depths[0], k, poses[0])
    out, rounds = [], []
    for i, p in enumerate(poses):
        if depths is not None:
            frame.depth = depths[i]
        frame.depth_to_world = p
        vol.set_view(frame, rounds=SET_VIEW_ROUNDS)
        ctr = vol.read_counters()
        out.append(int(ctr[T.VK_CTR_VISIBLE]))
        rounds.append(int(ctr[T.VK_CTR_ROUNDS]))
    per_frame = np.diff(np.array([0] + rounds))
    return np.array(out, dtype=np.float64), per_frame


def run_workload(workload, poses, warmup, steps, vd, with_roofline, sample_frames=0, stream_input=False, requests_ahead=None,
                 windows=1, room=None, after_timed=None):
    """W untimed + K timed frames (+ `windows` - 1 further windows of K frames of the same sequence, each bracketed like the
    first: the spread of the headline) (+ `sample_frames` untimed frames with event brackets: the roofline sample);
    returns the JSON fields of that workload. `after_timed(loop)` is called once the K timed frames are done, before
    anything else runs on the loop."""
    import torch
    from vulcan_amd import vk_types as T
    import scenes
    sequence = None
    if workload == "rgbd-icp":
        need = warmup + steps * windows + max(1, sample_frames)
        sequence = room.view(0, need) if room is not None else RoomSequence(need, T.Projection.make(*scenes.APP_INTRINSICS))
    loop = FrameLoop(workload, poses, sequence=sequence, stream_input=stream_input, requests_ahead=requests_ahead)

    for i in range(warmup):
        loop.step(i)
    vd.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        loop.step(warmup + i)
    torch.cuda.synchronize()
    vd.barrier()
    local = time.perf_counter() - t0
    elapsed = vd.max_over_ranks(local, device="cuda")
    frames_all = vd.sum_over_ranks(steps, device="cuda")
    per_rank_ms = vd.gather_over_ranks(1e3 * local / steps, device="cuda")      # value uses the max; these say who was slow
    if after_timed is not None:
        after_timed(loop)

    # The spread (a 20-step headline rests on 1.6 ms of wall time): the sequence simply continues for
    # `windows` - 1 further windows of K frames, each between its own barrier + synchronise pair and each the max over
    # ranks, exactly like the first. `value` stays the FIRST window's (steps / ms_per_step match the command line).
    window_s = [elapsed]
    for wnd in range(1, windows):
        vd.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            loop.step(warmup + wnd * steps + i)
        torch.cuda.synchronize()
        vd.barrier()
        window_s.append(vd.max_over_ranks(time.perf_counter() - t0, device="cuda"))
    steps_run = steps * windows

    # The roofline sample: ROOFLINE_SAMPLE_FRAMES more frames of the same sequence, AFTER the timed region, with HIP
    # events (created without the system-scope fence, vk_event_create) around the integrate launch of every frame and
    # around the raycast of every second one. A pair of records costs the stream ~2.7 us, so inside the timed region
    # they cost frames/s (round 3 sampled five frames of the driver's K = 20 run there: 0.48 against rocprofv3's 0.52
    # for the same kernel); out here they cost nothing that is reported, and 120 launches are averaged whatever K is.
    sampled = list(range(steps_run, steps_run + sample_frames)) if with_roofline else []
    traced = set(sampled[::2])
    # every third launch of the sample is timed the old way as well — two event records AROUND the call — so that the line
    # carries both figures from the same run (r04's 0.555 and r05's 0.58 were the same kernels, timed differently)
    bracketed = set(sampled[2::3]) if TIME_BY_DISPATCH else set()
    events = {i: tuple(loop.make_event() for _ in range(4 if i in traced else 2)) for i in sampled}
    for i in sampled:
        loop.step(warmup + i, events[i], by_dispatch=(i not in bracketed) and TIME_BY_DISPATCH)
    # what a pair of event records reads with nothing between them (stated next to the sample, never subtracted)
    pair_us = None
    if with_roofline:
        pairs = [(loop.make_event(), loop.make_event()) for _ in range(32)]
        for e0, e1 in pairs:
            loop.lib.vk_event_record(e0, loop.stream)
            loop.lib.vk_event_record(e1, loop.stream)
    torch.cuda.synchronize()
    if with_roofline:
        pair_us = float(np.mean([loop.elapsed_ms(e0, e1) for e0, e1 in pairs]) * 1e3)

    out = {"value": frames_all / elapsed, "ms_per_step": 1e3 * elapsed / steps, "steps": steps, "warmup": warmup,
           "per_rank_ms_per_step": per_rank_ms}
    if windows > 1:
        fps = [frames_all / w for w in window_s]
        out["windows"] = {"count": windows, "frames_each": steps, "median": float(np.median(fps)), "min": float(min(fps)),
                          "max": float(max(fps)), "frames_per_s": fps,
                          "what": f"{windows} consecutive windows of {steps} frames of the same sequence, each between its own "
                                  "barrier + synchronise pair (max over ranks); `value` is the first"}
    if with_roofline:
        integ_ms = [loop.elapsed_ms(events[i][0], events[i][1]) for i in sampled if i not in bracketed]
        bracket_ms = [loop.elapsed_ms(events[i][0], events[i][1]) for i in sampled if i in bracketed]
        trace_ms = [loop.elapsed_ms(events[i][2], events[i][3]) for i in sampled if i in traced]
        out["_integrate_ms"], out["_trace_ms"], out["_sampled"] = integ_ms, trace_ms, [i for i in sampled if i not in bracketed]
        out["_bracket_ms"], out["_bracketed"] = bracket_ms, sorted(bracketed)
        out["_event_pair_us"] = pair_us
    ctr = loop.vols[0]["vol"].read_counters()
    out["_counters"] = ctr
    # VK_CTR_ROUNDS counts every frame this volume has seen: warm-up, timed AND the roofline sample's
    out["set_view_rounds_run_per_frame"] = float(ctr[T.VK_CTR_ROUNDS]) / (warmup + steps_run + sample_frames * bool(with_roofline))
    # a frame rate measured on a pool that ran dry is not the configured workload: every entry says so
    out["dropped_requests"] = int(ctr[T.VK_CTR_DROPPED])
    if out["dropped_requests"]:
        out["error"] = (f"{out['dropped_requests']} allocation requests were dropped: the pool of {MAIN + EXCESS} blocks ran dry "
                        "during this run, the figure is not the configured workload's")
    if loop.tracker is not None:
        # the closed loop, scored against the ground truth it never saw
        errors = [pose_error(p, sequence.truth[i]) for i, p in enumerate(loop.tracked_poses)]
        timed = errors[warmup:warmup + steps_run]
        steps_timed = np.array(loop.gn_steps[max(0, warmup - 1):warmup + steps_run - 1], dtype=np.int64)
        hist = np.bincount(steps_timed, minlength=21)
        out["tracked_pose_drives_fusion"] = True
        out["pose_error_max"] = {"translation_m": max(e[0] for e in timed), "rotation_deg": max(e[1] for e in timed)}
        out["pose_error_last_frame"] = {"translation_m": timed[-1][0], "rotation_deg": timed[-1][1]}
        motion = pose_error(sequence.truth[warmup + steps_run - 1], sequence.truth[0])
        out["camera_motion_over_run"] = {"translation_m": motion[0], "rotation_deg": motion[1]}
        out["gn_steps_median"] = float(np.median(steps_timed))
        out["gn_steps_histogram_full_resolution_level"] = {str(n): int(c) for n, c in enumerate(hist) if c}
        out["_tracked"] = loop.tracked_poses
        out["_depths"] = sequence.depth
    return out, loop


def past_l3(workload, poses, warmup, frames, nvis, replicas=8):
    """The integrate kernel with its working set pushed past the 256 MiB Infinity Cache: the
    same sequence is applied to `replicas` volumes in lock step, so between two integrate
    launches on one volume the other replicas' voxels (replicas x ~75 MB) have gone through
    the caches. Returns algorithmic GB/s over the event-bracketed launches."""
    import torch
    loop = FrameLoop(workload, poses, volumes=replicas)
    for i in range(warmup):
        for v in range(replicas):
            loop.step(i, v=v)
    pairs = []
    for i in range(warmup, warmup + frames):
        for v in range(replicas):
            ev = (loop.make_event(), loop.make_event())
            loop.step(i, ev, v=v)
            pairs.append((i, ev))
    torch.cuda.synchronize()
    ms = np.array([loop.elapsed_ms(e[0], e[1]) for _, e in pairs])
    alg = np.array([nvis[i] * BYTES_PER_BLOCK + IMAGE_BYTES["depth" if workload == "depth" else "rgbd"] for i, _ in pairs])
    voxel_ws = float(np.mean([nvis[i] for i, _ in pairs])) * 10240 * replicas
    return {"achieved": float(alg.sum() / (ms.sum() * 1e-3) / 1e9), "avg_launch_us": float(ms.mean() * 1e3),
            "launches_timed": len(pairs), "replica_volumes": replicas,
            "voxel_working_set_bytes": voxel_ws, "exceeds_l3": bool(voxel_ws > 2 * L3_BYTES)}


def probes(loop, nvis_last):
    """What this GPU sustains outside the timed region: float4 copies of 1 GiB (four launch
    shapes, best reported) and the integrate kernel's block read-modify-write with the
    arithmetic removed (tools/probe, libvk_probe.so — not part of the product)."""
    import torch
    path = os.path.join(ROOT, "vulcan_amd", "lib", "libvk_probe.so")
    if not os.path.exists(path):
        return {}
    pl = C.CDLL(path)
    pl.vk_probe_stream_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    pl.vk_probe_stream_read.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    pl.vk_probe_block_rmw.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    s = loop.stream

    def timed(fn, bytes_moved, reps=6):
        e0, e1 = loop.make_event(), loop.make_event()
        fn()
        loop.lib.vk_event_record(e0, s)
        for _ in range(reps):
            fn()
        loop.lib.vk_event_record(e1, s)
        return bytes_moved * reps / (loop.elapsed_ms(e0, e1) * 1e-3) / 1e9

    n = 1 << 30
    a = torch.empty(n, dtype=torch.uint8, device="cuda")
    b = torch.empty(n, dtype=torch.uint8, device="cuda")
    a.zero_()
    sink = torch.zeros(4, dtype=torch.float32, device="cuda")
    ap, bp = C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr())
    shapes = {}
    for shape, name in enumerate(("one_float4_per_lane", "four_float4_per_lane", "persistent_grid", "four_float4_nontemporal")):
        shapes[name] = timed(lambda: pl.vk_probe_stream_copy(bp, ap, n, shape, s), 2 * n)
    read = timed(lambda: pl.vk_probe_stream_read(ap, n, C.c_void_p(sink.data_ptr()), s), n)
    del a, b
    vref = loop.vols[0]["vref"]
    nhit = touched_blocks(pl, loop)          # first: it compares against the last raycast of the loop, volume untouched since
    rmw = timed(lambda: pl.vk_probe_block_rmw(vref, 0, s), float(nvis_last) * 2 * 10240, reps=10)
    return {"raycast_blocks_touched": nhit,"measured_copy_GBps": max(shapes.values()), "copy_shapes_GBps": shapes, "measured_read_GBps": read,
            "measured_block_rmw_GBps": rmw, "copy_buffer_bytes": n}


def touched_blocks(pl, loop):
    """Nhit of SURVEY §8d: distinct voxel blocks the rays of the last raycast read, counted by
    the product's own ray march compiled with its counting hook (tools/probe)."""
    import torch
    vv = loop.vols[0]
    vol, tracer = vv["vol"], vv["tracer"]
    touched = torch.zeros(vol.max, dtype=torch.uint8, device="cuda")
    d2, c2 = torch.zeros_like(loop.key.depth), torch.zeros_like(loop.key.color)
    F = C.c_float
    pl.vk_probe_trace_touched.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, F, F, F, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p]
    # the pose of the LAST raycast: step() moves kdesc.depth_to_world, never the key frame's own field (which keeps the pose
    # the frame object was created with — rounds 3 and 4 passed that one here, the images differed and the figures went missing)
    rc = pl.vk_probe_trace_touched(vol.hash_entries.data_ptr(), vol.voxels.data_ptr(), tracer.bounds.data_ptr(), vol.main,
                                   F(np.float32(8) * np.float32(VOXEL)), F(VOXEL), F(TRUNC), C.byref(loop.kdesc.depth_to_world),
                                   C.byref(loop.k), d2.data_ptr(), c2.data_ptr(), W, H, tracer.BOUNDS_W, tracer.BOUNDS_H,
                                   touched.data_ptr(), None, loop.stream)
    torch.cuda.synchronize()
    # the counting kernel must reproduce the product's image; when it does not, the line says so instead of dropping the figures
    if rc != 0:
        return {"error": f"vk_probe_trace_touched returned {rc}"}
    if not torch.equal(d2, loop.key.depth):
        differing = int((d2 != loop.key.depth).sum())
        return {"error": f"the counting raycast's depth image differs from the product's in {differing} of {W * H} pixels"}
    if not torch.equal(c2, loop.key.color):
        return {"error": "the counting raycast's colour image differs from the product's"}
    return {"blocks_touched": int(touched.sum())}



# -------------------------------------------------- configs[0] and configs[3] ----

DENSE_ORIGIN = [[x, y, z] for z in range(42, 58) for y in range(-8, 8) for x in range(-8, 8)]


def dense_128_gpu(reps=64, replicas=8):
    """BASELINE configs[0] (SURVEY 8d Config 1) ON THE DEVICE: the same unit of work cpu_baseline.configs0_dense_128 times on
    the host — one 640x480 depth frame into a dense 128^3 voxel region = 4096 hand-placed blocks (tests/integrator_test.cu:
    141-199 is the arithmetic; tests/test_gpu_configs.py::test_configs0_dense_128_on_the_device holds the device to the
    oracle's bytes for exactly this volume) — through vk_integrate_depth, every launch timed by its own begin / end events.
    Twice: relaunched on ONE volume (its 42 MB of voxels stay in the 256 MiB Infinity Cache, as the CPU's stay in its caches:
    the figure beside the CPU's), and rotating over `replicas` such volumes (336 MB between two launches on the same voxels:
    they come from HBM — the figure that may be called a fraction of the HBM roofline)."""
    import torch
    from vulcan_amd import api, vk_types as T
    import scenes
    k = T.Projection.make(*scenes.APP_INTRINSICS)
    depth_np = sphere_room_depth(k)
    n = len(DENSE_ORIGIN)
    frame = api.Frame(depth_np, k, T.Transform.identity())
    lib, s = api.lib(), api.stream()
    fdesc, params = frame.desc(), T.Integrator.default()
    fref, pref = C.byref(fdesc), C.byref(params)

    def dense_volume():
        vol = api.Volume(8192, 1024, voxel_length=VOXEL, truncation_length=TRUNC)
        entries = vol.host_entries().copy()
        entries["block"]["origin"][:n] = np.array(DENSE_ORIGIN, dtype=np.int16)
        entries["data"][:n] = np.arange(n)
        entries["next"][:n] = -1
        vol.hash_entries.copy_(torch.from_numpy(np.frombuffer(entries.tobytes(), dtype=np.uint8).copy()).cuda())
        vol.visible_blocks[:n] = torch.arange(n, dtype=torch.int32, device="cuda")
        vol.counters[T.VK_CTR_VISIBLE] = n
        desc = vol.desc()
        return vol, desc, C.byref(desc)

    def event():
        e = C.c_void_p()
        api.check(lib.vk_event_create(C.byref(e)), "vk_event_create")
        return e

    def timed(vrefs, count):
        pairs, rc = [(event(), event()) for _ in range(count)], 0
        for i, (e0, e1) in enumerate(pairs):
            rc |= lib.vk_integrate_time_next(e0, e1)
            rc |= lib.vk_integrate_depth(vrefs[i % len(vrefs)], pref, fref, s)
        torch.cuda.synchronize()
        api.check(rc, "vk_integrate_depth (timed)")
        ms = []
        for e0, e1 in pairs:
            t = C.c_float()
            api.check(lib.vk_event_elapsed_ms(e0, e1, C.byref(t)), "vk_event_elapsed_ms")
            ms.append(t.value)
        return np.array(ms)

    volumes = [dense_volume() for _ in range(replicas)]
    vrefs = [v[2] for v in volumes]
    rc = 0
    for vref in vrefs:
        rc |= lib.vk_integrate_depth(vref, pref, fref, s)
    torch.cuda.synchronize()
    api.check(rc, "vk_integrate_depth")
    updated = int((volumes[0][0].host_voxels()["distance_weight"][:n * 512] > 0).sum())
    ms_cached = timed(vrefs[:1], reps)
    ms_hbm = timed(vrefs, reps)
    # back to back on one volume, no events: what a caller sees per call when it does nothing but integrate
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        rc |= lib.vk_integrate_depth(vrefs[0], pref, fref, s)
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) / reps * 1e3
    api.check(rc, "vk_integrate_depth")
    dt, dt_hbm = float(ms_cached.mean()) * 1e-3, float(ms_hbm.mean()) * 1e-3
    bytes_per_launch = n * BYTES_PER_BLOCK + IMAGE_BYTES["depth"]
    return {"ms": dt * 1e3, "ms_median": float(np.median(ms_cached)), "ms_back_to_back": wall_ms, "voxels": n * 512, "blocks": n,
            "voxels_per_s": n * 512 / dt, "voxels_updated": updated, "launches_timed": reps,
            "algorithmic_bytes_per_launch": bytes_per_launch, "algorithmic_GBps": bytes_per_launch / dt / 1e9,
            "memory_level": "infinity-cache assisted (one volume relaunched: its 42 MB of voxels never leave the 256 MiB cache, so the "
                            "rate is the cache's and is NOT a fraction of the HBM roofline; past_l3 is)",
            "past_l3": {"ms": dt_hbm * 1e3, "ms_median": float(np.median(ms_hbm)), "replica_volumes": replicas,
                        "voxel_bytes_between_reuse": replicas * n * 10240, "voxels_per_s": n * 512 / dt_hbm,
                        "algorithmic_GBps": bytes_per_launch / dt_hbm / 1e9,
                        "frac_of_8TBps": bytes_per_launch / dt_hbm / 1e9 / HBM_PEAK_GBS, "launches_timed": reps},
            "timed_by": "the dispatch's own begin / end events (vk_integrate_time_next); ms_back_to_back = wall time per call of "
                        f"{reps} calls enqueued back to back on one volume",
            "kernel": "integrate_pipelined_kernel<depth> (vk_integrate_depth)"}


def pyramid_case(name, w, h):
    """(intrinsics, key depth, key pose, frame depth, start pose, true pose) of a configs[3] case at base size w x h.
    "same surface": tests/test_gpu_configs.py::test_pyramid_tracker_matches_oracle's — a curved surface seen twice, the frame
    started 3.7 mm / 0.3 deg off (three steps at half resolution, one at full). "two views": the room scene (tests/scenes.py)
    rendered from two poses of the room sequence five frames apart (33 mm, 2.6 deg), the frame started at the key frame's
    pose as a live loop would — different images, projective association: eight steps and two to four
    (test_pyramid_tracker_two_views_matches_oracle)."""
    from vulcan_amd import vk_types as T
    import scenes
    scale = w / 640.0
    if name == "same surface":
        k = T.Projection.make(547.0 * scale, 547.0 * scale, 320.0 * scale, 240.0 * scale)
        y, x = np.mgrid[0:h, 0:w]
        depth = (1.0 + 0.05 * np.cos(3.0 * x / w) * np.sin(2.0 * y / h)).astype(np.float32)
        start = T.Transform.translate(0.002, -0.001, 0.003) * T.Transform.rotate(0.999995, 0.002, -0.0015, 0.001)
        return k, depth, T.Transform.identity(), depth, start, T.Transform.identity()
    k = T.Projection.make(*(v * scale for v in scenes.APP_INTRINSICS))
    key_pose, true_pose = scenes.room_pose(20), scenes.room_pose(25)
    key_depth, _ = scenes.room_frame(k, key_pose, w, h)
    frame_depth, _ = scenes.room_frame(k, true_pose, w, h)
    return k, key_depth, key_pose, frame_depth, key_pose, true_pose


PYRAMID_CASES = ("same surface", "two views")


def pyramid_icp(reps=30):
    """BASELINE configs[3]: PyramidTracker<DepthTracker>::Track (src/pyramid_tracker.cpp:52-90: the half-resolution level
    built by Frame::Downsample, src/image.cu:101-165; 15 Gauss-Newton steps on it, then 20 at full resolution, each loop
    ending early at |update| < 1e-6) at base sizes 320x240, 640x480 and 1280x960, through the one C entry point and
    Tracker::EndSolve's pose readback (vk_icp_pyramid_track_frame + vk_track_wait), descriptors built once as FrameLoop does.
    Two cases per size (pyramid_case): the same surface started a few millimetres off, and two views of the room scene — both
    held to the oracle's pose at all three sizes (tests/test_gpu_configs.py). Per size and case: us per Track (median and min of `reps`, host wall clock around the blocking call),
    the steps each level ran, and SURVEY 8(d)'s bytes — 2 * W * H * (4 + 12) per iteration at that level's size — as GB/s
    over the Track."""
    import torch
    from vulcan_amd import api, vk_types as T
    lib, s = api.lib(), api.stream()
    out = {}
    for (w, h) in ((320, 240), (640, 480), (1280, 960)):
        per_start = {}
        for name in PYRAMID_CASES:
            k, key_depth, key_pose, frame_depth, start, truth = pyramid_case(name, w, h)
            key = api.Frame(key_depth, k, key_pose)
            key.compute_normals()
            frame = api.Frame(frame_depth, k, start)
            frame.compute_normals()
            tracker = api.PyramidTracker()
            tracker.keyframe = key
            t = tracker.tracker
            # the half-resolution level alone, once, for its step count (the pyramid call leaves the full level's in its state)
            half_key, half_frame = key.downsample(), frame.downsample()
            t.max_iterations, t.keyframe = 15, half_key
            t.track(half_frame)
            steps_half = int(t.state.cpu()[0])
            t.max_iterations, t.keyframe = 20, key
            key_view, frame_view = t._view(key), t._view(frame)
            n = int(lib.vk_icp_pyramid_floats(w, h, w, h))
            pyramid = torch.empty(n, dtype=torch.float32, device="cuda")
            poll = t._poll()
            args = (C.byref(key_view), C.byref(key.depth_to_world), C.byref(frame_view), C.c_void_p(t.pose.data_ptr()), C.byref(start), 0,
                    C.c_void_p(pyramid.data_ptr()), C.c_void_p(t._workspace(frame).data_ptr()), C.c_void_p(t.system.data_ptr()),
                    C.c_void_p(t.state.data_ptr()), C.c_void_p(t.update.data_ptr()), None, None, poll, s)
            words = (C.c_int32 * 4).from_address(t._poll_host.value)
            times, rc = [], 0
            for i in range(reps + 3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rc |= lib.vk_icp_pyramid_track_frame(*args)
                rc |= lib.vk_track_wait(poll, s)                     # Tracker::EndSolve: the pose, from pinned memory
                if i >= 3:
                    times.append(time.perf_counter() - t0)
            api.check(rc, f"vk_icp_pyramid_track_frame at {w}x{h}")
            steps_full = int(words[0])
            aborted = int(t.state.cpu()[1]) < 0
            pose = T.Transform.from_buffer_copy(C.string_at(t._pose_host, 128))
            us = float(np.median(times) * 1e6)
            steps = steps_half + steps_full
            level_bytes = steps_half * 2 * (w // 2) * (h // 2) * 16 + steps_full * 2 * w * h * 16
            entry = {"us_per_track": us, "us_per_track_min": float(min(times) * 1e6), "tracks_timed": reps,
                     "steps_run": {"half_resolution": steps_half, "full_resolution": steps_full},
                     "us_per_step": us / max(1, steps),
                     "algorithmic_bytes_per_track": level_bytes, "algorithmic_GBps": level_bytes / (us * 1e-6) / 1e9,
                     "frac_of_8TBps": level_bytes / (us * 1e-6) / 1e9 / HBM_PEAK_GBS,
                     "start_off_by": dict(zip(("translation_m", "rotation_deg"), pose_error(start, truth))),
                     "pose_error_after_track": dict(zip(("translation_m", "rotation_deg"), pose_error(pose, truth)))}
            if aborted:
                entry["error"] = "the loop kernel ended with VK_TRACK_ABORTED"
            per_start[name] = entry
            del tracker, pyramid, frame, key
            torch.cuda.empty_cache()
        out[f"{w}x{h}"] = per_start
    return {"workload": "BASELINE configs[3]: PyramidTracker<DepthTracker>::Track, half-resolution level (15 steps enqueued, fewer run "
                        "once |update| < 1e-6) then full resolution (20), at base sizes 320x240 / 640x480 / 1280x960; one C call + "
                        "the pose readback per Track",
            "unit": "us per Track", "bound": "latency: a strict chain of Gauss-Newton steps (exchange + solve, ~9.4 us each), not bandwidth",
            "steps_enqueued": {"half_resolution": 15, "full_resolution": 20},
            "sizes": out}


# ----------------------------------------------------------------- multi-GPU rig ----

def rig_collective(rank, world, vd):
    """BASELINE configs[4]: a rigid rig of `world` cameras, one per GPU. Every rank evaluates
    the ICP normal system of its own view (a19); the packed 48-float system is all-reduced
    over RCCL once per Gauss-Newton iteration; every rank then runs the same solve and applies
    the same world-frame increment to its own camera."""
    import torch
    import torch.distributed as dist
    from vulcan_amd import api, vk_types as T
    import scenes
    k = T.Projection.make(*scenes.APP_INTRINSICS)
    y, x = np.mgrid[0:H, 0:W]
    depth = (1.5 + 0.08 * np.cos(3.0 * x / W + rank) * np.sin(2.0 * y / H + 0.5 * rank)).astype(np.float32)
    rig_pose = scenes.yaw(360.0 * rank / max(world, 1))                 # camera `rank` of the ring
    key = api.Frame(depth, k, rig_pose)
    key.compute_normals()
    # the whole rig has moved by `error` in the world frame: every camera's pose is off by it
    error = T.Transform.translate(0.003, -0.002, 0.004) * T.Transform.rotate(0.999995, 0.002, -0.0015, 0.001)
    frame = api.Frame(depth, k, error * rig_pose, normals=key.normals)
    tracker = api.DepthTracker()
    tracker.keyframe = key
    tracker.reduce_hook = vd.allreduce_system

    def one():
        frame.depth_to_world = error * rig_pose
        return tracker.track(frame)

    one()
    torch.cuda.synchronize()
    vd.barrier()
    frames = 20
    t0 = time.perf_counter()
    for _ in range(frames):
        got = one()
    torch.cuda.synchronize()
    track_ms = vd.max_over_ranks((time.perf_counter() - t0) / frames * 1e3, device="cuda")
    iterations = int(tracker.state.cpu()[0])

    # the bare collective: 48 floats, device memory, compute stream
    buf = torch.ones(48, dtype=torch.float32, device="cuda")
    for _ in range(10):
        dist.all_reduce(buf)
    torch.cuda.synchronize()
    vd.barrier()
    reps = 200
    t0 = time.perf_counter()
    for _ in range(reps):
        dist.all_reduce(buf)
    torch.cuda.synchronize()
    allreduce_us = vd.max_over_ranks((time.perf_counter() - t0) / reps * 1e6, device="cuda")

    identical = updates_identical(tracker, world)
    residual = float(np.abs((got.matrix() @ rig_pose.inverse_matrix()) - np.eye(4)).max())
    out = {"pattern": "all-reduce(sum) of the packed ICP system, 48 x f32, once per Gauss-Newton iteration",
           "backend": dist.get_backend(), "ranks": dist.get_world_size(), "allreduce_us": allreduce_us,
           "iterations_per_frame": iterations, "track_ms_per_frame": track_ms,
           "update_identical_on_all_ranks": bool(identical), "pose_error_after_track": residual, "ok": True}
    out["vk_comm"] = vk_comm_rig(rank, world, vd, tracker, key, frame, error * rig_pose)
    out["vk_comm_count"] = out["vk_comm"].get("vk_comm_count")      # did RCCL itself see `world` ranks (ncclCommCount)
    return out


def vk_comm_rig(rank, world, vd, tracker, key, frame, start):
    """The same rig step through the shipped C binding (libvk_comm.so: vk_comm_* over RCCL, no Python between the
    Gauss-Newton iterations). Every step that can fail on ONE rank alone (creating the communicator, RCCL's own rank
    count, attaching the exchange, a Track that raises) goes through vd.agreed_step: the ranks agree on its outcome before
    any of them enters the next collective, so all of them take the same branch and none waits in a collective another
    rank never reaches. A failure is reported in the line AND ends the run with a non-zero exit code on every rank
    (main: rig_failed), after the headline — measured before the rig step — has been printed."""
    import torch
    import torch.distributed as dist
    from vulcan_amd import api, comm

    def step(what, fn):
        return vd.agreed_step(what, fn, device="cuda")

    c = None
    out = {"ok": False}
    try:
        c = step("vk_comm_init", lambda: comm.Communicator.from_torch_group(rank, world))

        def count():
            seen = c.rccl_count()              # what RCCL itself says, not the launcher's environment
            if seen != world:
                raise RuntimeError(f"ncclCommCount says {seen} ranks, WORLD_SIZE is {world}")
            return seen
        out["vk_comm_count"] = out["ranks_rccl"] = step("vk_comm_count", count)

        tracker.reduce_hook = None

        def tracked(what, call, frames=20):
            """ms per Track; the warm-up and the timed loop are steps of their own, with the barrier BETWEEN them (a
            rank that raised inside a step must not leave its peers in a barrier the step contained)"""
            def once():
                frame.depth_to_world = start
                call(tracker, frame)
                torch.cuda.synchronize()

            def timed():
                t0 = time.perf_counter()
                for _ in range(frames):
                    frame.depth_to_world = start
                    call(tracker, frame)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / frames * 1e3
            step(what + " (first Track)", once)
            vd.barrier()
            return vd.max_over_ranks(step(what, timed), device="cuda")

        out["track_ms_per_frame"] = tracked("vk_icp_track with vk_comm_reduce_hook", c.track)
        out["allreduce_us"] = vd.max_over_ranks(step("vk_comm_allreduce_system", lambda: c.time_allreduce(200)), device="cuda")
        out["iterations_per_frame"] = int(tracker.state.cpu()[0])
        out["update_identical_on_all_ranks"] = updates_identical(tracker, world)
        out["ok"] = True

        # the same Track with the ranks' sums exchanged INSIDE the one-launch loop (peer-mapped areas,
        # vk_comm_exchange_attach + vk_icp_track_rig); reported, not required: until this line has run
        # on a multi-GPU node the path is unmeasured on hardware over xGMI (two processes on
        # one GPU: tests/test_gpu_rig_two_ranks.py)
        if not RIG_IN_LAUNCH_EXCHANGE:
            out["in_launch_exchange"] = {"ok": False, "not_run": True, "error": "not run: set VK_BENCH_RIG_EXCHANGE=1 (never run on "
                                         "more than one GPU; DESIGN.md section 6)"}
        else:
            x = {"ok": False}
            out["in_launch_exchange"] = x
            tracker.comm = None
            c.agree = comm.agree_over_torch_group()
            step("vk_comm_exchange_attach", c.attach_exchange)     # collective, and so is its outcome (vk_comm.h); agreed once more
            # (raises TrackAborted on EVERY rank if any rank gave up, c.agree; any other exception reaches the peers the same way)
            x["track_ms_per_frame"] = tracked("vk_icp_track_rig", c.track_rig)
            x["iterations_per_frame"] = int(tracker.state.cpu()[0])
            x["update_identical_on_all_ranks"] = updates_identical(tracker, world)
            x["ok"] = True
    except vd.StepFailed as e:
        failed = {"ok": False, "error": str(e)}
        if out.get("ok") and "in_launch_exchange" in out:
            out["in_launch_exchange"] = failed       # the RCCL path above stands; the in-launch exchange failed
        else:
            out.update(failed)
    if c is not None:
        try:
            c.close()
        except Exception as e:     # noqa: BLE001
            out.setdefault("close_error", f"{type(e).__name__}: {e}"[:200])
    return out


def updates_identical(tracker, world):
    """every rank solved the same system: the last update vector must be the same bits everywhere"""
    import torch
    import torch.distributed as dist
    upd = tracker.update.clone()
    gathered = [torch.empty_like(upd) for _ in range(world)]
    dist.all_gather(gathered, upd)
    return bool(all(torch.equal(g, gathered[0]) for g in gathered))


def rig_failed(collective):
    """did the rig step FAIL (as opposed to: ran, or was not asked to run)? Then the run ends non-zero on every rank."""
    if not isinstance(collective, dict):
        return False
    if collective.get("ok") is False:
        return True
    vk = collective.get("vk_comm", {})
    if vk.get("ok") is False:
        return True
    x = vk.get("in_launch_exchange", {})
    return x.get("ok") is False and not x.get("not_run")


RIG_FAILED_EXIT = 4


# --------------------------------------------------------------------------- main ----

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--full", action="store_true",
                    help="everything besides the headline as well: the windows' spread, the roofline sample and the "
                         "per-kernel figures, the other workloads, probes, the past-L3 pass, the CPU baseline and, at N > 1, "
                         "the rig step (a plain run sets up, warms up, times --steps frames and prints the line)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step computed (the raycast images, the frame's normals, the pose it was "
                         "fused at) as DIR/<name>.npy")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="--full: CPU-oracle sample budget (0 = skip)")
    ap.add_argument("--workload", default="rgbd", choices=["rgbd", "depth", "rgbd-icp"])
    ap.add_argument("--only", action="store_true", help="--full: skip the other workloads, probes and the past-L3 pass")
    ap.add_argument("--stream-input", action="store_true",
                    help="also run the headline workload with the frame's depth + colour images uploaded over PCIe every frame "
                         "(reported under other_workloads, never instead of the headline)")
    ap.add_argument("--sequences", type=int, default=1,
                    help="N > 1: ONLY time that many independent sequences of --workload on one GPU (a replica volume and a "
                         "stream each, MultiLoop) and print their aggregate frames/s; the default run reports x2 / x4 under "
                         "other_workloads")
    ap.add_argument("--selftest-launch", action="store_true",
                    help="CPU rehearsal of the N>1 launch path: ranks rendezvous over gloo, all-reduce one "
                         "48-float buffer and exit without touching a GPU (tests/test_bench_launch.py)")
    ap.add_argument("--selftest-fail-rank", type=int, default=-1, help=argparse.SUPPRESS)
    ap.add_argument("--selftest-rig-fail-rank", type=int, default=-1, help=argparse.SUPPRESS)
    args = ap.parse_args()

    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args, sys.argv[1:]))
    # stdout carries ONE json line and nothing else: gloo and RCCL print banners on fd 1, so
    # everything written there from here on goes to stderr and the line is written to the real one
    global _REAL_STDOUT
    sys.stdout.flush()
    _REAL_STDOUT = os.dup(1)
    os.dup2(2, 1)
    if args.selftest_launch:
        sys.exit(launch_selftest(args))

    import torch
    from vulcan_amd import api, dist as vd, vk_types as T
    import scenes

    rank, local_rank, world = vd.init()
    assert world == max(1, args.gpus), f"--gpus {args.gpus} but WORLD_SIZE={world}"
    assert torch.cuda.is_available(), "bench.py needs a GPU (no CPU fallback)"
    torch.cuda.set_device(local_rank % torch.cuda.device_count())   # == local_rank on a full node
    api.lib()
    if os.environ.get("VK_BENCH_STREAM", "created") != "legacy":
        # A created stream (what a C++ caller has, and vulcan_amd/host's classes) instead of the legacy default stream torch
        # starts on: launches on the legacy stream follow one another about 1 us later on some boxes of this pool — 85.6 / 86.8 /
        # 85.7 us per frame against 83.4 / 82.5 / 82.9 in three alternating pairs of runs (tools/debug/stream_ab.sh), the kernels
        # alike. VK_BENCH_STREAM=legacy: the old behaviour. The timed region's torch.cuda.synchronize() waits for the device.
        if os.environ.get("VK_BENCH_STREAM") == "vk":      # experiment: the library's own vk_stream_create, as the C++ loop has
            made = C.c_void_p()
            api.check(api.lib().vk_stream_create(C.byref(made)), "vk_stream_create")
            torch.cuda.set_stream(torch.cuda.ExternalStream(made.value))
        else:
            torch.cuda.set_stream(torch.cuda.Stream())

    if args.sequences > 1 or os.environ.get("VK_BENCH_SEQUENCES_ONLY") == "1":
        assert world == 1, "--sequences is a single-GPU measurement"
        room = RoomSequence(args.warmup + args.steps + 60 * (args.sequences - 1), T.Projection.make(*scenes.APP_INTRINSICS)) \
            if args.workload == "rgbd-icp" else None
        o, multi = run_sequences(args.workload, args.sequences, args.warmup, args.steps, room=room)
        o.update(metric=METRIC + f", {args.sequences} independent sequences on one GPU", n_gpus=1, higher_is_better=True, dtype="f32",
                 data="synthetic", ms_per_step=o["ms_per_frame_of_one_sequence"])
        if args.dump_outputs:
            write_outputs(args.dump_outputs, {f"seq{j}_{name}": a for j, loop in enumerate(multi.loops)
                                              for name, a in loop_outputs(loop).items()})
        emit(o)
        vd.shutdown()
        return
    # a plain run times --steps frames and prints the headline; --full adds the windows' spread and the roofline sample
    # behind them (and, further down, everything else the line reports)
    full = args.full
    windows = max(1, min(WINDOWS, (SEQUENCE_FRAMES - args.warmup - ROOFLINE_SAMPLE_FRAMES) // max(1, args.steps))) if full else 1
    sample_frames = ROOFLINE_SAMPLE_FRAMES if full else 0
    timed_frames = args.steps * windows
    # (a plain run still has the pose after its last frame: that frame is the step every other timed frame is, its raycast
    # making the next frame's request pass)
    total = args.warmup + timed_frames + (sample_frames if full else 1)
    # every rank walks the same arc, offset so ranks do not share poses (one degree per rank: the last rank of eight still
    # stays inside the frames the app's pool takes, SEQUENCE_FRAMES)
    poses = [scenes.orbit_pose(i + rank * 2, YAW_STEP) for i in range(total)]
    wl = args.workload
    outputs = {}
    res, loop = run_workload(wl, poses, args.warmup, args.steps, vd, with_roofline=full, sample_frames=sample_frames,
                             windows=windows, after_timed=(lambda lp: outputs.update(loop_outputs(lp)))
                             if args.dump_outputs and rank == 0 else None)
    if outputs:
        write_outputs(args.dump_outputs, outputs)

    tracked, depths = res.pop("_tracked", None), res.pop("_depths", None)
    ctr = res.pop("_counters")
    if full:
        nvis, rounds_per_frame = visible_counts(tracked or poses, depths)
        nvis_timed = nvis[args.warmup:]                   # the timed frames (every window), then the roofline sample's
        image_bytes = IMAGE_BYTES["depth" if wl == "depth" else "rgbd"]
        alg = nvis_timed * BYTES_PER_BLOCK + image_bytes
        sampled = res.pop("_sampled")
        integ_ms, trace_ms = np.array(res.pop("_integrate_ms")), np.array(res.pop("_trace_ms"))
        achieved = float(alg[sampled].sum() / (integ_ms.sum() * 1e-3) / 1e9)
        bracket_ms, bracketed = np.array(res.pop("_bracket_ms")), res.pop("_bracketed")
        by_bracket = float(alg[bracketed].sum() / (bracket_ms.sum() * 1e-3) / 1e9) if len(bracketed) else None
        pair_us = res.pop("_event_pair_us")
        frame_bytes = float(alg[:args.steps].mean())
        voxel_ws = float(nvis_timed[:args.steps].mean()) * 10240

    sphere = ", camera at the centre of a 2 m sphere yawing 0.5 deg/frame"
    names = {"rgbd": "BASELINE configs[2] fusion+raycast: 640x480 RGB-D, Frame::ComputeNormals + SetView x3 + LightIntegrator "
                     "(frame mask, depth, shaded colour in one pass) + Tracer" + sphere,
             "depth": "BASELINE configs[1]: 640x480 depth-only sequence, SetView x3 + DepthIntegrator + Tracer" + sphere,
             "rgbd-icp": "BASELINE configs[2], closed loop: 640x480 RGB-D, Frame::ComputeNormals + PyramidTracker<DepthTracker> "
                         "vs the previous raycast (from the previous tracked pose) + SetView x3 + LightIntegrator + Tracer at "
                         "the TRACKED pose; camera swinging +-24 deg and translating through a 4.4 x 3 x 5.2 m box room with "
                         "9 spheres (closed form, all six pose parameters observable)"}
    if full:
        set_view_policy = {
            "calls_per_frame_upstream": 3, "max_rounds": SET_VIEW_ROUNDS,
            "policy": "one vk_volume_set_view_rounds(.., 3) per frame = the state of upstream's three SetView calls "
                      "(apps/vulcan/vulcan.cu:316-318), bit for bit; rounds 2 and 3 run inside the last launch of round 1, "
                      "and only when the round before lost a request to a bucket contest or dropped one",
            "rounds_run_per_frame": res.pop("set_view_rounds_run_per_frame"),
            "frames_that_needed_more_than_one_round": int((rounds_per_frame > 1).sum()),
        }
        traffic_bytes, traffic_source = pmc_traffic(wl)
    result = {
        "metric": METRIC, "value": res["value"], "unit": "frames/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": res["ms_per_step"],
        "per_rank_ms_per_step": res["per_rank_ms_per_step"],     # rank order; ms_per_step is their max (barrier to barrier)
        **({"windows": res.get("windows", {"count": 1, "frames_each": args.steps, "median": res["value"], "min": res["value"],
                                           "max": res["value"], "frames_per_s": [res["value"]]})} if full else {}),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {
            "workload": names[wl] + ", 5 mm voxels, Volume(65024,8192)",
            **({"set_view": set_view_policy} if full else {}),
            "input_normals": ("Frame::ComputeNormals of the input frame (vulcan.cu:297) is part of every timed step: "
                              + ("by the launch that builds the tracker's pyramid (vk_icp_pyramid_track_frame)"
                                 + (", which also computes the PREVIOUS raycast's normal image (Tracer::Trace's last stage, "
                                    "tracer.cpp:97-100, left out of vk_trace_ahead: one launch less per frame)" if KEY_NORMALS_WITH_PYRAMID else "")
                                 if wl == "rgbd-icp" else
                                 "as a launch of its own" if not NORMALS_IN_SET_VIEW else
                                 "computed inside SetView's request pass (vk_light_prep.normals_out: same normal image, "
                                 "written to the frame; one launch less)"))
                             if wl != "depth" else "not needed by DepthIntegrator (configs[1])",
            "requests_ahead": ("the request pass of SetView(i + 1) rides behind the workgroups of Trace(i) in one launch "
                               "(vk_trace_ahead_requests; the poses are given, so frame i + 1 is known), SetView(i + 1) launches "
                               "its handle + visibility pass only: the same passes per frame, one launch boundary less; the step "
                               "without it is other_workloads['%s-requests-inside-set-view'] (--full)" % wl)
                              if loop.ahead is not None else
                              "no: SetView makes its own request pass" + (" (the next pose comes out of this frame's raycast)"
                                                                          if wl == "rgbd-icp" else ""),
            "frames_per_rank": args.steps, "image": [W, H], "voxel_length": VOXEL, "truncation_length": TRUNC,
            **({"visible_blocks_mean": float(nvis_timed[:args.steps].mean())} if full else {}),
            "allocated_blocks_end": int(min(MAIN + EXCESS, MAIN + EXCESS - 1 - ctr[T.VK_CTR_VOXEL_PTR])),
            "dropped_requests": int(ctr[T.VK_CTR_DROPPED]), "parallelism": f"replica volume per GPU x{world}",
        },
        **({"roofline": {
            "kernel": "integrate_pipelined_kernel<depth%s> (vk_integrate_ahead)" % ("" if wl == "depth" else "+light colour"),
            "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS, "traffic": traffic_bytes, "traffic_source": traffic_source,
            "algorithmic_bytes_per_launch": float(alg[sampled].mean()),
            "avg_launch_us": float(integ_ms.mean() * 1e3), "launches_timed": len(sampled),
            "sample": (f"HIP start / stop events OF every integrate dispatch (vk_integrate_time_next -> hipExtLaunchKernelGGL: the "
                       f"launch's own begin and end, what rocprofv3's kernel trace reports) of {len(sampled)} further frames of the "
                       "same sequence, right after the timed region (no event is recorded inside it)") if TIME_BY_DISPATCH else
                      (f"HIP events recorded AROUND every integrate launch of {len(sampled)} further frames of the same sequence, "
                       "right after the timed region (no event is recorded inside it); the bracket holds event_pair_us and the "
                       "launch latency behind its first event as well"),
            "timed_by": "dispatch" if TIME_BY_DISPATCH else "bracket",
            # the same kernels timed the way the lines up to round 4 timed them (two event records AROUND the call), on every
            # third launch of the same sample: round-over-round comparisons of `frac` must use like with like
            "by_bracket": None if by_bracket is None else {
                "achieved": by_bracket, "frac": by_bracket / HBM_PEAK_GBS, "avg_launch_us": float(bracket_ms.mean() * 1e3),
                "launches_timed": len(bracketed)},
            "event_pair_us": pair_us,      # two vk_event_record with nothing between them: what a bracket would add (not in avg_launch_us when timed_by = dispatch)
            # where the bytes come from at this size: a frame's voxel working set is ~75 MB and
            # consecutive frames overlap almost entirely, so it lives in the 256 MiB Infinity Cache
            "memory_level": "infinity-cache assisted" if voxel_ws < L3_BYTES else "hbm",
            # `frac` above is the kernel as the headline runs it; at this size that is "cache-assisted". `frac_hbm` (filled in below, next
            # to it) is the same kernel with its voxels coming from HBM: eight replica volumes in lock step push the working
            # set past the 256 MiB L3. A reader of ONE key should take frac_hbm for "fraction of the HBM roofline"
            "frac_is": ("cache-assisted: the ~75 MB voxel working set of consecutive frames lives in the 256 MiB Infinity Cache; "
                        "frac_hbm is the figure past it") if voxel_ws < L3_BYTES else "hbm: the working set exceeds the Infinity Cache",
            "frac_hbm": None if voxel_ws < L3_BYTES else achieved / HBM_PEAK_GBS,
            "voxel_working_set_bytes": voxel_ws,
            "frac_of_measured_copy_peak": achieved / HBM_COPY_GBS,
            "frame_level_GBps": frame_bytes / (res["ms_per_step"] * 1e-3) / 1e9,     # per GPU: integrate bytes / frame wall time
            "raycast": {"kernel": ("trace_and_request_kernel: the raycast, the NEXT frame's request pass and the raycast's "
                                   "normals in one launch (vk_trace_ahead_requests)") if loop.ahead is not None else
                                  "compute_points_kernel + compute_normals_kernel (vk_trace_ahead)",
                        "avg_us": float(trace_ms.mean() * 1e3)},
        }} if full else {}),
    }
    if res.get("error"):
        result["error"] = res["error"]           # e.g. the pool ran dry: the headline is not the configured workload's
    for key_ in ("tracked_pose_drives_fusion", "pose_error_max", "pose_error_last_frame", "camera_motion_over_run",
                 "gn_steps_median", "gn_steps_histogram_full_resolution_level"):
        if key_ in res:
            result["config"][key_] = res[key_]

    extras = full and not args.only and world == 1          # measured once, on a single GPU
    if extras:
        pr = probes(loop, nvis[-1])
        result["roofline"].update(pr)
        if pr.get("measured_copy_GBps"):
            result["roofline"]["frac_of_measured_copy_here"] = achieved / pr["measured_copy_GBps"]
        counted = result["roofline"].pop("raycast_blocks_touched", None) or {"error": "libvk_probe.so is not built"}
        nhit = counted.get("blocks_touched")
        if nhit is None:
            result["roofline"]["raycast"]["error"] = counted["error"]      # loud: SURVEY 8(d)'s raycast figures are missing, and why
        else:
            # outputs W*H*(4+12) + bounds 4800*8 + compulsory voxel traffic Nhit * 10240
            ray = result["roofline"]["raycast"]
            ray["blocks_touched"] = nhit
            ray["algorithmic_bytes"] = W * H * 16 + 4800 * 8 + nhit * 10240
            ray["algorithmic_GBps"] = ray["algorithmic_bytes"] / (ray["avg_us"] * 1e-6) / 1e9
            ray["bound"] = "latency / VALU issue (dependent hash -> voxel loads per march step), not bandwidth"
            # (with the next frame's request pass and the normals in the launch, the counters are that launch's)
            fused = "trace_and_request_kernel" in ray["kernel"]
            ray["traffic"], ray["traffic_source"] = pmc_traffic("raycast+requests" if fused else "raycast")
            if fused:
                # + the request pass: depth image read, normals + mask + records written; + the raycast's normals written
                ray["algorithmic_bytes_of_the_launch"] = ray["algorithmic_bytes"] + W * H * (4 + 12 + 4 + 16) + W * H * 12
                ray["algorithmic_GBps"] = ray["algorithmic_bytes_of_the_launch"] / (ray["avg_us"] * 1e-6) / 1e9
            ray["frac_of_8TBps"] = ray["algorithmic_GBps"] / HBM_PEAK_GBS
            # SURVEY §8d "report gather amplification = measured bytes / compulsory bytes": below 1 when a ray reads a few of
            # a block's 512 voxels and the lines it needs are shared between neighbouring rays
            if ray["traffic"]:
                ray["gather_amplification"] = ray["traffic"] / ray.get("algorithmic_bytes_of_the_launch", ray["algorithmic_bytes"])
    del loop
    torch.cuda.empty_cache()

    if extras:
        # the same kernel with the working set pushed out of the Infinity Cache
        if wl != "rgbd-icp":
            pl3 = past_l3(wl, poses, min(args.warmup, 10), 6, nvis)
            pl3["frac"] = pl3["achieved"] / HBM_PEAK_GBS
            pl3["frac_of_measured_copy_peak"] = pl3["achieved"] / HBM_COPY_GBS
            pl3["by_kernel_trace"] = recorded_past_l3(wl)
            result["roofline"]["past_l3"] = pl3
            # next to `frac`: the same kernel when its voxels come from HBM, not from the Infinity Cache
            result["roofline"]["frac_past_l3"] = pl3["frac"]
            result["roofline"]["frac_hbm"] = pl3["frac"]
            torch.cuda.empty_cache()

        others = {}
        k_steps, k_warm = min(args.steps, 100), min(args.warmup, 10)
        # the room sequence (tracking workloads): generated once, long enough for four cameras a quarter of the swing apart
        room = RoomSequence(k_warm + k_steps + 40 + 3 * 60, T.Projection.make(*scenes.APP_INTRINSICS))
        for other in ("depth", "rgbd", "rgbd-icp"):
            if other == wl:
                continue
            o, oloop = run_workload(other, poses[:k_warm + k_steps + 40], k_warm, k_steps, vd, with_roofline=True, sample_frames=40,
                                    room=room)
            o.pop("_event_pair_us", None)
            o.pop("_bracket_ms", None), o.pop("_bracketed", None)
            ims, tms, smp = np.array(o.pop("_integrate_ms")), np.array(o.pop("_trace_ms")), o.pop("_sampled")
            o.pop("_counters")
            onvis = nvis
            if "_tracked" in o:
                del oloop
                oloop = None
                torch.cuda.empty_cache()
                onvis, _ = visible_counts(o.pop("_tracked"), o.pop("_depths"))
                o["visible_blocks_mean"] = float(onvis[k_warm:k_warm + k_steps].mean())
            oalg = onvis[k_warm:k_warm + k_steps + 40] * BYTES_PER_BLOCK + IMAGE_BYTES["depth" if other == "depth" else "rgbd"]
            o["workload"] = names[other]
            o["unit"] = "frames/s"
            o["integrate_avg_us"] = float(ims.mean() * 1e3)
            o["integrate_GBps"] = float(oalg[smp].sum() / (ims.sum() * 1e-3) / 1e9)
            o["integrate_frac_of_8TBps"] = o["integrate_GBps"] / HBM_PEAK_GBS
            o["raycast_avg_us"] = float(tms.mean() * 1e3)
            others[other] = o
            del oloop
            torch.cuda.empty_cache()
        if wl != "rgbd-icp" and REQUESTS_AHEAD:
            # A/B: the same step with SetView making its own request pass (what a caller that does not know frame i + 1 runs)
            k_steps, k_warm = min(args.steps, 200), min(args.warmup, 20)
            o, oloop = run_workload(wl, poses[:k_warm + k_steps], k_warm, k_steps, vd, with_roofline=False, requests_ahead=False)
            assert oloop.ahead is None
            o.pop("_counters")
            o["workload"] = names[wl] + " — vk_volume_set_view_rounds + vk_trace_ahead (no request pass made ahead)"
            o["unit"] = "frames/s"
            others[wl + "-requests-inside-set-view"] = o
            del oloop
            torch.cuda.empty_cache()
        # Several sequences per GPU: replica volumes are 750 MB of 288 GB, and a tracked frame is a strict
        # chain that leaves the device idle in every tail. Aggregate frames/s of 2 and 4 independent sequences, beside the
        # single sequence measured the same way (MultiLoop with one sequence: the same host loop, one stream)
        s_steps, s_warm = min(args.steps, 100), min(args.warmup, 10)      # (what the room sequence above was sized for)
        for name, count in (("rgbd-icp", 1), ("rgbd-icp", 2), ("rgbd-icp", 4), (wl if wl != "rgbd-icp" else "rgbd", 1),
                            (wl if wl != "rgbd-icp" else "rgbd", 2)):
            try:
                o, multi = run_sequences(name, count, s_warm, s_steps, room=room)
                del multi
            except Exception as e:     # noqa: BLE001  (reported next to the headline, never instead of it)
                import traceback
                where = traceback.extract_tb(e.__traceback__)[-1]
                o = {"error": f"{type(e).__name__}: {e} ({os.path.basename(where.filename)}:{where.lineno} {where.line})"[:400]}
            torch.cuda.empty_cache()
            o["workload"] = names[name] + f" — {count} independent sequence(s) on one GPU, a replica volume and a stream each"
            others[f"{name} x{count}"] = o
        for name in ("rgbd-icp", wl if wl != "rgbd-icp" else "rgbd"):
            one = others.get(f"{name} x1", {}).get("value")
            for count in (2, 4):
                o = others.get(f"{name} x{count}")
                if o and one and "value" in o:
                    o["single_sequence_value"] = one
                    o["aggregate_over_single"] = o["value"] / one
        del room
        torch.cuda.empty_cache()
        try:
            others["pyramid-icp"] = pyramid_icp()
        except Exception as e:     # noqa: BLE001  (reported next to the headline, never instead of it)
            others["pyramid-icp"] = {"error": f"{type(e).__name__}: {e}"[:300]}
        result["other_workloads"] = others
        try:
            result["configs0_dense_128_gpu"] = dense_128_gpu()
        except Exception as e:     # noqa: BLE001
            result["configs0_dense_128_gpu"] = {"error": f"{type(e).__name__}: {e}"[:300]}

    if args.stream_input and world == 1 and wl != "rgbd-icp":
        # The input side (VERDICT r3 missing #3): the same step with the frame's images arriving from the host — pinned
        # staging, a copy stream, two slots — instead of waiting in HBM. Reported next to the headline, never as it.
        k_steps, k_warm = min(args.steps, 200), min(args.warmup, 20)
        o, oloop = run_workload(wl, poses[:k_warm + k_steps], k_warm, k_steps, vd, with_roofline=False, stream_input=True)
        o.pop("_counters")
        rate = oloop.upload.h2d_rate_GBps()
        o["workload"] = names[wl] + " — with the frame's depth" + (" + colour" if wl != "depth" else "") + \
            " image uploaded from pinned host memory every frame (ref: image.h:100-123, vulcan.cu:220,232), double-buffered on a copy stream"
        o["unit"] = "frames/s"
        o["input_bytes_per_frame"] = oloop.upload.bytes_per_frame
        o["h2d_GBps_alone"] = rate
        o["pcie_ceiling_frames_per_s"] = rate * 1e9 / oloop.upload.bytes_per_frame
        o["resident_input_frames_per_s"] = res["value"]
        result.setdefault("other_workloads", {})[wl + "-streamed-input"] = o
        del oloop
        torch.cuda.empty_cache()

    if world > 1 and full:
        # the rig step is reported next to the headline, never instead of it: a failure here is
        # recorded (vk_comm_rig makes the ranks agree on every step that can fail on one of them
        # alone before the next collective), and a rank that still waits for a peer longer than
        # RIG_TIMEOUT_S ends the run WITH the headline and a non-zero exit code
        import threading

        def give_up():
            # the headline is printed (it was measured before the rig step and is unaffected), and the run FAILS:
            # the launcher and the driver see a non-zero exit code, not a success
            result["collective"] = {"ok": False, "error": f"the rig step did not finish within {RIG_TIMEOUT_S} s; "
                                    "the headline above was measured before it and is unaffected"}
            if rank == 0:
                emit(result)
            os._exit(3)

        watchdog = threading.Timer(RIG_TIMEOUT_S, give_up)
        watchdog.daemon = True
        watchdog.start()
        try:
            result["collective"] = rig_collective(rank, world, vd)
        except Exception as e:     # noqa: BLE001
            result["collective"] = {"ok": False, "error": f"{type(e).__name__}: {e}"[:400]}
        watchdog.cancel()

    if full and rank == 0 and world == 1 and args.cpu_seconds > 0:   # the CPU leg is reported at N=1 only
        result["cpu_baseline"] = cpu_baseline(wl, poses, args.cpu_seconds)
    gpu_dense = result.pop("configs0_dense_128_gpu", None)
    if gpu_dense is not None:
        # beside the CPU's figure for the IDENTICAL unit of work (VERDICT r5 missing #3)
        if "cpu_baseline" in result:
            dense = result["cpu_baseline"]["configs0_dense_128"]
            dense["gpu"] = gpu_dense
            if "ms" in gpu_dense:
                cpu_keys = [key_ for key_ in dense if key_.endswith(("_core", "_cores"))]
                dense["gpu_over_cpu"] = {key_: dense[key_]["ms"] / gpu_dense["ms"] for key_ in cpu_keys}
                dense["same_voxels_updated"] = bool(dense.get("voxels_updated") == gpu_dense.get("voxels_updated"))
        else:
            result["configs0_dense_128_gpu"] = gpu_dense

    if rank == 0:
        emit(result)
    vd.shutdown()
    if rig_failed(result.get("collective")):
        # the line above carries the headline (measured before the rig step) and the error; the run still FAILS, on every
        # rank: the ranks agreed on the failure (vd.agreed_step), so all of them come through here
        sys.exit(RIG_FAILED_EXIT)


def pmc_traffic(workload):
    """HBM-side bytes per integrate launch from the committed rocprofv3 PMC passes
    (FETCH_SIZE x2 gfx950 correction + WRITE_SIZE, separate passes, tools/traffic.sh): counters
    cannot be collected from inside an unprofiled run, so the newest measurement on file for
    this workload is reported; None when there is none."""
    import glob
    tag = {"depth": "integrate", "raycast": "raycast", "raycast+requests": "trace_and_request"}.get(workload, "integrate_rgbd")
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_{tag}_traffic.json")))
    if not files:
        return None, "no PMC measurement on file for this workload"
    with open(files[-1]) as f:
        value = json.load(f)["bytes_per_launch"]
    return value, (f"profiles/{os.path.basename(files[-1])}: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of tools/traffic.sh, "
                   "read from that file — NOT measured in this run")


def recorded_past_l3(workload):
    """The same past-L3 launches timed by rocprofv3's kernel trace (tools/past_l3_profile.py): an event pair adds its own cost
    and the launch latency behind its first event to what it brackets — 2.7 to 5 us here, which is what separates 0.47 from
    0.50 of the HBM peak. A trace cannot be taken from inside an unprofiled run: the newest measurement on file is reported,
    marked as such; None when there is none."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_integrate_past_l3.json")))
    if not files:
        return None
    with open(files[-1]) as f:
        d = json.load(f).get(workload)
    if not d:
        return None
    return {"avg_launch_us": d["avg_us_rocprof"], "achieved": d["algorithmic_GBps_rocprof"], "frac": d["frac_of_8TBps_rocprof"],
            "launches": d["launches"],
            "source": f"profiles/{os.path.basename(files[-1])}: rocprofv3 --kernel-trace of tools/past_l3_profile.py, read from "
                      "that file — NOT measured in this run"}


def cpu_baseline(workload, poses, seconds):
    """The CPU oracle (oracle/, the restated reference kernels) on the first frames of the
    same sequence until `seconds` of CPU time are spent; OpenMP over blocks / pixels where
    the reference's threads are independent, allocation serial. Plus BASELINE configs[0]:
    one 640x480 depth frame into a dense 128^3 region (4096 blocks), 1 thread and all cores."""
    from oracle import oracle as orc
    from vulcan_amd import vk_types as T
    import scenes
    k = T.Projection.make(*scenes.APP_INTRINSICS)
    depth_np = sphere_room_depth(k)
    # a 1-GPU box owns a 16-core share of the host (not all 256 hardware threads)
    cores = min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1))
    orc.set_threads(cores)
    hv = orc.HostVolume(MAIN, EXCESS, voxel_length=VOXEL, truncation_length=TRUNC)
    color = scenes.checker_color(W, H, 0.1, 0.9) if workload != "depth" else None
    hf = orc.HostFrame(depth_np, k, poses[0], color=color)
    light = T.Light.make(*LIGHT)
    def frame(i):
        hf.depth_to_world = poses[i]
        if workload != "depth":
            hf.compute_normals()                  # Frame::ComputeNormals, every frame (vulcan.cu:297)
        for _ in range(SET_VIEW_ROUNDS):          # vulcan.cu:316-318
            hv.set_view(hf, orc.POLICY_SERIAL)
        orc.integrate_depth(hv, hf)
        if workload != "depth":
            mask = orc.light_frame_mask(hf, 0.2)
            orc.integrate_light_color(hv, hf, light, mask)
        orc.trace(hv, hf)

    for i in range(2):                       # untimed: the cold first frames allocate ~7k blocks
        frame(i)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < 0.7 * seconds and 2 + n < len(poses):
        frame(2 + n)
        n += 1
    dt = time.perf_counter() - t0

    out = {"value": n / dt, "unit": "frames/s", "cores": cores, "kind": "port",
           "sample": f"frames 2..{1 + n} of the same sequence ({dt:.1f} s: "
                     + ("" if workload == "depth" else "input normals + ") + "SetView x3 + "
                     + ("depth integrate" if workload == "depth" else "frame mask + depth + shaded-colour integrate")
                     + f" + raycast + normals each), allocation serial, the rest OpenMP x{cores}"}
    out["configs0_dense_128"] = dense_128(orc, T, depth_np, k, cores, 0.3 * seconds)
    orc.set_threads(1)
    return out


def dense_128(orc, T, depth_np, k, cores, seconds):
    """BASELINE configs[0] (SURVEY §8d Config 1): the integrate arithmetic of
    tests/integrator_test.cu:141-199 over a dense 128^3 voxel region = 16^3 = 4096 blocks of
    8^3 straddling the surface (away from block (0,0,0)), one 640x480 depth frame, identity
    pose; ms and voxels/s on 1 thread and on all cores."""
    hv = orc.HostVolume(8192, 1024, voxel_length=VOXEL, truncation_length=TRUNC)
    hf = orc.HostFrame(depth_np, k, T.Transform.identity())
    # 16^3 blocks centred on the optical axis at the sphere's surface (z = 2 m): x, y in [-8, 8), z in [42, 58)
    origin = np.array([[x, y, z] for z in range(42, 58) for y in range(-8, 8) for x in range(-8, 8)], dtype=np.int16)
    n = len(origin)
    hv.hash_entries["block"]["origin"][:n] = origin
    hv.hash_entries["data"][:n] = np.arange(n)
    hv.hash_entries["next"][:n] = -1
    hv.visible_blocks[:n] = np.arange(n)
    hv.counters[T.VK_CTR_VISIBLE] = n
    voxels = n * 512
    out = {"voxels": voxels, "blocks": n}
    for name, threads in (("1_core", 1), (f"{cores}_cores", cores)):
        orc.set_threads(threads)
        orc.integrate_depth(hv, hf)
        reps, t0 = 0, time.perf_counter()
        while reps < 3 or (time.perf_counter() - t0 < 0.5 * seconds and reps < 200):
            orc.integrate_depth(hv, hf)
            reps += 1
        dt = (time.perf_counter() - t0) / reps
        out[name] = {"ms": dt * 1e3, "voxels_per_s": voxels / dt, "threads": threads}
    touched = int((hv.voxels["distance_weight"][:voxels] > 0).sum())
    out["voxels_updated"] = touched
    return out


if __name__ == "__main__":
    main()
