"""Writes tests/golden/rig_views.json: what the CPU oracle's rig Track (oracle.rig_track, increment="rig") computes for
two rigid rings of cameras (BASELINE configs[4]) — per Gauss-Newton step the update and every view's packed float32
system, the final poses, the step counts, and the oracle's own error and rigidity. Results only: the inputs are analytic
(the rippled surface of bench.rig_collective per camera, camera r at yaw RINGS[..][r], the whole rig displaced by one of
ERRORS), so the device tests rebuild them from this module and hold the device to the file.

    python tests/golden/make_rig_views.py            # rewrites the file (a few seconds)

Also the one place the rig scenes are defined: tests/test_oracle_rig.py, tests/test_gpu_rig_oracle.py and
tests/rig_two_ranks_worker.py import RINGS, ERRORS, view_depth, projection, error and rigidity from here."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import scenes  # noqa: E402
from vulcan_amd import vk_types as T  # noqa: E402

FILE = os.path.join(HERE, "rig_views.json")

# camera yaws in degrees, in rank order
RINGS = {
    "pair_180": (0.0, 180.0),
    "pair_90": (0.0, 90.0),
    "three": (0.0, 120.0, 240.0),
    "four": (0.0, 90.0, 180.0, 270.0),
    "eight": tuple(45.0 * r for r in range(8)),
}

# the recorded rigs: ring, image size, how many of ERRORS are tracked
RECORDED = {"pair_90_320x240": ("pair_90", 320, 240, 3), "eight_160x120": ("eight", 160, 120, 1)}


def errors():
    """The world-frame displacements of the whole rig (tests/rig_two_ranks_worker.py; the first is bench.rig_collective's)."""
    return [T.Transform.translate(0.003, -0.002, 0.004) * T.Transform.rotate(0.999995, 0.002, -0.0015, 0.001),
            T.Transform.translate(-0.002, 0.001, 0.002), T.Transform.translate(0.001, 0.003, -0.002)]


def projection(w):
    """The app's intrinsics (given for 640 x 480) scaled to an image `w` wide, in float32."""
    scale = np.float32(w / 640.0)
    return T.Projection.make(*(scale * np.float32(v) for v in scenes.APP_INTRINSICS))


def view_depth(rank, w, h):
    """bench.rig_collective's surface for camera `rank`."""
    y, x = np.mgrid[0:h, 0:w]
    return (1.5 + 0.08 * np.cos(3.0 * x / w + rank) * np.sin(2.0 * y / h + 0.5 * rank)).astype(np.float32)


def truths(ring):
    return [scenes.yaw(a) for a in RINGS[ring]]


def oracle_rig(orc, ring, w, h, error, holes=()):
    """(keys, frames) as oracle HostFrames: camera r's keyframe at its true pose, its frame — the same image — at
    error * truth. A camera listed in `holes` sees nothing (depth 0 everywhere)."""
    keys, frames = [], []
    k = projection(w)
    for rank, truth in enumerate(truths(ring)):
        depth = view_depth(rank, w, h)
        key = orc.HostFrame(depth, k, truth)
        key.compute_normals()
        seen = np.zeros_like(depth) if rank in holes else depth
        frames.append(orc.HostFrame(seen, k, error * truth, normals=key.normals))
        keys.append(key)
    return keys, frames


def residuals(poses, ring):
    """P_r * truth_r^-1 per camera, float64: the world-frame motion camera r is still off by."""
    return [p.matrix().astype(np.float64) @ t.inverse_matrix().astype(np.float64) for p, t in zip(poses, truths(ring))]


def error_of(poses, ring):
    """max entry of |P_r truth_r^-1 - I| over the cameras"""
    return float(max(np.abs(m - np.eye(4)).max() for m in residuals(poses, ring)))


def rigidity_of(poses, ring):
    """max over r of |P_r truth_r^-1 - P_0 truth_0^-1|: 0 for a rig that moved as one body"""
    m = residuals(poses, ring)
    return float(max(np.abs(mr - m[0]).max() for mr in m))


def floats(a):
    """float32 values as JSON numbers that read back to the same bits (a float32 is exact in a double, repr round-trips)"""
    return [float(v) for v in np.asarray(a, dtype=np.float32).ravel()]


def packed27(system):
    """the 27 sums of a 48-float system: hessian [0, 21), gradient [36, 42)"""
    return floats(np.concatenate([system[:21], system[36:42]]))


def unpack27(values):
    system = np.zeros(48, dtype=np.float32)
    system[:21], system[36:42] = values[:21], values[21:27]
    return system


def oracle_track(orc, ring, w, h, error):
    record = []
    keys, frames = oracle_rig(orc, ring, w, h, error)
    poses, steps, _ = orc.rig_track(keys, frames, increment="rig", record=record)
    return {"steps": steps,
            "updates": [floats(r["update"]) for r in record],
            "systems": [[packed27(s) for s in r["systems"]] for r in record],
            "poses": [floats(p.matrix().T) for p in poses],              # column-major, vk_transform.m
            "error": error_of(poses, ring), "rigidity": rigidity_of(poses, ring)}


def make(orc, names=None, first_only=False):
    out = {}
    for name, (ring, w, h, count) in RECORDED.items():
        if names is not None and name not in names:
            continue
        tracks = [oracle_track(orc, ring, w, h, e) for e in errors()[:1 if first_only else count]]
        out[name] = {"ring": ring, "yaw_degrees": list(RINGS[ring]), "width": w, "height": h, "tracks": tracks}
    return out


def load():
    return json.load(open(FILE))


def pose_from(values):
    """T.Transform from a recorded pose (column-major rigid matrix; the inverse is R^T, -R^T t in float64)"""
    m = np.asarray(values, dtype=np.float32).reshape(4, 4).T
    return T.Transform.from_matrices(m, np.linalg.inv(m.astype(np.float64)).astype(np.float32))


if __name__ == "__main__":
    from oracle import oracle
    oracle.build()
    doc = {"what": "oracle.rig_track(increment='rig') per recorded rig: see tests/golden/make_rig_views.py", "rigs": make(oracle)}
    with open(FILE, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    for name, rig in doc["rigs"].items():
        print(name, [(t["steps"], t["error"], t["rigidity"]) for t in rig["tracks"]])
    print(FILE, os.path.getsize(FILE), "bytes")
