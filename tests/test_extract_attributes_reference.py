"""The definition of vk_extract_mesh_attributes (include/vk.h; tests/extract_attributes_reference.py states it in numpy) held
against what a mesh's colours and normals must be, on the CPU: the 160x120 `sphere` scene of tests/test_gpu_extract.py fused by
the oracle with checker_color(w, h, 0.1, 0.9) — 52 868 vertices in 1 209 blocks.

MEASURED HERE (the bound of the full-size GPU test, tests/test_gpu_extract_attributes.py, is 1.5 x this figure): the 99th
percentile of the angle between a vertex normal and the analytic normal of the scene's surface is 62.71 degrees (median
13.26, largest 72.99). The figure is large because this scene undersamples its surface: a pixel covers 10 to 15 mm at 1.4 to
2 m, more than the 8 mm voxel, so on the steep flanks the fused distance is a staircase of pixels (within 0.3 of the disc's
radius the median is 4.3 and the 99th percentile 7.3 degrees; the normals of the mesh's own faces are further off, median
20.0). At 640x480 and 5 mm a pixel is smaller than a voxel."""
import numpy as np
import pytest

import extract_attributes_reference as A
from extract_attributes_reference import ANGLE_P99_DEGREES


@pytest.fixture(scope="module")
def sphere(orc):
    hv = A.fused(orc, "sphere")
    points, faces, skipped = orc.extract_mesh(hv, True, True)
    statistics = {}
    colors, normals = A.extract_attributes(orc, hv, True, True, statistics)
    assert skipped == 0 and len(points) == len(colors) == len(normals) > 50000
    return hv, points, faces, colors, normals, statistics


def test_normals_have_unit_length_and_none_is_zero(sphere):
    _, _, _, _, normals, statistics = sphere
    # the condition under which no normal can vanish: along its own edge both endpoint gradients are non-zero (the forward
    # and backward forms are d(b) - d(a) of a cut edge; a central difference could cancel, and here none does)
    assert statistics["own_axis_zero"] == 0
    assert statistics["zero_normals"] == 0 and (normals != 0).any(axis=1).all()
    # sqrt, and per component a square and a division: three roundings of 6e-8 each stay below 1e-6
    length = np.linalg.norm(normals.astype(np.float64), axis=1)
    print("largest | |n| - 1 |", np.abs(length - 1).max())
    assert np.abs(length - 1).max() < 1e-6


def test_colours_stay_in_the_range_of_the_stored_colours(sphere):
    """A lerp of stored values cannot leave their range. The stored range is the checker's [0.1, 0.9] up to the float32
    rounding of the integrator's running average (colour * weight + sample) / (weight + 1): three operations, 6e-8 relative
    each, so 2e-7 at most — the largest stored channel is 0.90000004, one float32 step above 0.9f."""
    hv, _, _, colors, _, statistics = sphere
    stored = hv.voxels["color"][hv.voxels["color_weight"] != 0]
    lo, hi = stored.min(), stored.max()
    print("stored", repr(lo), repr(hi), "vertices", repr(colors.min()), repr(colors.max()))
    assert abs(float(lo) - 0.1) < 2e-7 and abs(float(hi) - 0.9) < 2e-7
    assert colors.min() >= lo and colors.max() <= hi
    assert statistics["color_none"] == 0                      # or a (0, 0, 0) would have left the range


def test_vertex_normals_agree_with_the_faces(sphere):
    _, points, faces, _, normals, _ = sphere
    tri = points[faces].astype(np.float64)
    face_normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    big = 0.5 * np.linalg.norm(face_normal, axis=1) >= 1e-12
    mean = normals[faces].astype(np.float64).mean(axis=1)
    dots = (face_normal * mean).sum(axis=1)
    print("faces", len(faces), "below 1e-12 in area", int((~big).sum()), "not agreeing", int((dots[big] <= 0).sum()))
    assert (dots[big] > 0).all()


def analytic_normal(p):
    """unit normal, towards the camera, of the surface the `sphere` scene's depth map describes:
    F(X, Y, Z) = Z - 2 + 0.6 sqrt(1 - q) = 0 with q = (136 / 50)^2 (X^2 + Y^2) / Z^2 (pixel u - 80 = 136 X / Z)"""
    X, Y, Z = p[:, 0].astype(np.float64), p[:, 1].astype(np.float64), p[:, 2].astype(np.float64)
    k = (136.0 / 50.0) ** 2
    q = k * (X * X + Y * Y) / (Z * Z)
    r = np.sqrt(np.maximum(1.0 - q, 1e-12))
    g = np.stack([-0.6 * k * X / (r * Z * Z), -0.6 * k * Y / (r * Z * Z), 1.0 + 0.6 * q / (r * Z)], axis=1)
    return -g / np.linalg.norm(g, axis=1)[:, None]


def test_normals_follow_the_analytic_surface(sphere):
    _, points, _, _, normals, _ = sphere
    want = analytic_normal(points)
    cosine = np.clip((normals.astype(np.float64) * want).sum(axis=1), -1.0, 1.0)
    angle = np.degrees(np.arccos(cosine))
    p50, p99, worst = np.percentile(angle, 50), np.percentile(angle, 99), angle.max()
    print(f"angle to the analytic normal: median {p50:.3f}, 99th percentile {p99:.3f}, largest {worst:.3f} degrees")
    assert (cosine > 0).all()                                  # the positive-distance side: towards the camera
    assert p99 <= ANGLE_P99_DEGREES                            # the figure the GPU bound is derived from stays what was measured
    assert p99 > ANGLE_P99_DEGREES - 0.01


def test_doctored_volumes_reach_the_rarer_rules(orc):
    """what tests/test_gpu_extract_attributes.py::test_doctored_volume relies on, shown without a device"""
    base = {}
    A.extract_attributes(orc, A.fused(orc, "sphere"), True, True, base)
    assert base["color_none"] == 0 and base["vertices"] == 52868
    seen = {}
    for kind in A.DOCTORED:
        seen[kind] = {}
        colors, normals = A.extract_attributes(orc, A.doctored(orc, kind), True, True, seen[kind])
        assert np.isfinite(colors).all() and np.isfinite(normals).all()
        assert seen[kind]["zero_normals"] == 0
    assert min(seen["color-weights"][rule] for rule in ("color_both", "color_one", "color_none")) > 1000
    assert seen["distance-slab"]["gradient"]["forward"] > 20000 > base["gradient"]["forward"]
    assert seen["unlinked-neighbour"]["absent_low"] > base["absent_low"]
    assert seen["unlinked-neighbour"]["absent_high"] > base["absent_high"]
    assert seen["corner-neighbour-in-excess"]["corner_neighbour_past_entry_0"] == base["corner_neighbour_past_entry_0"] + 8
    hv = A.doctored(orc, "unlinked-neighbour")
    assert orc.extract_mesh(hv, False, True)[2] > 0                   # the visible-list form skips cubes


def test_abi_validates_before_touching_a_device():
    import ctypes as C
    from vulcan_amd import api, vk_types as T
    lib = api.lib()
    one = C.c_void_p(16)
    assert lib.vk_extract_mesh_attributes(None, 1, 1, None, None, None, 0, None, 0, None, None, None) == -1
    v = T.Volume()
    for name in ("voxels", "hash_entries", "visible_blocks", "counters"):
        setattr(v, name, 16)
    v.main_block_count = 8
    for missing in range(4):                                          # points, faces, counts, workspace
        args = [one, one, one, one]
        args[missing] = None
        assert lib.vk_extract_mesh_attributes(C.byref(v), 1, 1, args[0], one, one, 4, args[1], 4, args[2], args[3], None) == -1
    assert lib.vk_extract_mesh_attributes(C.byref(v), 1, 1, one, one, one, -1, one, 4, one, one, None) == -1
    assert lib.vk_abi_version() == 7


def test_ply_attributes_round_trip_on_the_host(sphere, tmp_path):
    from vulcan_amd import io as vio
    _, points, faces, colors, normals, _ = sphere
    points, faces, colors, normals = points[:2000], faces[(faces < 2000).all(axis=1)][:1500], colors[:2000], normals[:2000]
    path = str(tmp_path / "mesh.ply")
    vio.write_ply(path, points, faces, colors=colors, normals=normals)
    got_p, got_f, got_c, got_n = vio.read_ply_attributes(path)
    F = np.float32
    assert np.array_equal(got_c, (np.minimum(np.maximum(colors, F(0)), F(1)) * F(255) + F(0.5)).astype(np.int32))
    printed = lambda a: np.array([[F(float("%g" % v)) for v in row] for row in a], dtype=F)       # six significant digits
    assert np.array_equal(got_f, faces) and np.array_equal(got_n, printed(normals)) and np.array_equal(got_p, printed(points))
    assert np.abs(got_n - normals).max() < 1e-6
    # clamped, rounded to nearest: -0.5 -> 0, 0.5 -> 128 (127.5 + 0.5), 2 -> 255
    vio.write_ply(path, points[:1], faces[:0], colors=np.array([[-0.5, 0.5, 2.0]], F))
    assert vio.read_ply_attributes(path)[2].tolist() == [[0, 128, 255]] and vio.read_ply_attributes(path)[3] is None
    # without attributes: the bytes of the three-argument call, the grey ramp
    vio.write_ply(path, points, faces)
    three = open(path, "rb").read()
    vio.write_ply(path, points, faces, colors=None, normals=None)
    assert open(path, "rb").read() == three and b"nx" not in three
    ramp = vio.read_ply(path)[1]
    assert (ramp[:, 0] == ramp[:, 2]).all() and np.array_equal(vio.read_ply_attributes(path)[2], ramp)
