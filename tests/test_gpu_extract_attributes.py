"""vk_extract_mesh_attributes on the device against its CPU statement (tests/extract_attributes_reference.py), bit for bit:
the device starts from an uploaded oracle state (the way tests/test_gpu_release.py does), so the visible list has the oracle's
order, and must write the colours and normals the numpy statement computes — same bits — beside exactly the points and faces
of vk_extract_mesh. Every value is one defined sequence of float32 operations, so there is no tolerance in this file except
where a file of printed decimals or a property of a full-size mesh is checked."""
import numpy as np
import pytest

import extract_attributes_reference as A
import scenes
from extract_attributes_reference import ANGLE_P99_DEGREES
from gpu_support import api, device_copy, sync  # noqa: F401
from vulcan_amd import io as vio, vk_types as T

pytestmark = pytest.mark.gpu

_REFERENCE = {}


def reference(orc, key, hv, all_allocated, interpolate):
    """(points, faces, skipped, colors, normals, statistics) of the CPU statement, computed once per volume and mode"""
    key = (key, all_allocated, interpolate)
    if key not in _REFERENCE:
        statistics = {}
        points, faces, skipped = orc.extract_mesh(hv, all_allocated, interpolate)
        colors, normals = A.extract_attributes(orc, hv, all_allocated, interpolate, statistics)
        _REFERENCE[key] = (points, faces, skipped, colors, normals, statistics)
    return _REFERENCE[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_device_matches(api, orc, key, hv, dv=None):
    """all_allocated x interpolate: attributes equal the statement's, points and faces equal vk_extract_mesh's"""
    dv = dv or device_copy(api, hv)
    ex = api.Extractor(dv)
    for all_allocated in (True, False):
        for interpolate in (True, False):
            ex.all_allocated, ex.interpolate = all_allocated, interpolate
            want_p, want_f, want_skipped, want_c, want_n, _ = reference(orc, key, hv, all_allocated, interpolate)
            plain = ex.extract()
            plain_counts = ex.counts.cpu().numpy().copy()
            mesh = ex.extract(colors=True, normals=True)
            sync()
            assert np.array_equal(ex.counts.cpu().numpy(), plain_counts)
            got_p, got_f = mesh.host()
            got_c, got_n = mesh.host_attributes()
            plain_p, plain_f = plain.host()
            assert len(want_p) > 10000 and got_c.shape == got_n.shape == got_p.shape == want_p.shape
            assert np.array_equal(bits(got_p), bits(plain_p)) and np.array_equal(got_f, plain_f)
            assert np.array_equal(bits(got_p), bits(want_p)) and np.array_equal(got_f, want_f)
            assert ex.skipped == want_skipped
            different = np.nonzero((bits(got_c) != bits(want_c)).any(axis=1) | (bits(got_n) != bits(want_n)).any(axis=1))[0]
            print(all_allocated, interpolate, len(want_p), "vertices,", len(different), "differ", different[:5])
            assert np.array_equal(bits(got_c), bits(want_c))
            assert np.array_equal(bits(got_n), bits(want_n))
    return dv


@pytest.mark.parametrize("scene", ["plane", "sphere", "ripple-tilted"])
def test_device_equals_reference(api, orc, scene):
    assert_device_matches(api, orc, scene, A.fused(orc, scene))


@pytest.mark.parametrize("kind", A.DOCTORED)
def test_doctored_volume(api, orc, kind):
    hv = A.doctored(orc, kind)
    base = reference(orc, "sphere", A.fused(orc, "sphere"), True, True)[5]
    stats = reference(orc, kind, hv, True, True)[5]
    visible_skipped = reference(orc, kind, hv, False, True)[2]
    print(kind, stats, visible_skipped)
    if kind == "color-weights":
        assert stats["color_both"] > 1000 and stats["color_one"] > 1000 and stats["color_none"] > 1000
    elif kind == "distance-slab":
        for form in ("forward", "backward", "none"):
            assert stats["gradient"][form] > base["gradient"][form]
        assert stats["gradient"]["forward"] > 20000 and stats["unknown_9"] > base["unknown_9"]
    elif kind == "unlinked-neighbour":
        assert stats["blocks"] == base["blocks"] - 1
        assert stats["absent_low"] > base["absent_low"] and stats["absent_high"] > base["absent_high"]
        assert visible_skipped > 0 and reference(orc, "sphere", A.fused(orc, "sphere"), False, True)[2] == 0
    else:
        assert stats["corner_neighbour_past_entry_0"] == base["corner_neighbour_past_entry_0"] + 8
    assert_device_matches(api, orc, kind, hv)


@pytest.fixture(scope="module")
def sphere(api, orc):
    hv = A.fused(orc, "sphere")
    return hv, device_copy(api, hv), reference(orc, "sphere", hv, True, True)


def call(api, dv, ex, points, colors, normals, point_capacity, faces, face_capacity):
    api.check(api.lib().vk_extract_mesh_attributes(api._ref(dv.desc()), 1, 1, api._ptr(points), api._ptr(colors), api._ptr(normals),
                                                   point_capacity, api._ptr(faces), face_capacity, api._ptr(ex.counts),
                                                   api._ptr(ex.workspace), api.stream()), "vk_extract_mesh_attributes")
    sync()
    return ex.counts.cpu().numpy().copy()


def test_nothing_is_written_past_a_capacity(api, sphere):
    import torch
    hv, dv, (want_p, want_f, _, want_c, want_n, _) = sphere
    ex = api.Extractor(dv)
    n, m = len(want_p), len(want_f)
    # 1000 points is inside the first blocks' vertices, 3 * 1000 floats is no multiple of a block's share
    arrays = [torch.full((n, 3), -7.0, dtype=torch.float32, device="cuda") for _ in range(3)]
    faces = torch.full((m, 3), -7, dtype=torch.int32, device="cuda")
    counts = call(api, dv, ex, arrays[0], arrays[1], arrays[2], 1000, faces, 500)
    assert counts[0] == n and counts[1] == m                         # the totals are still reported
    for got, want in zip(arrays, (want_p, want_c, want_n)):
        got = got.cpu().numpy()
        assert np.array_equal(bits(got[:1000]), bits(want[:1000]))
        assert (got[1000:] == -7.0).all()
    got = faces.cpu().numpy()
    assert np.array_equal(got[:500], want_f[:500]) and (got[500:] == -7).all()


def test_null_outputs_are_skipped(api, sphere):
    import torch
    hv, dv, (want_p, want_f, _, want_c, want_n, _) = sphere
    ex = api.Extractor(dv)
    n, m = len(want_p), len(want_f)
    for with_colors, with_normals in ((False, True), (True, False), (False, False)):
        points, colors, normals = (torch.full((n, 3), -7.0, dtype=torch.float32, device="cuda") for _ in range(3))
        faces = torch.full((m, 3), -7, dtype=torch.int32, device="cuda")
        counts = call(api, dv, ex, points, colors if with_colors else None, normals if with_normals else None, n, faces, m)
        assert counts[0] == n and counts[1] == m
        assert np.array_equal(bits(points.cpu().numpy()), bits(want_p)) and np.array_equal(faces.cpu().numpy(), want_f)
        assert np.array_equal(bits(colors.cpu().numpy()), bits(want_c)) if with_colors else bool((colors == -7.0).all())
        assert np.array_equal(bits(normals.cpu().numpy()), bits(want_n)) if with_normals else bool((normals == -7.0).all())
    ex.all_allocated = True
    mesh = ex.extract(colors=True)
    assert mesh.normals is None and mesh.host_attributes()[1] is None
    assert np.array_equal(bits(mesh.host_attributes()[0]), bits(want_c))
    plain = ex.extract()
    assert plain.colors is None and plain.normals is None and plain.host_attributes() == (None, None)
    assert len(plain.host()) == 2


def test_two_calls_give_equal_bytes(api, sphere):
    _, dv, _ = sphere
    ex = api.Extractor(dv)
    ex.all_allocated = True
    first, second = ex.extract(colors=True, normals=True), ex.extract(colors=True, normals=True)
    sync()
    for a, b in zip(first.host() + first.host_attributes(), second.host() + second.host_attributes()):
        assert a.tobytes() == b.tobytes()


def test_ply_round_trip(api, sphere, tmp_path):
    _, dv, _ = sphere
    ex = api.Extractor(dv)
    ex.all_allocated = True
    mesh = ex.extract(colors=True, normals=True)
    points, faces = mesh.host()
    colors, normals = mesh.host_attributes()
    path = str(tmp_path / "attributes.ply")
    vio.write_ply(path, points, faces, colors=colors, normals=normals)
    header = open(path).read().split("end_header")[0].split("\n")
    assert header[3:12] == ["property float x", "property float y", "property float z", "property float nx", "property float ny",
                            "property float nz", "property uchar red", "property uchar green", "property uchar blue"]
    got_p, got_f, got_c, got_n = vio.read_ply_attributes(path)
    F = np.float32
    want_c = (np.minimum(np.maximum(colors, F(0)), F(1)) * F(255) + F(0.5)).astype(np.int32)
    assert want_c.min() >= 25 and want_c.max() <= 230 and len(np.unique(want_c)) > 2
    assert np.array_equal(got_c, want_c) and np.array_equal(got_f, faces)
    printed = np.array([[F(float("%g" % v)) for v in row] for row in normals], dtype=F)
    assert np.array_equal(got_n, printed) and np.abs(got_n - normals).max() < 5e-6       # six significant digits
    assert np.array_equal(got_p, np.array([[F(float("%g" % v)) for v in row] for row in points], dtype=F))
    # colours alone: the ramp's place, no normals; nothing: today's bytes
    vio.write_ply(path, points, faces, colors=colors)
    _, _, only_c, no_n = vio.read_ply_attributes(path)
    assert no_n is None and np.array_equal(only_c, want_c)
    assert np.array_equal(vio.read_ply(path)[1], want_c)
    old, new = str(tmp_path / "three.ply"), str(tmp_path / "five.ply")
    vio.write_ply(old, points, faces)
    vio.write_ply(new, points, faces, colors=None, normals=None)
    assert open(old, "rb").read() == open(new, "rb").read()
    ramp = vio.read_ply(old)[1]
    assert (ramp[:, 0] == ramp[:, 1]).all() and np.array_equal(vio.read_ply_attributes(old)[2], ramp)


def test_full_size_normals(api, orc):
    """BASELINE sizes (640x480, 5 mm, Volume(65024, 8192)): the 2 m sphere room of test_full_size_mesh_properties seen from
    its centre. The analytic normal of the positive side is -p / |p|. The angle bound is 1.5 x the 99th percentile measured
    on the CPU (tests/test_extract_attributes_reference.py: 62.71 degrees on an undersampled 160x120 scene); here a pixel is
    smaller than a voxel and the figure printed below is what the full-size mesh reaches."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    k = T.Projection.make(*scenes.APP_INTRINSICS)
    depth = bench.sphere_room_depth(k)
    dv = api.Volume(bench.MAIN, bench.EXCESS, voxel_length=bench.VOXEL, truncation_length=bench.TRUNC)
    df = api.Frame(depth, k, T.Transform.identity())
    integ = api.DepthIntegrator(dv)
    for i in range(4):
        df.depth_to_world = scenes.orbit_pose(i, bench.YAW_STEP)
        dv.set_view(df)
        integ.integrate(df)
    ex = api.Extractor(dv)
    ex.all_allocated = True
    mesh = ex.extract(normals=True)
    sync()
    p, _ = mesh.host()
    n = mesh.host_attributes()[1].astype(np.float64)
    assert len(p) > 150000 and mesh.colors is None
    length = np.linalg.norm(n, axis=1)
    assert np.abs(length - 1).max() < 1e-6
    inward = -p.astype(np.float64) / np.linalg.norm(p.astype(np.float64), axis=1)[:, None]
    cosine = (n * inward).sum(axis=1)
    angle = np.degrees(np.arccos(np.clip(cosine, -1, 1)))
    print(f"angle to -p/|p|: median {np.percentile(angle, 50):.3f}, 99th percentile {np.percentile(angle, 99):.3f}, "
          f"largest {angle.max():.3f} degrees; smallest cosine {cosine.min():.4f}")
    assert (cosine > 0).all()
    assert np.percentile(angle, 99) < 1.5 * ANGLE_P99_DEGREES
