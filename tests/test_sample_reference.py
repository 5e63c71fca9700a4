"""The CPU statement of vk_volume_sample (tests/sample_reference.py) against what any definition of the call must give: a
voxel's centre gives the stored voxel, a linear field is reproduced with its gradient exactly, the oracle's mesh vertices
lie on the zero set, and the posed merge's samples are this sample at the destination voxels' centres. No GPU: the device
is held to the same statement in tests/test_gpu_sample.py."""
import ctypes as C

import numpy as np
import pytest

from abi_support import fake_volume
import merge_pose_reference as MP
import merge_reference as M
import register_reference as RR
import release_reference as R
import sample_reference as S
from vulcan_amd import vk_types as T

f32 = np.float32


@pytest.fixture(scope="module")
def generic_pair(orc):
    return RR.pair(orc, MP.generic())


def test_a_voxel_centre_gives_the_stored_voxel(orc, generic_pair):
    dst = generic_pair[0]
    coords, at = S.weighted_voxels(dst)
    centres = coords.astype(f32) + f32(0.5)
    got, _ = S.sample(dst, centres, voxel_units=True)
    print("weighted voxels", len(at))
    assert len(at) > 100000
    assert got.tobytes() == dst.voxels[at].tobytes()
    # in metres the centre has to survive * L / L: it does when L is a power of two
    dyadic = R.clone(orc, dst)
    dyadic.voxel_length = 2.0 ** -7
    got, _ = S.sample(dyadic, centres * f32(2.0 ** -7))
    assert got.tobytes() == dst.voxels[at].tobytes()
    # with 0.008 it does not: that is why VK_SAMPLE_VOXEL_UNITS exists
    L = f32(dst.voxel_length)
    survive = ((centres * L) / L == centres).all(-1)
    print("centres that survive * L / L with L = 0.008: %.1f %%" % (100.0 * survive.mean()))
    got, _ = S.sample(dst, centres * L)
    assert got[survive].tobytes() == dst.voxels[at][survive].tobytes()


def test_a_linear_field_and_its_gradient_are_exact(orc, generic_pair):
    """every voxel of every block holds (a x + b y + c z) / 64 at its lattice point (x, y, z): at points with dyadic fractions
    every operation of the sample is exact, so D is the function at g = p - 0.5 and the gradient is (a, b, c) / 64"""
    hv = R.clone(orc, generic_pair[0])
    a, b, c = 3, -2, 5
    for index in M.source_blocks(hv):
        slot = int(hv.hash_entries["data"][index])
        n = 8 * np.asarray(M.origin_of(hv, index), dtype=np.int64) + MP.OFFSETS
        block = hv.voxels[slot * 512:(slot + 1) * 512]
        block["distance"] = ((a * n[:, 0] + b * n[:, 1] + c * n[:, 2]).astype(f32) / f32(64))
        block["distance_weight"] = 1
    rng = np.random.default_rng(3)
    coords, _ = S.weighted_voxels(hv, 40000)
    fractions = rng.integers(0, 16, coords.shape).astype(f32) / f32(16)
    p = coords.astype(f32) + f32(0.5) + fractions
    got, gradients = S.sample(hv, p, voxel_units=True)
    inside = gradients[:, 3] != 0
    print("points with all eight neighbours", int(inside.sum()), "of", len(p))
    assert inside.sum() > 10000
    g = (p - f32(0.5)).astype(np.float64)
    want = ((a * g[:, 0] + b * g[:, 1] + c * g[:, 2]) / 64.0).astype(f32)
    assert (got["distance_weight"][inside] == 1).all()
    assert np.array_equal(got["distance"][inside], want[inside])
    assert np.array_equal(gradients[inside, :3], np.tile(np.array([a, b, c], dtype=f32) / f32(64), (int(inside.sum()), 1)))


def test_mesh_vertices_lie_on_the_zero_set(orc, generic_pair):
    """bound: 1e-4, the README's TSDF tolerance; measured 4.6e-6 worst"""
    vertices = S.point_sets(orc, False)["a"]
    got, _ = S.sample(generic_pair[0], vertices)
    worst = float(np.abs(got["distance"]).max())
    print("vertices", len(vertices), "worst |D|", worst)
    assert len(vertices) > 10000
    assert (got["distance_weight"] != 0).all()
    assert worst <= 1e-4


def test_the_posed_merge_is_its_samples(orc, generic_pair):
    dst, src = generic_pair
    pose = MP.generic()
    back = MP.rows(pose.inv, dst.voxel_length)
    table = RR.block_table(src)

    def find(origin):
        origin = tuple(int(c) for c in origin)
        return table.get(origin, -1) if all(-32768 <= c <= 32767 for c in origin) else -1

    origins = [M.origin_of(dst, i) for i in M.source_blocks(dst)[:40]]
    sampled = colored = 0
    for o in origins:
        want = MP.samples(src, o, back, find)
        got, _ = S.sample(src, MP.centres(o), pose=pose.inverse(), voxel_units=True, table=table)
        assert np.array_equal(got["distance_weight"], want["distance_weight"])
        assert np.array_equal(got["color_weight"], want["color_weight"])
        d, c = want["distance_weight"] != 0, want["color_weight"] != 0
        assert got["distance"][d].tobytes() == want["distance"][d].tobytes()
        assert got["color"][c].tobytes() == want["color"][c].tobytes()
        sampled, colored = sampled + int(d.sum()), colored + int(c.sum())
    print("blocks", len(origins), "voxels sampled", sampled, "with colour", colored)
    assert len(origins) == 40 and sampled > 5000 and colored > 1000


@pytest.mark.parametrize("voxel_units", [False, True], ids=["metres", "voxel-units"])
def test_the_point_sets_are_not_vacuous(orc, generic_pair, voxel_units):
    """conditions on the statement that the GPU tests rely on"""
    sets = S.point_sets(orc, voxel_units)
    print({name: len(points) for name, points in sets.items()})
    assert len(sets["a"]) > 10000 and len(sets["b"]) == 20000 and len(sets["c"]) > 1000 and len(sets["d"]) == 1500
    assert len(sets["e"]) == 256 and len(sets["f"]) == 12
    got, gradients = S.sample(generic_pair[0], S.all_points(orc, voxel_units), voxel_units=voxel_units)
    d, c, g = got["distance_weight"] != 0, got["color_weight"] != 0, gradients[:, 3] != 0
    print("distance and gradient", int((d & g).sum()), "distance, no gradient", int((d & ~g).sum()), "colour", int(c.sum()),
          "nothing", int((~d & ~c & ~g).sum()))
    assert (d & g).sum() >= 1000 and (d & ~g).sum() >= 100 and c.sum() >= 100 and (~d & ~c & ~g).sum() >= 100
    assert not (g & ~d).any()                                        # eight weighted points: the USED ones are among them
    last = slice(len(got) - 12, None)                                # (f)
    assert not d[last].any() and not c[last].any() and not g[last].any()
    nothing = ~d
    assert (got["distance"][nothing] == 1).all() and not gradients[~g].any()
    if voxel_units:
        # (c): f == 0 exactly, so the centre alone is USED, and (d): one or two axes with f == 0
        first = len(sets["a"]) + len(sets["b"])
        assert d[first:first + len(sets["c"])].all() and not g[first:first + len(sets["c"])].any()
        on_face = (sets["d"] - f32(0.5) == np.floor(sets["d"] - f32(0.5))).sum(-1)
        assert ((on_face >= 1) & (on_face <= 3)).all() and (on_face == 1).sum() > 100 and (on_face == 2).sum() > 100


def test_the_library_validates_before_touching_a_device():
    """every refusal vk.h lists, with addresses that are no memory: nothing may be enqueued (no GPU is needed, or touched)"""
    from vulcan_amd import api
    lib = api.lib()
    one, odd = C.c_void_p(4096), C.c_void_p(4096 + 8)

    good = T.SampleParams(0, 0)

    def call(v=fake_volume(), points=one, count=8, pose=None, params=good, samples=one, gradients=one):
        return lib.vk_volume_sample(C.byref(v) if v else None, points, count, pose, C.byref(params) if params else None, samples,
                                    gradients, None)

    assert call(v=None) == -1 and call(params=None) == -1
    broken = fake_volume()
    broken.hash_entries = None
    assert call(v=broken) == -1
    broken = fake_volume()
    broken.voxel_length = 0.0
    assert call(v=broken) == -1
    for flags in (4, 8, -1, 1 << 16):
        assert call(params=T.SampleParams(flags, 0)) == -1
    assert call(count=-1) == -1
    assert call(points=None) == -1
    assert call(samples=None, gradients=None) == -1
    assert call(gradients=odd) == -1 and call(samples=None, gradients=odd) == -1
    # count == 0 launches nothing, whatever the flags allow
    for flags in (0, 1, 2, 3):
        assert call(count=0, params=T.SampleParams(flags, 0)) == 0
    assert call(count=0, points=None) == 0 and call(count=0, gradients=None) == 0 and call(count=0, samples=None) == 0
    assert call(count=0, samples=None, gradients=None) == -1
