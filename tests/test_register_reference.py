"""The CPU statement of vk_volume_register (tests/register_reference.py) against what any definition of the call must give:
a volume is registered to its own copy, a source built in a frame shifted by whole blocks has no residual at that shift,
a displaced source comes back to its pose from the identity, and the gradient and the Jacobian are the derivatives of the
statement's own sample. No GPU: the device is held to the same statement in tests/test_gpu_register.py."""
import numpy as np
import pytest

from abi_support import fake_volume
import merge_pose_reference as MP
import register_reference as RR
import release_reference as R
from vulcan_amd import vk_types as T


@pytest.fixture(scope="module")
def generic_pair(orc):
    return RR.pair(orc, MP.generic())


def test_a_clone_is_already_registered(orc, generic_pair):
    dst = generic_pair[0]
    pair = RR.Pair(dst, R.clone(orc, dst))
    evaluated = RR.terms(pair, T.Transform.identity(), 0.75)
    total, _ = RR.system(evaluated)
    print("counts", evaluated.counts)
    assert evaluated.counts[2] > 100000 and evaluated.counts[2] == int(evaluated.valid.sum())
    assert not evaluated.r.any()
    assert not total[36:43].any()                                                   # the gradient, exactly
    result = RR.register(orc, dst, pair.src, T.Transform.identity(), iterations=1, pair=pair)
    assert (result.steps, result.code) == (1, 1)
    assert bytes(result.pose) == bytes(T.Transform.identity())


def test_a_block_shift_has_no_residual(orc):
    shift = MP.shift((8, -16, 0))
    assert [float(np.float32(t) / np.float32(R.VOXEL)) for t in shift.m[12:15]] == [8.0, -16.0, 0.0]
    dst, src = RR.pair(orc, shift, frames=(2, 2))
    evaluated = RR.terms(RR.Pair(dst, src), shift, 0.75)
    print("counts", evaluated.counts, "max |r|", float(np.abs(evaluated.r).max()))
    assert evaluated.counts[2] > 100000
    assert float(np.abs(evaluated.r).max()) == 0.0


def test_a_generic_pose_is_found_from_the_identity(orc, generic_pair):
    """measured: 8 steps, 0.071 mm and 0.0047 degrees from the truth, from 26.0 mm and 11.2 degrees; the bounds are a
    thirty-second of a voxel and 0.05 degrees"""
    truth = MP.generic()
    result = RR.register(orc, *generic_pair, T.Transform.identity(), iterations=20)
    metres, degrees = RR.pose_error(result.pose, truth)
    print("steps", result.steps, "code", result.code, "counts", result.counts, "error", metres, degrees,
          "from", RR.pose_error(T.Transform.identity(), truth))
    assert result.code == 1 and result.steps <= 20
    assert metres < 0.25e-3 and degrees < 0.05
    # m and inv move together
    assert np.abs(result.pose.matrix().astype(np.float64) @ result.pose.inverse_matrix().astype(np.float64) - np.eye(4)).max() < 1e-6


def test_the_gradient_is_the_derivative_of_the_sample():
    """central differences of the statement's own D in float64 (D is trilinear: the difference is exact but for rounding)"""
    rng = np.random.default_rng(5)
    v = [rng.uniform(-1.0, 1.0, 1000) for _ in range(8)]
    f = [rng.uniform(0.05, 0.95, 1000) for _ in range(3)]                           # strictly inside a cell
    _, gradient = RR.sample(v, f)
    h = 1e-3
    for axis in range(3):
        ahead, behind = [c.copy() for c in f], [c.copy() for c in f]
        ahead[axis] += h
        behind[axis] -= h
        numeric = (RR.sample(v, ahead)[0] - RR.sample(v, behind)[0]) / (2 * h)
        assert np.abs(numeric - gradient[axis]).max() < 1e-9


def test_the_jacobian_is_the_derivative_of_the_residual_under_a_left_twist():
    """r(u) = D(Tinc(u) x) - s at u = 0, by central differences in float64: the twist is applied on the left, in metres.
    The bound: D is a cubic in u whose third-order coefficient is at most 8 max|v| (|x| / voxel)^3 with |x| < 200 sqrt(3)
    voxels, so the central difference is off by at most h^2 * 8 * 346^3 = 4.7e-6; the rounding of D, |x| eps / (2 h) times
    a gradient of 2, adds 4e-7. 1e-5 covers both, against entries of J in the hundreds."""
    rng = np.random.default_rng(6)
    voxel_length = 0.008
    v = [rng.uniform(-1.0, 1.0, 1000) for _ in range(8)]
    base = np.floor(rng.uniform(-200.0, 200.0, (3, 1000)))
    f = rng.uniform(0.2, 0.8, (3, 1000))
    p = base + f + 0.5                                                              # voxels
    _, gradient = RR.sample(v, list(f))
    J = RR.jacobian(list(p), gradient, 1.0 / voxel_length)
    h = 2.0 ** -23                                                                  # (a float32 as well: tinc keeps it)

    def value(update):
        moved = RR.tinc(update).astype(np.float64)[:3] @ np.vstack([p * voxel_length, np.ones(1000)])
        return RR.sample(v, list(moved / voxel_length - 0.5 - base))[0]

    for i in range(6):
        ahead, behind = np.zeros(6), np.zeros(6)
        ahead[i], behind[i] = h, -h
        numeric = (value(ahead) - value(behind)) / (2 * h)
        scale = np.abs(J[i]).max()
        print(i, float(np.abs(numeric - J[i]).max()), float(scale))
        assert np.abs(numeric - J[i]).max() < 1e-5 and scale > 100.0


def test_the_library_validates_before_touching_a_device():
    """every refusal vk.h lists, with addresses that are no memory: nothing may be enqueued (no GPU is needed, or touched)"""
    import ctypes as C
    from vulcan_amd import api
    lib = api.lib()
    one = C.c_void_p(4096)

    good = T.RegisterParams(0, 20, 0.75, 0)

    def loop(dst, src, params=good, pose=one, system=one, state=one, counts=one, workspace=one):
        return lib.vk_volume_register(C.byref(dst), C.byref(src), pose, C.byref(params), system, state, counts, None, workspace, None)

    dst, src = fake_volume(1 << 20), fake_volume(2 << 20)
    for name in ("pose", "system", "state", "counts", "workspace"):
        assert loop(dst, src, **{name: None}) == -1
    assert lib.vk_volume_register(None, C.byref(src), one, C.byref(good), one, one, one, None, one, None) == -1
    assert lib.vk_volume_register(C.byref(dst), None, one, C.byref(good), one, one, one, None, one, None) == -1
    assert lib.vk_volume_register(C.byref(dst), C.byref(src), one, None, one, one, one, None, one, None) == -1
    for bad in (T.RegisterParams(1, 20, 0.75, 0), T.RegisterParams(0, 0, 0.75, 0), T.RegisterParams(0, 65, 0.75, 0),
                T.RegisterParams(0, 20, 0.0, 0), T.RegisterParams(0, 20, 1.5, 0), T.RegisterParams(0, 20, float("nan"), 0)):
        assert loop(dst, src, params=bad) == -1
    other = fake_volume(2 << 20)
    other.voxel_length = 0.005
    assert loop(dst, other) == -1
    other = fake_volume(2 << 20)
    other.truncation_length = 0.05
    assert loop(dst, other) == -1
    other = fake_volume(2 << 20)
    other.counters = None
    assert loop(dst, other) == -1 and loop(other, src) == -1
    assert lib.vk_volume_register_system(C.byref(dst), C.byref(src), one, C.byref(good), None, one, one, None) == -1
    assert lib.vk_volume_register_system(C.byref(dst), C.byref(src), one, C.byref(good), one, None, one, None) == -1
    for missing in range(3):
        buffers = [None if k == missing else one for k in range(3)]
        assert lib.vk_volume_register_terms(C.byref(dst), C.byref(src), one, C.byref(good), *buffers, one, None) == -1
    assert lib.vk_volume_register_terms(C.byref(dst), C.byref(src), one, C.byref(T.RegisterParams(2, 1, 0.75, 0)), one, one, one, one, None) == -1
    assert lib.vk_volume_register_workspace_bytes(0, 8) == 0 and lib.vk_volume_register_workspace_bytes(8, -1) == 0
    assert lib.vk_volume_register_workspace_bytes(509, 4096) >= 4605 + 64 + 1152 * 128
