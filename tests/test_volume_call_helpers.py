"""The caller-side helpers of the volume operations in vulcan_amd/api.py: the one pose coercion and the one
tensor check. No device is needed: CPU torch tensors have data_ptr."""
import numpy as np
import pytest
import torch

from vulcan_amd import api, vk_types as T


def rigid():
    """yaw 10 degrees, pitch 5 degrees, t = (0.3, -0.2, 0.5): every entry at most 1 in magnitude"""
    y, p = np.radians(10.0), np.radians(5.0)
    yaw = np.array([[np.cos(y), 0, np.sin(y)], [0, 1, 0], [-np.sin(y), 0, np.cos(y)]])
    pitch = np.array([[1, 0, 0], [0, np.cos(p), -np.sin(p)], [0, np.sin(p), np.cos(p)]])
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = yaw @ pitch, (0.3, -0.2, 0.5)
    return m


def test_pose_of_an_array_is_the_matrix_and_its_inverse():
    eye = api._as_pose(np.eye(4))
    assert isinstance(eye, T.Transform)
    assert eye.m[:] == T.Transform.identity().m[:] and eye.inv[:] == T.Transform.identity().inv[:]
    pose = api._as_pose(rigid().tolist())
    assert np.array_equal(pose.matrix(), rigid().astype(np.float32))
    # m and inv are each rounded to float32 once (eps32 / 2 relative), and an entry of the product sums four terms whose
    # magnitudes add up to at most 2 |t| + 1 < 4: the product, taken in float64, is within 4 eps32 of the identity
    product = pose.matrix().astype(np.float64) @ pose.inverse_matrix().astype(np.float64)
    assert np.abs(product - np.eye(4)).max() <= 4 * np.finfo(np.float32).eps


def test_pose_passes_through_what_is_a_pose_already():
    pose = T.Transform.translate(0.1, 0.2, 0.3)
    assert api._as_pose(pose) is pose and api._as_pose(pose, device=True) is pose and api._as_pose(pose, identity=True) is pose
    on_device = torch.zeros(32)                      # anything with data_ptr stands for a device vk_transform
    assert api._as_pose(on_device, device=True) is on_device
    with pytest.raises(ValueError):
        api._as_pose(on_device)                      # where no device pose is allowed it is read as an array: 32 values are no 4x4
    assert api._as_pose(None) is None and api._as_pose(None, device=True) is None
    identity = api._as_pose(None, identity=True)
    assert bytes(identity) == bytes(T.Transform.identity())


def test_pose_of_another_shape_raises():
    with pytest.raises(ValueError):
        api._as_pose(np.eye(3))
    with pytest.raises(ValueError):
        api._as_pose(np.eye(3), device=True, identity=True)


@pytest.mark.parametrize("last, message", [(3, "sample: points is a float32 [N, 3] device tensor"),
                                           (6, "cast_rays: rays is a float32 [N, 6] device tensor"),
                                           (6, "integrate_rays: rays is a float32 [N, 6] device tensor"),
                                           (None, "integrate_rays: ranges is a float32 [N] device tensor, one range per ray")])
def test_tensor_check(last, message):
    shape = (5,) if last is None else (5, last)
    good = torch.zeros(shape)
    assert api._float_tensor(good, last, message) is good                      # contiguous already: itself
    if last is not None:
        wide = torch.zeros((5, 2 * last))[:, ::2]
        got = api._float_tensor(wide, last, message)
        assert got.is_contiguous() and got.shape == wide.shape
    wrong = [torch.zeros(shape, dtype=torch.float64), torch.zeros(shape, dtype=torch.int32),       # dtype
             torch.zeros(shape + (1,)), torch.zeros(()),                                           # rank
             np.zeros(shape, dtype=np.float32), None]                                              # no tensor at all
    wrong.append(torch.zeros((5, 5)) if last is None else torch.zeros(5))                          # the other rank
    if last is not None:
        wrong += [torch.zeros((5, last + 1)), torch.zeros((5, last - 1))]                          # trailing dimension
    for x in wrong:
        with pytest.raises(api.VkError) as raised:
            api._float_tensor(x, last, message)
        assert str(raised.value) == message
    assert api._float_tensor(good, last, message, rows=5) is good
    with pytest.raises(api.VkError) as raised:
        api._float_tensor(good, last, message, rows=4)
    assert str(raised.value) == message


@pytest.mark.parametrize("voxel_units", [False, True])
@pytest.mark.parametrize("one_observation", [False, True])
def test_range_ray_arguments(voxel_units, one_observation):
    """The bounds an operation along range rays takes from the volume's depth range, and its flags. (0.25, 6.5) are float32
    numbers, so without voxel units the bounds are the depth range itself; a depth range that is not (the default's 0.1) is
    the same float32 the library reads from the parameter block."""
    rays, ranges = torch.zeros((5, 6)), torch.zeros(5)
    depth_range, voxel_length = (0.25, 6.5), 0.008
    got = api._range_ray_arguments("carve_rays", rays, ranges, depth_range, voxel_length, None, None, voxel_units, one_observation)
    assert got[0] is rays and got[1] is ranges
    if voxel_units:
        want = tuple(float(np.float32(depth_range[k]) / np.float32(voxel_length)) for k in range(2))
    else:
        want = depth_range
    assert got[2:4] == want and all(type(bound) is float for bound in got[2:4])
    assert got[4] == (T.VK_RAYS_VOXEL_UNITS if voxel_units else 0) | (T.VK_RAYS_ONE_OBSERVATION if one_observation else 0)
    default = api._range_ray_arguments("carve_rays", rays, ranges, (0.1, 5.0), voxel_length, None, None, voxel_units)
    scale = np.float32(voxel_length) if voxel_units else np.float32(1)
    assert default[2:4] == (float(np.float32(0.1) / scale), float(np.float32(5.0) / scale))
    # given bounds pass through untouched, each on its own
    given = api._range_ray_arguments("carve_rays", rays, ranges, depth_range, voxel_length, 0.3, 123.456, voxel_units)
    assert given[2] == 0.3 and given[3] == 123.456
    mixed = api._range_ray_arguments("carve_rays", rays, ranges, depth_range, voxel_length, None, 7, voxel_units)
    assert mixed[2] == want[0] and mixed[3] == 7 and type(mixed[3]) is int
    assert given[4] == mixed[4] == (T.VK_RAYS_VOXEL_UNITS if voxel_units else 0)        # one_observation defaults to off


@pytest.mark.parametrize("what", ["integrate_rays", "carve_rays", "color_rays", "register_rays", "score_poses", "localize_rays"])
def test_range_ray_arguments_name_the_operation(what):
    arguments = ((0.1, 5.0), 0.008, None, None, False)
    with pytest.raises(api.VkError) as raised:
        api._range_ray_arguments(what, torch.zeros((5, 6)), torch.zeros(4), *arguments)      # another row count
    assert str(raised.value) == f"{what}: ranges is a float32 [N] device tensor, one range per ray"
    with pytest.raises(api.VkError) as raised:
        api._range_ray_arguments(what, torch.zeros((5, 5)), torch.zeros(5), *arguments)
    assert str(raised.value) == f"{what}: rays is a float32 [N, 6] device tensor"
    wide = torch.zeros((5, 12))[:, ::2]
    assert api._range_ray_arguments(what, wide, torch.zeros(5), *arguments)[0].is_contiguous()
