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
