"""What the GPU tests share that belongs to no one operation: the `api` fixture, the comparisons of a device volume with the
oracle's HostVolume that the parity claim rests on, and the small helpers that put host data on the device. One statement of
each; the test modules import from here and never from one another (tests/test_support_layering.py).

Torch is imported inside the functions, so this module imports on a machine without a GPU. The range-ray writers' harness
is tests/ray_call_support.py; the CPU statements and their case tables are the tests/*_reference.py modules."""
import numpy as np
import pytest

import cast_reference as CR
import integrate_rays_reference as IR
import register_reference as RR
import register_rays_reference as RY
import release_reference as R
from vulcan_amd import vk_types as T

# (destination sizes, source sizes) of the volume operations' cases: long chains, and a destination whose bucket count is
# not the source's
SAME, OTHER = ((509, 4096), (509, 4096)), ((4093, 2048), (509, 4096))
_WORLDS = {}


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available()
    from vulcan_amd import api as a
    a.lib()
    return a


def sync():
    import torch
    torch.cuda.synchronize()


# ---- host data on the device ---------------------------------------------------------------------------------------------

def make_pair(api, orc, main, excess, voxel, trunc):
    hv = orc.HostVolume(main, excess, voxel_length=voxel, truncation_length=trunc)
    dv = api.Volume(main, excess, voxel_length=voxel, truncation_length=trunc)
    return hv, dv


def frames(api, orc, depth, k, pose, color=None, normals=None):
    hf = orc.HostFrame(depth, k, pose, color=color, normals=normals)
    df = api.Frame(depth, k, pose, color=color, normals=normals)
    return hf, df


def device_copy(api, hv):
    dv = api.Volume(hv.main, hv.excess, voxel_length=hv.voxel_length, truncation_length=hv.truncation_length)
    dv.upload(hv)
    return dv


def on_device(array):
    import torch
    return torch.as_tensor(np.ascontiguousarray(array, dtype=np.float32)).cuda()


def pose_on_device(pose):
    """a device buffer that already holds the pose: its 128 bytes"""
    import torch
    return torch.as_tensor(np.frombuffer(bytes(pose), dtype=np.uint8).copy()).cuda()


def pair_on_device(api, orc, truth, sizes=SAME, frames=(2, 3)):
    """(host dst, host src, device dst, device src) of register_reference.pair"""
    hd, hs = RR.pair(orc, truth, sizes, frames)
    return hd, hs, device_copy(api, hd), device_copy(api, hs)


def world(orc, sizes):
    """cast_reference.volume at these table sizes as a register_rays_reference.Map: once per size, only read"""
    if sizes not in _WORLDS:
        _WORLDS[sizes] = RY.Map(CR.volume(orc, sizes))
    return _WORLDS[sizes]


def form(units):
    """(flags, r_min, r_max) of a form"""
    return (RY.VOXEL_UNITS if units else 0,) + IR.bounds(units)


def overwrite(tensor, fill, seed):
    import torch
    if fill == "noise":
        generator = torch.Generator(device="cpu").manual_seed(seed)
        raw = torch.randint(0, 256, (tensor.numel() * tensor.element_size(),), dtype=torch.uint8, generator=generator)
        tensor.view(torch.uint8).copy_(raw.to(tensor.device))
    else:
        tensor.view(torch.uint8).fill_(0xFF)


def pin_bench_defaults(monkeypatch):
    """the forms of the tracked step that bench.py times when no VK_BENCH_* variable is set — whatever the environment says"""
    import bench
    monkeypatch.setattr(bench, "SET_VIEW_AT_DEVICE_POSE", 2)
    monkeypatch.setattr(bench, "PYRAMID_AHEAD", False)
    monkeypatch.setattr(bench, "KEY_NORMALS_WITH_PYRAMID", True)
    monkeypatch.setattr(bench, "NORMALS_IN_SET_VIEW", True)
    return bench


# ---- a device volume against the oracle's ---------------------------------------------------------------------------------

def assert_volume_equal(dv, hv, voxels=True, order_free_visible=True):
    """Whole-state comparison; allocation is deterministic on both sides (max-key
    winner, scan-ordered slots), so raw buffers must match byte for byte."""
    sync()
    ctr = dv.read_counters()
    for i in (T.VK_CTR_VISIBLE, T.VK_CTR_VOXEL_PTR, T.VK_CTR_EXCESS_PTR, T.VK_CTR_DROPPED):
        assert ctr[i] == hv.counters[i], (i, ctr, hv.counters)
    assert np.array_equal(dv.host_entries(), hv.hash_entries)
    assert np.array_equal(dv.host_visibility(), hv.block_visibility)
    assert np.array_equal(dv.host_allocation_types(), hv.allocation_types)
    assert np.array_equal(dv.host_allocation_blocks(), hv.allocation_blocks)
    n = int(ctr[T.VK_CTR_VISIBLE])
    got = dv.visible_blocks[:n].cpu().numpy()
    assert np.array_equal(np.sort(got), hv.visible())     # order is unspecified (volume.cu:80-83)
    if voxels:
        assert dv.host_voxels().tobytes() == hv.voxels.tobytes()


DEFINED_COUNTERS = (T.VK_CTR_VISIBLE, T.VK_CTR_VOXEL_PTR, T.VK_CTR_EXCESS_PTR, T.VK_CTR_DROPPED, T.VK_CTR_BANDED)


def state_arrays(dv):
    """the state of an api.Volume as host arrays, with the dtypes of the oracle's HostVolume: what the comparisons below
    take — from a device volume in most tests, from the files of a replay in test_gpu_chain_replay"""
    return {"hash_entries": dv.host_entries(), "block_visibility": dv.host_visibility(),
            "free_voxel_blocks": dv.free_voxel_blocks.cpu().numpy(), "voxels": dv.host_voxels(), "counters": dv.read_counters(),
            "allocation_types": dv.host_allocation_types(), "allocation_blocks": dv.host_allocation_blocks(),
            "visible_blocks": dv.visible_blocks.cpu().numpy()}


def assert_arrays_same_state(got, hv, all_counters=True):
    """assert_same_state on the arrays of state_arrays"""
    assert np.array_equal(got["hash_entries"], hv.hash_entries)
    assert np.array_equal(got["block_visibility"], hv.block_visibility)
    assert np.array_equal(got["free_voxel_blocks"], hv.free_voxel_blocks)
    assert got["voxels"].tobytes() == hv.voxels.tobytes()
    counters = got["counters"]
    print("counters", counters, hv.counters[:T.VK_CTR_PUBLIC])
    if all_counters:
        assert np.array_equal(counters, hv.counters[:T.VK_CTR_PUBLIC])
    for counter in DEFINED_COUNTERS:
        assert counters[counter] == hv.counters[counter], counter
    assert np.array_equal(got["allocation_types"], hv.allocation_types)


def assert_same_state(dv, hv, all_counters=True):
    """everything a volume operation defines, and the rest of the volume with it. `all_counters`: the device has run nothing
    but uploads and such operations, so all its public counters are the host's (the oracle does not keep the SetView
    statistics)"""
    sync()
    assert_arrays_same_state(state_arrays(dv), hv, all_counters)


def assert_arrays_volume_equal(got, hv):
    """assert_volume_equal on the arrays of state_arrays"""
    ctr = got["counters"]
    for i in (T.VK_CTR_VISIBLE, T.VK_CTR_VOXEL_PTR, T.VK_CTR_EXCESS_PTR, T.VK_CTR_DROPPED):
        assert ctr[i] == hv.counters[i], (i, ctr, hv.counters)
    assert np.array_equal(got["hash_entries"], hv.hash_entries)
    assert np.array_equal(got["block_visibility"], hv.block_visibility)
    assert np.array_equal(got["allocation_types"], hv.allocation_types)
    assert np.array_equal(got["allocation_blocks"], hv.allocation_blocks)
    n = int(ctr[T.VK_CTR_VISIBLE])
    assert np.array_equal(np.sort(got["visible_blocks"][:n]), hv.visible())     # order is unspecified (volume.cu:80-83)
    assert got["voxels"].tobytes() == hv.voxels.tobytes()


def assert_arrays_state(got, hv, defined):
    """the arrays of state_arrays hold the host's state. `defined`: VK_CTR_BANDED is the statements' too — everything
    assert_same_state compares; after a frame step it is the device's own, and the comparison is continue_both's: the
    volume, and the free list up to VK_CTR_VOXEL_PTR"""
    if defined:
        assert_arrays_same_state(got, hv, all_counters=False)
        return
    assert_arrays_volume_equal(got, hv)
    free = max(int(hv.counters[T.VK_CTR_VOXEL_PTR]) + 1, 0)
    assert np.array_equal(got["free_voxel_blocks"][:free], hv.free_voxel_blocks[:free])


def assert_untouched(dv, before):
    """what the call must leave byte for byte as it found it: everything but the voxels"""
    sync()
    assert np.array_equal(dv.host_entries(), before.hash_entries)
    assert np.array_equal(dv.host_visibility(), before.block_visibility)
    assert np.array_equal(dv.free_voxel_blocks.cpu().numpy(), before.free_voxel_blocks)
    assert np.array_equal(dv.host_allocation_types(), before.allocation_types)
    assert np.array_equal(dv.host_allocation_blocks(), before.allocation_blocks)
    assert np.array_equal(dv.read_counters(), before.counters[:T.VK_CTR_PUBLIC])


def continue_both(api, orc, dv, hv, yaw_deg):
    """three SetView calls, a depth integration and a raycast on both sides. vk_volume_set_view_rounds ends its rounds with
    the first round that drops a request (vk.h), so where the oracle's three calls drop one the device makes three calls too."""
    dropped = int(hv.counters[T.VK_CTR_DROPPED])
    want = R.continue_at(orc, hv, yaw_deg)
    hf = R.frame_at(orc, yaw_deg)
    df = api.Frame(hf.depth, hf.depth_projection, hf.depth_to_world)
    if int(hv.counters[T.VK_CTR_DROPPED]) != dropped:
        for _ in range(3):
            dv.set_view(df)
    else:
        dv.set_view(df, rounds=3)
    api.DepthIntegrator(dv).integrate(df)
    out = api.Frame(np.zeros((R.H, R.W), np.float32), hf.depth_projection, hf.depth_to_world)
    api.Tracer(dv).trace(out)
    assert_volume_equal(dv, hv)
    assert np.array_equal(dv.free_voxel_blocks.cpu().numpy()[:max(int(hv.counters[T.VK_CTR_VOXEL_PTR]) + 1, 0)],
                          hv.free_voxel_blocks[:max(int(hv.counters[T.VK_CTR_VOXEL_PTR]) + 1, 0)])
    for got, expected in zip((out.depth, out.color, out.normals), want):
        assert got.cpu().numpy().tobytes() == expected.tobytes()
    assert (want[0] > 0).sum() > 1000


# ---- the 27 sums of a Gauss-Newton system --------------------------------------------------------------------------------

def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def assert_system(got, want, absolute):
    """test_icp_system's rule"""
    error = np.abs(got.astype(np.float64) - want)
    bound = 2e-5 * absolute + 1e-12
    print("system: worst error / bound", float((error / bound).max()))
    assert (error <= bound).all()
    assert not got[21:36].any() and not got[43:48].any()


def _without_parameter(packed, gradient, n, drop):
    """The packed n x n system with row and column `drop` zeroed (and that gradient entry): rank n - 1."""
    H = np.zeros((n, n), np.float32)
    H[np.tril_indices(n)] = packed[: n * (n + 1) // 2]
    H[drop, :] = 0
    H[:, drop] = 0
    g = np.array(gradient[:n], np.float32)
    g[drop] = 0
    return H[np.tril_indices(n)].copy(), g
