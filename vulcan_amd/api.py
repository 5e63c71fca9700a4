"""ctypes bindings of libvk_hip.so (include/vk.h) and thin host classes that mirror
the reference's Volume / Integrator / Tracer / Frame surface for tests and
bench.py. Device memory lives in torch tensors (plumbing only): every compute
call goes through the C ABI on the HIP stream torch is currently using.

There is NO CPU fallback: loading fails loudly when the library is missing, and
every wrapper raises VkError on a non-zero return code.
"""
import ctypes as C
import os

import numpy as np

from . import vk_types as T

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libvk_hip.so")
_LIB = None

# name -> argtypes, in the order of include/vk.h (restype is int unless noted)
_P, _I, _F, _SZ = C.c_void_p, C.c_int, C.c_float, C.c_size_t
_PP = C.POINTER(C.c_void_p)
_SIGNATURES = {
    "vk_error_string": ([_I], C.c_char_p),
    "vk_version": ([], _I),
    "vk_abi_version": ([], _I),
    "vk_abi_check": ([_I, _SZ, _SZ, _I], _I),
    "vk_device_count": ([C.POINTER(_I)], _I),
    "vk_set_device": ([_I], _I),
    "vk_device_name": ([C.c_char_p, _SZ], _I),
    "vk_stream_create": ([_PP], _I),
    "vk_stream_destroy": ([_P], _I),
    "vk_stream_synchronize": ([_P], _I),
    "vk_malloc": ([_PP, _SZ], _I),
    "vk_free": ([_P], _I),
    "vk_memcpy_h2d": ([_P, _P, _SZ, _P], _I),
    "vk_memcpy_d2h": ([_P, _P, _SZ, _P], _I),
    "vk_memcpy_d2d": ([_P, _P, _SZ, _P], _I),
    "vk_memset": ([_P, _I, _SZ, _P], _I),
    "vk_malloc_host": ([_PP, _SZ], _I),
    "vk_free_host": ([_P], _I),
    "vk_event_create": ([_PP], _I),
    "vk_event_destroy": ([_P], _I),
    "vk_event_record": ([_P, _P], _I),
    "vk_event_elapsed_ms": ([_P, _P, C.POINTER(_F)], _I),
    "vk_memcpy_h2d_async": ([_P, _P, _SZ, _P], _I),
    "vk_event_create_ordering": ([_PP, _I], _I),
    "vk_stream_wait_event": ([_P, _P], _I),
    "vk_event_synchronize": ([_P], _I),
    "vk_volume_initialize": ([_P, _P], _I),
    "vk_volume_reset_block_visibility": ([_P, _P], _I),
    "vk_volume_create_allocation_requests": ([_P, _P, _I, _I, _P, _P, _P], _I),
    "vk_volume_handle_allocation_requests": ([_P, _P], _I),
    "vk_volume_update_block_visibility": ([_P, _I, _I, _P, _P, _P], _I),
    "vk_volume_set_view": ([_P, _P, _P], _I),
    "vk_volume_read_counters_sync": ([_P, _P, _P], _I),
    "vk_integrate_depth": ([_P, _P, _P, _P], _I),
    "vk_integrate_color": ([_P, _P, _P, _P], _I),
    "vk_integrate_depth_color": ([_P, _P, _P, _P], _I),
    "vk_light_compute_frame_mask": ([_P, _F, _P, _P], _I),
    "vk_integrate_light_color": ([_P, _P, _P, _P, _P, _P], _I),
    "vk_integrate_depth_light": ([_P, _P, _P, _P, _P, _P], _I),
    "vk_trace_compute_patches": ([_P, _P, _P, _P, _F, _F, _F, _I, _P, _I, _I, _I, _I, _P, _I, _P, _P], _I),
    "vk_trace_compute_bounds": ([_P, _P, _I, _I, _P, _P], _I),
    "vk_trace_reset_bounds": ([_P, _I, _P], _I),
    "vk_trace_compute_block_bounds": ([_P, _P, _P, _P, _F, _F, _F, _I, _P, _I, _I, _I, _I, _P, _P], _I),
    "vk_trace_compute_points": ([_P, _P, _P, _I, _F, _F, _F, _P, _P, _P, _P, _I, _I, _I, _I, _P], _I),
    "vk_frame_compute_normals": ([_P, _P, _P, _I, _I, _P], _I),
    "vk_frame_filter_depths": ([_I, _I, _P, _P, _P], _I),
    "vk_trace_bounds_floats": ([_I, _I], _SZ),
    "vk_trace": ([_P, _P, _F, _F, _P, _I, _I, _P, _P, _P, _P], _I),
    "vk_light_prepare": ([_P, _F, _P, _P, _P], _I),
    "vk_integrate_ahead": ([_P, _P, _P, _I, _P, _P, _P, _P, _P], _I),
    "vk_integrate_time_next": ([_P, _P], _I),
    "vk_trace_ahead": ([_P, _P, _P, _P, _P, _P, _P], _I),
    "vk_image_downsample": ([_I, _I, _P, _P, _I, _P], _I),
    "vk_color_image_downsample": ([_I, _I, _P, _P, _I, _P], _I),
    "vk_icp_compute_residuals": ([_P, _P, _P, _P, _P, _P], _I),
    "vk_icp_compute_jacobian": ([_P, _P, _P, _P, _I, _P, _P], _I),
    "vk_icp_workspace_floats": ([_I, _I], _SZ),
    "vk_icp_compute_system": ([_P, _P, _P, _P, _P, _I, _P, _P, _P, _P], _I),
    "vk_icp_solve_update": ([_P, _P, _I, _P, _P, _P, _P], _I),
    "vk_icp_solve_update_rig": ([_P, _P, _I, _P, _P, _P, _P], _I),
    "vk_icp_track": ([_P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P], _I),
    "vk_transform_upload": ([_P, _P, _P], _I),
    "vk_icp_pyramid_floats": ([_I, _I, _I, _I], _SZ),
    "vk_icp_pyramid_track": ([_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P], _I),
    "vk_icp_pyramid_track_frame": ([_P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P], _I),
    "vk_track_wait": ([_P, _P], _I),
    "vk_reduce_nothing": ([_P, _I, _P, _P], _I),
    "vk_rig_area_bytes": ([], _SZ),
    "vk_icp_track_rig": ([_P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P], _I),
    "vk_icp_track_rig_hook": ([_P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P], _I),
    "vk_color_tracker_begin": ([_P, _P, _P, _P, _P, _P, _F, _P, _P, _P, _P, _P], _I),
    "vk_frame_downsample": ([_P, _P, _P, _P, _P], _I),
    "vk_volume_set_view_prepare": ([_P, _P, _P, _P], _I),
    "vk_volume_set_view_rounds": ([_P, _P, _P, _I, _P], _I),
    "vk_volume_set_view_rounds_split": ([_P, _P, _P, _I, _P, _P, _P], _I),
    "vk_trace_ahead_requests": ([_P, _P, _P, _P, _P, _P, _P, _P, _P, _P], _I),
    "vk_volume_set_view_rounds_ahead": ([_P, _P, _P, _I, _P, _P], _I),
    "vk_requests_ahead_cancel": ([_P, _P, _I, _P], _I),
    "vk_trace_normals_settle": ([_P, _P], _I),
    "vk_light_prepared": ([_P, _P, C.c_float], _I),
    "vk_color_image_convert": ([_I, _P, _P, _P], _I),
    "vk_image_gradients": ([_I, _I, _P, _P, _P, _P], _I),
    "vk_color_tracker_compute_residuals": ([_P, _P, _P, _P, _P], _I),
    "vk_color_tracker_compute_jacobian": ([_P, _P, _P, _I, _P, _P], _I),
    "vk_color_tracker_compute_system": ([_P, _P, _P, _P, _I, _P, _P, _P, _P], _I),
    "vk_color_tracker_solve_update": ([_P, _P, _I, _P, _P, _P, _P, _P, _P], _I),
    "vk_color_tracker_track": ([_P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P], _I),
    "vk_light_tracker_compute_residuals": ([_P, _P, _P, _P, _P, _P], _I),
    "vk_light_tracker_compute_jacobian": ([_P, _P, _P, _P, _I, _P, _P], _I),
    "vk_light_tracker_compute_system": ([_P, _P, _P, _P, _P, _I, _P, _P, _P, _P], _I),
    "vk_light_tracker_track": ([_P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P], _I),
    "vk_compact_workspace_bytes": ([C.c_int32], _SZ),
    "vk_compact_offsets": ([_P, C.c_int32, _P, _P, _P, _P], _I),
    "vk_extract_workspace_bytes": ([C.c_int32, C.c_int32], _SZ),
    "vk_extract_mesh": ([_P, _I, _I, _P, C.c_int32, _P, C.c_int32, _P, _P, _P], _I),
    "vk_extract_mesh_attributes": ([_P, _I, _I, _P, _P, _P, C.c_int32, _P, C.c_int32, _P, _P, _P], _I),
    "vk_volume_release_workspace_bytes": ([C.c_int32, C.c_int32], _SZ),
    "vk_volume_release_blocks": ([_P, _P, _P, _P, _P], _I),
    "vk_volume_merge_workspace_bytes": ([C.c_int32, C.c_int32], _SZ),
    "vk_volume_merge": ([_P, _P, _P, _P, _P, _P], _I),
    "vk_volume_merge_posed_workspace_bytes": ([C.c_int32, C.c_int32, C.c_int32, C.c_int32], _SZ),
    "vk_volume_merge_posed": ([_P, _P, _P, _P, _P, _P], _I),
    "vk_volume_merge_resampled_workspace_bytes": ([C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32], _SZ),
    "vk_volume_merge_resampled": ([_P, _P, _P, _P, _P, _P], _I),
    "vk_volume_pack_workspace_bytes": ([C.c_int32, C.c_int32], _SZ),
    "vk_volume_pack": ([_P, _P, _P, _P, _P, _P], _I),
    "vk_volume_merge_packed_workspace_bytes": ([C.c_int32], _SZ),
    "vk_volume_merge_packed": ([_P, _P, C.c_int32, _F, _F, _P, _P, _P, _P], _I),
    "vk_volume_register_workspace_bytes": ([C.c_int32, C.c_int32], _SZ),
    "vk_volume_register_terms": ([_P, _P, _P, _P, _P, _P, _P, _P, _P], _I),
    "vk_volume_register_system": ([_P, _P, _P, _P, _P, _P, _P, _P], _I),
    "vk_volume_register": ([_P, _P, _P, _P, _P, _P, _P, _P, _P, _P], _I),
    "vk_volume_sample": ([_P, _P, C.c_int32, _P, _P, _P, _P, _P], _I),
    "vk_volume_cast_rays": ([_P, _P, C.c_int32, _P, _P, _P, _P, _P, _P, _P], _I),
    "vk_volume_integrate_rays_workspace_bytes": ([C.c_int32, C.c_int32], C.c_size_t),
    "vk_volume_integrate_rays": ([_P, _P, _P, C.c_int32, _P, _P, _P, _P, _P], _I),
    "vk_volume_integrate_rays_time_next": ([_P, C.c_int32], _I),
    "vk_volume_carve_rays_workspace_bytes": ([C.c_int32, C.c_int32], C.c_size_t),
    "vk_volume_carve_rays": ([_P, _P, _P, C.c_int32, _P, _P, _P, _P, _P], _I),
    "vk_volume_color_rays_workspace_bytes": ([C.c_int32, C.c_int32], C.c_size_t),
    "vk_volume_color_rays": ([_P, _P, _P, _P, C.c_int32, _P, _P, _P, _P, _P], _I),
    "vk_volume_color_rays_time_next": ([_P, C.c_int32], _I),
    "vk_volume_register_rays_workspace_bytes": ([C.c_int32], C.c_size_t),
    "vk_volume_register_rays_terms": ([_P, _P, _P, C.c_int32, _P, _P, _P, _P, _P, _P, _P], _I),
    "vk_volume_register_rays_system": ([_P, _P, _P, C.c_int32, _P, _P, _P, _P, _P, _P], _I),
    "vk_volume_register_rays": ([_P, _P, _P, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P], _I),
    "vk_volume_score_poses_workspace_bytes": ([C.c_int32, C.c_int32], C.c_size_t),
    "vk_volume_score_poses": ([_P, _P, _P, C.c_int32, _P, C.c_int32, _P, _P, _P, _P], _I),
    "vk_volume_score_poses_best": ([_P, _P, C.c_int32, _P, _P, _P, _P], _I),
    "vk_volume_classify_cells": ([_P, _P, _F, _P, _P], _I),
    "vk_grid_distance_transform_workspace_bytes": ([_P], C.c_size_t),
    "vk_grid_distance_transform": ([_P, _P, C.c_int32, C.c_int32, _P, _P, _P], _I),
    "vk_volume_distance_field_workspace_bytes": ([_P, _P], C.c_size_t),
    "vk_volume_distance_field": ([_P, _P, _P, _P, _P, _P, _P, _P], _I),
    "vk_detect_workspace_bytes": ([C.c_int32], _SZ),
    "vk_detect_filter": ([_P, _P, C.c_int32, _P, _P, _P, _P], _I),
    "vk_detect": ([_P, _P, C.c_int32, _P, _P, _P, _P], _I),
    "vk_test_hooks_set": ([_P], _I),
    "vk_test_hooks_get": ([_P], _I),
    "vk_test_hooks_loop_count": ([_P, _P, _P], _I),
    "vk_trace_ahead_pyramid": ([_P, _P, _P, _P, _P, _P, _P, _P, _P, _P], _I),
    "vk_volume_requests_at_device_pose": ([_P, _P, _P, _P, _P, _P], _I),
    "vk_volume_set_view_at_device_pose": ([_P, _P, _P, _P, _I, _P], _I),
    "vk_icp_pyramid_track_built": ([_P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P], _I),
}
EXPORTS = tuple(_SIGNATURES)
_REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p)   # vk_icp_reduce_fn


class test_hooks:
    """`with api.test_hooks(set_view_unfused=1): ...` — vk_test_hooks (vk.h) for the duration of the block: the
    test suites' switches (a small posted / retry list, the three-launch SetView, a forced loop abort, a capped
    loop grid) and the cooperative-launch option. The library reads no environment variable on a call path."""

    def __init__(self, **fields):
        self.fields = fields

    def __enter__(self):
        self.saved = T.TestHooks()
        check(lib().vk_test_hooks_get(C.byref(self.saved)), "vk_test_hooks_get")
        new = T.TestHooks.from_buffer_copy(bytes(self.saved))
        for name, value in self.fields.items():
            setattr(new, name, int(value))
        check(lib().vk_test_hooks_set(C.byref(new)), "vk_test_hooks_set")
        return self

    def __exit__(self, *exc):
        check(lib().vk_test_hooks_set(C.byref(self.saved)), "vk_test_hooks_set")
        return False


class TrackAborted(RuntimeError):
    """A Gauss-Newton loop kernel gave up waiting for the other workgroups (vk.h VK_TRACK_ABORTED)."""


class VkError(RuntimeError):
    pass


def lib():
    """Load libvk_hip.so. torch is imported first so the HIP runtime it bundles
    (libamdhip64.so.7) is the one the library binds to."""
    global _LIB, LIB_PATH
    if _LIB is None:
        # VK_HIP_LIBRARY selects another build of the same ABI (the debug build that syncs and
        # checks after every launch, libvk_hip_debug.so, or an experiment) — never a fallback
        LIB_PATH = os.environ.get("VK_HIP_LIBRARY") or LIB_PATH
        if not os.path.exists(LIB_PATH):
            raise VkError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback)")
        import torch  # noqa: F401  (loads the HIP runtime)
        handle = C.CDLL(LIB_PATH)
        for name, (argtypes, restype) in _SIGNATURES.items():
            fn = getattr(handle, name)
            fn.argtypes, fn.restype = argtypes, restype
        # the structs and sizes of vk_types.py against the ones the library was compiled with (vk.h VK_ABI_VERSION)
        if handle.vk_abi_check(T.VK_ABI_VERSION, C.sizeof(T.Volume), C.sizeof(T.Frame), T.VK_CTR_COUNT) != 0:
            raise VkError(f"{LIB_PATH} has binary interface version {handle.vk_abi_version()}, these bindings were written "
                          f"for {T.VK_ABI_VERSION} (or a struct / VK_CTR_COUNT differs): rebuild the library")
        _LIB = handle
    return _LIB


def check(code, what=""):
    if code != 0:
        raise VkError(f"{what}: {lib().vk_error_string(code).decode()} [{code}]")


def _ptr(t):
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


def _ref(s):
    return C.byref(s)


def stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev_bytes(n, device):
    import torch
    return torch.empty(int(n), dtype=torch.uint8, device=device)


def to_numpy(t, dtype):
    """Device byte tensor -> numpy structured array."""
    return np.frombuffer(t.cpu().numpy().tobytes(), dtype=dtype).copy()


# -- what the callers of the volume operations share
def _as_pose(pose, device=False, identity=False):
    """The pose argument of a volume operation. None: None, or the identity with `identity`. A T.Transform: itself. With
    `device`, anything with data_ptr (a device buffer that holds a vk_transform): itself. Anything else is a 4x4 array:
    the Transform of the matrix and its inverse, taken once, on the host."""
    if pose is None:
        return T.Transform.identity() if identity else None
    if isinstance(pose, T.Transform) or (device and hasattr(pose, "data_ptr")):
        return pose
    matrix = np.asarray(pose, dtype=np.float64).reshape(4, 4)
    return T.Transform.from_matrices(matrix, np.linalg.inv(matrix))


def _float_tensor(x, last, message, rows=None):
    """`x`, contiguous, if it is a float32 tensor [N, last] (`last` None: [N]; `rows`: with that N); VkError(message) if not"""
    import torch
    if not (hasattr(x, "data_ptr") and x.dtype == torch.float32 and x.dim() == (1 if last is None else 2)
            and (last is None or x.shape[1] == last) and (rows is None or x.shape[0] == rows)):
        raise VkError(message)
    return x.contiguous()


def _range_ray_arguments(what, rays, ranges, depth_range, voxel_length, r_min, r_max, voxel_units, one_observation=False):
    """The arguments the operations along range rays share, for the operation `what`: (rays, ranges, r_min, r_max, flags).
    `rays` [N, 6] and `ranges` [N] are checked (_float_tensor); a bound that is None is the volume's depth range, in float32
    and divided by the voxel length with `voxel_units`; the flags are VK_RAYS_*."""
    rays = _float_tensor(rays, 6, f"{what}: rays is a float32 [N, 6] device tensor")
    ranges = _float_tensor(ranges, None, f"{what}: ranges is a float32 [N] device tensor, one range per ray", rays.shape[0])
    scale = np.float32(voxel_length) if voxel_units else np.float32(1)
    r_min = float(np.float32(depth_range[0]) / scale) if r_min is None else r_min
    r_max = float(np.float32(depth_range[1]) / scale) if r_max is None else r_max
    flags = (T.VK_RAYS_VOXEL_UNITS if voxel_units else 0) | (T.VK_RAYS_ONE_OBSERVATION if one_observation else 0)
    return rays, ranges, r_min, r_max, flags


def _registration(pose, state, counts, system, device_pose=None):
    """the Registration of what a registration loop left: its pose, (steps, code), counts and system[48]"""
    return Registration(pose, state[0], state[1] == 1, state[1] != T.VK_REGISTER_NO_OVERLAP, counts[2],
                        float(np.sqrt(float(system[42]) / counts[2])) if counts[2] else 0.0, device_pose)


def _ints(counts):
    """a device tensor of counts as a tuple of int: one blocking read"""
    return tuple(int(c) for c in counts.cpu().numpy())


_STAMP = [0]


def _next_stamp():
    _STAMP[0] += 1
    return _STAMP[0]


class Frame:
    """vulcan::Frame (frame.h:11-32) with images in device memory.

    vk_frame.content_id (which content the images hold) = the stamp of the last change this class
    saw — a tensor assigned to .depth / .color / .normals, compute_normals, filter_depths, a raycast
    into the frame — mixed with the tensors' own torch version counters (in-place torch ops).
    A kernel of your own that writes through data_ptr() is invisible: call touch() after it."""

    def __setattr__(self, name, value):
        if name in ("depth", "color", "normals"):
            object.__setattr__(self, "_stamp", _next_stamp())
        object.__setattr__(self, name, value)

    def touch(self):
        self._stamp = _next_stamp()

    def content_id(self):
        h = self._stamp
        for t in (self.depth, self.color, self.normals):
            h = (h * 0x9E3779B97F4A7C15 + (0 if t is None else (t._version + 1) * 0xC2B2AE3D27D4EB4F + t.data_ptr())) & (2 ** 64 - 1)
        return h | 1

    def __init__(self, depth, depth_projection, depth_to_world=None, color=None, normals=None,
                 color_projection=None, depth_to_color=None, device="cuda"):
        import torch
        self.device = device
        self.depth = torch.as_tensor(np.ascontiguousarray(depth, dtype=np.float32)).to(device) \
            if not hasattr(depth, "data_ptr") else depth
        self.height, self.width = self.depth.shape
        self.color = None
        self.normals = None
        if color is not None:
            self.color = torch.as_tensor(np.ascontiguousarray(color, dtype=np.float32)).to(device) \
                if not hasattr(color, "data_ptr") else color
        if normals is not None:
            self.normals = torch.as_tensor(np.ascontiguousarray(normals, dtype=np.float32)).to(device) \
                if not hasattr(normals, "data_ptr") else normals
        self.depth_projection = depth_projection
        self.color_projection = color_projection or depth_projection
        self.depth_to_world = depth_to_world or T.Transform.identity()
        self.depth_to_color = depth_to_color or T.Transform.identity()

    def desc(self):
        d = T.Frame()
        d.depth = self.depth.data_ptr()
        d.color = None if self.color is None else self.color.data_ptr()
        d.normals = None if self.normals is None else self.normals.data_ptr()
        d.width, d.height = self.width, self.height
        if self.color is not None:
            d.color_height, d.color_width = self.color.shape[0], self.color.shape[1]
        d.depth_projection, d.color_projection = self.depth_projection, self.color_projection
        d.depth_to_world, d.depth_to_color = self.depth_to_world, self.depth_to_color
        d.content_id = self.content_id()
        return d

    def compute_normals(self):
        """Frame::ComputeNormals (frame.cpp:21-36)"""
        import torch
        if self.normals is None:
            self.normals = torch.empty((self.height, self.width, 3), dtype=torch.float32, device=self.device)
        k = self.depth_projection
        check(lib().vk_frame_compute_normals(_ptr(self.depth), _ref(k), _ptr(self.normals),
                                             self.width, self.height, stream()), "vk_frame_compute_normals")
        self.touch()
        return self.normals

    def filter_depths(self):
        """Frame::FilterDepths (frame.cpp:8-19)"""
        import torch
        tmp = torch.empty_like(self.depth)
        check(lib().vk_frame_filter_depths(self.width, self.height, _ptr(self.depth), _ptr(tmp), stream()),
              "vk_frame_filter_depths")
        self.depth.copy_(tmp)
        self.touch()

    def downsample(self):
        """Frame::Downsample (frame.cpp:38-58): nearest depth/normals, box colour,
        intrinsics halved."""
        import torch
        w2, h2 = self.width // 2, self.height // 2
        depth = torch.empty((h2, w2), dtype=torch.float32, device=self.device)
        check(lib().vk_image_downsample(self.width, self.height, _ptr(self.depth), _ptr(depth), 1, stream()),
              "vk_image_downsample")
        color = normals = None
        if self.color is not None:
            ch, cw = self.color.shape[0], self.color.shape[1]     # ColorImage::Downsample uses its own size
            color = torch.empty((ch // 2, cw // 2, 3), dtype=torch.float32, device=self.device)
            check(lib().vk_color_image_downsample(cw, ch, _ptr(self.color), _ptr(color), 0,
                                                  stream()), "vk_color_image_downsample")
        if self.normals is not None:
            normals = torch.empty((h2, w2, 3), dtype=torch.float32, device=self.device)
            check(lib().vk_color_image_downsample(self.width, self.height, _ptr(self.normals), _ptr(normals), 1,
                                                  stream()), "vk_color_image_downsample")
        f32 = np.float32

        def half(k):  # Vector2f / 2 multiplies by 1/2 (matrix.h:279-295)
            return T.Projection.make(f32(k.fx) * f32(0.5), f32(k.fy) * f32(0.5),
                                     f32(k.cx) * f32(0.5), f32(k.cy) * f32(0.5))
        return Frame(depth, half(self.depth_projection), self.depth_to_world, color, normals,
                     half(self.color_projection), self.depth_to_color, self.device)


class Registration:
    """what Volume.register and Volume.register_rays return. `device_pose` (register_rays; None from register): a device
    buffer of its own that holds `pose` as a vk_transform — what integrate_rays, carve_rays, color_rays, cast_rays and sample
    take as `pose` without a copy through the host."""

    def __init__(self, pose, steps, converged, overlap, residuals, rms, device_pose=None):
        self.pose, self.steps, self.converged, self.overlap, self.residuals, self.rms = pose, steps, converged, overlap, residuals, rms
        self.device_pose = device_pose

    def __repr__(self):
        return (f"Registration(steps={self.steps}, converged={self.converged}, overlap={self.overlap}, "
                f"residuals={self.residuals}, rms={self.rms:.3g})")


class PoseScores:
    """what Volume.score_poses returns: `scores`, the device buffer of vk_pose_score vk_volume_score_poses wrote, and `poses`,
    the device buffer of the `count` candidate vk_transforms it scored. Nothing is read until host() is called."""

    def __init__(self, scores, poses, count, device):
        self.scores, self.poses, self.count, self.device = scores, poses, int(count), device
        self._host = None

    def __len__(self):
        return self.count

    def host(self):
        """the scores as a structured array (vk_types.pose_score_dtype): one blocking read, kept"""
        if self._host is None:
            self._host = to_numpy(self.scores[:self.count * T.pose_score_dtype.itemsize], T.pose_score_dtype)
        return self._host

    def _per_residual(self, field):
        h = self.host()
        return np.where(h["residuals"] > 0, h[field] / 1048576.0 / np.maximum(h["residuals"], 1), 0.0)

    @property
    def mean_abs(self):
        """per pose, the mean |D| over its residuals in truncation lengths (0 where there is none)"""
        return self._per_residual("sum_abs")

    @property
    def rms(self):
        """per pose, the root of the mean D^2 over its residuals in truncation lengths (0 where there is none)"""
        return np.sqrt(self._per_residual("sum_squares"))

    def _best_call(self, min_residuals, best, pose_out):
        params = T.ScorePosesParams(0, int(min_residuals), 0.0, 0.0, 0.0, 0)
        check(lib().vk_volume_score_poses_best(_ptr(self.scores), _ptr(self.poses), self.count, _ref(params), _ptr(best), _ptr(pose_out),
                                               stream()), "vk_volume_score_poses_best")

    def best(self, min_residuals=1):
        """vk_volume_score_poses_best: (index, device_pose) of the pose with the most residuals, then the smallest sum of |D|,
        then the smallest index — `device_pose` a device buffer of its own that holds that vk_transform, what register_rays,
        integrate_rays and the other ray operations take as `pose` — or (-1, None) when that pose has fewer than
        `min_residuals` residuals. One blocking read of the index."""
        import torch
        best = torch.zeros(1, dtype=torch.int32, device=self.device)
        pose_out = _dev_bytes(C.sizeof(T.Transform), self.device)
        self._best_call(min_residuals, best, pose_out)
        index = int(best.cpu()[0])
        return (index, pose_out) if index >= 0 else (-1, None)


class Samples:
    """what Volume.sample returns: tensor views of the two device buffers vk_volume_sample wrote. `distance` [N] is in
    truncation lengths and 1.0 where `distance_weight` [N] (int16) is 0; `color` [N, 3] with `color_weight` [N] (None when
    the colour was not asked for); `gradient` [N, 3] in truncation lengths per voxel and `gradient_valid` [N] (1.0 or 0.0),
    None when the gradient was not asked for."""

    def __init__(self, samples, gradients, color, truncation_length):
        self.samples, self.gradients, self.truncation_length = samples, gradients, truncation_length
        import torch
        floats, shorts = samples.view(torch.float32), samples.view(torch.int16)
        self.distance, self.distance_weight = floats[:, 0], shorts[:, 8]
        self.color, self.color_weight = (floats[:, 1:4], shorts[:, 9]) if color else (None, None)
        self.gradient, self.gradient_valid = (None, None) if gradients is None else (gradients[:, :3], gradients[:, 3])

    def metres(self):
        """the distance in metres (a new tensor)"""
        return self.distance * self.truncation_length


class RayHits:
    """what Volume.cast_rays returns: tensor views of the device buffers vk_volume_cast_rays wrote. `status` [N] int32 is
    VK_RAY_MISS, _HIT, _STEPS (max_steps ran out) or _INVALID per ray; `t` [N] the distance along the normalised direction
    in the unit the rays came in, 0.0 where there is no hit; the fields of the hit's sample are Samples' (`distance`,
    `distance_weight`, `color`, `color_weight`, `gradient`, `gradient_valid`), Voxel::Empty() and zeros without a hit."""

    def __init__(self, t, status, samples, gradients, color, truncation_length):
        self.t, self.status = t, status
        self.hit = status == T.VK_RAY_HIT
        at = Samples(samples, gradients, color, truncation_length)
        self.samples, self.gradients = at.samples, at.gradients
        self.distance, self.distance_weight, self.color, self.color_weight = at.distance, at.distance_weight, at.color, at.color_weight
        self.gradient, self.gradient_valid = at.gradient, at.gradient_valid


CELL_UNKNOWN, CELL_FREE, CELL_OCCUPIED = T.CELL_UNKNOWN, T.CELL_FREE, T.CELL_OCCUPIED


class DistanceField:
    """what Volume.distance_field returns: the device tensors vk_volume_distance_field wrote, each [nz, ny, nx] over the
    grid of `origin` (lattice coordinates of the first voxel), `stride` voxels per cell and `cell_length` metres per cell.
    `classes` uint8 (CELL_UNKNOWN, CELL_FREE, CELL_OCCUPIED); `distance` float32, metres to the nearest site cell, +inf
    beyond the cap (with `signed`: negative on site cells); `squared_cells` int32, the squared distance in cells and
    VK_FIELD_BEYOND beyond the cap, or None when it was not asked for."""

    def __init__(self, classes, distance, squared_cells, origin, stride, cell_length):
        self.classes, self.distance, self.squared_cells = classes, distance, squared_cells
        self.origin, self.stride, self.cell_length = tuple(int(o) for o in origin), int(stride), float(cell_length)


def grid_for_box(lo, hi, stride, voxel_length):
    """(origin, dims) of the smallest grid of `stride`-voxel cells, aligned to the stride, that covers the metric box
    [lo, hi] of a volume of this voxel length: host arithmetic, in float64"""
    stride = int(stride)
    first = np.floor(np.asarray(lo, dtype=np.float64) / voxel_length / stride).astype(np.int64)
    last = np.floor(np.asarray(hi, dtype=np.float64) / voxel_length / stride).astype(np.int64)
    if np.any(last < first):
        raise VkError("grid_for_box: hi lies below lo")
    return tuple(int(f) * stride for f in first), tuple(int(n) for n in last - first + 1)


def _grid_workspace_bytes(nx, ny, nz):
    return lib().vk_grid_distance_transform_workspace_bytes((C.c_int32 * 3)(nx, ny, nz))


def _grid_shape(dims):
    """[nz, ny, nx] of a grid of dims = (nx, ny, nz) cells that the library takes; VkError for any other"""
    nx, ny, nz = (int(d) for d in dims)
    if not (all(1 <= n <= 1024 for n in (nx, ny, nz)) and _grid_workspace_bytes(nx, ny, nz)):
        raise VkError(f"a grid has 1 .. 1024 cells per axis and at most 2^27 in all, not {(nx, ny, nz)}")
    return nz, ny, nx


def distance_transform(classes, site_mask=T.CELL_OCCUPIED, max_cells=256):
    """vk_grid_distance_transform (not upstream): the exact squared Euclidean distance, in cells, from every cell of the
    uint8 [nz, ny, nx] device tensor `classes` to the nearest cell with class & site_mask != 0, as an int32 tensor of that
    shape; VK_FIELD_BEYOND where there is none within `max_cells`. With other masks: the distance to unobserved space, or
    the depth inside an obstacle. Three launches, nothing is read back."""
    import torch
    if not (hasattr(classes, "data_ptr") and classes.dtype == torch.uint8 and classes.dim() == 3):
        raise VkError("distance_transform: classes is a uint8 [nz, ny, nx] device tensor")
    classes = classes.contiguous()
    nz, ny, nx = (int(n) for n in classes.shape)
    dims = (C.c_int32 * 3)(nx, ny, nz)
    workspace = _dev_bytes(_grid_workspace_bytes(nx, ny, nz), classes.device)
    d2 = torch.empty((nz, ny, nx), dtype=torch.int32, device=classes.device)
    check(lib().vk_grid_distance_transform(_ptr(classes), dims, int(site_mask), int(max_cells), _ptr(d2), _ptr(workspace), stream()),
          "vk_grid_distance_transform")
    return d2


class PackedVolume:
    """The blocks of a volume, compact and in a defined order (vk_block_pack, vk.h): what Volume.pack returns and
    Volume.merge takes in a volume's place. `origins`: int16 [count, 4] (x, y, z, 0), `voxels`: uint8 [count * 10240],
    both on one device; `voxel_length`, `truncation_length`: the lattice the voxels belong to. Not upstream."""
    BLOCK_BYTES = T.BLOCK_VOXELS * 20

    def __init__(self, origins, voxels, voxel_length, truncation_length):
        self.origins, self.voxels = origins, voxels
        self.count = int(origins.shape[0])
        if self.voxels.numel() != self.count * self.BLOCK_BYTES:
            raise VkError(f"PackedVolume: {self.count} origins and {self.voxels.numel()} bytes of voxels")
        self.voxel_length, self.truncation_length = float(voxel_length), float(truncation_length)

    def __len__(self):
        return self.count

    @property
    def device(self):
        return self.voxels.device

    def desc(self):
        d = T.BlockPack()
        d.capacity = self.count
        d.origins, d.voxels = self.origins.data_ptr(), self.voxels.data_ptr()
        return d

    def host(self):
        """(origins [count, 4] int16, voxels [512 * count] of vk_types.voxel_dtype): one blocking read each"""
        return self.origins.cpu().numpy(), to_numpy(self.voxels, T.voxel_dtype)

    def to(self, device):
        """the pack on `device`: two plain copies (the pack itself when it is there already)"""
        return PackedVolume(self.origins.to(device), self.voxels.to(device), self.voxel_length, self.truncation_length)

    def save(self, path):
        """io.write_map: the pack as one file, at the size of its blocks"""
        from . import io
        io.write_map(path, self.origins.cpu().numpy(), self.voxels.cpu().numpy(), self.voxel_length, self.truncation_length)

    @classmethod
    def load(cls, path, device="cuda"):
        """io.read_map, which refuses a malformed file (ValueError) before anything reaches a device"""
        import torch
        from . import io
        origins, voxels, voxel_length, truncation_length = io.read_map(path)
        return cls(torch.from_numpy(origins).to(device), torch.from_numpy(voxels).to(device), voxel_length, truncation_length)


class Volume:
    """vulcan::Volume (volume.h:16-117): owns the device buffers, forwards to vk_volume_*."""

    def __init__(self, main_block_count, excess_block_count, voxel_length=0.008,
                 truncation_length=0.04, depth_range=(0.1, 5.0), device="cuda"):
        import torch
        self.device = device
        n = main_block_count + excess_block_count
        self.main, self.excess, self.max = main_block_count, excess_block_count, n
        self.voxels = _dev_bytes(n * 512 * 20, device)
        self.hash_entries = _dev_bytes(n * 16, device)
        self.free_voxel_blocks = torch.empty(n, dtype=torch.int32, device=device)
        self.allocation_types = _dev_bytes(main_block_count, device)
        self.allocation_blocks = _dev_bytes(main_block_count * 8, device)
        self.block_visibility = _dev_bytes(n, device)
        self.visible_blocks = torch.empty(n, dtype=torch.int32, device=device)
        self.counters = torch.zeros(T.VK_CTR_COUNT, dtype=torch.int32, device=device)
        self.voxel_length = voxel_length
        self.truncation_length = truncation_length
        self.depth_range = depth_range
        # raycast bounds computed ahead, inside the integrate launch (vk_view_bounds);
        # a Tracer attaches its scratch and settings here
        self.view_bounds = None
        self._view_records = []      # every Tracer's record: all go stale when the visible list changes
        self._workspaces = {}        # {operation: (size, device bytes of its workspace, its counts tensor)}, see _workspace
        check(lib().vk_volume_initialize(_ref(self.desc()), stream()), "vk_volume_initialize")

    def attach_view_bounds(self, record):
        """A Tracer registers its vk_view_bounds: the integrators prepare the bounds of
        the most recently attached one; every attached record is invalidated together."""
        self._view_records.append(record)
        self.view_bounds = record

    def _view_changed(self):
        for record in self._view_records:
            record.valid = 0

    def desc(self):
        d = T.Volume()
        d.voxels = self.voxels.data_ptr()
        d.hash_entries = self.hash_entries.data_ptr()
        d.free_voxel_blocks = self.free_voxel_blocks.data_ptr()
        d.allocation_types = self.allocation_types.data_ptr()
        d.allocation_blocks = self.allocation_blocks.data_ptr()
        d.block_visibility = self.block_visibility.data_ptr()
        d.visible_blocks = self.visible_blocks.data_ptr()
        d.counters = self.counters.data_ptr()
        d.main_block_count, d.excess_block_count = self.main, self.excess
        d.voxel_length, d.truncation_length = self.voxel_length, self.truncation_length
        d.min_depth, d.max_depth = self.depth_range
        return d

    # -- Volume::SetView and its four protected stages (volume.cu:430-535)
    light_prep = None      # T.LightPrep of an attached LightIntegrator (attach_light_preparation)
    requests_ahead = None  # T.RequestsAhead: the frame Tracer.trace(.., next_frame=) announced (vk_requests_ahead)

    def attach_light_preparation(self, prep):
        """A LightIntegrator's mask / record buffers: set_view fills them in its own request pass
        (vk_volume_set_view_prepare) for the integrate that follows."""
        self.light_prep = prep

    def set_view(self, frame, rounds=1, compute_normals=False):
        """Volume::SetView. `rounds` > 1: the state of that many consecutive SetView calls with this
        frame (the reference's frame loop makes three, apps/vulcan/vulcan.cu:316-318), in one call.
        `compute_normals`: frame.compute_normals() is still due and is done by this call — inside its
        request pass when a LightIntegrator's preparation rides along (vk_light_prep.normals_out)."""
        import torch
        self._view_changed()
        announced = self.requests_ahead is not None and self.requests_ahead.valid == 1
        stale_prep = False
        if announced and compute_normals:
            # Tracer.trace(.., next_frame=frame, next_needs_normals=True) has computed this frame's normals with the pass
            # (or, without a riding preparation, as a launch of their own): nothing is due any more. Touching the frame
            # now would give it a content id the record does not name, and the library would refuse the very frame that
            # was announced. Any OTHER frame is refused below, by the library, with the record kept.
            r = self.requests_ahead
            if not (r.depth == (frame.depth.data_ptr() if frame.depth is not None else None) and r.content_id == frame.desc().content_id):
                raise VkError("set_view(compute_normals=True): another frame was announced by Tracer.trace(next_frame=...); "
                              "fuse that frame first, or Volume.cancel_requests_ahead()")
            if not r.normals_made:
                # announced WITHOUT its normals (trace(next_frame=frame), next_needs_normals left False): they are still due
                # (skipped until round 5 on the record's validity alone). Written in place and without a new stamp
                # — the record names the frame by its content id — and whatever the pass prepared from the old normals is
                # void after this SetView: LightIntegrator.integrate prepares again from the new ones.
                if frame.normals is None:
                    raise VkError("set_view(compute_normals=True): the announced frame has no normal image to write to")
                check(lib().vk_frame_compute_normals(_ptr(frame.depth), _ref(frame.depth_projection), _ptr(frame.normals),
                                                     frame.width, frame.height, stream()), "vk_frame_compute_normals")
                stale_prep = self.light_prep is not None
            compute_normals = False
        if compute_normals:
            if self.light_prep is None:
                frame.compute_normals()
            else:
                if frame.normals is None:
                    frame.normals = torch.empty((frame.height, frame.width, 3), dtype=torch.float32, device=frame.device)
                frame.touch()                                  # the normal image's content is new
                self.light_prep.normals_out = frame.normals.data_ptr()
        prep = _ref(self.light_prep) if self.light_prep is not None else None
        if announced:
            # Tracer.trace(frame, next_frame=...) announced a frame: its request pass is made, this must be its SetView
            # (vk_volume_set_view_rounds_ahead refuses any other frame)
            check(lib().vk_volume_set_view_rounds_ahead(_ref(self.desc()), _ref(frame.desc()), prep, int(rounds),
                                                        _ref(self.requests_ahead), stream()), "vk_volume_set_view_rounds_ahead")
        elif compute_normals and prep is not None:
            check(lib().vk_volume_set_view_rounds(_ref(self.desc()), _ref(frame.desc()), prep, int(rounds), stream()),
                  "vk_volume_set_view_rounds")
        elif rounds != 1:
            check(lib().vk_volume_set_view_rounds(_ref(self.desc()), _ref(frame.desc()), prep, int(rounds), stream()),
                  "vk_volume_set_view_rounds")
        elif prep is not None:
            check(lib().vk_volume_set_view_prepare(_ref(self.desc()), _ref(frame.desc()), prep, stream()),
                  "vk_volume_set_view_prepare")
        else:
            check(lib().vk_volume_set_view(_ref(self.desc()), _ref(frame.desc()), stream()), "vk_volume_set_view")
        if stale_prep:
            self.light_prep.valid = 0

    def set_view_at_device_pose(self, frame, pose_dev, rounds=1):
        """Volume::SetViewAtDevicePose (not upstream, round 6): SetView(frame, rounds) at the pose in `pose_dev` (a device
        vk_transform: what a tracker's launches in front of this call leave there), enqueued before the host has that pose.
        frame.depth_to_world is ignored. False: not possible in this state (an announced frame, the three-launch test form,
        normals still due) — nothing was launched, call set_view once the pose is known."""
        if self.requests_ahead is not None and self.requests_ahead.valid == 1:
            return False
        prep = _ref(self.light_prep) if self.light_prep is not None else None
        if self.light_prep is not None and self.light_prep.normals_out:
            return False
        rc = lib().vk_volume_set_view_at_device_pose(_ref(self.desc()), _ref(frame.desc()), _ptr(pose_dev), prep, int(rounds), stream())
        if rc == T.VK_ERR_UNSUPPORTED:
            return False
        check(rc, "vk_volume_set_view_at_device_pose")
        self._view_changed()
        return True

    def cancel_requests_ahead(self, rounds=1):
        """vk_requests_ahead_cancel: the way out of an announced frame that will not be fused as announced — its SetView is
        completed from the record (handle + visibility pass), after which any frame may follow."""
        if self.requests_ahead is None:
            return
        self._view_changed()
        check(lib().vk_requests_ahead_cancel(_ref(self.desc()), _ref(self.requests_ahead), int(rounds), stream()),
              "vk_requests_ahead_cancel")

    # -- what the volume operations below share
    _sample_pose = None        # the device vk_transform a host pose of sample / cast_rays / integrate_rays is uploaded to

    def _workspace(self, operation, size, workspace_bytes, counts, flags=0):
        """(workspace, counts tensor) of `operation`: allocated by its first call, again for another `size` (the block
        counts `workspace_bytes` takes) — which a call that continues the one before (VK_MERGE_CONTINUE) cannot start from"""
        import torch
        held = self._workspaces.get(operation)
        if held is None or held[0] != size:
            if flags & T.VK_MERGE_CONTINUE:
                raise VkError("merge: nothing to continue")
            held = self._workspaces[operation] = (size, _dev_bytes(workspace_bytes(*size), self.device),
                                                  torch.zeros(counts, dtype=torch.int32, device=self.device))
        return held[1], held[2]

    def _pose_on_device(self, pose):
        """`pose` as a launch reads it: a T.Transform is uploaded into this volume's device vk_transform (allocated by the
        first) and that buffer returned; a device buffer or None passes through — no library call, no allocation"""
        if not isinstance(pose, T.Transform):
            return pose
        if self._sample_pose is None:
            self._sample_pose = _dev_bytes(C.sizeof(T.Transform), self.device)
        check(lib().vk_transform_upload(_ptr(self._sample_pose), _ref(pose), stream()), "vk_transform_upload")
        return self._sample_pose

    def _table_changes(self):
        """the hash table and the visible list are about to change: what was made ahead for them is void"""
        self._view_changed()
        if self.light_prep is not None:
            self.light_prep.valid = 0

    def release_blocks(self, unobserved=False, min_abs_distance=None, keep_box=None):
        """vk_volume_release_blocks (not upstream): give back the blocks a rule names — `unobserved`: no voxel was ever
        integrated; `min_abs_distance`: observed, but no observed voxel's stored distance (normalised to (-1, 1]) is
        nearer the surface than this; `keep_box` = ((lo x, y, z), (hi x, y, z)) in block coordinates, inclusive: the
        block's origin lies outside — then compact the hash table and rebuild the free list. With no rule: the repair
        alone (ghost entries and leaked slots of an exhausted pool come back). Between SetView calls only: raises while
        a frame is announced. The visible list is empty afterwards (the next set_view rebuilds it) and what was
        prepared ahead for the volume is void. Returns (blocks released, blocks kept, excess entries in use, free
        slots) from one blocking read."""
        self._no_requests_pending("release_blocks")
        rule = T.ReleaseRule()
        if unobserved:
            rule.flags |= T.VK_RELEASE_UNOBSERVED
        if min_abs_distance is not None:
            rule.flags |= T.VK_RELEASE_NO_SURFACE
            rule.min_abs_distance = float(min_abs_distance)
        if keep_box is not None:
            rule.flags |= T.VK_RELEASE_OUTSIDE_BOX
            rule.keep_lo[:] = [int(c) for c in keep_box[0]]
            rule.keep_hi[:] = [int(c) for c in keep_box[1]]
        workspace, counts = self._workspace("release", (self.main, self.excess), lib().vk_volume_release_workspace_bytes, 4)
        self._table_changes()
        check(lib().vk_volume_release_blocks(_ref(self.desc()), _ref(rule), _ptr(counts), _ptr(workspace), stream()),
              "vk_volume_release_blocks")
        return _ints(counts)

    def _merge_call(self, other, flags, max_rounds, max_distance_weight, max_color_weight):
        """one vk_volume_merge(self <- other): the six counts from one blocking read"""
        self._no_requests_pending("merge")
        other._no_requests_pending("merge")
        workspace, counts = self._workspace("merge", (other.main, other.excess), lib().vk_volume_merge_workspace_bytes, 6, flags)
        params = T.MergeParams(int(flags), int(max_rounds), float(max_distance_weight), float(max_color_weight))
        self._table_changes()
        check(lib().vk_volume_merge(_ref(self.desc()), _ref(other.desc()), _ref(params), _ptr(counts), _ptr(workspace), stream()),
              "vk_volume_merge")
        return _ints(counts)

    def _merge_posed_call(self, other, pose, flags, max_rounds, max_distance_weight, max_color_weight):
        """one vk_volume_merge_posed(self <- other through `pose`, a T.Transform): the eight counts from one blocking read"""
        self._no_requests_pending("merge")
        other._no_requests_pending("merge")
        workspace, counts = self._workspace("merge_posed", (other.main, other.excess, self.main, self.excess),
                                            lib().vk_volume_merge_posed_workspace_bytes, 8, flags)
        params = T.MergePoseParams(T.MergeParams(int(flags), int(max_rounds), float(max_distance_weight), float(max_color_weight)), pose)
        self._table_changes()
        check(lib().vk_volume_merge_posed(_ref(self.desc()), _ref(other.desc()), _ref(params), _ptr(counts), _ptr(workspace),
                                          stream()), "vk_volume_merge_posed")
        return _ints(counts)

    def _resample_ratios(self, other):
        """(r_fwd, r_back, K) of vk_volume_merge_resampled(self <- other): the two ratios of the voxel lengths as the library
        takes them, one float32 division each, and the blocks per axis of a source block's box that sizes the workspace"""
        mine, theirs = np.float32(self.voxel_length), np.float32(other.voxel_length)
        r_fwd, r_back = theirs / mine, mine / theirs
        if not (0.25 <= r_fwd <= 4.0 and 0.25 <= r_back <= 4.0):
            raise VkError(f"merge_resampled: voxel lengths {other.voxel_length} and {self.voxel_length} are more than a factor of "
                          "4 apart; chain two calls")
        return float(r_fwd), float(r_back), min(8, int(r_fwd * np.float32(1.7320508)) + 2)

    def _merge_resampled_call(self, other, pose, supersample, flags, max_rounds, max_distance_weight, max_color_weight):
        """one vk_volume_merge_resampled(self <- other through `pose`, a T.Transform): the eight counts from one blocking read"""
        self._no_requests_pending("merge_resampled")
        other._no_requests_pending("merge_resampled")
        box = self._resample_ratios(other)[2]
        workspace, counts = self._workspace("merge_resampled", (other.main, other.excess, self.main, self.excess, box),
                                            lib().vk_volume_merge_resampled_workspace_bytes, 8, flags)
        params = T.MergeResampleParams(T.MergeParams(int(flags), int(max_rounds), float(max_distance_weight), float(max_color_weight)),
                                       pose, int(supersample), 0)
        self._table_changes()
        check(lib().vk_volume_merge_resampled(_ref(self.desc()), _ref(other.desc()), _ref(params), _ptr(counts), _ptr(workspace),
                                              stream()), "vk_volume_merge_resampled")
        return _ints(counts)

    def merge_resampled(self, other, pose=None, supersample=None, max_distance_weight=16, max_color_weight=16, skip_unobserved=False,
                        max_rounds=8):
        """vk_volume_merge_resampled (not upstream): merge(other, pose=...) for a volume `other` of another voxel length (up to
        a factor of 4 either way), another truncation length, or both. Every voxel of the blocks of this volume that
        `other`'s blocks reach takes the mean of `supersample`^3 trilinear samples of `other` spread over the voxel — a
        box filter, so a coarser copy does not alias; None: as many per axis as voxels of `other` lie along one of
        this volume's, min(4, max(1, ceil(ratio))) — and a stored distance is carried from `other`'s truncation length
        into this volume's: values beyond this volume's band saturate at 1 or, behind the surface, are left out.
        `pose` (a 4x4 array or a Transform, T_self_other in metres; None: the identity). Everything else — the rounds, the
        call that continues, what is refused and when, the eight counts — is merge(other, pose=...)'s. A PackedVolume
        has no table to sample: TypeError."""
        if isinstance(other, PackedVolume):
            raise TypeError("merge_resampled: a PackedVolume has no table to sample; load it into a Volume first")
        flags = T.VK_MERGE_SKIP_UNOBSERVED if skip_unobserved else 0
        pose = _as_pose(pose, identity=True)
        if supersample is None:
            supersample = min(4, max(1, int(np.ceil(self._resample_ratios(other)[1] - 1e-6))))
        # (considered, candidates, fused, allocated, left out, rounds, skipped, sampled)
        return self._merge_rounds(lambda go_on: self._merge_resampled_call(other, pose, supersample, flags | go_on, max_rounds,
                                                                           max_distance_weight, max_color_weight),
                                  max_rounds, 4, 5, (2, 3, 5, 7))

    def resampled(self, voxel_length, truncation_length, main_block_count, excess_block_count, pose=None, supersample=None,
                  depth_range=(0.1, 5.0), max_rounds=8):
        """This map at another resolution: a fresh Volume of the given voxel length, truncation length and table sizes on
        this volume's device, and merge_resampled(self) into it with both caps 32767, which into empty blocks keeps
        the sampled weights (as Volume.load is built). `pose`: T_new_self. Raises when the blocks do not fit the sizes."""
        volume = Volume(main_block_count, excess_block_count, voxel_length=voxel_length, truncation_length=truncation_length,
                        depth_range=depth_range, device=self.device)
        counts = volume.merge_resampled(self, pose=pose, supersample=supersample, max_distance_weight=32767,
                                        max_color_weight=32767, max_rounds=max_rounds)
        if counts[4]:
            raise VkError(f"Volume.resampled: {counts[4]} of {counts[1]} blocks did not fit ({main_block_count} main, "
                          f"{excess_block_count} excess entries)")
        return volume

    def _merge_packed_call(self, pack, flags, max_rounds, max_distance_weight, max_color_weight):
        """one vk_volume_merge_packed(self <- pack): the six counts from one blocking read"""
        self._no_requests_pending("merge")
        workspace, counts = self._workspace("merge_packed", (pack.count,), lib().vk_volume_merge_packed_workspace_bytes, 6, flags)
        params = T.MergeParams(int(flags), int(max_rounds), float(max_distance_weight), float(max_color_weight))
        self._table_changes()
        check(lib().vk_volume_merge_packed(_ref(self.desc()), _ref(pack.desc()), pack.count, pack.voxel_length, pack.truncation_length,
                                           _ref(params), _ptr(counts), _ptr(workspace), stream()), "vk_volume_merge_packed")
        return _ints(counts)

    def _pack_call(self, rule, origins, voxels, capacity):
        """one vk_volume_pack: (source blocks, selected, written, skipped as unobserved) from one blocking read"""
        workspace, counts = self._workspace("pack", (self.main, self.excess), lib().vk_volume_pack_workspace_bytes, 4)
        pack = T.BlockPack()
        pack.capacity = int(capacity)
        pack.origins = origins.data_ptr() if origins is not None else None
        pack.voxels = voxels.data_ptr() if voxels is not None else None
        check(lib().vk_volume_pack(_ref(self.desc()), _ref(rule) if rule is not None else None, _ref(pack), _ptr(counts),
                                   _ptr(workspace), stream()), "vk_volume_pack")
        return _ints(counts)

    def pack(self, box=None, skip_unobserved=False):
        """vk_volume_pack (not upstream): this volume's blocks as a PackedVolume — the origin and the 10 240 bytes of
        every block, in ascending order of the blocks' table entries, at the cost of the blocks that exist and not of
        the pool. `box` = ((lo x, y, z), (hi x, y, z)) in block coordinates, inclusive: only the blocks inside;
        `skip_unobserved`: without the blocks no voxel was ever integrated into. A call that counts, one blocking read
        of the count, an allocation of exactly that size, the call that packs. The volume is only read: allowed while
        a frame is announced. What to do with the pack: save(path), to(another device), other_volume.merge(pack)."""
        import torch
        rule = None
        if box is not None or skip_unobserved:
            rule = T.PackRule()
            if skip_unobserved:
                rule.flags |= T.VK_PACK_SKIP_UNOBSERVED
            if box is not None:
                rule.flags |= T.VK_PACK_BOX
                rule.lo[:] = [int(c) for c in box[0]]
                rule.hi[:] = [int(c) for c in box[1]]
        selected = self._pack_call(rule, None, None, 0)[1]
        origins = torch.empty((selected, 4), dtype=torch.int16, device=self.device)
        voxels = _dev_bytes(selected * PackedVolume.BLOCK_BYTES, self.device)
        if selected:
            written = self._pack_call(rule, origins, voxels, selected)[2]
            if written != selected:
                raise VkError(f"pack: {selected} blocks counted, {written} written: the volume changed between the two calls")
        return PackedVolume(origins, voxels, self.voxel_length, self.truncation_length)

    @classmethod
    def load(cls, path, main_block_count, excess_block_count, depth_range=(0.1, 5.0), device="cuda", max_rounds=8):
        """A map file (PackedVolume.save, io.write_map) as a fresh volume of the given table sizes, which need not be
        those of the volume that was saved: a new Volume with the file's voxel and truncation length, and merge(pack)
        with both caps 32767, which into empty blocks is a copy. Raises when the blocks do not fit the sizes."""
        pack = PackedVolume.load(path, device=device)
        volume = cls(main_block_count, excess_block_count, voxel_length=pack.voxel_length,
                     truncation_length=pack.truncation_length, depth_range=depth_range, device=device)
        counts = volume.merge(pack, max_distance_weight=32767, max_color_weight=32767, max_rounds=max_rounds)
        if counts[3]:
            raise VkError(f"Volume.load: {counts[3]} of {len(pack)} blocks did not fit ({main_block_count} main, "
                          f"{excess_block_count} excess entries)")
        volume._workspaces.clear()          # the load's own workspace, sized by the file: the volume it hands out has made no call
        return volume

    def _merge_rounds(self, call, max_rounds, left_out, rounds, summed):
        """`call(0)`, then `call(VK_MERGE_CONTINUE)` while a call posted requests in every round, dropped none and still left
        blocks out. Of the later calls' counts those at `summed` add up and the one at `left_out` replaces; the rest are
        the first call's."""
        dropped = int(self.read_counters()[T.VK_CTR_DROPPED])
        counts = call(0)
        total = list(counts)
        while counts[rounds] == int(max_rounds) and counts[left_out] > 0 and int(self.read_counters()[T.VK_CTR_DROPPED]) == dropped:
            counts = call(T.VK_MERGE_CONTINUE)
            for i in summed:
                total[i] += counts[i]
            total[left_out] = counts[left_out]
        return tuple(total)

    def merge(self, other, pose=None, max_distance_weight=16, max_color_weight=16, skip_unobserved=False, max_rounds=8):
        """vk_volume_merge (not upstream): fuse the volume `other` — same voxel and truncation length, on this device,
        any bucket and pool size — into this one. The blocks this volume lacks are allocated (`max_rounds` rounds of
        requests and handle pass per call), then every voxel's running average goes on with the other voxel's value and
        weight, the weights capped as an integrator's are. `skip_unobserved`: blocks of `other` that no voxel was ever
        integrated into are left where they are. Each block of `other` is fused once: while a call posted requests in
        every round, dropped none and still left blocks out, the merge goes on with another call for those
        (VK_MERGE_CONTINUE). Between SetView calls only: raises while either volume has a frame announced. `other` is
        only read. The visible list is empty afterwards (the next set_view rebuilds it) and what was prepared ahead
        for this volume is void. Returns (source blocks considered, fused, allocated, left out — the pool or the excess
        list ran out —, rounds that posted a request, source blocks skipped as unobserved).
        `pose` (a 4x4 array or a Transform, T_self_other in metres): the two volumes do not share a frame or a lattice —
        vk_volume_merge_posed: every voxel of the blocks of this volume that `other`'s blocks reach takes a trilinear
        sample of `other`. Returns (source blocks considered, candidate blocks, candidates fused, blocks allocated,
        candidates left out, rounds that posted, source blocks skipped as unobserved, voxels that took a distance
        sample); a candidate no sample reaches stays allocated and empty (release_blocks(unobserved=True) frees those).
        `other` may be a PackedVolume (Volume.pack, PackedVolume.load) in a volume's place — vk_volume_merge_packed: the
        same options and the same six counts, and for a pack made without a rule the state merge(that volume) leaves.
        A pack has no table to sample through a pose: `pose` with a pack raises TypeError."""
        flags = T.VK_MERGE_SKIP_UNOBSERVED if skip_unobserved else 0
        if isinstance(other, PackedVolume):
            if pose is not None:
                raise TypeError("merge: a PackedVolume is merged block into block; pose= takes a Volume")
            self._no_requests_pending("merge")
            if (np.float32(other.voxel_length) != np.float32(self.voxel_length) or
                    np.float32(other.truncation_length) != np.float32(self.truncation_length)):
                raise VkError(f"merge: the pack's voxel / truncation length ({other.voxel_length}, {other.truncation_length}) "
                              f"is not the volume's ({self.voxel_length}, {self.truncation_length})")
            if len(other) == 0:
                return (0, 0, 0, 0, 0, 0)                  # no blocks: no call
            return self._merge_rounds(lambda go_on: self._merge_packed_call(other, flags | go_on, max_rounds, max_distance_weight,
                                                                            max_color_weight), max_rounds, 3, 4, (1, 2, 4))
        if pose is None:
            # (considered, fused, allocated, left out, rounds, skipped)
            return self._merge_rounds(lambda go_on: self._merge_call(other, flags | go_on, max_rounds, max_distance_weight,
                                                                     max_color_weight), max_rounds, 3, 4, (1, 2, 4))
        pose = _as_pose(pose)
        # (considered, candidates, fused, allocated, left out, rounds, skipped, sampled)
        return self._merge_rounds(lambda go_on: self._merge_posed_call(other, pose, flags | go_on, max_rounds, max_distance_weight,
                                                                       max_color_weight), max_rounds, 4, 5, (2, 3, 5, 7))

    _register_buffers = None         # device buffers of vk_volume_register, per source size
    _register_rays_buffers = None    # device buffers of vk_volume_register_rays, per ray count

    def _registration_buffers(self, held, operation, size, workspace_bytes, pose):
        """the device buffers of a registration, `held` or — when _workspace handed out a new workspace — new ones, with
        `pose` (a T.Transform) uploaded as the start"""
        import torch
        workspace, counts = self._workspace(operation, size, workspace_bytes, 4)
        if held is None or held["workspace"] is not workspace:
            held = {"workspace": workspace, "counts": counts, "pose": _dev_bytes(C.sizeof(T.Transform), self.device),
                    "system": torch.zeros(48, dtype=torch.float32, device=self.device),
                    "state": torch.zeros(2, dtype=torch.int32, device=self.device),
                    "update": torch.zeros(6, dtype=torch.float32, device=self.device)}
        check(lib().vk_transform_upload(_ptr(held["pose"]), _ref(pose), stream()), "vk_transform_upload")
        return held

    @staticmethod
    def _registration_read(b):
        """what a loop left in the buffers `b`: (pose, (steps, code), counts, system[48], update[6]), a blocking read each"""
        out = T.Transform.from_buffer_copy(b["pose"].cpu().numpy().tobytes())
        return out, _ints(b["state"]), _ints(b["counts"]), b["system"].cpu().numpy(), b["update"].cpu().numpy()

    def _register_setup(self, other, pose, iterations, band):
        """the device buffers of a registration against `other`, the start pose uploaded: (buffers, vk_register_params)"""
        b = self._register_buffers = self._registration_buffers(self._register_buffers, "register", (other.main, other.excess),
                                                                lib().vk_volume_register_workspace_bytes, pose)
        return b, T.RegisterParams(0, int(iterations), float(band), 0)

    def _register_terms_call(self, other, pose, band):
        """vk_volume_register_terms at `pose` (a T.Transform): (valid, residuals, jacobians [.., 6]) per pool slot and voxel of `other`"""
        import torch
        b, params = self._register_setup(other, pose, 1, band)
        voxels = (other.main + other.excess) * 512
        valid = torch.empty(voxels, dtype=torch.uint8, device=self.device)
        residuals = torch.empty(voxels, dtype=torch.float32, device=self.device)
        jacobians = torch.empty((voxels, 6), dtype=torch.float32, device=self.device)
        check(lib().vk_volume_register_terms(_ref(self.desc()), _ref(other.desc()), _ptr(b["pose"]), _ref(params), _ptr(residuals),
                                             _ptr(jacobians), _ptr(valid), _ptr(b["workspace"]), stream()), "vk_volume_register_terms")
        return valid.cpu().numpy(), residuals.cpu().numpy(), jacobians.cpu().numpy()

    def _register_system_call(self, other, pose, band):
        """vk_volume_register_system at `pose`: (system[48], the four counts) from one blocking read each"""
        b, params = self._register_setup(other, pose, 1, band)
        check(lib().vk_volume_register_system(_ref(self.desc()), _ref(other.desc()), _ptr(b["pose"]), _ref(params), _ptr(b["system"]),
                                              _ptr(b["counts"]), _ptr(b["workspace"]), stream()), "vk_volume_register_system")
        return b["system"].cpu().numpy(), _ints(b["counts"])

    def _register_call(self, other, pose, iterations, band):
        """one vk_volume_register from `pose` (a T.Transform): (pose, (steps, code), counts, system[48], update[6])"""
        b, params = self._register_setup(other, pose, iterations, band)
        b["state"].zero_()
        check(lib().vk_volume_register(_ref(self.desc()), _ref(other.desc()), _ptr(b["pose"]), _ref(params), _ptr(b["system"]),
                                       _ptr(b["state"]), _ptr(b["counts"]), _ptr(b["update"]), _ptr(b["workspace"]), stream()),
              "vk_volume_register")
        return self._registration_read(b)

    def register(self, other, pose=None, iterations=20, max_abs_distance=0.75):
        """vk_volume_register (not upstream): refine the rigid pose T_self_other between this volume and `other` — same
        voxel and truncation length, on this device, any bucket and pool size — by Gauss-Newton on the two TSDFs: every
        voxel of `other` whose distance is within `max_abs_distance` truncation lengths of the surface is carried into
        this volume and compared with the trilinear sample there. `pose` (a 4x4 array or a Transform, what merge(pose=)
        accepts; None: the identity) is the guess to start from: it has to bring the two surfaces within roughly a
        truncation length of each other where they overlap — this call refines, it does not search. Both volumes are
        only read. At most `iterations` steps (1 .. 64), all enqueued at once; one blocking read at the end. Returns a
        Registration: `pose` (the result; merge(other, pose=result.pose) fuses through it), `steps`, `converged`,
        `overlap` (False: a step found no voxel to compare and the pose is the one it had then), `residuals` and `rms`
        (in truncation lengths) of the last evaluated step."""
        return _registration(*self._register_call(other, _as_pose(pose, identity=True), iterations, max_abs_distance)[:4])

    def _sample_call(self, points, pose=None, flags=0, samples=True, gradients=True, count=None, out=None):
        """one vk_volume_sample at `points` (a float32 device tensor of 3 * count floats or more): the raw output buffers
        (uint8 [n, 20] or None, float32 [n, 4] or None), allocated here or `out`'s. `pose`: a T.Transform (uploaded), a device
        buffer that holds a vk_transform, or None."""
        import torch
        count = points.numel() // 3 if count is None else int(count)
        pose = self._pose_on_device(pose)
        if out is None:
            out = (torch.empty((count, 20), dtype=torch.uint8, device=self.device) if samples else None,
                   torch.empty((count, 4), dtype=torch.float32, device=self.device) if gradients else None)
        params = T.SampleParams(int(flags), 0)
        check(lib().vk_volume_sample(_ref(self.desc()), _ptr(points), count, _ptr(pose), _ref(params), _ptr(out[0]), _ptr(out[1]),
                                     stream()), "vk_volume_sample")
        return out

    def sample(self, points, pose=None, color=True, gradient=False, voxel_units=False):
        """vk_volume_sample (not upstream): the volume's field at `points`, a float32 [N, 3] device tensor — in metres, or in
        voxels with `voxel_units` — in the frame that `pose` (a Transform, a 4x4 array, or a device buffer holding a
        vk_transform, e.g. a tracker's; None: the volume's own frame) carries into the volume's. Every point takes the
        trilinear sample of the stored voxels, as merge(pose=) takes it at a voxel's centre; `gradient`: and the gradient of
        the distance. The volume is only read; one launch, nothing is read back. Returns a Samples: where a weight is 0
        there is no sample of that field and the distance reads 1.0, "far from any surface"."""
        points = _float_tensor(points, 3, "sample: points is a float32 [N, 3] device tensor")
        flags = (T.VK_SAMPLE_VOXEL_UNITS if voxel_units else 0) | (0 if color else T.VK_SAMPLE_DISTANCE_ONLY)
        samples, gradients = self._sample_call(points, _as_pose(pose, device=True), flags, True, bool(gradient), points.shape[0])
        return Samples(samples, gradients, bool(color), self.truncation_length)

    def grid_for_box(self, lo, hi, stride=1):
        """(origin, dims) of the smallest aligned grid of `stride`-voxel cells that covers the metric box [lo, hi]"""
        return grid_for_box(lo, hi, stride, self.voxel_length)

    def classify_cells(self, origin, dims, stride=1, occupied_below=0.0):
        """vk_volume_classify_cells (not upstream): the grid of dims = (nx, ny, nz) cells of `stride`^3 voxels from the voxel
        `origin` (lattice coordinates, multiples of the stride) as a uint8 [nz, ny, nx] device tensor of CELL_UNKNOWN,
        CELL_FREE and CELL_OCCUPIED: a cell is occupied where an observed voxel stores a distance <= `occupied_below`
        (truncation lengths), else free where a voxel is observed. Blocks exist only in the truncation band: open space
        in front of it reads CELL_UNKNOWN. The volume is only read; two launches, nothing is read back."""
        import torch
        grid = T.CellGrid.make(origin, dims, stride)
        classes = torch.empty(_grid_shape(dims), dtype=torch.uint8, device=self.device)
        check(lib().vk_volume_classify_cells(_ref(self.desc()), _ref(grid), float(occupied_below), _ptr(classes), stream()),
              "vk_volume_classify_cells")
        return classes

    def distance_field(self, origin, dims, stride=1, max_distance=None, max_cells=None, occupied_below=0.0, sites=CELL_OCCUPIED,
                       signed=False, squared=False):
        """vk_volume_distance_field (not upstream): how far every cell of a dense grid is from the nearest surface — the
        clearance a planner asks for, which the stored distance cannot give beyond one truncation length. The grid is
        classify_cells' (`origin`, `dims`, `stride`, `occupied_below`); a cell is a site where its class & `sites` != 0, and
        every cell takes the exact Euclidean distance to the nearest site cell, centre to centre, in metres, +inf where
        none lies within the cap: `max_cells` cells (1 .. 256), or `max_distance` metres, rounded up to whole cells and
        clamped to 256 (neither: 256). `signed`: a site cell takes minus its distance to the nearest cell that is no site.
        `squared`: also the squared distance in cells as int32. The volume is only read; one enqueue, nothing is read back.
        Returns a DistanceField."""
        import torch
        stride = int(stride)
        cell_length = float(np.float32(np.float32(stride) * np.float32(self.voxel_length)))
        if max_cells is None:
            max_cells = 256 if max_distance is None else min(256, max(1, int(np.ceil(float(max_distance) / cell_length))))
        grid = T.CellGrid.make(origin, dims, stride)
        shape = _grid_shape(dims)
        workspace, _ = self._workspace("distance_field", shape[::-1], _grid_workspace_bytes, 1)
        classes = torch.empty(shape, dtype=torch.uint8, device=self.device)
        distance = torch.empty(shape, dtype=torch.float32, device=self.device)
        d2 = torch.empty(shape, dtype=torch.int32, device=self.device) if squared else None
        params = T.DistanceFieldParams(T.VK_FIELD_SIGNED if signed else 0, int(sites), int(max_cells), float(occupied_below))
        check(lib().vk_volume_distance_field(_ref(self.desc()), _ref(grid), _ref(params), _ptr(classes), _ptr(d2), _ptr(distance),
                                             _ptr(workspace), stream()), "vk_volume_distance_field")
        return DistanceField(classes, distance, d2, origin, stride, cell_length)

    def _cast_call(self, rays, pose=None, flags=0, t_min=0.0, t_max=5.0, max_steps=500, samples=True, gradients=True, count=None,
                   out=None):
        """one vk_volume_cast_rays of `rays` (a float32 device tensor of 6 * count floats or more): the raw output buffers
        (float32 [n], int32 [n], uint8 [n, 20] or None, float32 [n, 4] or None), allocated here or `out`'s. `pose`: a
        T.Transform (uploaded), a device buffer that holds a vk_transform, or None."""
        import torch
        count = rays.numel() // 6 if count is None else int(count)
        pose = self._pose_on_device(pose)
        if out is None:
            out = (torch.empty(count, dtype=torch.float32, device=self.device), torch.empty(count, dtype=torch.int32, device=self.device),
                   torch.empty((count, 20), dtype=torch.uint8, device=self.device) if samples else None,
                   torch.empty((count, 4), dtype=torch.float32, device=self.device) if gradients else None)
        params = T.CastParams(int(flags), int(max_steps), float(t_min), float(t_max))
        check(lib().vk_volume_cast_rays(_ref(self.desc()), _ptr(rays), count, _ptr(pose), _ref(params), _ptr(out[0]), _ptr(out[1]),
                                        _ptr(out[2]), _ptr(out[3]), stream()), "vk_volume_cast_rays")
        return out

    def cast_rays(self, rays, pose=None, t_min=0.0, t_max=None, max_steps=500, color=True, gradient=False, voxel_units=False):
        """vk_volume_cast_rays (not upstream): what each ray of `rays`, a float32 [N, 6] device tensor of origins and
        directions (any length) — origins in metres, or in voxels with `voxel_units` — hits first in the volume, in the
        frame that `pose` (a Transform, a 4x4 array, or a device buffer holding a vk_transform; None: the volume's own
        frame) carries into the volume's. The raycast's march between `t_min` and `t_max` along the ray (in the origins'
        unit; `t_max` None: the far end of the volume's depth range), at most `max_steps` steps: a surface is reported
        where the ray crosses it from its observed free side. The volume is only read; one launch, nothing is read back.
        Returns a RayHits: status, t and the sample (`gradient`: and the gradient) at every hit."""
        rays = _float_tensor(rays, 6, "cast_rays: rays is a float32 [N, 6] device tensor")
        pose = _as_pose(pose, device=True)
        if t_max is None:
            t_max = float(np.float32(self.depth_range[1]) / np.float32(self.voxel_length)) if voxel_units else self.depth_range[1]
        flags = (T.VK_CAST_VOXEL_UNITS if voxel_units else 0) | (0 if color else T.VK_CAST_DISTANCE_ONLY)
        t, status, samples, gradients = self._cast_call(rays, pose, flags, t_min, t_max, max_steps, True, bool(gradient), rays.shape[0])
        return RayHits(t, status, samples, gradients, bool(color), self.truncation_length)

    def _integrate_rays_call(self, rays, ranges, pose=None, flags=0, max_rounds=8, r_min=0.1, r_max=5.0, max_distance_weight=16.0,
                             count=None):
        """one vk_volume_integrate_rays of `rays` and `ranges` (float32 device tensors of 6 * count and count floats or more):
        the eight counts from one blocking read. `pose`: a T.Transform (uploaded), a device buffer that holds a vk_transform,
        or None."""
        self._no_requests_pending("integrate_rays")
        count = ranges.numel() if count is None else int(count)
        pose = self._pose_on_device(pose)
        workspace, counts = self._workspace("integrate_rays", (self.main, self.excess), lib().vk_volume_integrate_rays_workspace_bytes, 8)
        params = T.IntegrateRaysParams(int(flags), int(max_rounds), float(r_min), float(r_max), float(max_distance_weight), 0)
        self._table_changes()
        check(lib().vk_volume_integrate_rays(_ref(self.desc()), _ptr(rays), _ptr(ranges), count, _ptr(pose), _ref(params),
                                             _ptr(counts), _ptr(workspace), stream()), "vk_volume_integrate_rays")
        return _ints(counts)

    def integrate_rays(self, rays, ranges, pose=None, r_min=None, r_max=None, max_distance_weight=16, one_observation=False,
                       voxel_units=False, max_rounds=8):
        """vk_volume_integrate_rays (not upstream): fuse range measurements along arbitrary rays — a LiDAR sweep, a fisheye
        depth camera, a point cloud seen from known origins, or what cast_rays returned for another volume. `rays` is a
        float32 [N, 6] device tensor of origins and directions (any length), `ranges` a float32 [N] device tensor of
        distances along the normalised directions — origins and ranges in metres, or in voxels with `voxel_units` — in the
        frame that `pose` (a Transform, a 4x4 array, or a device buffer holding a vk_transform; None: the volume's own frame)
        carries into the volume's. A ray whose range lies outside [`r_min`, `r_max`] (None: the volume's depth range), a NaN
        included, carries no measurement and is skipped: cast_rays' t == 0 feeds in unchanged. The blocks within one
        truncation length either side of a measurement are allocated (`max_rounds` rounds of requests and handle pass; 0:
        only blocks that exist are updated), then every voxel whose cell a ray crosses inside that band continues its running
        average with the mean of what the rays through it measured, weighted with their number (`one_observation`: with 1),
        the weight capped at `max_distance_weight`. Colours are left alone. The result does not depend on the order of the
        rays. Between SetView calls only: raises while a frame is announced. The visible list is empty afterwards (the next
        set_view rebuilds it) and what was prepared ahead for this volume is void. Returns (rays integrated, valid rays
        without a measurement, invalid rays, blocks allocated, rounds that posted a request, blocks updated, voxels updated,
        cell visits lost to a block that could not be allocated)."""
        rays, ranges, r_min, r_max, flags = _range_ray_arguments("integrate_rays", rays, ranges, self.depth_range, self.voxel_length, r_min,
                                                                 r_max, voxel_units, one_observation)
        pose = _as_pose(pose, device=True)
        if rays.shape[0] == 0:
            return (0,) * 8
        return self._integrate_rays_call(rays, ranges, pose, flags, max_rounds, r_min, r_max, max_distance_weight, rays.shape[0])

    def _carve_rays_call(self, rays, ranges, pose=None, flags=0, max_blocks=1024, r_min=0.1, r_max=5.0, t_from=0.0,
                         max_distance_weight=16.0, count=None):
        """one vk_volume_carve_rays of `rays` and `ranges` (float32 device tensors of 6 * count and count floats or more): the
        eight counts from one blocking read. `pose`: a T.Transform (uploaded), a device buffer that holds a vk_transform, or
        None. The table and the visible list are left alone, so nothing made ahead is void."""
        self._no_requests_pending("carve_rays")
        count = ranges.numel() if count is None else int(count)
        pose = self._pose_on_device(pose)
        workspace, counts = self._workspace("carve_rays", (self.main, self.excess), lib().vk_volume_carve_rays_workspace_bytes, 8)
        params = T.CarveRaysParams(int(flags), int(max_blocks), float(r_min), float(r_max), float(t_from), float(max_distance_weight))
        check(lib().vk_volume_carve_rays(_ref(self.desc()), _ptr(rays), _ptr(ranges), count, _ptr(pose), _ref(params),
                                         _ptr(counts), _ptr(workspace), stream()), "vk_volume_carve_rays")
        return _ints(counts)

    def carve_rays(self, rays, ranges, pose=None, t_from=0.0, r_min=None, r_max=None, max_distance_weight=16, one_observation=False,
                   voxel_units=False, max_blocks=1024):
        """vk_volume_carve_rays (not upstream): carve the free space in front of range measurements — what is no longer
        there. `rays`, `ranges`, `pose`, `r_min`, `r_max` and `voxel_units` are integrate_rays'. Every voxel of an existing
        block whose cell a measured ray crosses between `t_from` (along the ray, in the origins' unit) and the start of the
        band that integrate_rays fuses, one truncation length in front of the measurement, takes an observation of the
        distance 1, "free": weighted with the number of rays through it (`one_observation`: with 1), the weight capped at
        `max_distance_weight`. A ray crosses at most `max_blocks` blocks; what it does not reach is not carved. Nothing is
        allocated: absent blocks are passed over, and the table, the free list, the visible list and the counters keep their
        bytes. Colours are left alone. The result does not depend on the order of the rays. Between SetView calls only:
        raises while a frame is announced. Returns (rays that carved, measured rays with nothing to carve, valid rays
        without a measurement, invalid rays, rays cut short by `max_blocks`, blocks updated, voxels updated, carves)."""
        rays, ranges, r_min, r_max, flags = _range_ray_arguments("carve_rays", rays, ranges, self.depth_range, self.voxel_length, r_min,
                                                                 r_max, voxel_units, one_observation)
        pose = _as_pose(pose, device=True)
        if rays.shape[0] == 0:
            return (0,) * 8
        return self._carve_rays_call(rays, ranges, pose, flags, max_blocks, r_min, r_max, t_from, max_distance_weight, rays.shape[0])

    def _color_rays_call(self, rays, ranges, colors, pose=None, flags=0, r_min=0.1, r_max=5.0, band=0.04, max_color_weight=16.0,
                         count=None):
        """one vk_volume_color_rays of `rays`, `ranges` and `colors` (float32 device tensors of 6 * count, count and 3 * count
        floats or more): the eight counts from one blocking read. `pose`: a T.Transform (uploaded), a device buffer that
        holds a vk_transform, or None. The table and the visible list are left alone, so nothing made ahead is void."""
        self._no_requests_pending("color_rays")
        count = ranges.numel() if count is None else int(count)
        pose = self._pose_on_device(pose)
        workspace, counts = self._workspace("color_rays", (self.main, self.excess), lib().vk_volume_color_rays_workspace_bytes, 8)
        params = T.ColorRaysParams(int(flags), float(r_min), float(r_max), float(band), float(max_color_weight), 0)
        check(lib().vk_volume_color_rays(_ref(self.desc()), _ptr(rays), _ptr(ranges), _ptr(colors), count, _ptr(pose), _ref(params),
                                         _ptr(counts), _ptr(workspace), stream()), "vk_volume_color_rays")
        return _ints(counts)

    def color_rays(self, rays, ranges, colors, pose=None, band=None, r_min=None, r_max=None, max_color_weight=16,
                   one_observation=False, voxel_units=False):
        """vk_volume_color_rays (not upstream): fuse a colour per range ray — a LiDAR return coloured by a camera, or the
        colour cast_rays returned for another volume. `rays`, `ranges`, `pose`, `r_min`, `r_max` and `voxel_units` are
        integrate_rays'; `colors` is a float32 [N, 3] device tensor of r, g, b in [0, 1]: a measured ray with a channel
        outside that, a NaN included, has no colour and is skipped. Every voxel of an existing block whose cell a coloured
        ray crosses within `band` of its measurement (in the origins' unit; None: the truncation length), and whose stored
        distance is near the surface (|distance| < 1), continues its colour's running average with the mean colour of the
        rays through it, weighted with their number (`one_observation`: with 1), the weight capped at `max_color_weight`.
        Nothing is allocated — colouring where no block exists is a lost visit, so call integrate_rays first — and the
        distances, their weights, the table, the free list, the visible list and the counters keep their bytes. The result
        does not depend on the order of the rays. At most 1 << 21 rays a call. Between SetView calls only: raises while a
        frame is announced. Returns (rays coloured, measured rays without a colour, valid rays without a measurement,
        invalid rays, blocks updated, voxels updated, voxels visited but not near a surface, visits lost to an absent
        block)."""
        rays, ranges, r_min, r_max, flags = _range_ray_arguments("color_rays", rays, ranges, self.depth_range, self.voxel_length, r_min,
                                                                 r_max, voxel_units, one_observation)
        colors = _float_tensor(colors, 3, "color_rays: colors is a float32 [N, 3] device tensor, one colour per ray", rays.shape[0])
        pose = _as_pose(pose, device=True)
        if band is None:
            band = float(np.float32(self.truncation_length) / (np.float32(self.voxel_length) if voxel_units else np.float32(1)))
        if rays.shape[0] == 0:
            return (0,) * 8
        return self._color_rays_call(rays, ranges, colors, pose, flags, r_min, r_max, band, max_color_weight, rays.shape[0])

    def _register_rays_setup(self, count, pose, iterations, band, flags, r_min, r_max):
        """the device buffers of a registration of `count` rays, the start pose uploaded: (buffers, vk_register_rays_params)"""
        b = self._register_rays_buffers = self._registration_buffers(self._register_rays_buffers, "register_rays", (int(count),),
                                                                     lib().vk_volume_register_rays_workspace_bytes, pose)
        return b, T.RegisterRaysParams(int(flags), int(iterations), float(r_min), float(r_max), float(band), 0)

    def _register_rays_terms_call(self, rays, ranges, pose, band, flags=0, r_min=0.1, r_max=5.0, count=None, out=None):
        """vk_volume_register_rays_terms at `pose` (a T.Transform) of `rays` and `ranges` (float32 device tensors of 6 * count and
        count floats or more): the device buffers (valid uint8 [n], residuals [n], jacobians [n, 6]), allocated here or `out`'s"""
        import torch
        count = ranges.numel() if count is None else int(count)
        b, params = self._register_rays_setup(count, pose, 1, band, flags, r_min, r_max)
        if out is None:
            out = (torch.empty(count, dtype=torch.uint8, device=self.device), torch.empty(count, dtype=torch.float32, device=self.device),
                   torch.empty((count, 6), dtype=torch.float32, device=self.device))
        check(lib().vk_volume_register_rays_terms(_ref(self.desc()), _ptr(rays), _ptr(ranges), count, _ptr(b["pose"]), _ref(params),
                                                  _ptr(out[1]), _ptr(out[2]), _ptr(out[0]), _ptr(b["workspace"]), stream()),
              "vk_volume_register_rays_terms")
        return out

    def _register_rays_system_call(self, rays, ranges, pose, band, flags=0, r_min=0.1, r_max=5.0, count=None):
        """vk_volume_register_rays_system at `pose`: (system[48], the four counts) from one blocking read each"""
        count = ranges.numel() if count is None else int(count)
        b, params = self._register_rays_setup(count, pose, 1, band, flags, r_min, r_max)
        check(lib().vk_volume_register_rays_system(_ref(self.desc()), _ptr(rays), _ptr(ranges), count, _ptr(b["pose"]), _ref(params),
                                                   _ptr(b["system"]), _ptr(b["counts"]), _ptr(b["workspace"]), stream()),
              "vk_volume_register_rays_system")
        return b["system"].cpu().numpy(), _ints(b["counts"])

    def _register_rays_enqueue(self, rays, ranges, count, b, params):
        """one vk_volume_register_rays from the pose in the buffers `b` (_register_rays_setup's): enqueued, nothing is read"""
        b["state"].zero_()
        check(lib().vk_volume_register_rays(_ref(self.desc()), _ptr(rays), _ptr(ranges), count, _ptr(b["pose"]), _ref(params),
                                            _ptr(b["system"]), _ptr(b["state"]), _ptr(b["counts"]), _ptr(b["update"]),
                                            _ptr(b["workspace"]), stream()), "vk_volume_register_rays")

    def _register_rays_call(self, rays, ranges, pose, iterations, band, flags=0, r_min=0.1, r_max=5.0, count=None):
        """one vk_volume_register_rays from `pose` (a T.Transform): (pose, (steps, code), counts, system[48], update[6]); the
        result stays in the buffers' "pose" on the device"""
        count = ranges.numel() if count is None else int(count)
        b, params = self._register_rays_setup(count, pose, iterations, band, flags, r_min, r_max)
        self._register_rays_enqueue(rays, ranges, count, b, params)
        return self._registration_read(b)

    def register_rays(self, rays, ranges, pose=None, iterations=20, max_abs_distance=0.75, r_min=None, r_max=None, voxel_units=False):
        """vk_volume_register_rays (not upstream): where the sensor is — refine the pose T_volume_rays of a sweep of range
        rays (a LiDAR revolution, a fisheye depth image, a point cloud with known origins) against this volume, by
        Gauss-Newton on "the endpoint of a return lies on the mapped surface". `rays`, `ranges`, `r_min`, `r_max` and
        `voxel_units` are integrate_rays'. `pose` (a 4x4 array or a Transform; None: the identity) is the guess to start from:
        it has to bring the endpoints within roughly a truncation length of the surface — this call refines, it does not
        search. A return whose endpoint samples a distance of `max_abs_distance` truncation lengths or more (a moved object,
        a spurious return), or lies where the map holds nothing, takes no part: that band is the only outlier rule. A sweep
        that sees a single plane does not fix the pose: the step is then zero and the call reports convergence where it
        started. The volume is only read, so the call is allowed while a frame is announced. At most `iterations` steps
        (1 .. 64), all enqueued at once; one blocking read at the end. Returns a Registration: `pose`, and `device_pose`,
        the same on the device for integrate_rays(pose=...); `steps`, `converged`, `overlap` (False: a step found no return
        to compare and the pose is the one it had then), `residuals` and `rms` (in truncation lengths) of the last evaluated
        step."""
        rays, ranges, r_min, r_max, flags = _range_ray_arguments("register_rays", rays, ranges, self.depth_range, self.voxel_length,
                                                                 r_min, r_max, voxel_units)
        start = _as_pose(pose, identity=True)
        if rays.shape[0] == 0:
            return Registration(start, 0, False, False, 0, 0.0, self._pose_on_device(start).clone())
        result = self._register_rays_call(rays, ranges, start, iterations, max_abs_distance, flags, r_min, r_max, rays.shape[0])
        return _registration(*result[:4], self._register_rays_buffers["pose"].clone())

    def _poses_on_device(self, poses, what):
        """(device buffer of vk_transforms, how many): `poses` a sequence of T.Transform (or 4x4 arrays), uploaded, or a device
        tensor that holds whole vk_transforms, passed through"""
        import torch
        if hasattr(poses, "data_ptr"):
            size = poses.numel() * poses.element_size()
            if size == 0 or size % C.sizeof(T.Transform) or not poses.is_contiguous():
                raise VkError(f"{what}: poses is a contiguous device tensor of whole vk_transforms (128 bytes each)")
            return poses, size // C.sizeof(T.Transform)
        host = b"".join(bytes(_as_pose(pose)) for pose in poses)
        if not host:
            raise VkError(f"{what}: no pose to score")
        return torch.from_numpy(np.frombuffer(host, dtype=np.uint8).copy()).to(self.device), len(host) // C.sizeof(T.Transform)

    def _score_poses_call(self, rays, ranges, poses, pose_count, band, flags=0, r_min=0.1, r_max=5.0, count=None, scores=None,
                          workspace=None):
        """vk_volume_score_poses of `rays` and `ranges` (float32 device tensors of 6 * count and count floats or more) at the
        `pose_count` vk_transforms of the device buffer `poses`: the device buffer of scores, allocated here or `scores`"""
        count = ranges.numel() if count is None else int(count)
        if workspace is None:
            workspace, _ = self._workspace("score_poses", (count, int(pose_count)), lib().vk_volume_score_poses_workspace_bytes, 1)
        if scores is None:
            scores = _dev_bytes(int(pose_count) * C.sizeof(T.PoseScore), self.device)
        params = T.ScorePosesParams(int(flags), 1, float(r_min), float(r_max), float(band), 0)
        check(lib().vk_volume_score_poses(_ref(self.desc()), _ptr(rays), _ptr(ranges), count, _ptr(poses), int(pose_count), _ref(params),
                                          _ptr(scores), _ptr(workspace), stream()), "vk_volume_score_poses")
        return scores

    def _score_poses_arguments(self, what, rays, ranges, poses, r_min, r_max, voxel_units):
        rays, ranges, r_min, r_max, flags = _range_ray_arguments(what, rays, ranges, self.depth_range, self.voxel_length, r_min, r_max,
                                                                 voxel_units)
        poses, pose_count = self._poses_on_device(poses, what)
        return rays, ranges, poses, pose_count, r_min, r_max, flags

    def score_poses(self, rays, ranges, poses, max_abs_distance=0.75, r_min=None, r_max=None, voxel_units=False):
        """vk_volume_score_poses (not upstream): how well each of many candidate poses T_volume_rays explains a sweep of range
        rays — the search register_rays does not make. `rays`, `ranges`, `r_min`, `r_max` and `voxel_units` are
        integrate_rays'; `poses` is a sequence of Transforms (or 4x4 arrays), or a device tensor of vk_transforms; producing
        the candidates is the caller's. At every pose, every ray is put to register_rays' residual test (a measured return
        whose endpoint samples a distance below `max_abs_distance` truncation lengths where the map holds all eight
        voxels): the score is register_rays' four counts at that pose and the sums of |D| and D^2 over the residuals as
        integers in units of 2^-20, so it does not depend on the order of the rays or on timing. At most 65 536 poses,
        1 << 22 rays and 1 << 28 pairs a call. The volume is only read, so the call is allowed while a frame is announced;
        nothing is read back. Returns a PoseScores: host(), mean_abs, rms, best(min_residuals)."""
        rays, ranges, poses, pose_count, r_min, r_max, flags = self._score_poses_arguments("score_poses", rays, ranges, poses, r_min,
                                                                                          r_max, voxel_units)
        import torch
        if rays.shape[0] == 0:          # no rays are no call: every pose scores nothing
            return PoseScores(torch.zeros(pose_count * C.sizeof(T.PoseScore), dtype=torch.uint8, device=self.device), poses, pose_count,
                              self.device)
        scores = self._score_poses_call(rays, ranges, poses, pose_count, max_abs_distance, flags, r_min, r_max, rays.shape[0])
        return PoseScores(scores, poses, pose_count, self.device)

    def localize_rays(self, rays, ranges, poses, min_residuals=None, iterations=20, max_abs_distance=0.75, r_min=None, r_max=None,
                      voxel_units=False):
        """where the sensor is, from far away: score_poses at the candidates `poses`, the best of them chosen on the device,
        and register_rays from it — three calls enqueued before anything is read. Returns register_rays' Registration with
        `best_index`, the candidate the refinement started from. Raises VkError when no candidate reaches `min_residuals`
        residuals (None: half the rays whose range is a measurement, counted with one read before the enqueue), or when there
        is no ray. `result.scores` is the PoseScores of the candidates."""
        rays, ranges, poses, pose_count, r_min, r_max, flags = self._score_poses_arguments("localize_rays", rays, ranges, poses, r_min,
                                                                                          r_max, voxel_units)
        import torch
        count = rays.shape[0]
        if count == 0:
            raise VkError("localize_rays: no rays")
        if min_residuals is None:       # half the measured rays: the measurement test does not depend on the pose
            min_residuals = max(1, int(((ranges >= r_min) & (ranges <= r_max)).sum()) // 2)
        b, params = self._register_rays_setup(count, T.Transform.identity(), iterations, max_abs_distance, flags, r_min, r_max)
        best = torch.zeros(1, dtype=torch.int32, device=self.device)
        scored = PoseScores(self._score_poses_call(rays, ranges, poses, pose_count, max_abs_distance, flags, r_min, r_max, count), poses,
                            pose_count, self.device)
        scored._best_call(min_residuals, best, b["pose"])
        self._register_rays_enqueue(rays, ranges, count, b, params)
        index = int(best.cpu()[0])
        if index < 0:
            raise VkError(f"localize_rays: none of the {pose_count} candidates has {min_residuals} residuals")
        result = _registration(*self._registration_read(b)[:4], b["pose"].clone())
        result.best_index, result.scores = index, scored
        return result

    def _no_requests_pending(self, stage):
        # the staged SetView stages on top of an announced frame's requests would mix two frames' state (vk.h)
        if self.requests_ahead is not None and self.requests_ahead.valid == 1:
            raise VkError(f"{stage}: a frame announced by Tracer.trace(next_frame=...) has its requests in the volume; "
                          "set_view(that frame) or cancel_requests_ahead() first")

    def reset_block_visibility(self):
        self._no_requests_pending("reset_block_visibility")
        check(lib().vk_volume_reset_block_visibility(_ref(self.desc()), stream()), "reset_block_visibility")

    def create_allocation_requests(self, frame):
        self._no_requests_pending("create_allocation_requests")
        check(lib().vk_volume_create_allocation_requests(
            _ref(self.desc()), _ptr(frame.depth), frame.width, frame.height,
            _ref(frame.depth_projection), _ref(frame.depth_to_world), stream()), "create_allocation_requests")

    def handle_allocation_requests(self):
        self._no_requests_pending("handle_allocation_requests")
        check(lib().vk_volume_handle_allocation_requests(_ref(self.desc()), stream()), "handle_allocation_requests")

    def update_block_visibility(self, frame):
        self._view_changed()
        tdw = frame.depth_to_world.inverse()
        check(lib().vk_volume_update_block_visibility(
            _ref(self.desc()), frame.width, frame.height, _ref(frame.depth_projection), _ref(tdw), stream()),
            "update_block_visibility")

    # -- host views (blocking)
    def read_counters(self):
        out = (C.c_int32 * T.VK_CTR_PUBLIC)()
        check(lib().vk_volume_read_counters_sync(_ref(self.desc()), out, stream()), "read_counters")
        return np.array(out[:], dtype=np.int32)

    @property
    def visible_count(self):
        return int(self.read_counters()[T.VK_CTR_VISIBLE])

    def visible(self):
        return self.visible_blocks[:self.visible_count].cpu().numpy()

    def host_voxels(self):
        return to_numpy(self.voxels, T.voxel_dtype)

    def host_entries(self):
        return to_numpy(self.hash_entries, T.hash_entry_dtype)

    def host_visibility(self):
        return self.block_visibility.cpu().numpy()

    def host_allocation_types(self):
        return self.allocation_types.cpu().numpy()

    def host_allocation_blocks(self):
        return to_numpy(self.allocation_blocks, T.block_dtype)

    def upload(self, host):
        """Copy an oracle HostVolume (same sizes) into this volume's buffers — lets a
        test start the device path from an exactly known state."""
        import torch
        assert host.main == self.main and host.excess == self.excess
        self._view_changed()
        for name in ("voxels", "hash_entries", "allocation_types", "allocation_blocks", "block_visibility"):
            src = torch.from_numpy(np.frombuffer(getattr(host, name).tobytes(), dtype=np.uint8).copy())
            getattr(self, name).copy_(src.to(self.device))
        self.free_voxel_blocks.copy_(torch.from_numpy(host.free_voxel_blocks).to(self.device))
        self.visible_blocks.copy_(torch.from_numpy(host.visible_blocks).to(self.device))
        self.counters.copy_(torch.from_numpy(host.counters).to(self.device))
        self.voxel_length, self.truncation_length = host.voxel_length, host.truncation_length
        self.depth_range = host.depth_range


class Integrator:
    """vulcan::Integrator (integrator.h:12-45): depth range (0.1,5), max weights 16."""

    def __init__(self, volume):
        self.volume = volume
        self.params = T.Integrator.default()

    def _call(self, fn, frame, *extra):
        check(getattr(lib(), fn)(_ref(self.volume.desc()), _ref(self.params), *extra,
                                 _ref(frame.desc()), stream()), fn)

    def _fused(self, frame, mode, light=None, mask=None, records=None):
        """depth (+ colour) in one pass; when a Tracer is attached to the volume the
        same launch also prepares the raycast bounds of this frame's view."""
        vb = self.volume.view_bounds
        check(lib().vk_integrate_ahead(_ref(self.volume.desc()), _ref(self.params), _ref(frame.desc()), mode,
                                       _ref(light) if light is not None else None, _ptr(mask), _ptr(records),
                                       _ref(vb) if vb is not None else None, stream()), "vk_integrate_ahead")


class DepthIntegrator(Integrator):
    def integrate(self, frame):                      # depth_integrator.cu:89-115
        self._fused(frame, 0)


class ColorIntegrator(Integrator):
    def integrate(self, frame):                      # color_integrator.cu:144-148, one pass
        self._fused(frame, 1)

    def integrate_depth(self, frame):                # color_integrator.cu:150-176
        self._call("vk_integrate_depth", frame)

    def integrate_color(self, frame):                # color_integrator.cu:178-204
        self._call("vk_integrate_color", frame)


class LightIntegrator(Integrator):
    def __init__(self, volume):
        super().__init__(volume)
        self.light = T.Light.make(1.0, (0, 0, 0))    # light.h:14-18
        self.depth_threshold = 0.2                   # light_integrator.cu:256
        self.frame_mask = None
        self.pixel_records = None

    def compute_frame_mask(self, frame):             # light_integrator.cu:277-293
        import torch
        if self.frame_mask is None or tuple(self.frame_mask.shape) != (frame.height, frame.width):
            self.frame_mask = torch.empty((frame.height, frame.width), dtype=torch.float32, device=frame.device)
        check(lib().vk_light_compute_frame_mask(_ref(frame.desc()), self.depth_threshold,
                                                _ptr(self.frame_mask), stream()), "vk_light_compute_frame_mask")
        return self.frame_mask

    def prepare(self, frame):
        """ComputeFrameMask + the per-pixel half of IntegrateColor (vk_light_prepare): the mask
        and one {Tcd * normal, mask} record per pixel."""
        import torch
        shape = (frame.height, frame.width)
        if self.frame_mask is None or tuple(self.frame_mask.shape) != shape:
            self.frame_mask = torch.empty(shape, dtype=torch.float32, device=frame.device)
        if self.pixel_records is None or tuple(self.pixel_records.shape[:2]) != shape:
            self.pixel_records = torch.empty(shape + (4,), dtype=torch.float32, device=frame.device)
        prep = getattr(self, "_prep", None)
        if prep is None or self.volume.light_prep is not prep or prep.mask != self.frame_mask.data_ptr() \
                or prep.records != self.pixel_records.data_ptr():
            # (re)attach: the volume's next set_view prepares these buffers in its request pass
            prep = T.LightPrep()
            prep.mask, prep.records = self.frame_mask.data_ptr(), self.pixel_records.data_ptr()
            prep.capacity = frame.width * frame.height
            self._prep = prep
            self.volume.attach_light_preparation(prep)
        prep.depth_threshold = self.depth_threshold
        if lib().vk_light_prepared(_ref(prep), _ref(frame.desc()), self.depth_threshold):
            prep.valid = 0                           # used once: a second integrate of the frame prepares again
            return
        check(lib().vk_light_prepare(_ref(frame.desc()), self.depth_threshold, _ptr(self.frame_mask),
                                     _ptr(self.pixel_records), stream()), "vk_light_prepare")

    def integrate(self, frame):                      # light_integrator.cu:270-275
        self.prepare(frame)
        self._fused(frame, 2, self.light, self.frame_mask, self.pixel_records)

    def integrate_depth(self, frame):
        self._call("vk_integrate_depth", frame)

    def integrate_color(self, frame):                # light_integrator.cu:323-354
        self._call("vk_integrate_light_color", frame, _ref(self.light), _ptr(self.frame_mask))


class Tracer:
    """vulcan::Tracer (tracer.h:24-77): 80x60 bounds grid, 262144 patch capacity."""

    BOUNDS_W, BOUNDS_H, PATCH_CAPACITY = 80, 60, 262144   # tracer.cpp:56-57,134

    def __init__(self, volume):
        import torch
        self.volume = volume
        self.depth_range = (0.1, 5.0)
        dev = volume.device
        n = int(lib().vk_trace_bounds_floats(self.BOUNDS_W, self.BOUNDS_H))
        self.bounds_scratch = torch.empty(n, dtype=torch.float32, device=dev)
        self.bounds = self.bounds_scratch[:self.BOUNDS_W * self.BOUNDS_H * 2].view(self.BOUNDS_H, self.BOUNDS_W, 2)
        self.patches = _dev_bytes(self.PATCH_CAPACITY * 16, dev)
        self.patch_count = torch.zeros(1, dtype=torch.int32, device=dev)
        # let the volume's integrators prepare this tracer's bounds ahead of time
        vb = T.ViewBounds()
        vb.scratch = self.bounds_scratch.data_ptr()
        vb.bounds_width, vb.bounds_height = self.BOUNDS_W, self.BOUNDS_H
        vb.min_depth, vb.max_depth = self.depth_range
        # the pinned word a normals workgroup sets when its bounded wait expires (vk.h vk_view_bounds.late_host)
        self._late = C.c_void_p()
        check(lib().vk_malloc_host(C.byref(self._late), 4), "vk_malloc_host")
        C.memset(self._late, 0, 4)
        vb.late_host = self._late.value
        self.view_bounds = vb
        volume.attach_view_bounds(vb)

    def __del__(self):
        late = getattr(self, "_late", None)
        if late is not None and late.value and _LIB is not None:
            self.view_bounds.late_host = None
            _LIB.vk_free_host(late)
            self._late = None

    def settle_normals(self):
        """vk_trace_normals_settle: synchronises, and raises VkError (VK_ERR_TIMEOUT) when a normals workgroup of the last
        trace(next_frame=...) gave up its wait — the normals have then been recomputed by a launch of their own."""
        check(lib().vk_trace_normals_settle(_ref(self.view_bounds), stream()), "vk_trace_normals_settle")

    def trace(self, frame, next_frame=None, next_needs_normals=False, normals=True):
        """Tracer::Trace (tracer.cpp:41-47): writes frame.depth / color / normals. `normals=False` (not upstream): the last
        stage is left out — for the tracking loop, whose next PyramidTracker.track(.., keyframe_normals_due=True) computes the
        key frame's normal image in its pyramid launch (one launch less per frame). `next_frame` (not upstream): the frame the
        volume's next set_view will be called with — its request pass (and, with `next_needs_normals` and a LightIntegrator's
        preparation attached, its normal image) is made behind the raycast's workgroups, in the same launch
        (vk_trace_ahead_requests)."""
        import torch
        if frame.color is None:
            frame.color = torch.empty((frame.height, frame.width, 3), dtype=torch.float32, device=frame.device)
        if frame.normals is None:
            frame.normals = torch.empty((frame.height, frame.width, 3), dtype=torch.float32, device=frame.device)
        vb = self.view_bounds
        if (vb.min_depth, vb.max_depth) != tuple(np.float32(d) for d in self.depth_range):
            vb.min_depth, vb.max_depth = self.depth_range
            vb.valid = 0
        if next_frame is None:
            check(lib().vk_trace_ahead(_ref(self.volume.desc()), _ref(frame.desc()), _ref(vb), _ptr(frame.depth),
                                       _ptr(frame.color), _ptr(frame.normals) if normals else None, stream()), "vk_trace_ahead")
            frame.touch()
            return
        v = self.volume
        if v.requests_ahead is None:
            v.requests_ahead = T.RequestsAhead()
        prep = v.light_prep
        if next_needs_normals:
            if prep is None:
                next_frame.compute_normals()
            else:
                if next_frame.normals is None:
                    next_frame.normals = torch.empty((next_frame.height, next_frame.width, 3), dtype=torch.float32, device=next_frame.device)
                next_frame.touch()
                prep.normals_out = next_frame.normals.data_ptr()
        check(lib().vk_trace_ahead_requests(_ref(v.desc()), _ref(frame.desc()), _ref(vb), _ptr(frame.depth), _ptr(frame.color),
                                            _ptr(frame.normals), _ref(next_frame.desc()), _ref(prep) if prep is not None else None,
                                            _ref(v.requests_ahead), stream()), "vk_trace_ahead_requests")
        if next_needs_normals and prep is None and v.requests_ahead.valid == 1:
            v.requests_ahead.normals_made = 1              # (the library knows of the riding normals only)
        if prep is not None and prep.normals_out and v.requests_ahead.valid != 1:
            prep.normals_out = None                        # the pass could not be made ahead: the normals as a launch of their own
            next_frame.compute_normals()
        frame.touch()

    # the tracer.cuh free functions, for the stage-by-stage tests
    def compute_patches(self, frame, block_count=None):
        v = self.volume
        self.patch_count.zero_()
        tcw = frame.depth_to_world.inverse()
        n = v.max if block_count is None else block_count
        dev_count = C.c_void_p(v.counters.data_ptr()) if block_count is None else None
        check(lib().vk_trace_compute_patches(
            _ptr(v.visible_blocks), _ptr(v.hash_entries), _ref(tcw), _ref(frame.depth_projection),
            np.float32(8) * np.float32(v.voxel_length), self.depth_range[0], self.depth_range[1], n, dev_count,
            frame.width, frame.height, self.BOUNDS_W, self.BOUNDS_H, _ptr(self.patches), self.PATCH_CAPACITY,
            _ptr(self.patch_count), stream()), "vk_trace_compute_patches")

    def compute_bounds(self):
        check(lib().vk_trace_reset_bounds(_ptr(self.bounds), self.BOUNDS_W * self.BOUNDS_H, stream()),
              "vk_trace_reset_bounds")
        check(lib().vk_trace_compute_bounds(_ptr(self.patches), _ptr(self.bounds), self.BOUNDS_W,
                                            self.PATCH_CAPACITY, _ptr(self.patch_count), stream()),
              "vk_trace_compute_bounds")

    def compute_block_bounds(self, frame):
        v = self.volume
        tcw = frame.depth_to_world.inverse()
        check(lib().vk_trace_compute_block_bounds(
            _ptr(v.visible_blocks), _ptr(v.hash_entries), _ref(tcw), _ref(frame.depth_projection),
            np.float32(8) * np.float32(v.voxel_length), self.depth_range[0], self.depth_range[1], v.max,
            C.c_void_p(v.counters.data_ptr()), frame.width, frame.height, self.BOUNDS_W, self.BOUNDS_H,
            _ptr(self.bounds), stream()), "vk_trace_compute_block_bounds")

    def compute_points(self, frame, depth_out, color_out):
        v = self.volume
        check(lib().vk_trace_compute_points(
            _ptr(v.hash_entries), _ptr(v.voxels), _ptr(self.bounds), v.main,
            np.float32(8) * np.float32(v.voxel_length), v.voxel_length, v.truncation_length,
            _ref(frame.depth_to_world), _ref(frame.depth_projection), _ptr(depth_out), _ptr(color_out),
            frame.width, frame.height, self.BOUNDS_W, self.BOUNDS_H, stream()), "vk_trace_compute_points")

    def host_patches(self):
        n = min(int(self.patch_count.cpu()[0]), self.PATCH_CAPACITY)
        return to_numpy(self.patches[:n * 16], T.patch_dtype)


class _PollMixin:
    """Early exit of the device-side Gauss-Newton loop (vk_track_poll): a pinned
    {iterations, converged} mirror the enqueuing call looks at every `poll_chunk` steps."""

    poll_chunk = int(os.environ.get("VK_TRACK_POLL_CHUNK", "4"))   # 0: enqueue every step, never block

    def _poll(self):
        if getattr(self, "_poll_desc", None) is None:
            host, pose = C.c_void_p(), C.c_void_p()
            check(lib().vk_malloc_host(C.byref(host), 16), "vk_malloc_host")
            check(lib().vk_malloc_host(C.byref(pose), C.sizeof(T.Transform)), "vk_malloc_host")
            C.memset(host, 0, 16)
            self._poll_host, self._pose_host = host, pose
            self._poll_desc = T.TrackPoll(host.value, 0, pose.value)
        self._poll_desc.chunk = int(self.poll_chunk)          # 0: enqueue every step, never look
        return _ref(self._poll_desc)

    def _wait_pose(self):
        """Tracker::EndSolve (tracker.cpp:78-82): the pose of the Track just issued, picked up from
        pinned memory (vk_track_wait) instead of a copy + stream synchronisation."""
        rc = lib().vk_track_wait(_ref(self._poll_desc), stream())
        if rc != 0 and int(self.state.cpu()[1]) == T.VK_TRACK_ABORTED:
            raise TrackAborted("the one-launch loop ended with VK_TRACK_ABORTED")
        check(rc, "vk_track_wait")
        return T.Transform.from_buffer_copy(C.string_at(self._pose_host, C.sizeof(T.Transform)))

    _staged = False                          # falling back from an aborted one-launch loop

    def _with_fallback(self, frame, run):
        """A one-launch loop that could not get its workgroups onto the device together ends with
        VK_TRACK_ABORTED and no pose: run the Track again from the start pose with a reduce hook
        that changes nothing, i.e. one launch per stage (vk_reduce_nothing, vk.h)."""
        start = frame.depth_to_world
        try:
            return run(frame)
        except TrackAborted:
            frame.depth_to_world = start
            self._staged = True
            try:
                return run(frame)
            finally:
                self._staged = False

    comm = None                              # vulcan_amd.comm.Communicator: the rig's all-reduce, from C

    def _c_hook(self):
        """(vk_icp_reduce_fn, user): the communicator's C hook, or the python reduce hook
        wrapped in a callback, or (None, None)."""
        fn = self._c_hook_fn()
        return fn, (self.comm.handle if self.comm is not None else None)

    def _c_hook_fn(self):
        if self.comm is not None:
            return self.comm.hook_fn
        if self.reduce_hook is None:
            if self._staged:
                return C.cast(lib().vk_reduce_nothing, C.c_void_p)
            return None
        system, py_hook = self.system, self.reduce_hook

        def _call(ptr, count, user, strm):
            py_hook(system)
            return 0
        self._hook_keepalive = _REDUCE_FN(_call)          # must outlive the C call
        return C.cast(self._hook_keepalive, C.c_void_p)

    def __del__(self):
        # a loop kernel that is still running writes both pinned blocks: drain the stream first
        host, pose = getattr(self, "_poll_host", None), getattr(self, "_pose_host", None)
        if (host is not None or pose is not None) and _LIB is not None:
            try:
                _LIB.vk_stream_synchronize(stream())
            except Exception:      # noqa: BLE001  (interpreter shutdown: torch may be gone; the process ends anyway)
                return
            for block in (host, pose):
                if block is not None:
                    _LIB.vk_free_host(block)
            self._poll_host = self._pose_host = None


class DepthTracker(_PollMixin):
    """vulcan::DepthTracker (depth_tracker.h, tracker.h): Gauss-Newton ICP against a
    keyframe; the pose, the 27-float system and the solve stay on the device."""

    def __init__(self, device="cuda"):
        import torch
        self.device = device
        self.translation_enabled = True      # tracker.cpp:11
        self.max_iterations = 20             # tracker.cpp:12
        self.keyframe = None
        # one 48-float buffer = 36 hessian + 6 gradient + pad, so a multi-GPU rig
        # needs ONE all-reduce per Gauss-Newton iteration
        self.system = torch.zeros(48, dtype=torch.float32, device=device)
        self.hessian = self.system[:36]
        self.gradient = self.system[36:42]
        self.pose = _dev_bytes(128, device)
        self.state = torch.zeros(2, dtype=torch.int32, device=device)
        self.update = torch.zeros(6, dtype=torch.float32, device=device)
        self.workspace = None
        self.reduce_hook = None              # e.g. an all-reduce over ranks
        # True: this tracker is one camera of a rigid rig whose systems the hook (reduce_hook or comm) adds over the
        # ranks, and the solve applies the rig's pose-independent increment (vk_icp_track_rig_hook, vk.h "THE RIG'S
        # INCREMENT"). False: ApplyUpdate as upstream has it, whatever the hook does — a hook alone makes no rig
        self.rig_increment = False

    @staticmethod
    def _view(frame):
        v = T.IcpView()
        v.depths, v.normals = frame.depth.data_ptr(), frame.normals.data_ptr()
        v.width, v.height = frame.width, frame.height
        v.projection = frame.depth_projection
        return v

    def _workspace(self, frame):
        import torch
        n = int(lib().vk_icp_workspace_floats(frame.width, frame.height))
        if self.workspace is None or self.workspace.numel() < n:
            # zeroed: memory that comes back from the allocator may hold anything, and the library — which clears a workspace
            # only when it is new to it, old, grown or overwritten by a staged loop (vk.h) — cannot see that
            self.workspace = torch.zeros(n, dtype=torch.float32, device=self.device)
        return self.workspace

    def compute_residuals(self, frame):      # depth_tracker.cu:272-300
        import torch
        out = torch.empty((frame.height, frame.width), dtype=torch.float32, device=self.device)
        check(lib().vk_icp_compute_residuals(_ref(self._view(self.keyframe)), _ref(self.keyframe.depth_to_world),
                                             _ref(self._view(frame)), _ref(frame.depth_to_world), _ptr(out),
                                             stream()), "vk_icp_compute_residuals")
        return out

    def compute_jacobian(self, frame):       # depth_tracker.cu:302-336
        import torch
        out = torch.empty((frame.height, frame.width, 6), dtype=torch.float32, device=self.device)
        check(lib().vk_icp_compute_jacobian(_ref(self._view(self.keyframe)), _ref(self.keyframe.depth_to_world),
                                            _ref(self._view(frame)), _ref(frame.depth_to_world),
                                            int(self.translation_enabled), _ptr(out), stream()),
              "vk_icp_compute_jacobian")
        return out

    def compute_system(self, frame, pose_on_device=False):   # depth_tracker.cu:338-378
        ws = self._workspace(frame)
        check(lib().vk_icp_compute_system(
            _ref(self._view(self.keyframe)), _ref(self.keyframe.depth_to_world), _ref(self._view(frame)),
            _ref(frame.depth_to_world), _ptr(self.pose) if pose_on_device else None,
            int(self.translation_enabled), _ptr(ws), _ptr(self.hessian), _ptr(self.gradient), stream()),
            "vk_icp_compute_system")

    def track(self, frame):
        return self._with_fallback(frame, self._track)

    def _track(self, frame):
        """Tracker::Track (tracker.cpp:53-63): <= max_iterations Gauss-Newton steps,
        all enqueued without a host sync; one 128-byte readback of the pose at the end."""
        import torch
        check(lib().vk_transform_upload(_ptr(self.pose), _ref(frame.depth_to_world), stream()), "vk_transform_upload")
        self.state.zero_()
        # one C call: the whole loop is one launch (with a reduce hook: 3 launches per step,
        # enqueuing stops once the loop has converged)
        hook, hook_user = self._c_hook()
        rig = bool(self.rig_increment)
        if rig and self.comm is None and self.reduce_hook is None:
            raise ValueError("rig_increment needs the hook that adds the rig's systems (reduce_hook or comm)")
        name = "vk_icp_track_rig_hook" if rig else "vk_icp_track"
        check(getattr(lib(), name)(_ref(self._view(self.keyframe)), _ref(self.keyframe.depth_to_world),
                                   _ref(self._view(frame)), _ptr(self.pose), self.max_iterations,
                                   int(self.translation_enabled), _ptr(self._workspace(frame)), _ptr(self.system),
                                   _ptr(self.state), _ptr(self.update), hook, hook_user, self._poll(), stream()),
              name)
        out = self._wait_pose()
        frame.depth_to_world = out
        return out


def track_rig(tracker, frame, exchange):
    """vk_icp_track_rig: DepthTracker::Track of one camera of a rigid rig, the ranks' normal systems
    added inside the one-launch loop through `exchange` (a T.RigExchange, vulcan_amd.comm). With more than
    one rank the library applies the rig's increment; a rig of one rank is vk_icp_track."""
    check(lib().vk_transform_upload(_ptr(tracker.pose), _ref(frame.depth_to_world), stream()), "vk_transform_upload")
    tracker.state.zero_()
    check(lib().vk_icp_track_rig(_ref(tracker._view(tracker.keyframe)), _ref(tracker.keyframe.depth_to_world),
                                 _ref(tracker._view(frame)), _ptr(tracker.pose), tracker.max_iterations,
                                 int(tracker.translation_enabled), _ptr(tracker._workspace(frame)), _ptr(tracker.system),
                                 _ptr(tracker.state), _ptr(tracker.update), _ref(exchange), tracker._poll(), stream()),
          "vk_icp_track_rig")
    out = tracker._wait_pose()
    frame.depth_to_world = out
    return out


class ColorTracker(_PollMixin):
    """vulcan::ColorTracker (color_tracker.h): photometric Gauss-Newton tracking of a
    frame against a keyframe — intensity residuals sampled bilinearly in the frame,
    one per keyframe pixel. Pose, system and solve stay on the device."""

    def __init__(self, device="cuda"):
        import torch
        self.device = device
        self.translation_enabled = True      # tracker.cpp:11
        self.max_iterations = 20             # tracker.cpp:12
        self._keyframe = None
        self._key_side = None
        self.system = torch.zeros(48, dtype=torch.float32, device=device)
        self.hessian = self.system[:36]
        self.gradient = self.system[36:42]
        self.pose = _dev_bytes(C.sizeof(T.ColorPose), device)
        self.state = torch.zeros(2, dtype=torch.int32, device=device)
        self.update = torch.zeros(6, dtype=torch.float32, device=device)
        self.workspace = None
        self.reduce_hook = None

    @property
    def keyframe(self):
        return self._keyframe

    @keyframe.setter
    def keyframe(self, frame):
        self._keyframe = frame
        self._key_side = None

    # -- ColorTracker::ComputeKeyframeIntensities / FrameIntensities / FrameGradients ------
    def _side(self, frame, with_gradients):
        import torch
        h, w = frame.height, frame.width
        inten = torch.empty((h, w), dtype=torch.float32, device=self.device)
        check(lib().vk_color_image_convert(h * w, _ptr(frame.color), _ptr(inten), stream()), "vk_color_image_convert")
        gx = gy = None
        if with_gradients:
            gx, gy = torch.empty_like(inten), torch.empty_like(inten)
            check(lib().vk_image_gradients(w, h, _ptr(inten), _ptr(gx), _ptr(gy), stream()), "vk_image_gradients")
        v = T.ColorView()
        v.depths, v.normals, v.intensities = frame.depth.data_ptr(), frame.normals.data_ptr(), inten.data_ptr()
        v.gradient_x = gx.data_ptr() if gx is not None else None
        v.gradient_y = gy.data_ptr() if gy is not None else None
        v.width, v.height = w, h
        v.projection = frame.color_projection
        return v, (inten, gx, gy)          # the tensors must outlive the view

    def _key(self):
        if self._key_side is None:
            self._key_side = self._side(self._keyframe, False)
        return self._key_side

    def tcm(self, frame):
        """color_tracker.cu:312-320"""
        key_Tcw = self._keyframe.depth_to_color * self._keyframe.depth_to_world.inverse()
        frame_Tcw = frame.depth_to_color * frame.depth_to_world.inverse()
        return frame_Tcw * key_Tcw.inverse()

    def _workspace(self):
        import torch
        n = int(lib().vk_icp_workspace_floats(self._keyframe.width, self._keyframe.height))
        if self.workspace is None or self.workspace.numel() < n:
            # zeroed: memory that comes back from the allocator may hold anything, and the library — which clears a workspace
            # only when it is new to it, old, grown or overwritten by a staged loop (vk.h) — cannot see that
            self.workspace = torch.zeros(n, dtype=torch.float32, device=self.device)
        return self.workspace

    def compute_residuals(self, frame):      # color_tracker.cu:296-344
        import torch
        kv, keep_k = self._key()
        fv, keep_f = self._side(frame, False)
        out = torch.empty((self._keyframe.height, self._keyframe.width), dtype=torch.float32, device=self.device)
        check(lib().vk_color_tracker_compute_residuals(_ref(kv), _ref(fv), _ref(self.tcm(frame)), _ptr(out), stream()),
              "vk_color_tracker_compute_residuals")
        return out

    def compute_jacobian(self, frame):       # color_tracker.cu:346-410
        import torch
        kv, keep_k = self._key()
        fv, keep_f = self._side(frame, True)
        out = torch.empty((self._keyframe.height, self._keyframe.width, 6), dtype=torch.float32, device=self.device)
        check(lib().vk_color_tracker_compute_jacobian(_ref(kv), _ref(fv), _ref(self.tcm(frame)),
                                                      int(self.translation_enabled), _ptr(out), stream()),
              "vk_color_tracker_compute_jacobian")
        return out

    def compute_system(self, frame):         # color_tracker.cu:412-470
        kv, keep_k = self._key()
        fv, keep_f = self._side(frame, True)
        check(lib().vk_color_tracker_compute_system(_ref(kv), _ref(fv), _ref(self.tcm(frame)), None,
                                                    int(self.translation_enabled), _ptr(self._workspace()),
                                                    _ptr(self.hessian), _ptr(self.gradient), stream()),
              "vk_color_tracker_compute_system")

    def track(self, frame):
        return self._with_fallback(frame, self._track)

    def _track(self, frame):
        """Tracker::Track (tracker.cpp:53-63) with ColorTracker::BeginSolve
        (color_tracker.cpp:19-25): intensities and gradients once, then
        max_iterations steps enqueued without a host sync."""
        import torch
        kv, keep_k = self._key()
        fv, keep_f = self._side(frame, True)
        pose = T.ColorPose()
        pose.depth_to_world = frame.depth_to_world
        host = np.frombuffer(bytes(pose), dtype=np.uint8).copy()
        self.pose.copy_(torch.from_numpy(host).to(self.device))
        self.state.zero_()
        key_Twc = (self._keyframe.depth_to_color * self._keyframe.depth_to_world.inverse()).inverse()
        hook, hook_user = self._c_hook()
        check(lib().vk_color_tracker_track(_ref(kv), _ref(fv), _ref(frame.depth_to_color), _ref(key_Twc),
                                           _ptr(self.pose), self.max_iterations, int(self.translation_enabled),
                                           _ptr(self._workspace()), _ptr(self.system), _ptr(self.state),
                                           _ptr(self.update), hook, hook_user, self._poll(), stream()),
              "vk_color_tracker_track")
        out = self._wait_pose()
        frame.depth_to_world = out
        return out


class LightTracker(ColorTracker):
    """vulcan::LightTracker (light_tracker.h): the colour tracker with a shading model —
    residual Ic - albedo * light.GetShading(Xcp, n) where the frame mask is set,
    point-to-plane elsewhere. The keyframe's colour image is read as albedo."""

    def __init__(self, device="cuda"):
        super().__init__(device)
        self.light = T.Light.make(1.0, (0, 0, 0))    # light.h:14-18
        self.depth_threshold = 0.2                   # light_tracker.cpp:13-14
        self.frame_mask = None

    def compute_frame_mask(self, frame):             # light_tracker.cu:548-564
        import torch
        self.frame_mask = torch.empty((frame.height, frame.width), dtype=torch.float32, device=self.device)
        check(lib().vk_light_compute_frame_mask(_ref(frame.desc()), self.depth_threshold, _ptr(self.frame_mask),
                                                stream()), "vk_light_compute_frame_mask")
        return self.frame_mask

    def _terms(self, frame, mask=None):
        t = T.LightTerms()
        m = mask if mask is not None else self.compute_frame_mask(frame)
        t.frame_mask = m.data_ptr()
        t.light = self.light
        t.frame_Tcd = frame.depth_to_color
        return t, m

    def compute_residuals(self, frame, mask=None):   # light_tracker.cu:566-608 (the mask is computed here)
        import torch
        kv, keep_k = self._key()
        fv, keep_f = self._side(frame, False)
        terms, keep_m = self._terms(frame, mask)
        out = torch.empty((self._keyframe.height, self._keyframe.width), dtype=torch.float32, device=self.device)
        check(lib().vk_light_tracker_compute_residuals(_ref(kv), _ref(fv), _ref(terms), _ref(self.tcm(frame)),
                                                       _ptr(out), stream()), "vk_light_tracker_compute_residuals")
        return out

    def compute_jacobian(self, frame, mask=None):    # light_tracker.cu:610-668
        import torch
        kv, keep_k = self._key()
        fv, keep_f = self._side(frame, True)
        terms, keep_m = self._terms(frame, mask)
        out = torch.empty((self._keyframe.height, self._keyframe.width, 6), dtype=torch.float32, device=self.device)
        check(lib().vk_light_tracker_compute_jacobian(_ref(kv), _ref(fv), _ref(terms), _ref(self.tcm(frame)),
                                                      int(self.translation_enabled), _ptr(out), stream()),
              "vk_light_tracker_compute_jacobian")
        return out

    def compute_system(self, frame, mask=None):      # light_tracker.cu:670-732
        kv, keep_k = self._key()
        fv, keep_f = self._side(frame, True)
        terms, keep_m = self._terms(frame, mask)
        check(lib().vk_light_tracker_compute_system(_ref(kv), _ref(fv), _ref(terms), _ref(self.tcm(frame)), None,
                                                    int(self.translation_enabled), _ptr(self._workspace()),
                                                    _ptr(self.hessian), _ptr(self.gradient), stream()),
              "vk_light_tracker_compute_system")

    def track(self, frame):
        return self._with_fallback(frame, self._track)

    def _track(self, frame):
        """Tracker::Track with LightTracker::BeginSolve (light_tracker.cpp:34-41)."""
        import torch
        kv, keep_k = self._key()
        fv, keep_f = self._side(frame, True)
        terms, keep_m = self._terms(frame)
        pose = T.ColorPose()
        pose.depth_to_world = frame.depth_to_world
        host = np.frombuffer(bytes(pose), dtype=np.uint8).copy()
        self.pose.copy_(torch.from_numpy(host).to(self.device))
        self.state.zero_()
        key_Twc = (self._keyframe.depth_to_color * self._keyframe.depth_to_world.inverse()).inverse()
        check(lib().vk_light_tracker_track(_ref(kv), _ref(fv), _ref(terms), _ref(key_Twc), _ptr(self.pose),
                                           self.max_iterations, int(self.translation_enabled), _ptr(self._workspace()),
                                           _ptr(self.system), _ptr(self.state), _ptr(self.update), *self._c_hook(),
                                           self._poll(), stream()), "vk_light_tracker_track")
        out = self._wait_pose()
        frame.depth_to_world = out
        return out


class PyramidTracker:
    """vulcan::PyramidTracker<DepthTracker> (pyramid_tracker.cpp:52-90): half
    resolution (15 iterations) then full resolution (20)."""

    def __init__(self, tracker=None, device="cuda"):
        self.tracker = tracker or DepthTracker(device)
        self.keyframe = None

    def track(self, frame, compute_normals=False, keyframe_normals_due=False, set_view_of=None, rounds=1):
        """`compute_normals` (not upstream): frame.compute_normals() is still due; with a DepthTracker it is done by the launch
        that builds the pyramid (vk_icp_pyramid_track_frame). `keyframe_normals_due`: the key frame came from
        Tracer.trace(.., normals=False); its normal image is computed by the same launch. `set_view_of` (round 6;
        PyramidTracker<DepthTracker>::ComputeNormalsTrackAndSetView): a Volume whose set_view(frame, rounds) follows this Track
        — with a DepthTracker it is enqueued BEHIND the Track at the pose the loop leaves on the device, before this call waits
        for that pose (Volume.set_view_at_device_pose); otherwise, and after a Track that aborted, it is called afterwards."""
        if set_view_of is not None:
            self._set_view_of, self._set_view_rounds, self._set_view_done = set_view_of, int(rounds), False
            try:
                pose = self.track(frame, compute_normals, keyframe_normals_due)
            finally:
                done, self._set_view_of = self._set_view_done, None
            if not done:
                set_view_of.set_view(frame, rounds=rounds)
            return pose
        t = self.tracker
        if keyframe_normals_due and not isinstance(t, DepthTracker):
            self.keyframe.compute_normals()
            keyframe_normals_due = False
        self._key_normals_due = bool(keyframe_normals_due)
        if isinstance(t, DepthTracker):
            if compute_normals:
                import torch
                if frame.normals is None:
                    frame.normals = torch.empty((frame.height, frame.width, 3), dtype=torch.float32, device=frame.device)
                frame.touch()
            self._normals_due = bool(compute_normals)
            try:
                return self._track_depth(frame)
            finally:
                self._normals_due = False
        if compute_normals:
            frame.compute_normals()
        half_frame = frame.downsample()
        half_key = self.keyframe.downsample()
        t.max_iterations, t.translation_enabled = 15, True
        t.keyframe = half_key
        t.track(half_frame)
        t.max_iterations = 20
        frame.depth_to_world = half_frame.depth_to_world
        t.keyframe = self.keyframe
        return t.track(frame)


    def _track_depth(self, frame):
        return self.tracker._with_fallback(frame, self._track_depth_once)

    def _track_depth_once(self, frame):
        """PyramidTracker<DepthTracker>::Track as ONE call (vk_icp_pyramid_track): both levels
        are enqueued from C, the pose stays on the device in between, one readback at the end."""
        import torch
        t, key = self.tracker, self.keyframe
        n = int(lib().vk_icp_pyramid_floats(key.width, key.height, frame.width, frame.height))
        if getattr(self, "_pyramid", None) is None or self._pyramid.numel() < n:
            self._pyramid = torch.empty(n, dtype=torch.float32, device=t.device)
        t.max_iterations, t.translation_enabled, t.keyframe = 20, True, key
        due = (1 if getattr(self, "_normals_due", False) else 0) | (2 if getattr(self, "_key_normals_due", False) else 0)
        self._normals_due = self._key_normals_due = False       # (a second attempt after an aborted loop finds them computed)
        check(lib().vk_icp_pyramid_track_frame(_ref(t._view(key)), _ref(key.depth_to_world), _ref(t._view(frame)),
                                               _ptr(t.pose), _ref(frame.depth_to_world), due, _ptr(self._pyramid),
                                               _ptr(t._workspace(frame)), _ptr(t.system), _ptr(t.state), _ptr(t.update),
                                               *t._c_hook(), t._poll(), stream()),
              "vk_icp_pyramid_track_frame")
        # (round 6) the caller's SetView at the pose this Track leaves on the device, enqueued before the host waits for it;
        # the first attempt only: after an aborted loop the staged Track follows and the caller's own SetView after it
        volume = getattr(self, "_set_view_of", None)
        early = False
        if volume is not None and not t._staged and t.reduce_hook is None and t.comm is None:
            early = volume.set_view_at_device_pose(frame, t.pose, self._set_view_rounds)
        out = t._wait_pose()
        if volume is not None:
            self._set_view_done = early
        frame.depth_to_world = out
        return out


class Mesh:
    """vulcan::DeviceMesh (mesh.h:16-21): points [n, 3] float32, faces [m, 3] int32 on the device; colors and normals
    [n, 3] float32 when the extractor was asked for them (vk_extract_mesh_attributes), else None."""

    def __init__(self, points, faces, colors=None, normals=None):
        self.points, self.faces, self.colors, self.normals = points, faces, colors, normals

    def host(self):
        return self.points.cpu().numpy(), self.faces.cpu().numpy()

    def host_attributes(self):
        """(colors, normals) as numpy arrays, None for what was not extracted"""
        return (None if self.colors is None else self.colors.cpu().numpy(),
                None if self.normals is None else self.normals.cpu().numpy())


class Extractor:
    """vulcan::Extractor (extractor.h:116-134): the whole volume in four launches, five with attributes."""

    def __init__(self, volume):
        import torch
        self.volume = volume
        self.all_allocated = False       # upstream walks the visible blocks (extractor.cu:455-457)
        self.interpolate = True
        n = int(lib().vk_extract_workspace_bytes(volume.main, volume.excess))
        self.workspace = torch.empty(n, dtype=torch.uint8, device=volume.device)
        self.counts = torch.zeros(4, dtype=torch.int32, device=volume.device)

    def extract(self, point_capacity=None, face_capacity=None, colors=False, normals=False):
        """Extractor::Extract(DeviceMesh&). Capacities default to upstream's ResizeMesh bound
        for the visible blocks (extractor.cu:700-716: 3 points per voxel, 5 faces per cube),
        capped; a second call with the reported totals follows when they did not suffice.
        `colors` / `normals`: one colour / unit normal per vertex (vk_extract_mesh_attributes)."""
        import torch
        v = self.volume
        blocks = v.max if self.all_allocated else max(v.visible_count, 1)
        pc = point_capacity if point_capacity is not None else min(blocks * 1536, 1 << 24)
        fc = face_capacity if face_capacity is not None else min(blocks * 5 * 512, 1 << 25)
        for _ in range(2):
            points = torch.empty((pc, 3), dtype=torch.float32, device=v.device)
            faces = torch.empty((fc, 3), dtype=torch.int32, device=v.device)
            if colors or normals:
                c = torch.empty((pc, 3), dtype=torch.float32, device=v.device) if colors else None
                n = torch.empty((pc, 3), dtype=torch.float32, device=v.device) if normals else None
                check(lib().vk_extract_mesh_attributes(_ref(v.desc()), int(self.all_allocated), int(self.interpolate),
                                                       _ptr(points), _ptr(c), _ptr(n), pc, _ptr(faces), fc, _ptr(self.counts),
                                                       _ptr(self.workspace), stream()), "vk_extract_mesh_attributes")
            else:
                c = n = None
                check(lib().vk_extract_mesh(_ref(v.desc()), int(self.all_allocated), int(self.interpolate), _ptr(points), pc,
                                            _ptr(faces), fc, _ptr(self.counts), _ptr(self.workspace), stream()), "vk_extract_mesh")
            np_, nf, self.skipped, self.blocks = (int(k) for k in self.counts.cpu())
            if np_ <= pc and nf <= fc:
                return Mesh(points[:np_], faces[:nf], None if c is None else c[:np_], None if n is None else n[:np_])
            pc, fc = max(np_, 1), max(nf, 1)
        raise VkError("vk_extract_mesh: capacities did not settle")


class Detector:
    """vulcan::Detector (detector.h:10-72): radius / interval filter, 1.5-sigma
    outlier removal, centroid. Everything stays on the device until `detect`
    reads the 48-byte state back."""

    def __init__(self, device="cuda"):
        import torch
        self.device = device
        self.params = T.Detector.default()
        self.state = torch.zeros(C.sizeof(T.DetectState) // 4, dtype=torch.int32, device=device)
        self.inliers = None
        self._workspace = None

    # -- reference accessors -------------------------------------------------------------
    @property
    def radius(self):
        return self.params.radius

    @radius.setter
    def radius(self, value):
        self.params.radius = float(value)

    @property
    def origin(self):
        return tuple(self.params.origin)

    @origin.setter
    def origin(self, value):
        self.params.origin[:] = [float(v) for v in value]

    def get_bounds(self, axis):
        return tuple(self.params.bounds[axis])

    def set_bounds(self, axis, bounds):
        self.params.bounds[axis][0], self.params.bounds[axis][1] = float(bounds[0]), float(bounds[1])

    @property
    def min_inlier_count(self):
        return self.params.min_inlier_count

    @min_inlier_count.setter
    def min_inlier_count(self, value):
        self.params.min_inlier_count = int(value)

    # -- device work ---------------------------------------------------------------------
    def _prepare(self, points):
        import torch
        assert points.dtype == torch.float32 and points.is_contiguous() and points.shape[-1] == 3
        count = points.numel() // 3
        need = lib().vk_detect_workspace_bytes(count)
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        if self.inliers is None or self.inliers.shape[0] < max(count, 1):
            self.inliers = torch.empty((max(count, 1), 3), dtype=torch.float32, device=self.device)
        return count

    def filter(self, points):
        """Detector::Filter; returns nothing, see read_state()/inlier_points()."""
        count = self._prepare(points)
        check(lib().vk_detect_filter(_ref(self.params), _ptr(points), count, _ptr(self.inliers), _ptr(self.state),
                                     _ptr(self._workspace), stream()), "vk_detect_filter")

    def enqueue(self, points):
        """Detector::Detect without the readback."""
        count = self._prepare(points)
        check(lib().vk_detect(_ref(self.params), _ptr(points), count, _ptr(self.inliers), _ptr(self.state),
                              _ptr(self._workspace), stream()), "vk_detect")

    def read_state(self):
        return T.DetectState.from_buffer_copy(self.state.cpu().numpy().tobytes())

    def inlier_points(self):
        return self.inliers[: self.read_state().inlier_count]

    def detect(self, points):
        """Detector::Detect: the box position as 3 floats (NaN when not detected)."""
        self.enqueue(points)
        return np.array(self.read_state().position, dtype=np.float32)
