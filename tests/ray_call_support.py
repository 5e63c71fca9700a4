"""One harness for the three operations that write a volume from range rays — integrate_rays, carve_rays, color_rays: the volume
a case starts from, the CPU statement of the case (computed once a process), the device call with the same keywords, and
the comparison of the two. A test module builds one RayCall from its operation's statement, ray sets, device call and
keywords function, and keeps its own tests, thresholds and cases."""
import cast_reference as CR
import integrate_rays_reference as IR
import merge_pose_reference as MP
import merge_reference as M
import release_reference as R
from gpu_support import assert_same_state, assert_untouched, device_copy, on_device, pose_on_device
from vulcan_amd import vk_types as T

_WANT = {}


def start(orc, sizes, target):
    """a host volume the call starts from: the scene volume of cast_reference at these table sizes, or a fresh one"""
    return R.clone(orc, CR.volume(orc, sizes)) if target == "scene" else M.fresh(orc, *sizes[0])


class RayCall:
    """`statement(hv, *arrays, pose=, r_min=, r_max=, flags=, **kw)`: the operation's CPU statement. `ray_sets(orc, units)`:
    the arrays of its ray sets, (rays, ranges) or (rays, ranges, colours). `call_name`: the api.Volume method that makes the
    device call, `cap_keyword` that method's name for the weight cap the cases call `cap`. `keywords(flags, kw)`: (r_min,
    r_max, the keywords of statement and call) for one case. `voxels_only`: the call may touch nothing but voxels, and
    `both` holds it to that."""

    def __init__(self, statement, ray_sets, call_name, cap_keyword, keywords, voxels_only):
        self._statement, self.ray_sets, self.call_name, self.cap_keyword = statement, ray_sets, call_name, cap_keyword
        self.keywords, self.voxels_only = keywords, voxels_only

    start = staticmethod(start)

    def statement(self, orc, sizes, target, flags, pose=None, **kw):
        """(host volume after the statement, its Result) on the ray sets in the form `flags`: once per case, never changed"""
        key = (self.call_name, sizes, target, flags, None if pose is None else bytes(pose), tuple(sorted(kw.items())))
        if key not in _WANT:
            hv = start(orc, sizes, target)
            r_min, r_max, kw = self.keywords(flags, kw)
            arrays = self.ray_sets(orc, bool(flags & IR.VOXEL_UNITS))
            _WANT[key] = (hv, self._statement(hv, *arrays, pose=pose, r_min=r_min, r_max=r_max, flags=flags, **kw))
        return _WANT[key]

    def call(self, dv, *arguments, **kw):
        """the device call: `arguments` are the arrays on the device, the pose and the flags"""
        r_min, r_max, kw = self.keywords(arguments[-1], kw)
        kw.setdefault(self.cap_keyword, kw.pop("cap", 16.0))
        return getattr(dv, self.call_name)(*arguments, r_min=r_min, r_max=r_max, **kw)

    def both(self, api, orc, sizes, target, flags, pose=None, device_pose="same", **kw):
        hv, want = self.statement(orc, sizes, target, flags, pose, **kw)
        before = start(orc, sizes, target)
        dv = device_copy(api, before)
        arrays = [on_device(array) for array in self.ray_sets(orc, bool(flags & IR.VOXEL_UNITS))]
        got = self.call(dv, *arrays, pose if device_pose == "same" else device_pose, flags, **kw)
        print("counts", got, want.counts)
        assert got == want.counts
        assert_same_state(dv, hv)                   # what the statement leaves: voxels, entries, visibility, free list, counters
        if self.voxels_only:
            assert_untouched(dv, before)
        return dv, hv, want

    def a_pose_on_the_device(self, api, orc, sizes, flags):
        """the case through generic() from the host, from a device buffer that already holds the pose, and the identity pose
        against no pose: (the Result through generic(), the host volume through the identity, the one with no pose)"""
        _, _, want = self.both(api, orc, sizes, "scene", flags, MP.generic())
        # a device buffer that already holds the pose: the same call
        self.both(api, orc, sizes, "scene", flags, MP.generic(), device_pose=pose_on_device(MP.generic()))
        # the identity pose against no pose: the statement of each, and the same volume
        _, with_identity, _ = self.both(api, orc, sizes, "scene", flags, T.Transform.identity())
        without, _ = self.statement(orc, sizes, "scene", flags)
        assert with_identity.voxels.tobytes() == without.voxels.tobytes()
        return want, with_identity, without
