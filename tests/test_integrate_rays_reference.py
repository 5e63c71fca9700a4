"""The CPU statement of vk_volume_integrate_rays (tests/integrate_rays_reference.py) against what any definition of the call
must give: one ray along an axis leaves the analytic distances, the shared ray sets reach every branch of the definition, the
order of the rays changes no byte, what cast_rays sees in a volume can be fused into another and seen there again, and the
pixel rays of a depth frame build the surface the reference's integrator builds from that frame. No GPU: the device is held to
the same statement in tests/test_gpu_integrate_rays.py."""
import ctypes as C

import numpy as np
import pytest

from abi_support import fake_volume
import cast_reference as CR
import integrate_rays_reference as IR
import merge_reference as M
import register_reference as RR
import release_reference as R
from vulcan_amd import vk_types as T

f32 = np.float32
# The round trip, one ray per pixel (k = 1 of {1, 2, 3, 4} is enough: every ray that hits in the source hits again, 19 200 of
# 19 200): |t' - t| median 2.08e-4 m, 99th percentile 1.26e-3 m, 7.57e-3 m at worst. Against the reference's integrator on the
# same depth frame, the oracle's raycast of both volumes: the rays' volume has a depth on every pixel the oracle's has (19 171
# of 19 171); |dz| median 2.31e-4 m, 99th percentile 8.24e-3 m, 2.24e-2 m at worst — the reference measures along z, the rays
# along the ray, and the worst pixels lie on the rim of the image, as in test_cast_reference.py. Asserted: twice each measured
# maximum, the margin for nothing more than another host libm or numpy build.
ROUND_TRIP_BOUND, ORACLE_DEPTH_BOUND = 2 * 7.57e-3, 2 * 2.24e-2
SUPERSAMPLING = 1


def state(hv):
    return (hv.voxels.tobytes(), hv.hash_entries.tobytes(), hv.free_voxel_blocks.tobytes(), hv.block_visibility.tobytes(),
            hv.counters[:T.VK_CTR_PUBLIC].tobytes(), hv.allocation_types.tobytes())


def test_one_ray_along_an_axis():
    """origin (0.5, 2.5, 3.5) voxels, along +x, r = 20.25, tr = 5: through voxel centres, so raw = r - (c + 0.5 - o) exactly"""
    import oracle.oracle as orc
    hv = orc.HostVolume(61, 16, voxel_length=2.0 ** -7, truncation_length=5 * 2.0 ** -7)
    tr = f32(hv.truncation_length) / f32(hv.voxel_length)
    assert tr == 5
    o, r = f32(0.5), f32(20.25)
    rays = np.array([[o, 2.5, 3.5, 3.0, 0, 0]], dtype=f32)
    out = IR.integrate(hv, rays, np.array([r], dtype=f32), r_min=1.0, r_max=100.0, flags=IR.VOXEL_UNITS)
    # from floor(o + ta) = 15 to the last cell whose far face is crossed by tb = 25.25: the crossing into cell 25 is at 24.5
    cells = list(range(15, 26))
    table = RR.block_table(hv)
    touched = np.flatnonzero(hv.voxels["distance_weight"] != 0)
    want = {}
    for c in cells:
        raw = r - (f32(c) + f32(0.5) - o)
        if raw > -tr:
            want[table[(c >> 3, 0, 0)] * 512 + 3 * 64 + 2 * 8 + (c & 7)] = f32(np.rint(min(f32(1), raw / tr) * f32(2 ** 20)) * 2.0 ** -20)
    assert len(want) == 11 and sorted(want) == sorted(touched.tolist())
    for index, distance in want.items():
        assert hv.voxels["distance"][index] == distance and hv.voxels["distance_weight"][index] == 1
    assert hv.voxels["distance"][touched].min() < 0 < hv.voxels["distance"][touched].max() == 1
    assert out.counts[:4] == (1, 0, 0, 3) and out.counts[4] >= 1 and out.counts[5:] == (3, 11, 0)
    assert not hv.voxels["color"].any() and not hv.voxels["color_weight"].any()


@pytest.fixture(scope="module")
def everything(orc):
    """the statement on all sets into the scene volume, as the GPU tests integrate them"""
    hv = R.clone(orc, CR.volume(orc))
    rays, ranges = IR.all_rays(orc, False)
    return hv, IR.integrate(hv, rays, ranges)


def test_the_ray_sets_reach_every_branch(orc, everything):
    hv, out = everything
    sets = IR.ray_sets(orc, False)
    print({name: len(s[1]) for name, s in sets.items()})
    print("counts", out.counts, out.branches)
    b = out.branches
    assert len(sets["a"][1]) == 19200 and len(sets["b"][1]) == 4096 and len(sets["e"][1]) == 12 and len(sets["f"][1]) == 25
    for name, least in (("ties", 1000), ("zero_component", 1000), ("negative_step", 1000), ("ta_clamped", 100), ("refused", 1000),
                        ("u_clamped", 1000), ("outside_int16", 100), ("lost", 100), ("shared_voxels", 1000)):
        assert b[name] >= least, name
    assert b["most_on_a_voxel"] >= 4096                                  # the 4 096 copies, and whoever else crosses the voxel
    integrated, unmeasured, invalid = out.counts[:3]
    # every ray of (e) is valid and has no measurement; (a) adds the pixels cast_rays did not hit, if any
    spans = IR.spans(orc)
    kinds = IR.carried(hv, *IR.all_rays(orc, False), None, IR.R_MIN, IR.R_MAX, False)[3]
    assert (kinds[spans["e"]] == IR.NO_MEASUREMENT).all() and (kinds[spans["f"]] == IR.INVALID).all()
    assert invalid == 25 and unmeasured >= 12 and integrated + unmeasured + invalid == len(kinds)
    # N >= 2 from different rays: a voxel of the pixel rays alone
    alone = IR.integrate(M.fresh(orc, 4093, 2048), *sets["a"])
    assert alone.branches["shared_voxels"] > 1000
    # a visit lost to an absent block: no round at all, and a pool small enough to run dry
    fixed = R.clone(orc, CR.volume(orc))
    none = IR.integrate(fixed, *IR.all_rays(orc, False), max_rounds=0)
    assert none.counts[3] == 0 and none.counts[4] == 0 and none.counts[7] > 1000
    assert fixed.hash_entries.tobytes() == CR.volume(orc).hash_entries.tobytes()
    small = M.fresh(orc, 61, 16)
    dry = IR.integrate(small, *IR.all_rays(orc, False))
    print("exhausted", dry.counts, "dropped", int(small.counters[T.VK_CTR_DROPPED]))
    assert small.counters[T.VK_CTR_DROPPED] > 0 and dry.counts[3] <= 77 and dry.counts[7] > 100000
    # the voxel-units form of the sets fuses the same map wherever / L gave the same numbers: the counts of rays agree
    units = IR.integrate(R.clone(orc, CR.volume(orc)), *IR.all_rays(orc, True), r_min=IR.bounds(True)[0], r_max=IR.bounds(True)[1],
                         flags=IR.VOXEL_UNITS)
    assert units.counts[2] == 25 and abs(units.counts[0] - integrated) <= 2


def test_a_ray_visits_a_cell_once_and_its_cells_are_face_neighbours(orc):
    hv = CR.volume(orc)
    rays, ranges = IR.all_rays(orc, False)
    o, n, r, kind = IR.carried(hv, rays, ranges, None, IR.R_MIN, IR.R_MAX, False)
    fused = kind == IR.INTEGRATED
    who, cells = IR.walk(o[fused], n[fused], r[fused], f32(5))
    order = np.argsort(who, kind="stable")
    who, cells = who[order], cells[order]
    same = who[1:] == who[:-1]
    assert (np.abs(cells[1:] - cells[:-1]).sum(-1)[same] == 1).all()
    keys = np.concatenate([who[:, None], cells], -1)
    assert len(np.unique(keys, axis=0)) == len(keys)


def test_the_order_of_the_rays_changes_no_byte(orc, everything):
    hv, out = everything
    other = R.clone(orc, CR.volume(orc))
    again = IR.integrate(other, *IR.permuted(*IR.all_rays(orc, False)))
    assert again.counts == out.counts
    assert state(other) == state(hv)
    assert np.array_equal(again.S, out.S) and np.array_equal(again.N, out.N)


def test_the_colours_and_the_unvisited_voxels_keep_their_bytes(orc, everything):
    hv, out = everything
    before = CR.volume(orc)
    total = before.max * 512
    assert (before.voxels["color_weight"] != 0).sum() > 1000
    kept = np.ones(total, dtype=bool)
    kept[np.flatnonzero(out.N > 0)] = False
    was, now = R.block_voxels(before), R.block_voxels(hv)
    for origin, data in was.items():
        old, new = np.frombuffer(data, dtype=T.voxel_dtype), np.frombuffer(now[origin], dtype=T.voxel_dtype)
        slot = R.find(hv, origin)
        assert new["color"].tobytes() == old["color"].tobytes() and np.array_equal(new["color_weight"], old["color_weight"])
        assert new[kept[slot * 512:(slot + 1) * 512]].tobytes() == old[kept[slot * 512:(slot + 1) * 512]].tobytes()
    # an allocated block that took no update is Voxel::Empty()
    empty = np.zeros(512, dtype=T.voxel_dtype)
    empty["distance"] = 1
    untouched = [o for o in now if o not in was and not out.N[R.find(hv, o) * 512:(R.find(hv, o) + 1) * 512].any()]
    print("allocated blocks without an update", len(untouched))
    assert all(now[o] == empty.tobytes() for o in untouched)


def test_round_trip_with_cast_rays(orc):
    """cast the fusing camera's pixel rays in the scene volume, integrate the hits into a fresh volume, cast again there"""
    rays, t = IR.pixel_hits(orc, SUPERSAMPLING)
    hv = M.fresh(orc, 4093, 2048)
    out = IR.integrate(hv, rays, t, r_min=0.1)
    again = CR.cast(hv, rays)
    hit, hit_again = t > 0, again.status == CR.HIT
    share = (hit & hit_again).sum() / hit.sum()
    d = np.abs(again.t[hit & hit_again].astype(np.float64) - t[hit & hit_again])
    print("k", SUPERSAMPLING, "hits", int(hit.sum()), "hit again %.4f" % share, "counts", out.counts)
    print("|t' - t| median %.3g m, 99th percentile %.3g m, max %.3g m" % (np.median(d), np.percentile(d, 99), d.max()))
    assert hit.sum() > 10000 and out.counts[0] == hit.sum() and out.counts[7] == 0
    assert share >= 0.95
    assert d.max() <= ROUND_TRIP_BOUND


def test_against_the_reference_integrator(orc):
    """one depth frame: the oracle's SetView and depth integration into one fresh volume, the frame's pixel rays with
    range = depth |K^-1 (u, v, 1)| as one observation into another; the oracle's raycast of both at the fusing view"""
    frame = CR.fusing_frame(orc)
    ho = M.fresh(orc, 4093, 2048)
    for _ in range(8):
        ho.set_view(frame, orc.POLICY_MAXKEY)
    orc.integrate_depth(ho, frame)
    rays, xs, ys = IR.pixel_rays(SUPERSAMPLING)
    d = rays[:, 3:]
    ranges = RR.bumps(RR.W, RR.H)[ys, xs] * np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    hr = M.fresh(orc, 4093, 2048)
    out = IR.integrate(hr, rays, ranges, r_min=0.1, flags=IR.ONE_OBSERVATION)
    assert int(hr.voxels["distance_weight"].max()) == 1 and out.counts[7] == 0
    for _ in range(3):
        hr.set_view(frame, orc.POLICY_MAXKEY)                           # the raycast reads the visible list
    theirs, ours = orc.trace(ho, frame)[0], orc.trace(hr, frame)[0]
    seen, also = theirs > 0, ours > 0
    share = (seen & also).sum() / seen.sum()
    e = np.abs(theirs[seen & also].astype(np.float64) - ours[seen & also])
    print("oracle depth > 0 at", int(seen.sum()), "the rays' volume on %.4f of them" % share)
    print("|dz| median %.3g m, 99th percentile %.3g m, max %.3g m" % (np.median(e), np.percentile(e, 99), e.max()))
    assert seen.sum() > 10000 and share >= 0.95
    assert e.max() <= ORACLE_DEPTH_BOUND


def test_the_library_validates_before_touching_a_device():
    """every refusal vk.h lists, with addresses that are no memory: nothing may be enqueued (no GPU is needed, or touched)"""
    from vulcan_amd import api
    lib = api.lib()
    one, odd = C.c_void_p(4096), C.c_void_p(4096 + 8)

    def params(flags=0, max_rounds=8, r_min=0.1, r_max=5.0, cap=16.0):
        return T.IntegrateRaysParams(flags, max_rounds, r_min, r_max, cap, 0)

    def call(v=fake_volume(), rays=one, ranges=one, count=8, pose=None, p=params(), counts=one, workspace=one):
        return lib.vk_volume_integrate_rays(C.byref(v) if v else None, rays, ranges, count, pose, C.byref(p) if p else None, counts,
                                            workspace, None)

    assert call(v=None) == -1 and call(p=None) == -1 and call(counts=None) == -1 and call(workspace=None) == -1
    for field, value in (("hash_entries", None), ("voxel_length", 0.0), ("main_block_count", 0), ("voxels", (1 << 20) + 8),
                         ("truncation_length", 0.008 * 64.5)):
        broken = fake_volume()
        setattr(broken, field, value)
        assert call(v=broken) == -1, field
    for flags in (4, 8, -1, 1 << 16):
        assert call(p=params(flags=flags)) == -1
    for max_rounds in (-1, 65, 1 << 30):
        assert call(p=params(max_rounds=max_rounds)) == -1
    for cap in (0.5, 0.0, 32768.0, float("nan"), float("inf")):
        assert call(p=params(cap=cap)) == -1
    for r_min, r_max in ((-0.001, 5.0), (1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (0.0, float("nan")), (float("nan"), 5.0),
                         (float("-inf"), 5.0), (0.0, 0.0)):
        assert call(p=params(r_min=r_min, r_max=r_max)) == -1
    assert call(count=-1) == -1 and call(count=(1 << 22) + 1) == -1
    assert call(rays=None) == -1 and call(ranges=None) == -1 and call(workspace=odd) == -1
    # count == 0 launches nothing, whatever else is allowed, but is checked like any call
    for flags in (0, 1, 2, 3):
        assert call(count=0, p=params(flags=flags)) == 0
    assert call(count=0, rays=None, ranges=None) == 0 and call(count=0, p=params(max_rounds=0)) == 0
    assert call(count=0, p=params(max_rounds=64, cap=32767.0)) == 0 and call(count=0, p=params(cap=1.0)) == 0
    assert call(count=0, counts=None) == -1 and call(count=0, workspace=None) == -1 and call(count=0, p=params(max_rounds=65)) == -1
    assert lib.vk_volume_integrate_rays_workspace_bytes(0, 0) == 0 and lib.vk_volume_integrate_rays_workspace_bytes(8, -1) == 0
    assert lib.vk_volume_integrate_rays_workspace_bytes(509, 96) >= 605 * (512 * 12 + 1)
    assert C.sizeof(T.IntegrateRaysParams) == 24
