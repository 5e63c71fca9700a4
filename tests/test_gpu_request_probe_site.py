"""The request pass of SetView collects the blocks a wave's rays cross in a per-wave list and probes them at ONE site,
64 at a time (vk_requests.hpp request_walk). Whatever the pass leaves — the hash table, allocation_types /
allocation_blocks, the plain visibility bytes, the visible set, the pool pointers, the request and dropped counts — must be
what the oracle's SetView leaves, in every form the pass is launched in:

  stand-alone   vk_volume_set_view / _prepare / _rounds     create_requests_kernel<true, PREP 0 / 1 / 2>
  device pose   vk_volume_set_view_at_device_pose           create_requests_at_kernel<PREP 0 / 1>
  riding        vk_trace_ahead_requests, then SetView       trace_and_request_kernel<., PREP 0 / 1 / 2>

The shapes are the smallest at which the list can go wrong. A 96 x 8 image: the second wave of every row holds 32 lanes past
the image. Row 3 has zero and out-of-range depths in the middle of its first wave: lanes whose left neighbour walks nothing.
"long": 2 mm voxels (16 mm blocks) against 80 mm of truncation: every ray crosses ten blocks or more — more than any fixed
number of probe slots — and the 64 pixels of a wave cross several hundred different blocks, several lists' worth (checked on
the oracle below): the list is probed and restarted in the middle of the walk. Its table has 37 buckets for some thousands of
blocks: every bucket is contested, chains grow with every round, later rounds post EXCESS requests. With the hooks the posted
list holds 4 buckets and the retry list 8 keys: the handle pass scans the flags, the rounds end after the first.
"origin": the surface passes through the world's origin and bucket 0 is unallocated, so block (0,0,0) is met in an unallocated
main entry (volume.cu:186-191).
With a LightIntegrator's preparation riding (PREP 1 / 2) the frame is integrated afterwards and the voxels are compared: mask,
records and — PREP 2 — the normal image come from LDS areas the visit lists share."""
import numpy as np
import pytest

import scenes
from gpu_support import api, assert_volume_equal, frames, make_pair, sync  # noqa: F401
from vulcan_amd import vk_types as T

pytestmark = pytest.mark.gpu

W, H = 96, 8
K_IMAGE = T.Projection.make(80.0, 80.0, 48.0, 4.0)
LIST_SLOTS = 96            # kVisitSlots, vk_requests.hpp
WAVES = 2 * H              # 64-pixel runs of the image

GEOMETRY = {
    # main, excess, voxel, truncation, pose of the frame under test
    "long": (37, 512, 0.002, 0.08, T.Transform.translate(0.013, -0.021, 0.007)),
    "origin": (4096, 512, 0.008, 0.04, T.Transform.translate(0.0, 0.0, -1.0)),
}
FORMS = ["alone-0", "alone-1", "alone-2", "pose-0", "pose-1", "riding-0", "riding-1", "riding-2"]
SMALL_LISTS = {"posted_capacity": 4, "retry_capacity": 8}


def depth_image():
    depth = scenes.plane(W, H, 1.0).copy()
    depth += (np.arange(W, dtype=np.float32) * np.float32(0.0005))[None, :]     # no two columns at the same depth
    depth[3, 20:31] = 0.0                                                         # no measurement
    depth[3, 40:45] = 100.0                                                       # out of range
    depth[3, 50] = 0.05                                                           # below the range
    return depth.astype(np.float32)


def colour_image():
    return scenes.checker_color(W, H, 0.1, 0.9)


_DISTINCT = {}


def distinct_buckets(orc, name):
    """Buckets one SetView of the frame under test requests in a table with room for every block: a lower bound of the
    different blocks its rays cross (the oracle, once per geometry)."""
    if name not in _DISTINCT:
        _, _, voxel, trunc, pose = GEOMETRY[name]
        hv = orc.HostVolume(65521, 64, voxel_length=voxel, truncation_length=trunc)
        hv.set_view(orc.HostFrame(depth_image(), K_IMAGE, pose), orc.POLICY_MAXKEY)
        _DISTINCT[name] = int(hv.counters[T.VK_CTR_REQUESTS])
    return _DISTINCT[name]


def run_case(api, orc, geometry, form, rounds, hooks):
    import torch
    kind, prep_level = form.split("-")
    prep_level = int(prep_level)
    main, excess, voxel, trunc, pose = GEOMETRY[geometry]
    depth, colour = depth_image(), colour_image()
    light = T.Light.make(2.0, (0.025, 0.08, 0.0))
    hv, dv = make_pair(api, orc, main, excess, voxel, trunc)
    integ = api.LightIntegrator(dv) if prep_level else api.DepthIntegrator(dv)
    if prep_level:
        integ.light = light
    tracer = api.Tracer(dv)

    def fuse(hf, df):
        orc.integrate_depth(hv, hf)
        if prep_level:
            orc.integrate_light_color(hv, hf, light, orc.light_frame_mask(hf, 0.2))
        integ.integrate(df)

    # a first frame three metres away (none of its blocks is crossed again): the table is not empty, the integrator's
    # preparation is registered with the volume, and there is something to raycast
    first_pose = T.Transform.translate(3.0, 0.0, 0.0) * pose
    hf0, df0 = frames(api, orc, depth, K_IMAGE, first_pose, color=colour)
    hf0.compute_normals()
    df0.compute_normals()
    hv.set_view(hf0, orc.POLICY_MAXKEY)
    dv.set_view(df0)
    fuse(hf0, df0)
    assert_volume_equal(dv, hv)
    if geometry == "origin":
        assert hv.hash_entries["data"][0] == -1, "bucket 0 must still be unallocated"

    hf, df = frames(api, orc, depth, K_IMAGE, pose, color=colour)
    hf.compute_normals()
    if prep_level != 2:
        df.compute_normals()
    before = int(dv.read_counters()[T.VK_CTR_ROUNDS])
    with api.test_hooks(**hooks):
        if kind == "alone":
            dv.set_view(df, rounds=rounds, compute_normals=(prep_level == 2))
        elif kind == "pose":
            pose_dev = torch.from_numpy(np.frombuffer(bytes(pose), dtype=np.uint8).copy()).cuda()
            assert dv.set_view_at_device_pose(df, pose_dev, rounds)
        else:
            out = api.Frame(np.zeros((H, W), np.float32), K_IMAGE, first_pose)
            tracer.trace(out, next_frame=df, next_needs_normals=(prep_level == 2))
            sync()
            assert dv.requests_ahead is not None and dv.requests_ahead.valid == 1, "the request pass was not made ahead"
            dv.set_view(df, rounds=rounds)
            assert dv.requests_ahead.valid == 0
        sync()
    if prep_level:
        assert integ._prep.valid == 1, "the preparation did not ride"

    # vk.h: the rounds end early only with VK_CTR_UNSETTLED set, and the state is then that of as many calls as ran
    ctr = dv.read_counters()
    ran = int(ctr[T.VK_CTR_ROUNDS]) - before
    assert 1 <= ran <= rounds
    calls = ran if (ctr[T.VK_CTR_UNSETTLED] == 1 and ran < rounds) else rounds
    if geometry == "long":
        # thousands of blocks lose their bucket in the first round: a retry list of 8 keys ends the rounds there, the
        # library's own (8192) holds them all
        assert calls == (1 if hooks else rounds), (ran, ctr)
    for _ in range(calls):
        hv.set_view(hf, orc.POLICY_MAXKEY)
    assert_volume_equal(dv, hv, voxels=False)
    assert ctr[T.VK_CTR_REQUESTS] == hv.counters[T.VK_CTR_REQUESTS], (ctr, hv.counters)
    assert hv.counters[T.VK_CTR_DROPPED] == 0

    if geometry == "long":
        assert hv.counters[T.VK_CTR_REQUESTS] == main                       # every bucket asked for, every round
        if calls > 1:
            assert hv.counters[T.VK_CTR_EXCESS_PTR] > hv.main + main         # chains: EXCESS requests were posted and served
    else:
        # the origin block was met in bucket 0's unallocated main entry: visible, never requested
        assert hv.block_visibility[0] == 2 and hv.hash_entries["data"][0] == -1

    if prep_level == 2:
        assert np.array_equal(df.normals.cpu().numpy(), hf.normals, equal_nan=True), "normals made with the pass differ"
    if prep_level:
        fuse(hf, df)
        assert_volume_equal(dv, hv)
        assert (hv.voxels["color_weight"] > 0).sum() > 0, "the light pass integrated nothing"


def test_the_shapes_are_the_ones_the_list_can_go_wrong_at(orc):
    """On the oracle: the 'long' frame's rays cross more different blocks than the image's waves have list slots — at least
    one wave fills its list and restarts it — and each ray crosses 2 * truncation / block length = 10 blocks or more."""
    assert distinct_buckets(orc, "long") > WAVES * LIST_SLOTS
    _, _, voxel, trunc, _ = GEOMETRY["long"]
    assert 2 * trunc / (8 * voxel) >= 10


@pytest.mark.parametrize("hooks", [{}, SMALL_LISTS], ids=["library lists", "small lists"])
@pytest.mark.parametrize("rounds", [1, 3])
@pytest.mark.parametrize("form", FORMS)
def test_long_walks_in_a_contested_table(api, orc, form, rounds, hooks):
    run_case(api, orc, "long", form, rounds, hooks)


@pytest.mark.parametrize("rounds", [1, 3])
@pytest.mark.parametrize("form", FORMS)
def test_the_origin_block_in_an_unallocated_entry(api, orc, form, rounds):
    run_case(api, orc, "origin", form, rounds, {})
