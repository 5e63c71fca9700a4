"""The trackers' 27 sums (6 gradient + 21 packed Hessian sums of a Gauss-Newton step) held to answers that do
not depend on the order of summation, at image sizes whose pixel groups end raggedly. Both reduction paths —
launch per stage (compute_system: store_partial / sum_partials) and the one-launch loop (track:
publish_partial / gather_partials) — and the three pixel walks (vk_icp.hip, vk_color_tracker.hip).

  size       N        G     groups  what it reaches
  1x1        1        256   1       one pixel, one lane
  17x9       153      256   1       fewer pixels than half a workgroup
  16x16      256      256   1       exactly one full group
  257x1      257      256   2       the second group holds one pixel; height 1
  101x77     7 777    256   31      last group 97 pixels; fewer partials than slices of the second stage
  96x88      8 448    256   33      all groups full; slice 0 gets two partials
  263x251    66 013   512   129     first size with G > 256; last group 477 pixels
  1031x515   530 965  2 304 231     G > 2 048: the depth tracker's second batch of trips, its last trip half
                                    empty; last group 1 045 pixels (one launch per test only)

The scenes (tests/tracker_sum_cases.py; their conditions are checked in tests/test_tracker_sum_cases.py) make
three expectations exact by construction:

  count    with flat normals (0, 0, -1) and translation enabled J[5] = -1 and J[3] = J[4] = 0 for every
           contributing pixel of the depth tracker and of the light tracker's point-to-plane branch, so packed
           entry (5,5) IS the number of contributing pixels — a sum of ones below 2^24, exact in any order —
           and (3,3) (4,3) (4,4) (5,3) (5,4) are exactly 0. A pixel dropped or taken twice shows as N -+ 1.
  impulse  one contributing pixel: all 27 outputs are the float32 products of the oracle's row, bit for bit
           (one term plus zeros is exact, contracted to an FMA or not; a -0 product arrives as +0).
  sparse   one pixel in each of K <= 48 groups, against the float64 sum of the float32 products:
           |got - want| <= 2 K 2^-24 sum|terms| — one rounding per product and one per addition, to first
           order, doubled. A missing or doubled partial moves a sum by about sum|terms| / K.

The dense scene's sums are compared with the oracle's double sums to the project's 2e-5 sum|terms| + 1e-12
(test_gpu_parity.py::test_icp_system), and the loop's published system with the staged one byte for byte."""
import numpy as np
import pytest

import tracker_sum_cases as tc
from gpu_support import api, sync  # noqa: F401

pytestmark = pytest.mark.gpu

SIZE_IDS = [tc.size_id(s) for s in tc.SIZES]
SMALL_IDS = [tc.size_id(s) for s in tc.SMALL_SIZES]
COLOR_IDS = [tc.size_id(s) for s in tc.COLOR_SIZES]
LOOP_IDS = [tc.size_id(s) for s in tc.LOOP_SIZES]
COLOR_LOOP_IDS = [tc.size_id(s) for s in tc.COLOR_LOOP_SIZES]
SENTINEL = 7.0                    # what the system buffer holds before a call: every output must be written


def assert_exact(got, J, r, translation, what):
    """The device's 42 floats are the float32 products of the single row (J, r), bit for bit; of no row: all zero."""
    want, _ = tc.expected_sums(J, r, translation)
    assert np.array_equal(tc.bits(got), tc.bits(want)), (what, got, want.astype(np.float32))
    if not translation:
        assert np.all(got[6:36] == 0) and np.all(got[39:42] == 0), what


def assert_count(got, count, what):
    assert got[tc.PACKED_55] == count, (what, got[tc.PACKED_55], count)
    assert np.all(got[tc.PACKED_ZERO_WITH_FLAT_NORMALS] == 0), (what, got[tc.PACKED_ZERO_WITH_FLAT_NORMALS])


def assert_within(got, want, bound, translation, what):
    worst = np.max(np.abs(got - want) / np.where(bound > 0, bound, 1.0))
    print(f"{what}: worst |got - want| / bound = {worst:.3g}")
    assert np.all(np.abs(got - want) <= bound), (what, got - want, bound)
    assert np.all(got[21:36] == 0), what
    if not translation:
        assert np.all(got[6:21] == 0) and np.all(got[39:42] == 0), what


class DepthRig:
    """Scene D on the device: the images stay there, the frame's depth is rewritten in place."""

    def __init__(self, api, scene):
        import torch
        self.api, self.scene = api, scene
        self.dense = torch.from_numpy(scene.frame_depth).cuda()
        self.key_dense = torch.from_numpy(scene.key_depth).cuda()
        self.key = api.Frame(self.key_dense.clone(), scene.k, scene.key_pose, normals=scene.normals)
        self.frame = api.Frame(self.dense.clone(), scene.k, scene.frame_pose, normals=scene.normals)
        self.tracker = api.DepthTracker()
        self.tracker.keyframe = self.key
        self.tracker.max_iterations = 1

    def show(self, depth=None):
        """The frame's depth image: the dense one, or a host array."""
        import torch
        self.frame.depth.copy_(self.dense if depth is None else torch.from_numpy(depth).cuda())

    def show_only(self, pixel):
        self.frame.depth.zero_()
        self.frame.depth.view(-1)[pixel] = self.dense.view(-1)[pixel]

    def silence(self, pixel, on=True):
        """Takes away (or puts back) the keyframe depth that frame pixel `pixel` lands on."""
        self.key.depth.view(-1)[pixel] = 0.0 if on else self.key_dense.view(-1)[pixel]

    def staged(self, translation):
        t = self.tracker
        t.translation_enabled = translation
        t.system.fill_(SENTINEL)
        t.compute_system(self.frame)
        return t.system[:42].cpu().numpy()

    def loop(self, translation, hook=False):
        """(system published by workgroup 0, pose) of a one-step Track from the scene's pose."""
        t = self.tracker
        t.translation_enabled = translation
        t.reduce_hook = (lambda system: None) if hook else None
        t.system.fill_(SENTINEL)
        self.frame.depth_to_world = self.scene.frame_pose
        try:
            pose = t.track(self.frame)
        finally:
            t.reduce_hook = None
            self.frame.depth_to_world = self.scene.frame_pose
        assert t.state.cpu().numpy()[0] == 1
        return t.system[:42].cpu().numpy(), pose


class ColorRig:
    """Scene C on the device for the colour tracker (kind "color") or the light tracker ("light"); the
    keyframe's and the frame's depth are rewritten in place."""

    def __init__(self, api, scene, kind):
        import torch
        self.api, self.scene, self.kind = api, scene, kind
        self.key_dense = torch.from_numpy(scene.key_depth).cuda()
        self.frame_dense = torch.from_numpy(scene.frame_depth).cuda()
        self.key = api.Frame(self.key_dense.clone(), scene.key_k, scene.key_pose, color=scene.key_color, normals=scene.key_normals)
        self.frame = api.Frame(self.frame_dense.clone(), scene.frame_k, scene.frame_pose, color=scene.frame_color,
                               normals=scene.frame_normals)
        self.tracker = api.LightTracker() if kind == "light" else api.ColorTracker()
        if kind == "light":
            self.tracker.light = tc.light()
        self.tracker.keyframe = self.key
        self.tracker.max_iterations = 1
        self.masks = {}

    def mask(self, orc, name):
        """The device copy of the light tracker's frame mask `name` ("zero" / "own": of the dense frame); None: the tracker's own."""
        import torch
        if self.kind != "light" or name is None:
            return None
        if name not in self.masks:
            self.masks[name] = torch.from_numpy(self.scene.mask(orc, name)).cuda()
        return self.masks[name]

    def show(self, depth=None):
        import torch
        self.frame.depth.copy_(self.frame_dense if depth is None else torch.from_numpy(depth).cuda())

    def show_key_only(self, pixel):
        self.key.depth.zero_()
        self.key.depth.view(-1)[pixel] = self.key_dense.view(-1)[pixel]

    def show_key(self, depth=None):
        import torch
        self.key.depth.copy_(self.key_dense if depth is None else torch.from_numpy(depth).cuda())

    def silence(self, pixel, on=True):
        """Takes away (or puts back) the frame depth that keyframe pixel `pixel` lands on."""
        at = self.scene.frame_index(pixel)
        self.frame.depth.view(-1)[at] = 0.0 if on else self.frame_dense.view(-1)[at]

    def staged(self, translation, mask=None):
        t = self.tracker
        t.translation_enabled = translation
        t.system.fill_(SENTINEL)
        if self.kind == "light":
            t.compute_system(self.frame, mask)
        else:
            t.compute_system(self.frame)
        return t.system[:42].cpu().numpy()

    def loop(self, translation, hook=False, mask=None):
        """(system published by workgroup 0, pose) of a one-step Track from the scene's pose; the light tracker
        makes its own frame mask unless `mask` is given."""
        t = self.tracker
        t.translation_enabled = translation
        t.reduce_hook = (lambda system: None) if hook else None
        if mask is not None:
            t._terms = lambda frame, given=None: type(t)._terms(t, frame, mask)
        t.system.fill_(SENTINEL)
        self.frame.depth_to_world = self.scene.frame_pose
        try:
            pose = t.track(self.frame)
        finally:
            t.reduce_hook = None
            t.__dict__.pop("_terms", None)
            self.frame.depth_to_world = self.scene.frame_pose
        assert t.state.cpu().numpy()[0] == 1
        return t.system[:42].cpu().numpy(), pose


def _light(kind):
    return tc.light() if kind == "light" else None


def _masks(kind):
    return ("zero", "own") if kind == "light" else (None,)


def test_group_table():
    """G = max(256, ceil(ceil(N / 256) / 256) * 256) pixels per group (group_pixels_for, vk_gauss_newton.hpp) and
    groups = ceil(N / G), restated: the sizes reach what the table says as long as that rule stands."""
    ceil_div = lambda a, b: (a + b - 1) // b
    for (w, h), groups in tc.GROUPS.items():
        n = w * h
        g = max(256, ceil_div(ceil_div(n, 256), 256) * 256)
        assert ceil_div(n, g) == groups, (w, h)
        assert (tc.group_pixels(n), tc.group_count(n)) == (g, groups)
    assert [tc.GROUPS[s] for s in tc.SIZES] == [1, 1, 1, 2, 31, 33, 129, 231]


# ------------------------------------------------------------------ depth tracker --

@pytest.mark.parametrize("size", tc.SIZES, ids=SIZE_IDS)
def test_depth_count_is_exact(api, orc, size):
    scene = tc.SceneD(*size)
    rig = DepthRig(api, scene)
    assert_count(rig.staged(True), scene.n, "dense")
    holed = scene.holed()
    J, _ = scene.rows(orc, True, frame_depth=holed)
    rig.show(holed)
    assert_count(rig.staged(True), int(np.any(J != 0, axis=1).sum()), "holes")


@pytest.mark.parametrize("size", tc.SMALL_SIZES, ids=SMALL_IDS)
def test_depth_impulse_is_the_products(api, orc, size):
    scene = tc.SceneD(*size)
    rig = DepthRig(api, scene)
    for translation in (True, False):
        J, r = scene.rows(orc, translation)
        for p in tc.impulse_positions(scene.n):
            rig.show_only(p)
            assert_exact(rig.staged(translation), J[p], r[p], translation, (p, translation))
        p = tc.silent_position(scene.n)
        rig.show_only(p)
        rig.silence(p)
        got = rig.staged(translation)
        rig.silence(p, False)
        assert np.all(got == 0), (p, got)


@pytest.mark.parametrize("size", tc.SMALL_SIZES, ids=SMALL_IDS)
def test_depth_sparse_sums(api, orc, size):
    scene = tc.SceneD(*size)
    rig = DepthRig(api, scene)
    pixels = tc.sparse_positions(scene.n)
    rig.show(scene.only(pixels))
    for translation in (True, False):
        J, r = scene.rows(orc, translation)
        want, scale = tc.expected_sums(J[pixels], r[pixels], translation)
        got = rig.staged(translation)
        assert_within(got, want, 2 * len(pixels) * 2.0 ** -24 * scale, translation, f"sparse K={len(pixels)}")
        if translation:
            assert_count(got, len(pixels), "sparse")


@pytest.mark.parametrize("size", tc.SIZES, ids=SIZE_IDS)
def test_depth_dense_sums_match_the_oracle(api, orc, size):
    scene = tc.SceneD(*size)
    rig = DepthRig(api, scene)
    for translation in (True, False):
        J, r = scene.rows(orc, translation)
        _, scale = tc.expected_sums(J, r, translation)
        want = tc.oracle_sums(*scene.system(orc, translation))
        assert_within(rig.staged(translation), want, 2e-5 * scale + 1e-12, translation, "dense")


@pytest.mark.parametrize("size", tc.SIZES, ids=SIZE_IDS)
def test_depth_loop_equals_staged(api, orc, size):
    """compute_system against the system workgroup 0 of the one-launch loop publishes: as the device sizes the
    grid, with one and three workgroups (the non-resident form, several groups per workgroup) and launch per
    stage behind a reduce hook. The one-pixel image's system has rank one: its pose is not looked at."""
    scene = tc.SceneD(*size)
    rig = DepthRig(api, scene)
    for translation in (True, False):
        staged = rig.staged(translation).tobytes()
        runs = [("loop", rig.loop(translation))]
        for cap in (1, 3):
            with api.test_hooks(loop_grid_cap=cap):
                runs.append((f"cap {cap}", rig.loop(translation)))
        runs.append(("hook", rig.loop(translation, hook=True)))
        for name, (system, pose) in runs:
            assert system.tobytes() == staged, (name, translation)
            if scene.n > 1:
                assert np.all(np.isfinite(pose.matrix())) and np.all(np.isfinite(pose.inverse_matrix())), name


@pytest.mark.parametrize("size", tc.LOOP_SIZES, ids=LOOP_IDS)
def test_depth_loop_count_and_impulse(api, orc, size):
    scene = tc.SceneD(*size)
    rig = DepthRig(api, scene)
    assert_count(rig.loop(True)[0], scene.n, "dense")
    holed = scene.holed()
    J, _ = scene.rows(orc, True, frame_depth=holed)
    rig.show(holed)
    assert_count(rig.loop(True)[0], int(np.any(J != 0, axis=1).sum()), "holes")
    for translation in (True, False):
        J, r = scene.rows(orc, translation)
        for p in tc.impulse_positions(scene.n):
            rig.show_only(p)
            assert_exact(rig.loop(translation)[0], J[p], r[p], translation, (p, translation))
        p = tc.silent_position(scene.n)
        rig.show_only(p)
        rig.silence(p)
        got = rig.loop(translation)[0]
        rig.silence(p, False)
        assert np.all(got == 0), (p, got)


# ------------------------------------------------------- colour and light trackers --

@pytest.mark.parametrize("size", tc.COLOR_SIZES, ids=COLOR_IDS)
def test_light_count_is_exact(api, orc, size):
    """The light tracker with an all-zero mask: the point-to-plane branch, J[5] = n.z = -1 (Tcm is a pure translation)."""
    scene = tc.SceneC(*size)
    rig = ColorRig(api, scene, "light")
    zero = rig.mask(orc, "zero")
    assert_count(rig.staged(True, zero), scene.n, "dense")
    holed = scene.holed()
    J, _ = scene.rows(orc, True, tc.light(), "zero", frame_depth=holed)
    rig.show(holed)
    assert_count(rig.staged(True, zero), int(np.any(J != 0, axis=1).sum()), "holes")


@pytest.mark.parametrize("size", tc.COLOR_SIZES, ids=COLOR_IDS)
@pytest.mark.parametrize("kind", ("color", "light"))
def test_color_impulse_is_the_products(api, orc, size, kind):
    scene = tc.SceneC(*size)
    rig = ColorRig(api, scene, kind)
    for name in _masks(kind):
        mask = rig.mask(orc, name)
        for translation in (True, False):
            J, r = scene.rows(orc, translation, _light(kind), name)
            for p in tc.impulse_positions(scene.n):
                rig.show_key_only(p)
                assert_exact(rig.staged(translation, mask), J[p], r[p], translation, (name, p, translation))
            p = tc.silent_position(scene.n)
            rig.show_key_only(p)
            rig.silence(p)
            got = rig.staged(translation, mask)
            rig.silence(p, False)
            assert np.all(got == 0), (name, p, got)


@pytest.mark.parametrize("size", tc.COLOR_SIZES, ids=COLOR_IDS)
@pytest.mark.parametrize("kind", ("color", "light"))
def test_color_sparse_sums(api, orc, size, kind):
    scene = tc.SceneC(*size)
    rig = ColorRig(api, scene, kind)
    pixels = tc.sparse_positions(scene.n)
    rig.show_key(scene.only(pixels))
    for name in _masks(kind):
        for translation in (True, False):
            J, r = scene.rows(orc, translation, _light(kind), name)
            want, scale = tc.expected_sums(J[pixels], r[pixels], translation)
            got = rig.staged(translation, rig.mask(orc, name))
            assert_within(got, want, 2 * len(pixels) * 2.0 ** -24 * scale, translation, f"sparse {name} K={len(pixels)}")
            if translation and name == "zero":
                assert_count(got, len(pixels), "sparse")


@pytest.mark.parametrize("size", tc.COLOR_SIZES, ids=COLOR_IDS)
@pytest.mark.parametrize("kind", ("color", "light"))
def test_color_dense_sums_match_the_oracle(api, orc, size, kind):
    scene = tc.SceneC(*size)
    rig = ColorRig(api, scene, kind)
    for name in _masks(kind):
        for translation in (True, False):
            J, r = scene.rows(orc, translation, _light(kind), name)
            _, scale = tc.expected_sums(J, r, translation)
            want = tc.oracle_sums(*scene.system(orc, translation, _light(kind), name))
            got = rig.staged(translation, rig.mask(orc, name))
            assert_within(got, want, 2e-5 * scale + 1e-12, translation, f"dense {name}")


@pytest.mark.parametrize("size", tc.COLOR_SIZES, ids=COLOR_IDS)
@pytest.mark.parametrize("kind", ("color", "light"))
def test_color_loop_equals_staged(api, orc, size, kind):
    """As test_depth_loop_equals_staged; the light tracker makes its own frame mask on both paths."""
    scene = tc.SceneC(*size)
    rig = ColorRig(api, scene, kind)
    if kind == "light":
        own = rig.tracker.compute_frame_mask(rig.frame)
        assert np.array_equal(own.cpu().numpy(), scene.mask(orc, "own"))
    for translation in (True, False):
        staged = rig.staged(translation).tobytes()
        runs = [("loop", rig.loop(translation))]
        for cap in (1, 3):
            with api.test_hooks(loop_grid_cap=cap):
                runs.append((f"cap {cap}", rig.loop(translation)))
        runs.append(("hook", rig.loop(translation, hook=True)))
        for name, (system, pose) in runs:
            assert system.tobytes() == staged, (name, translation)
            assert np.all(np.isfinite(pose.matrix())) and np.all(np.isfinite(pose.inverse_matrix())), name


@pytest.mark.parametrize("size", tc.COLOR_LOOP_SIZES, ids=COLOR_LOOP_IDS)
@pytest.mark.parametrize("kind", ("color", "light"))
def test_color_loop_count_and_impulse(api, orc, size, kind):
    """Count (light tracker, all-zero mask handed to the loop) and impulse (each tracker as it runs: the
    light tracker with the mask it makes itself) on the system the one-launch loop publishes."""
    scene = tc.SceneC(*size)
    rig = ColorRig(api, scene, kind)
    if kind == "light":
        zero = rig.mask(orc, "zero")
        assert_count(rig.loop(True, mask=zero)[0], scene.n, "dense")
        holed = scene.holed()
        J, _ = scene.rows(orc, True, tc.light(), "zero", frame_depth=holed)
        rig.show(holed)
        assert_count(rig.loop(True, mask=zero)[0], int(np.any(J != 0, axis=1).sum()), "holes")
        rig.show()
    name = "own" if kind == "light" else None
    for translation in (True, False):
        J, r = scene.rows(orc, translation, _light(kind), name)
        for p in tc.impulse_positions(scene.n):
            rig.show_key_only(p)
            assert_exact(rig.loop(translation)[0], J[p], r[p], translation, (p, translation))
        p = tc.silent_position(scene.n)
        rig.show_key_only(p)
        rig.silence(p)
        got = rig.loop(translation)[0]
        rig.silence(p, False)
        assert np.all(got == 0), (p, got)
