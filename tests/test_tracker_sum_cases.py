"""The conditions tests/test_gpu_tracker_sums.py rests on, checked on the CPU oracle alone: the table of
pixel groups, that every chosen pixel really has a term in scenes D and C (tests/tracker_sum_cases.py), that
the oracle's system of a one-term frame is the float32 products of its row, bit for bit, and that the holes
pattern leaves a mixed image. A bad choice of inputs shows up here, without a GPU."""
import numpy as np
import pytest

import tracker_sum_cases as tc

SIZE_IDS = [tc.size_id(s) for s in tc.SIZES]
SMALL_IDS = [tc.size_id(s) for s in tc.SMALL_SIZES]
COLOR_IDS = [tc.size_id(s) for s in tc.COLOR_SIZES]
# the colour tracker, and the light tracker in its point-to-plane branch (mask 0) and with the oracle's own mask
COLOR_TRACKERS = [("color", None), ("light", "zero"), ("light", "own")]


def _light(kind):
    return tc.light() if kind == "light" else None


def test_group_table():
    """The rule of group_pixels_for, restated, gives the groups the sizes were chosen for."""
    want = {(1, 1): (256, 1, 1), (17, 9): (256, 1, 153), (16, 16): (256, 1, 256), (257, 1): (256, 2, 1),
            (101, 77): (256, 31, 97), (96, 88): (256, 33, 256), (263, 251): (512, 129, 477), (1031, 515): (2304, 231, 1045)}
    for (w, h), (g, groups, last) in want.items():
        n = w * h
        assert (tc.group_pixels(n), tc.group_count(n), n - (groups - 1) * g) == (g, groups, last), (w, h)
        assert tc.GROUPS[(w, h)] == groups
    # 640x480, 320x240 and 1280x960 as vk_gauss_newton.hpp states them
    assert [(tc.group_count(n), tc.group_pixels(n)) for n in (640 * 480, 320 * 240, 1280 * 960)] == [(240, 1280), (150, 512), (253, 4864)]
    # G > 2048 is what sends the depth tracker into a second batch of four 512-lane trips
    assert tc.group_pixels(1031 * 515) > 2048 >= tc.group_pixels(263 * 251)


def test_positions():
    for (w, h) in tc.SIZES:
        n = w * h
        g, groups = tc.group_pixels(n), tc.group_count(n)
        pos = tc.impulse_positions(n)
        assert pos[0] == 0 and pos[-1] == n - 1 and len(pos) == len(set(pos)) <= 14 and all(0 <= p < n for p in pos)
        assert (groups - 1) * g in pos
        sparse = tc.sparse_positions(n)
        assert len(sparse) == min(groups, tc.MAX_SPARSE) and all(0 <= p < n for p in sparse)
        assert len({p // g for p in sparse}) == len(sparse)              # one per group
        assert sparse[0] // g == 0 and sparse[-1] // g == groups - 1     # the first and the last group among them


@pytest.mark.parametrize("size", tc.SIZES, ids=SIZE_IDS)
def test_scene_d_every_pixel_has_a_term(orc, size):
    """Dense: every frame pixel contributes, with J[5] = -1 and J[3] = J[4] = 0 exactly. Holes: 60 to 80 % do
    (the pattern removes 30 %; sizes of at least 153 pixels, where that is three standard deviations)."""
    scene = tc.SceneD(*size)
    for translation in (True, False):
        J, r = scene.rows(orc, translation)
        assert np.all(np.any(J != 0, axis=1)) and np.all(r != 0)
        if translation:
            assert np.all(J[:, 5] == -1) and np.all(J[:, 3:5] == 0) and np.all(J[:, 2] == 0)
        else:
            assert np.all(J[:, 3:] == 0)
    J, r = scene.rows(orc, True, frame_depth=scene.holed())
    share = np.any(J != 0, axis=1).mean()
    assert np.array_equal(np.any(J != 0, axis=1), scene.holed().reshape(-1) > 0)
    if scene.n >= 153:
        assert 0.6 <= share <= 0.8, share


@pytest.mark.parametrize("size", tc.COLOR_SIZES, ids=COLOR_IDS)
@pytest.mark.parametrize("kind,mask", COLOR_TRACKERS)
def test_scene_c_every_pixel_has_a_term(orc, size, kind, mask):
    scene = tc.SceneC(*size)
    for translation in (True, False):
        J, r = scene.rows(orc, translation, _light(kind), mask)
        assert np.all(np.any(J != 0, axis=1)), np.flatnonzero(~np.any(J != 0, axis=1))[:8]
        for p in tc.impulse_positions(scene.n) + tc.sparse_positions(scene.n):
            assert r[p] != 0, p
        if mask == "zero" and translation:
            assert np.all(J[:, 5] == -1) and np.all(J[:, 3:5] == 0)
    if mask == "zero":
        holed = scene.holed()
        J, r = scene.rows(orc, True, _light(kind), mask, frame_depth=holed)
        share = np.any(J != 0, axis=1).mean()
        assert 0.6 <= share <= 0.8, share
    # with a frame of the keyframe's own size the last row and column would not contribute: the margin is needed
    assert scene.fw == scene.w + 4 and scene.fh == scene.h + 4


@pytest.mark.parametrize("size", tc.SMALL_SIZES, ids=SMALL_IDS)
def test_scene_d_impulse_system_is_the_products(orc, size):
    """The oracle's system of a frame with one valid pixel is that pixel's float32 products, bit for bit (one
    term plus zeros is exact in any order), and a pixel whose keyframe depth is gone leaves an all-zero system."""
    scene = tc.SceneD(*size)
    for translation in (True, False):
        J, r = scene.rows(orc, translation)
        for p in tc.impulse_positions(scene.n):
            want, _ = tc.expected_sums(J[p], r[p], translation)
            got = tc.oracle_sums(*scene.system(orc, translation, frame_depth=scene.only([p])))
            assert np.array_equal(tc.bits(got), tc.bits(want)), (p, translation)
            assert np.count_nonzero(want) >= (6 if translation else 4)
        p = tc.silent_position(scene.n)
        key = scene.key_depth.copy()
        key.reshape(-1)[p] = 0
        H, g = scene.system(orc, translation, frame_depth=scene.only([p]), key_depth=key)
        assert np.all(H == 0) and np.all(g == 0)


@pytest.mark.parametrize("size", tc.COLOR_SIZES, ids=COLOR_IDS)
@pytest.mark.parametrize("kind,mask", COLOR_TRACKERS)
def test_scene_c_impulse_system_is_the_products(orc, size, kind, mask):
    scene = tc.SceneC(*size)
    light = _light(kind)
    for translation in (True, False):
        J, r = scene.rows(orc, translation, light, mask)
        for p in tc.impulse_positions(scene.n):
            want, _ = tc.expected_sums(J[p], r[p], translation)
            got = tc.oracle_sums(*scene.system(orc, translation, light, mask, key_depth=scene.only([p])))
            assert np.array_equal(tc.bits(got), tc.bits(want)), (p, translation)
        p = tc.silent_position(scene.n)
        H, g = scene.system(orc, translation, light, mask, frame_depth=scene.without_frame_pixel(p), key_depth=scene.only([p]))
        assert np.all(H == 0) and np.all(g == 0)


@pytest.mark.parametrize("size", tc.SMALL_SIZES, ids=SMALL_IDS)
def test_sparse_bound_holds_for_the_oracle(orc, size):
    """The oracle's double sums of the sparse frames lie within the derived bound of the float64 sums of the
    float32 products — trivially (they are those sums), which is what shows the expectation is the right one."""
    scene = tc.SceneD(*size)
    pixels = tc.sparse_positions(scene.n)
    J, r = scene.rows(orc, True)
    want, scale = tc.expected_sums(J[pixels], r[pixels], True)
    got = tc.oracle_sums(*scene.system(orc, True, frame_depth=scene.only(pixels)))
    assert np.all(np.abs(got - want) <= 2 * len(pixels) * 2.0 ** -24 * scale)
    assert want[tc.PACKED_55] == len(pixels)
