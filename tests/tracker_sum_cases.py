"""Scenes, image sizes and pixel positions for the tests of the trackers' 27 sums (the 6 gradient and 21
packed Hessian sums of a Gauss-Newton step) at ragged image sizes: tests/test_tracker_sum_cases.py checks
on the CPU oracle the conditions the choices below rest on, tests/test_gpu_tracker_sums.py holds the
device to them.

Every frame carries its normals explicitly, (0, 0, -1) everywhere, so a border pixel is as valid as an
interior one.

Scene D (depth tracker): keyframe depth 1 + 0.05 cos(3x/w) sin(2y/h), frame depth the same + 0.003, both
poses the identity. Every frame pixel has the row J = (-Y, X, 0, 0, 0, -1) and the residual -0.003.

Scene C (colour and light trackers): the sums run over keyframe pixels, and a projection outside
[0.5, w - 0.5) of the frame is rejected, so the frame is two pixels larger on every side — size
(w + 4) x (h + 4), principal point + 2, content shifted by 2 — and seen from translate(0.001, 0.0005, 0).
Then every keyframe pixel contributes, the first and the last included."""
import numpy as np

from vulcan_amd import vk_types as T

# (width, height) -> pixel groups; what each size reaches is said in the GPU tests' module docstring
GROUPS = {(1, 1): 1, (17, 9): 1, (16, 16): 1, (257, 1): 2, (101, 77): 31, (96, 88): 33, (263, 251): 129, (1031, 515): 231}
SIZES = list(GROUPS)
LARGE = (1031, 515)                                          # one launch per test only
SMALL_SIZES = [s for s in SIZES if s != LARGE]
COLOR_SIZES = [(17, 9), (16, 16), (101, 77), (96, 88), (263, 251)]     # keyframe sizes; a keyframe one pixel high has no interior
LOOP_SIZES = [(17, 9), (257, 1), (101, 77)]                  # count and impulse on the one-launch loop's system
COLOR_LOOP_SIZES = [(17, 9), (101, 77)]
MARGIN = 2                                                   # scene C: the frame's extra pixels on every side
OFFSET = np.float32(0.003)
HOLE_SHARE, HOLE_SEED = 0.3, 1
MAX_SPARSE = 48

# packed lower triangle, (r, c <= r) row-major: index of (r, c) is r (r + 1) / 2 + c
PACKED_55 = 20
PACKED_ZERO_WITH_FLAT_NORMALS = [9, 13, 14, 18, 19]          # (3,3) (4,3) (4,4) (5,3) (5,4)


def group_pixels(n):
    """group_pixels_for (vk_gauss_newton.hpp), restated: the smallest multiple of 256 pixels that gives at most 256 groups."""
    return max(256, _ceil_div(_ceil_div(n, 256), 256) * 256)


def group_count(n):
    return _ceil_div(n, group_pixels(n))


def _ceil_div(a, b):
    return -(-a // b)


def size_id(size):
    return f"{size[0]}x{size[1]}"


def projection(w, h, shift=0):
    return T.Projection.make(0.85 * w + 3, 0.85 * w + 3, 0.49 * w + shift, 0.52 * h + shift)


def surface(w, h, shift=0):
    """The keyframe's depth image; with `shift` the same content in an image `shift` pixels larger on every side."""
    y, x = np.mgrid[-shift:h + shift, -shift:w + shift]
    return (1.0 + 0.05 * np.cos(3.0 * x / w) * np.sin(2.0 * y / h)).astype(np.float32)


def texture(w, h, shift=0):
    y, x = np.mgrid[-shift:h + shift, -shift:w + shift]
    c = (0.5 + 0.3 * np.sin(x / 3.0) * np.cos(y / 4.0)).astype(np.float32)
    return np.repeat(c[:, :, None], 3, axis=2).copy()


def flat_normals(w, h):
    n = np.zeros((h, w, 3), np.float32)
    n[..., 2] = -1.0
    return n


def holes(shape):
    """True where the holes pattern zeroes the frame's depth."""
    return np.random.default_rng(HOLE_SEED).random(shape) < HOLE_SHARE


class SceneD:
    """Host images of scene D at w x h."""

    def __init__(self, w, h):
        self.w, self.h, self.n = w, h, w * h
        self.k = projection(w, h)
        self.key_depth = surface(w, h)
        self.frame_depth = (self.key_depth + OFFSET).astype(np.float32)
        self.normals = flat_normals(w, h)
        self.key_pose = self.frame_pose = T.Transform.identity()

    def host(self, orc, frame_depth=None, key_depth=None):
        hk = orc.HostFrame(self.key_depth if key_depth is None else key_depth, self.k, self.key_pose, normals=self.normals)
        hf = orc.HostFrame(self.frame_depth if frame_depth is None else frame_depth, self.k, self.frame_pose, normals=self.normals)
        return hk, hf

    def holed(self):
        d = self.frame_depth.copy()
        d[holes(d.shape)] = 0
        return d

    def only(self, pixels):
        """The frame's depth, zero everywhere but at the flat pixel indices `pixels`."""
        d = np.zeros_like(self.frame_depth)
        d.reshape(-1)[pixels] = self.frame_depth.reshape(-1)[pixels]
        return d

    def rows(self, orc, translation, frame_depth=None, key_depth=None):
        """(J [n, 6], r [n]) of the oracle, float32."""
        hk, hf = self.host(orc, frame_depth, key_depth)
        return orc.icp_jacobian(hk, hf, translation).reshape(-1, 6), orc.icp_residuals(hk, hf).reshape(-1)

    def system(self, orc, translation, frame_depth=None, key_depth=None):
        hk, hf = self.host(orc, frame_depth, key_depth)
        return orc.icp_system(hk, hf, translation)


class SceneC:
    """Host images of scene C: a w x h keyframe and a frame MARGIN pixels larger on every side."""

    def __init__(self, w, h):
        self.w, self.h, self.n = w, h, w * h
        self.fw, self.fh = w + 2 * MARGIN, h + 2 * MARGIN
        self.key_k, self.frame_k = projection(w, h), projection(w, h, MARGIN)
        self.key_depth = surface(w, h)
        self.frame_depth = (surface(w, h, MARGIN) + OFFSET).astype(np.float32)
        self.key_color, self.frame_color = texture(w, h), texture(w, h, MARGIN)
        self.key_normals, self.frame_normals = flat_normals(w, h), flat_normals(self.fw, self.fh)
        self.key_pose = T.Transform.identity()
        self.frame_pose = T.Transform.translate(0.001, 0.0005, 0.0)

    def host(self, orc, frame_depth=None, key_depth=None):
        """(keyframe, frame, keyframe side, frame side, Tcm) of the oracle."""
        hk = orc.HostFrame(self.key_depth if key_depth is None else key_depth, self.key_k, self.key_pose,
                           color=self.key_color, normals=self.key_normals)
        hf = orc.HostFrame(self.frame_depth if frame_depth is None else frame_depth, self.frame_k, self.frame_pose,
                           color=self.frame_color, normals=self.frame_normals)
        return hk, hf, orc.ColorSide(hk, False), orc.ColorSide(hf, True), orc.color_tcm(hk, hf)

    def holed(self):
        d = self.frame_depth.copy()
        d[holes(d.shape)] = 0
        return d

    def only(self, pixels):
        """The keyframe's depth, zero everywhere but at the flat pixel indices `pixels`."""
        d = np.zeros_like(self.key_depth)
        d.reshape(-1)[pixels] = self.key_depth.reshape(-1)[pixels]
        return d

    def frame_index(self, pixel):
        """Flat index of the frame pixel that keyframe pixel `pixel` lands on (the sub-pixel shift of the
        frame's pose stays under half a pixel at these sizes: tests/test_tracker_sum_cases.py)."""
        return (pixel // self.w + MARGIN) * self.fw + pixel % self.w + MARGIN

    def without_frame_pixel(self, pixel):
        d = self.frame_depth.copy()
        d.reshape(-1)[self.frame_index(pixel)] = 0
        return d

    def mask(self, orc, light_mask, frame_depth=None):
        """The light tracker's frame mask: "zero" (point-to-plane branch everywhere) or "own" (the oracle's)."""
        if light_mask == "zero":
            return np.zeros((self.fh, self.fw), np.float32)
        return orc.light_frame_mask(self.host(orc, frame_depth)[1], 0.2)

    def rows(self, orc, translation, light=None, light_mask=None, frame_depth=None, key_depth=None):
        """(J [n, 6], r [n]) of the oracle, float32: the colour tracker's, or with `light` the light tracker's."""
        hk, hf, ks, fs, Tcm = self.host(orc, frame_depth, key_depth)
        if light is None:
            return orc.color_jacobian(ks, fs, Tcm, translation).reshape(-1, 6), orc.color_residuals(ks, fs, Tcm).reshape(-1)
        mask = self.mask(orc, light_mask, frame_depth)
        terms = orc.light_terms(hf, light, mask)
        return (orc.light_jacobian(ks, fs, terms, Tcm, translation).reshape(-1, 6),
                orc.light_residuals(ks, fs, terms, Tcm).reshape(-1))

    def system(self, orc, translation, light=None, light_mask=None, frame_depth=None, key_depth=None):
        hk, hf, ks, fs, Tcm = self.host(orc, frame_depth, key_depth)
        if light is None:
            return orc.color_system(ks, fs, Tcm, translation)
        mask = self.mask(orc, light_mask, frame_depth)
        return orc.light_system(ks, fs, orc.light_terms(hf, light, mask), Tcm, translation)


def light():
    return T.Light.make(2.0, (0.1, 0.0, 0.0))


def impulse_positions(n):
    """Flat pixel indices at which a single term is placed: the ends of the image, of a wave, of a workgroup's
    trip, of a group, of the first batch of four trips, of the last group and of the second stage's 32 slices."""
    g, groups = group_pixels(n), group_count(n)
    wanted = [0, n - 1, 63, 64, 511, 512, g - 1, g, 2047, 2048, (groups - 1) * g, (groups - 1) * g - 1, 32 * g - 1, 32 * g]
    return sorted({p for p in wanted if 0 <= p < n})


def silent_position(n):
    """The pixel whose partner is taken away, so that it has no term."""
    return n // 2


def sparse_positions(n):
    """One pixel in each of K = min(groups, 48) groups spread evenly from the first to the last, at the in-group
    offset (37 g) mod min(G, pixels in group g)."""
    g, groups = group_pixels(n), group_count(n)
    k = min(groups, MAX_SPARSE)
    chosen = sorted({int(round(i * (groups - 1) / max(k - 1, 1))) for i in range(k)})
    assert len(chosen) == k
    return [gi * g + (37 * gi) % min(g, n - gi * g) for gi in chosen]


def expected_sums(J, r, translation):
    """(sums [42], scale [42]) of the float32 rows J [k, 6], r [k]: the float64 sums of the float32 products
    J[r] J[c] (packed, [0, 36)) and J[i] r ([36, 42)) as the device lays them out, and the sums of their
    magnitudes. Entries the device does not compute (translation disabled) are 0."""
    J, r = np.asarray(J, np.float32).reshape(-1, 6), np.asarray(r, np.float32).reshape(-1)
    n = 6 if translation else 3
    sums, scale = np.zeros(42), np.zeros(42)
    idx = 0
    for rr in range(n):
        for c in range(rr + 1):
            t = (J[:, rr] * J[:, c]).astype(np.float64)           # float32 products, as the kernels form them
            sums[idx], scale[idx] = t.sum(), np.abs(t).sum()
            idx += 1
    for i in range(n):
        t = (J[:, i] * r).astype(np.float64)
        sums[36 + i], scale[36 + i] = t.sum(), np.abs(t).sum()
    return sums, scale


def oracle_sums(hessian, gradient):
    """The oracle's (hessian [21], gradient [6]) in the device's 42-float layout."""
    out = np.zeros(42)
    out[:21], out[36:42] = hessian, gradient
    return out


def bits(x):
    """float32 bit patterns; a sum that starts at +0 is never -0, so a -0 product counts as +0."""
    return (np.asarray(x, np.float64).astype(np.float32) + np.float32(0)).view(np.uint32)
