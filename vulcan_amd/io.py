"""Files on either side of the hot path: the mesh the extractor
produces and the RGB-D frames a sequence consists of. Host code; no device work.

write_ply     vulcan::Exporter::Export (src/exporter.cpp:19-71), byte for byte: ASCII PLY,
              `element vertex` with x y z and the red/green/blue debug colouring upstream
              marks "REMOVE" (a grey ramp over z from a fixed 0.35 to the largest z),
              `element face` as `3 i j k`; numbers as a C++ ostream prints floats.
              With `colors` the fused colours are written instead of the ramp, with `normals`
              nx / ny / nz follow z (both from Extractor.extract(colors=True, normals=True)).
read_ply      the inverse, for tests; read_ply_attributes reads the header's property list.
load_depth / save_depth, load_color / save_color
              Image::Load / Save and ColorImage::Load / Save (include/vulcan/image.h:100-133,
              228-253; src/image.cu:213-221,264-273) for the formats that need no OpenCV:
              binary PGM (8 or 16 bit, the depth maps a sensor delivers in millimetres) and binary
              PPM. Load: pixel * scale as float32; Save: pixel * alpha + beta, rounded to
              nearest even and saturated to the integer type, as cv::Mat::convertTo does.
SequenceWriter / SequenceReader
              a directory of depth_%06d.pgm / color_%06d.ppm plus sequence.txt (size,
              intrinsics, depth scale, one depth_to_world matrix + inverse per frame): what stands in for the
              HAL camera the upstream app reads from (apps/vulcan/vulcan.cu:181-232).
write_map / read_map
              the packed blocks of a volume (Volume.pack, vk_volume_pack) as one binary file: what PackedVolume.save /
              load and the C++ layer's PackedVolume::Save / Load read and write.
"""
import os

import numpy as np


def _g(x):
    """`std::ostream << float`: %g with 6 significant digits."""
    return "%g" % float(np.float32(x))


def write_ply(path, points, faces, colors=None, normals=None):
    """Without attributes: upstream's bytes. `colors` [n, 3] in [0, 1] replace the grey ramp: each channel
    int(min(max(c, 0), 1) * 255 + 0.5), in float32. `normals` [n, 3] add `property float nx / ny / nz` between z and
    red, printed as the coordinates are."""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    if colors is not None:
        colors = np.asarray(colors, dtype=np.float32).reshape(-1, 3)
        assert len(colors) == len(points)
    if normals is not None:
        normals = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
        assert len(normals) == len(points)
    out = ["ply", "format ascii 1.0", f"element vertex {len(points)}", "property float x", "property float y",
           "property float z"]
    if normals is not None:
        out += ["property float nx", "property float ny", "property float nz"]
    out += ["property uchar red", "property uchar green", "property uchar blue",
            f"element face {len(faces)}", "property list uchar int vertex_indices", "end_header"]
    # exporter.cpp:38-56: dmax = largest z; dmin is overwritten with 0.35f
    F = np.float32
    dmin = F(0.35)
    dmax = points[:, 2].max() if len(points) else F(0)
    if colors is not None:
        bytes_ = (np.minimum(np.maximum(colors, F(0)), F(1)) * F(255) + F(0.5)).astype(np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i, p in enumerate(points):
            line = f"{_g(p[0])} {_g(p[1])} {_g(p[2])}"
            if normals is not None:
                line += f" {_g(normals[i][0])} {_g(normals[i][1])} {_g(normals[i][2])}"
            if colors is not None:
                line += f" {bytes_[i][0]} {bytes_[i][1]} {bytes_[i][2]}"
            else:
                ratio = F(F(p[2] - dmin) / F(dmax - dmin))                 # exporter.cpp:62
                value = F(255) * (ratio if ratio < F(1.0) else F(1.0))     # min(1.0f, ratio), math.h:9-15
                color = int(value) if np.isfinite(value) else 0             # int(float) truncates; non-finite is undefined upstream
                line += f" {color} {color} {color}"
            out.append(line)
    for f in faces:
        out.append(f"3 {int(f[0])} {int(f[1])} {int(f[2])}")
    with open(path, "w") as fh:
        fh.write("\n".join(out) + "\n")


def read_ply(path):
    with open(path) as fh:
        lines = fh.read().split("\n")
    assert lines[0] == "ply" and lines[1] == "format ascii 1.0"
    nv = int(lines[2].split()[-1])
    end = lines.index("end_header")
    nf = int([l for l in lines[:end] if l.startswith("element face")][0].split()[-1])
    body = lines[end + 1:]
    verts = np.array([[float(t) for t in body[i].split()[:3]] for i in range(nv)], dtype=np.float32).reshape(-1, 3)
    colors = np.array([[int(t) for t in body[i].split()[3:6]] for i in range(nv)], dtype=np.int32).reshape(-1, 3)
    faces = np.array([[int(t) for t in body[nv + i].split()[1:4]] for i in range(nf)], dtype=np.int32).reshape(-1, 3)
    return verts, colors, faces


def read_ply_attributes(path):
    """A file of write_ply by its header's property list: (points, faces, colors, normals) — colors [n, 3] int32 from
    red / green / blue, normals [n, 3] float32 from nx / ny / nz, None for what the header does not name."""
    with open(path) as fh:
        lines = fh.read().split("\n")
    assert lines[0] == "ply" and lines[1] == "format ascii 1.0"
    end = lines.index("end_header")
    element, counts, names = None, {}, []
    for line in lines[2:end]:
        t = line.split()
        if t[0] == "element":
            element = t[1]
            counts[element] = int(t[2])
        elif t[0] == "property" and element == "vertex":
            names.append(t[-1])
    nv, nf = counts.get("vertex", 0), counts.get("face", 0)
    body = lines[end + 1:]
    table = np.array([[float(t) for t in body[i].split()] for i in range(nv)], dtype=np.float64).reshape(nv, len(names))

    def columns(wanted, dtype):
        if not all(w in names for w in wanted):
            return None
        return np.ascontiguousarray(table[:, [names.index(w) for w in wanted]].astype(dtype))
    faces = np.array([[int(t) for t in body[nv + i].split()[1:4]] for i in range(nf)], dtype=np.int32).reshape(-1, 3)
    return (columns(("x", "y", "z"), np.float32), faces, columns(("red", "green", "blue"), np.int32),
            columns(("nx", "ny", "nz"), np.float32))


# ---- Netpbm -------------------------------------------------------------------------

def _read_pnm(path):
    with open(path, "rb") as fh:
        data = fh.read()
    tokens, pos = [], 0
    while len(tokens) < 4:
        while data[pos:pos + 1].isspace():
            pos += 1
        if data[pos:pos + 1] == b"#":
            pos = data.index(b"\n", pos) + 1
            continue
        end = pos
        while not data[end:end + 1].isspace():
            end += 1
        tokens.append(data[pos:end])
        pos = end
    pos += 1                                    # the single whitespace after maxval
    magic, w, h, maxval = tokens[0], int(tokens[1]), int(tokens[2]), int(tokens[3])
    channels = {b"P5": 1, b"P6": 3}[magic]
    dtype = np.dtype(">u2") if maxval > 255 else np.uint8
    pixels = np.frombuffer(data, dtype=dtype, count=w * h * channels, offset=pos).reshape(h, w, channels)
    return pixels.astype(np.uint16 if maxval > 255 else np.uint8)


def _write_pnm(path, pixels):
    pixels = np.asarray(pixels)
    h, w = pixels.shape[:2]
    channels = 1 if pixels.ndim == 2 else pixels.shape[2]
    maxval = 65535 if pixels.dtype == np.uint16 else 255
    with open(path, "wb") as fh:
        fh.write(b"%s\n%d %d\n%d\n" % (b"P5" if channels == 1 else b"P6", w, h, maxval))
        fh.write(pixels.astype(">u2" if maxval > 255 else np.uint8).tobytes())


def _convert_to(values, integer_type, alpha, beta):
    """cv::Mat::convertTo(type, alpha, beta): saturate_cast<T>(cvRound(v * alpha + beta))."""
    v = np.asarray(values, dtype=np.float64) * alpha + beta
    info = np.iinfo(integer_type)
    return np.clip(np.rint(v), info.min, info.max).astype(integer_type)


def load_depth(path, scale=1.0):
    """Image::Load(file, scale) (image.h:100-111): grey PGM -> float32 [h, w]; an RGB file is
    reduced to grey first as cv::cvtColor(RGB2GRAY) does (0.299 R + 0.587 G + 0.114 B)."""
    px = _read_pnm(path)
    if px.shape[2] == 3:
        grey = 0.299 * px[..., 0].astype(np.float64) + 0.587 * px[..., 1] + 0.114 * px[..., 2]
        px = np.rint(grey).astype(px.dtype)[..., None]
    return (px[..., 0].astype(np.float32) * np.float32(scale)).astype(np.float32)


def save_depth(path, image, bits=8, alpha=1.0, beta=0.0):
    """Image::Save(file, CV_8UC1 | CV_16UC1, alpha, beta) (image.cu:213-221)."""
    _write_pnm(path, _convert_to(image, np.uint16 if bits == 16 else np.uint8, alpha, beta))


def load_color(path, scale=1.0):
    """ColorImage::Load(file, scale) (image.h:228-240): PPM -> float32 [h, w, 3] in R, G, B order;
    a grey file is replicated to three channels (cvtColor GRAY2RGB)."""
    px = _read_pnm(path)
    if px.shape[2] == 1:
        px = np.repeat(px, 3, axis=2)
    return (px.astype(np.float32) * np.float32(scale)).astype(np.float32)


def save_color(path, image, bits=8, alpha=1.0, beta=0.0):
    """ColorImage::Save (image.cu:264-273)."""
    _write_pnm(path, _convert_to(image, np.uint16 if bits == 16 else np.uint8, alpha, beta))


# ---- sequences ----------------------------------------------------------------------

class SequenceWriter:
    """depth_%06d.pgm (16 bit, depth / depth_scale), color_%06d.ppm (8 bit, colour * 255) and
    sequence.txt."""

    def __init__(self, directory, width, height, depth_projection, color_projection=None, depth_scale=0.001):
        os.makedirs(directory, exist_ok=True)
        self.directory, self.depth_scale, self.count = directory, float(depth_scale), 0
        k, c = depth_projection, color_projection or depth_projection
        self.header = [f"vulcan-sequence 1", f"size {width} {height}", f"depth_scale {self.depth_scale:.9g}",
                       "depth_projection " + " ".join(f"{float(v):.9g}" for v in (k.fx, k.fy, k.cx, k.cy)),
                       "color_projection " + " ".join(f"{float(v):.9g}" for v in (c.fx, c.fy, c.cx, c.cy))]
        self.poses = []

    def append(self, depth, color=None, depth_to_world=None):
        i = self.count
        save_depth(os.path.join(self.directory, "depth_%06d.pgm" % i), depth, bits=16, alpha=1.0 / self.depth_scale)
        if color is not None:
            save_color(os.path.join(self.directory, "color_%06d.ppm" % i), color, alpha=255.0)
        # matrix and cached inverse, both row-major: a Transform carries its inverse and never
        # recomputes it (transform.h:168-170), so the file keeps both
        if depth_to_world is None:
            m = inv = np.eye(4, dtype=np.float32)
        else:
            m = np.asarray(depth_to_world.matrix(), dtype=np.float32)
            inv = np.asarray(depth_to_world.inverse_matrix(), dtype=np.float32)
        self.poses.append("pose %d " % i + " ".join(f"{float(v):.9g}" for v in np.concatenate([m.reshape(-1), inv.reshape(-1)])))
        self.count += 1

    def close(self):
        with open(os.path.join(self.directory, "sequence.txt"), "w") as fh:
            fh.write("\n".join(self.header + [f"frames {self.count}"] + self.poses) + "\n")


class SequenceReader:
    def __init__(self, directory):
        self.directory = directory
        self.poses, self.inverse_poses = {}, {}
        for line in open(os.path.join(directory, "sequence.txt")):
            t = line.split()
            if not t:
                continue
            if t[0] == "size":
                self.width, self.height = int(t[1]), int(t[2])
            elif t[0] == "depth_scale":
                self.depth_scale = float(t[1])
            elif t[0] == "depth_projection":
                self.depth_projection = tuple(float(v) for v in t[1:5])
            elif t[0] == "color_projection":
                self.color_projection = tuple(float(v) for v in t[1:5])
            elif t[0] == "frames":
                self.count = int(t[1])
            elif t[0] == "pose":
                values = np.array([float(v) for v in t[2:34]], dtype=np.float32)
                self.poses[int(t[1])] = values[:16].reshape(4, 4)
                self.inverse_poses[int(t[1])] = values[16:32].reshape(4, 4)

    def __len__(self):
        return self.count

    def frame(self, i):
        """(depth [h, w] in metres, colour [h, w, 3] in [0, 1] or None, depth_to_world 4x4)."""
        depth = load_depth(os.path.join(self.directory, "depth_%06d.pgm" % i), self.depth_scale)
        path = os.path.join(self.directory, "color_%06d.ppm" % i)
        color = load_color(path, 1.0 / 255.0) if os.path.exists(path) else None
        return depth, color, self.poses.get(i, np.eye(4, dtype=np.float32))


# ---- maps ---------------------------------------------------------------------------

MAP_MAGIC, MAP_VERSION = b"VULCANMP", 1
MAP_HEADER_BYTES, MAP_BLOCK_BYTES = 32, 512 * 20


def write_map(path, origins, voxels, voxel_length, truncation_length):
    """The packed blocks of a volume (vk_volume_pack, vk.h) as a file, little-endian: the 8-byte magic, int32 version,
    int32 block count, float32 voxel length, float32 truncation length, 8 reserved bytes (zero), then the origins
    (int16 x, y, z, 0 per block) and the voxels (10 240 bytes per block) as the pack holds them. `origins` [n, 4] int16,
    `voxels` any array of n * 10 240 bytes. Not upstream: its Volume never leaves the device (src/volume.cu:17-21)."""
    origins = np.ascontiguousarray(np.asarray(origins, dtype="<i2").reshape(-1, 4))
    body = np.ascontiguousarray(voxels).tobytes()
    if len(body) != len(origins) * MAP_BLOCK_BYTES:
        raise ValueError(f"write_map: {len(origins)} origins and {len(body)} bytes of voxels")
    header = (MAP_MAGIC + np.array([MAP_VERSION, len(origins)], dtype="<i4").tobytes() +
              np.array([voxel_length, truncation_length], dtype="<f4").tobytes() + bytes(8))
    with open(path, "wb") as fh:
        fh.write(header)
        fh.write(origins.tobytes())
        fh.write(body)


def read_map(path):
    """A file of write_map: (origins [n, 4] int16, voxels [n * 10 240] uint8, voxel length, truncation length — both
    np.float32). ValueError for a file that is not one: a wrong magic or version, a negative count, a length that does
    not match the count, a fourth origin component that is not 0, two blocks with one origin (vk_volume_merge_packed
    leaves duplicates undefined) — all on the host, before anything is given to a device."""
    with open(path, "rb") as fh:
        data = fh.read()
    if len(data) < MAP_HEADER_BYTES or data[:8] != MAP_MAGIC:
        raise ValueError(f"{path}: not a map file (magic)")
    version, count = (int(x) for x in np.frombuffer(data, dtype="<i4", count=2, offset=8))
    if version != MAP_VERSION:
        raise ValueError(f"{path}: map file version {version}, this reader knows {MAP_VERSION}")
    if count < 0:
        raise ValueError(f"{path}: block count {count}")
    if len(data) != MAP_HEADER_BYTES + count * (8 + MAP_BLOCK_BYTES):
        raise ValueError(f"{path}: {len(data)} bytes do not hold {count} blocks")
    voxel_length, truncation_length = np.frombuffer(data, dtype="<f4", count=2, offset=16)
    origins = np.frombuffer(data, dtype="<i2", count=4 * count, offset=MAP_HEADER_BYTES).reshape(count, 4).astype(np.int16)
    if (origins[:, 3] != 0).any():
        raise ValueError(f"{path}: an origin's fourth component is not 0")
    if count and len(np.unique(origins, axis=0)) != count:
        raise ValueError(f"{path}: two blocks have the same origin")
    voxels = np.frombuffer(data, dtype=np.uint8, count=count * MAP_BLOCK_BYTES, offset=MAP_HEADER_BYTES + 8 * count).copy()
    return origins, voxels, np.float32(voxel_length), np.float32(truncation_length)
