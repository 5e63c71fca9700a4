"""The CPU statement of the per-vertex colours and normals of vk_extract_mesh_attributes (include/vk.h), in numpy on an
oracle.HostVolume. Upstream's mesh has neither attribute (src/extractor.cu:320-389 writes positions only,
include/vulcan/mesh.h holds points and faces), so the header comment is the definition and this file states it; the device
is held to it bit for bit (tests/test_gpu_extract_attributes.py).

The vertex order is the oracle's (oracle.extract_mesh): listed blocks in list order, cubes by z*64 + y*8 + x, axes x, y, z.
This file recomputes which edges are cut and asserts that it finds as many vertices as the oracle.

All arithmetic is float32 and every operation is a numpy call of its own, so each result is rounded once — what the
library's -ffp-contract=off build does. `/` and sqrt are IEEE-rounded on both sides."""
import numpy as np

F = np.float32
# the 99th percentile of the angle between a vertex normal and the analytic normal of the 160x120 `sphere` scene, measured by
# tests/test_extract_attributes_reference.py (62.702), rounded up: the full-size GPU test's bound is 1.5 x this figure
ANGLE_P99_DEGREES = 62.71
P1, P2, P3 = 73856093, 19349669, 83492791
M32 = 0xFFFFFFFF


class Table:
    """find_slot (volume.cu:183-190): from the origin's main bucket along `next` until an entry holds the origin or the
    chain ends; that entry's data (-1 for an entry without a block), -1 when none holds it."""

    def __init__(self, hv):
        e = hv.hash_entries
        self.origin = [tuple(int(c) for c in o) for o in e["block"]["origin"]]
        self.data = e["data"].tolist()
        self.next = e["next"].tolist()
        self.main = hv.main
        self.found, self.found_at = {}, {}

    def find(self, origin):
        if origin not in self.found:
            wrapped = tuple(((c + 32768) & 0xFFFF) - 32768 for c in origin)       # entry_is compares int16
            bx, by, bz = origin
            index = ((((bx * P1) & M32) ^ ((by * P2) & M32) ^ ((bz * P3) & M32)) & M32) % self.main
            steps = 0
            while self.origin[index] != wrapped and self.next[index] != -1 and steps < (1 << 24):
                index = self.next[index]
                steps += 1
            self.found[origin] = self.data[index] if self.origin[index] == wrapped else -1
            self.found_at[origin] = index if self.origin[index] == wrapped else -1
        return self.found[origin]


def listed_entries(hv, all_allocated):
    """hash entry indices of the listed blocks, in list order (oracle_extract.c:72-80)"""
    if all_allocated:
        return [int(i) for i in np.nonzero(hv.hash_entries["data"] >= 0)[0]]
    visible = hv.visible_blocks[:int(hv.counters[_visible_counter()])]
    return [int(i) for i in visible if hv.hash_entries["data"][i] >= 0]


def _visible_counter():
    from vulcan_amd import vk_types as T
    return T.VK_CTR_VISIBLE


# the 11^3 lattice -1 ... 9 per axis around a block: which of the 27 blocks and which of its voxels hold lattice point i
_Q = np.arange(-1, 10)
_LZ, _LY, _LX = np.meshgrid(_Q, _Q, _Q, indexing="ij")
_NEIGHBOUR = (((_LX + 8) >> 3) + 3 * ((_LY + 8) >> 3) + 9 * ((_LZ + 8) >> 3)).reshape(-1)
_VOXEL = ((_LZ & 7) * 64 + (_LY & 7) * 8 + (_LX & 7)).reshape(-1)


def extract_attributes(orc, hv, all_allocated, interpolate, statistics=None):
    """(colors [n, 3], normals [n, 3]) float32 of the n vertices of orc.extract_mesh(hv, all_allocated, interpolate).
    `statistics`: a dict that receives how often each rule of the definition was taken."""
    points, _, _ = orc.extract_mesh(hv, all_allocated, interpolate)
    entries = listed_entries(hv, all_allocated)
    table = Table(hv)
    if not entries:
        assert len(points) == 0
        return np.zeros((0, 3), F), np.zeros((0, 3), F)

    # pool slots of the 27 blocks around every listed block; its own is its entry's data, as in the four passes
    slots = np.empty((len(entries), 27), dtype=np.int64)
    for i, entry in enumerate(entries):
        ox, oy, oz = (int(c) for c in hv.hash_entries["block"]["origin"][entry])
        for m in range(27):
            slots[i, m] = table.data[entry] if m == 13 else table.find((ox + m % 3 - 1, oy + (m // 3) % 3 - 1, oz + m // 9 - 1))

    at = slots[:, _NEIGHBOUR]                                     # [blocks, 1331] pool slot of every lattice point
    present = at >= 0
    voxel = np.where(present, at * 512 + _VOXEL[None, :], 0)      # index into hv.voxels
    known = (present & (hv.voxels["distance_weight"][voxel] != 0)).reshape(-1, 11, 11, 11)
    distance = np.where(present, hv.voxels["distance"][voxel], F(0)).astype(F).reshape(-1, 11, 11, 11)
    voxel = voxel.reshape(-1, 11, 11, 11)

    # cut edges: lattice point (x, y, z) is [z + 1, y + 1, x + 1]
    def shifted(a, axis):
        lo = [1, 1, 1]
        lo[2 - axis] = 2
        return a[:, lo[0]:lo[0] + 8, lo[1]:lo[1] + 8, lo[2]:lo[2] + 8]
    ka, da = known[:, 1:9, 1:9, 1:9], distance[:, 1:9, 1:9, 1:9]
    cut = np.stack([ka & shifted(known, axis) & ((da > 0) != (shifted(distance, axis) > 0)) for axis in range(3)], axis=-1)
    block, z, y, x, axis = np.nonzero(cut)                         # C order: block, cube z*64 + y*8 + x, axis
    assert len(block) == len(points), (len(block), len(points))
    step = np.eye(3, dtype=np.int64)[axis]                         # e_axis as (x, y, z)
    a = (block, z + 1, y + 1, x + 1)
    b = (block, z + 1 + step[:, 2], y + 1 + step[:, 1], x + 1 + step[:, 0])

    d0, dc = distance[a], distance[b]
    t = d0 / (d0 - dc) if interpolate else np.full(len(block), F(0.5), F)

    # colour
    va, vb = voxel[a], voxel[b]
    ca, cb = hv.voxels["color"][va], hv.voxels["color"][vb]
    wa, wb = hv.voxels["color_weight"][va] != 0, hv.voxels["color_weight"][vb] != 0
    lerp = ca + t[:, None] * (cb - ca)
    colors = np.zeros((len(block), 3), F)
    colors[wa & wb] = lerp[wa & wb]
    colors[wa & ~wb] = ca[wa & ~wb]
    colors[~wa & wb] = cb[~wa & wb]

    # gradient at a lattice point, component k
    taken = {"central": 0, "forward": 0, "backward": 0, "none": 0}

    def gradient(p, k):
        e = [0, 0, 0]
        e[2 - k] = 1
        after = (p[0], p[1] + e[0], p[2] + e[1], p[3] + e[2])
        before = (p[0], p[1] - e[0], p[2] - e[1], p[3] - e[2])
        ka_, kb_ = known[after], known[before]
        d, da_, db_ = distance[p], distance[after], distance[before]
        g = np.zeros(len(d), F)
        both, fwd, bwd = ka_ & kb_, ka_ & ~kb_, ~ka_ & kb_
        g[both] = ((da_ - db_) * F(0.5))[both]
        g[fwd] = (da_ - d)[fwd]
        g[bwd] = (d - db_)[bwd]
        taken["central"] += int(both.sum())
        taken["forward"] += int(fwd.sum())
        taken["backward"] += int(bwd.sum())
        taken["none"] += int((~ka_ & ~kb_).sum())
        return g

    assert known[a].all() and known[b].all()
    g, own_axis_zero = [], 0
    for k in range(3):
        ga, gb = gradient(a, k), gradient(b, k)
        g.append(ga + t * (gb - ga))
        own_axis_zero += int((((ga == 0) | (gb == 0)) & (axis == k)).sum())     # an endpoint without slope along its own edge
    n2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
    normals = np.zeros((len(block), 3), F)
    positive = n2 > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        length = np.sqrt(n2)
        for k in range(3):
            normals[positive, k] = (g[k] / length)[positive]

    if statistics is not None:
        # lattice points at -1 or 9 that an endpoint's gradient asked for and found unknown because their block is absent
        # what the gradients asked for beyond the block's own 8^3: lattice points -1 and 8 whose block is absent, and
        # lattice points 9 that are unknown (9 is asked for only from b = 8 along the edge, so its block is b's: present)
        there = present.reshape(-1, 11, 11, 11)
        absent_low = absent_high = unknown_9 = 0
        for p in (a, b):
            for k in range(3):
                for sign in (-1, 1):
                    q = [p[1], p[2], p[3]]
                    q[2 - k] = q[2 - k] + sign
                    at_q = (p[0], q[0], q[1], q[2])
                    absent_low += int(((q[2 - k] == 0) & ~there[at_q]).sum())
                    absent_high += int(((q[2 - k] == 9) & ~there[at_q]).sum())
                    unknown_9 += int(((q[2 - k] == 10) & ~known[at_q]).sum())
        # blocks with a vertex whose neighbour at (-1, -1, -1) is found behind entry 0 of its chain
        with_vertices = np.unique(block)
        past_entry_0 = 0
        for i in with_vertices:
            origin = tuple(int(c) - 1 for c in hv.hash_entries["block"]["origin"][entries[i]])
            past_entry_0 += 1 if table.found_at.get(origin, -1) >= hv.main else 0
        statistics.update(vertices=len(block), color_both=int((wa & wb).sum()), color_one=int((wa ^ wb).sum()),
                          color_none=int((~wa & ~wb).sum()), gradient=taken, absent_low=absent_low, absent_high=absent_high, unknown_9=unknown_9,
                          corner_neighbour_past_entry_0=past_entry_0, blocks_with_vertices=len(with_vertices),
                          zero_normals=int((~positive).sum()), own_axis_zero=own_axis_zero, blocks=len(entries))
    return colors, normals


# ---- the states the CPU and the GPU tests start from ---------------------------------------------------------------

W, H = 160, 120
MAIN, EXCESS = 8192, 2048
_FUSED = {}


def projection():
    from vulcan_amd import vk_types as T
    return T.Projection.make(136, 136, 80, 60)


def scene(name):
    """(depth, pose) of the scenes of tests/test_gpu_extract.py"""
    import scenes
    from vulcan_amd import vk_types as T
    if name == "plane":
        return scenes.plane(W, H, 1.5), T.Transform.identity()
    if name == "sphere":
        y, x = np.mgrid[0:H, 0:W]
        r2 = (x - 80.0) ** 2 + (y - 60.0) ** 2
        depth = np.where(r2 < 50.0 ** 2, 2.0 - 0.6 * np.sqrt(np.maximum(50.0 ** 2 - r2, 0)) / 50.0, 0.0).astype(np.float32)
        return depth, T.Transform.identity()
    assert name == "ripple-tilted"
    return (scenes.ripple(W, H) * 1.3).astype(np.float32), scenes.tracer_test_pose()


def clone(orc, hv):
    out = orc.HostVolume(hv.main, hv.excess, voxel_length=hv.voxel_length, truncation_length=hv.truncation_length,
                         depth_range=hv.depth_range)
    for name in ("voxels", "hash_entries", "free_voxel_blocks", "allocation_types", "allocation_blocks", "block_visibility",
                 "visible_blocks", "counters"):
        getattr(out, name)[:] = getattr(hv, name)
    return out


def fused(orc, name):
    """the scene with checker_color(w, h, 0.1, 0.9), six SetView calls and three depth + colour integrations on the oracle in
    HostVolume(8192, 2048) at 8 mm (the `fused` of tests/test_gpu_extract.py): computed once, handed out as copies"""
    if name not in _FUSED:
        import scenes
        depth, pose = scene(name)
        frame = orc.HostFrame(depth, projection(), pose, color=scenes.checker_color(W, H, 0.1, 0.9))
        hv = orc.HostVolume(MAIN, EXCESS, voxel_length=0.008, truncation_length=0.04)
        for _ in range(6):
            hv.set_view(frame, orc.POLICY_MAXKEY)
        for _ in range(3):
            orc.integrate_depth(hv, frame)
            orc.integrate_color(hv, frame)
        _FUSED[name] = hv
    return clone(orc, _FUSED[name])


def blocks_with_vertices(orc, hv):
    """{origin: hash entry index} of the allocated blocks that own a vertex (all_allocated, interpolated)"""
    out = {}
    entries = listed_entries(hv, True)
    for entry in entries:
        slot = int(hv.hash_entries["data"][entry])
        v = hv.voxels[slot * 512:(slot + 1) * 512]
        seen = v["distance_weight"] != 0
        if seen.any() and (v["distance"][seen] > 0).any() and not (v["distance"][seen] > 0).all():
            out[tuple(int(c) for c in hv.hash_entries["block"]["origin"][entry])] = entry
    return out


DOCTORED = ("color-weights", "distance-slab", "unlinked-neighbour", "corner-neighbour-in-excess")


def doctored(orc, kind):
    """the fused `sphere` volume with one edit that sends the definition down a rule the fused scenes rarely take"""
    from vulcan_amd import vk_types as T
    hv = fused(orc, "sphere")
    index = np.arange(len(hv.voxels))
    x, y, z = index & 7, (index >> 3) & 7, (index >> 6) & 7
    if kind == "color-weights":
        # a checker of 2x2x2 cells without a colour: edges inside a cell have both ends or neither, edges between cells one
        hv.voxels["color_weight"][(((x >> 1) + (y >> 1) + (z >> 1)) & 1) == 1] = 0
    elif kind == "distance-slab":
        # the voxels one to two steps in front of the surface (a voxel is 0.2 of the truncation length) become unobserved:
        # the cut edges stay, the central differences across the slab do not
        d = hv.voxels["distance"]
        hv.voxels["distance_weight"][(d > 0.25) & (d < 0.45)] = 0
    elif kind == "unlinked-neighbour":
        # a block with vertices between two others along x leaves the table (its chain stays whole); another one leaves
        # the visible list only, so the cubes that need its vertices are skipped there
        owners = blocks_with_vertices(orc, hv)
        middle = [o for o in sorted(owners) if (o[0] - 1, o[1], o[2]) in owners and (o[0] + 1, o[1], o[2]) in owners]
        gone, unlisted = middle[len(middle) // 2], middle[len(middle) // 4]
        e = hv.hash_entries
        entry = owners[gone]
        before = np.nonzero(e["next"] == entry)[0]
        if len(before):                                          # an excess entry: its predecessor links past it
            e["next"][before[0]] = e["next"][entry]
            e["next"][entry] = -1
        e["data"][entry] = -1
        e["block"]["origin"][entry] = 0
        count = int(hv.counters[T.VK_CTR_VISIBLE])
        visible = [int(i) for i in hv.visible_blocks[:count] if int(i) not in (entry, owners[unlisted])]
        hv.visible_blocks[:len(visible)] = visible
        hv.counters[T.VK_CTR_VISIBLE] = len(visible)
    else:
        assert kind == "corner-neighbour-in-excess"
        # the (-1, -1, -1) neighbour of a block with vertices moves from its main entry to a fresh excess entry; the main
        # entry keeps the chain's head as an entry without a block and with an origin nobody asks for
        owners = blocks_with_vertices(orc, hv)
        table = Table(hv)
        e = hv.hash_entries
        at = int(hv.counters[T.VK_CTR_EXCESS_PTR])
        moved = 0
        for origin in sorted(owners):
            corner = (origin[0] - 1, origin[1] - 1, origin[2] - 1)
            table.find(corner)
            home = table.found_at[corner]
            if 0 <= home < hv.main and table.data[home] >= 0 and table.next[home] == -1 and at < hv.max:
                e[at] = e[home]
                hv.block_visibility[at] = hv.block_visibility[home]
                e["block"]["origin"][home] = (32000, 32000, 32000)
                e["data"][home], e["next"][home] = -1, at
                at, moved = at + 1, moved + 1
                table = Table(hv)
                if moved == 8:
                    break
        assert moved == 8
        hv.counters[T.VK_CTR_EXCESS_PTR] = at
    return hv
