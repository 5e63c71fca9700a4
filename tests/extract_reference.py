"""The CPU statement of vk_extract_mesh (include/vk.h) in numpy on an oracle.HostVolume, the volumes it is held against the
oracle and the device on, and the builder that makes them. Upstream's extractor stops after the vertices, so the header comment
of oracle/oracle_extract.c and vk.h are the definition; the oracle and the device come from the same hand, and this file is the
second statement of that definition, written from its words:

  - corner c of cube (x, y, z) is lattice point (x + (c & 1), y + (c >> 1 & 1), z + (c >> 2)); a lattice point beyond 7 is a
    voxel of the neighbouring block, found by the chain walk (extract_attributes_reference.Table.find, int16 origins); it is
    KNOWN iff that block is allocated and the voxel's distance_weight != 0; bit c of the cube's state is set when the corner's
    distance is > 0; a cube with an unknown corner is empty;
  - the edges are the classic twelve, as pairs of corners (EDGES below: the classic cube's vertices 0 ... 7 are the corners
    0, 1, 3, 2, 4, 5, 7, 6). An edge belongs to the cube whose corner 0 is its lower end, as that cube's edge 0, 3 or 8 (+x, +y,
    +z): the owner and the axis of an edge follow from its two corners and are not a table of their own here;
  - a vertex sits on every owned edge whose two ends are known and differ in `distance > 0`;
  - the list: all entries with a block in table order, or the visible list without the entries that have none;
  - vertices are numbered by listed block, cube z*64 + y*8 + x, axis x, y, z;
  - the point: voxel (x, y, z) of block o is at (8 * L) * o + L * (xyz + 0.5) per component, moved along its axis by t * L
    with t = d(a) / (d(a) - d(b)), or 0.5 without `interpolate`. float32, every operation a numpy call of its own;
  - a cube that is valid and neither all positive nor all non-positive emits the triangles of its state in table order, each
    corner the vertex of the named edge in that edge's owner; when one of those owners is a block that is not listed the whole
    cube is skipped and counted.

The triangle table is an argument (oracle.mc_triangles); tests/test_extract_reference.py pins it by a property.
Imported by tests, never importing one."""
import numpy as np

import distance_field_reference as DF
import extract_attributes_reference as A
from vulcan_amd import vk_types as T

F = np.float32
CORNERS = [(c & 1, (c >> 1) & 1, c >> 2) for c in range(8)]
_CLASSIC = [0, 1, 3, 2, 4, 5, 7, 6]
EDGES = [(_CLASSIC[a], _CLASSIC[b]) for a, b in ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))]
# (offset of the owner cube, axis) of each edge: the lower end is the corner with the bits both ends share
OWNERS = [(CORNERS[a & b], (a ^ b).bit_length() - 1) for a, b in EDGES]
assert [o for o in range(12) if OWNERS[o][0] == (0, 0, 0)] == [0, 3, 8] and [OWNERS[e][1] for e in (0, 3, 8)] == [0, 1, 2]

# the 9^3 corner lattice of a block, [z, y, x]: which of the eight blocks and which of its voxels hold a lattice point
_Q = np.arange(9)
_LZ, _LY, _LX = np.meshgrid(_Q, _Q, _Q, indexing="ij")
_NEIGHBOUR = ((_LX >> 3) | ((_LY >> 3) << 1) | ((_LZ >> 3) << 2)).reshape(-1)
_VOXEL = ((_LZ & 7) * 64 + (_LY & 7) * 8 + (_LX & 7)).reshape(-1)
_TABLES = {}


def triangle_table(triangles):
    """(count [256], edges [256, 15], used [256, 12]) of a table given as triangles(state) -> [n, 3] edge numbers"""
    if triangles not in _TABLES:
        count, edges, used = np.zeros(256, np.int64), np.zeros((256, 15), np.int64), np.zeros((256, 12), bool)
        for state in range(256):
            rows = np.asarray(triangles(state), dtype=np.int64).reshape(-1)
            count[state] = len(rows) // 3
            edges[state, :len(rows)] = rows
            used[state, rows] = True
        _TABLES[triangles] = (count, edges, used)
    return _TABLES[triangles]


def cubes(hv, entries, table=None):
    """the listed blocks' cubes: (slots [n, 8] pool slots of the block and its seven positive neighbours, known [n, 9, 9, 9],
    distance [n, 9, 9, 9], valid [n, 8, 8, 8], state [n, 8, 8, 8]), lattice and cubes indexed [z, y, x]"""
    table = table or A.Table(hv)
    n = len(entries)
    slots = np.empty((n, 8), dtype=np.int64)
    for i, entry in enumerate(entries):
        o = table.origin[entry]
        for m in range(8):
            slots[i, m] = table.data[entry] if m == 0 else table.find((o[0] + (m & 1), o[1] + ((m >> 1) & 1), o[2] + (m >> 2)))
    at = slots[:, _NEIGHBOUR]
    present = at >= 0
    voxel = np.where(present, at * 512 + _VOXEL[None, :], 0)
    known = (present & (hv.voxels["distance_weight"][voxel] != 0)).reshape(n, 9, 9, 9)
    distance = np.where(present, hv.voxels["distance"][voxel], F(0)).astype(F).reshape(n, 9, 9, 9)
    valid = np.ones((n, 8, 8, 8), bool)
    state = np.zeros((n, 8, 8, 8), np.int64)
    for c, (cx, cy, cz) in enumerate(CORNERS):
        k, d = known[:, cz:cz + 8, cy:cy + 8, cx:cx + 8], distance[:, cz:cz + 8, cy:cy + 8, cx:cx + 8]
        valid &= k
        state |= (k & (d > 0)).astype(np.int64) << c
    return slots, known, distance, valid, state


def mesh_structure(hv, all_allocated, triangles):
    """everything of the mesh that does not depend on `interpolate`: a dict of the listed `entries`, per vertex its place
    `vertex` [n, 3] = (list position, cube, axis), its voxel's `base` point [n, 3] and the distances `da`, `db` at the two ends
    of its edge; `faces` [m, 3] int32 with their places `face` [m, 3] = (list position, cube, state); `skipped`"""
    count, edges, used = triangle_table(triangles)
    entries = A.listed_entries(hv, all_allocated)
    n = len(entries)
    if n == 0:
        return dict(entries=entries, vertex=np.zeros((0, 3), np.int64), base=np.zeros((0, 3), F), da=np.zeros(0, F), db=np.zeros(0, F),
                    faces=np.zeros((0, 3), np.int32), face=np.zeros((0, 3), np.int64), skipped=0)
    table = A.Table(hv)
    slots, known, distance, valid, state = cubes(hv, entries, table)
    listed = np.full(hv.max, -1, dtype=np.int64)               # pool slot -> position in the list
    listed[slots[:, 0]] = np.arange(n)
    owner = np.where(slots >= 0, listed[np.maximum(slots, 0)], -1)

    # vertices
    k0, d0 = known[:, :8, :8, :8], distance[:, :8, :8, :8]
    cut = []
    for axis in range(3):
        cx, cy, cz = CORNERS[1 << axis]
        k1, d1 = known[:, cz:cz + 8, cy:cy + 8, cx:cx + 8], distance[:, cz:cz + 8, cy:cy + 8, cx:cx + 8]
        cut.append(k0 & k1 & ((d0 > 0) != (d1 > 0)))
    block, z, y, x, axis = np.nonzero(np.stack(cut, axis=-1))  # C order: block, cube z*64 + y*8 + x, axis
    vertex_of = np.full((n, 8, 8, 8, 3), -1, dtype=np.int64)
    vertex_of[block, z, y, x, axis] = np.arange(len(block))
    length = F(hv.voxel_length)
    block_length = F(8) * length
    origin = np.array([table.origin[e] for e in entries], dtype=np.int64)
    base = np.empty((len(block), 3), F)
    for k, q in enumerate((x, y, z)):
        base[:, k] = block_length * origin[block, k].astype(F) + length * (q.astype(F) + F(0.5))
    step = np.eye(3, dtype=np.int64)[axis]
    out = dict(entries=entries, vertex=np.stack([block, z * 64 + y * 8 + x, axis], axis=1), base=base, da=distance[block, z, y, x],
               db=distance[block, z + step[:, 2], y + step[:, 1], x + step[:, 0]])

    # faces
    block, z, y, x = np.nonzero(valid & (state != 0) & (state != 255))
    s = state[block, z, y, x]
    edge_vertex = np.empty((len(s), 12), dtype=np.int64)
    for e, ((ox, oy, oz), a) in enumerate(OWNERS):
        qx, qy, qz = x + ox, y + oy, z + oz
        at = owner[block, (qx >> 3) | ((qy >> 3) << 1) | ((qz >> 3) << 2)]
        edge_vertex[:, e] = np.where(at < 0, -2, vertex_of[np.maximum(at, 0), qz & 7, qy & 7, qx & 7, a])
    complete = ~((edge_vertex < 0) & used[s]).any(axis=1)
    block, cube, s, edge_vertex = block[complete], (z * 64 + y * 8 + x)[complete], s[complete], edge_vertex[complete]
    per = count[s]
    of = np.repeat(np.arange(len(s)), per)                     # the cube of every face
    nth = np.arange(len(of)) - np.repeat(np.cumsum(per) - per, per)
    faces = np.stack([edge_vertex[of, edges[s[of], 3 * nth + k]] for k in range(3)], axis=1).astype(np.int32).reshape(-1, 3)
    out.update(faces=faces, face=np.stack([block[of], cube[of], s[of]], axis=1), skipped=int((~complete).sum()))
    return out


def place(structure, voxel_length, interpolate):
    """the points of mesh_structure's vertices: each voxel's point moved along the edge's axis by t * L"""
    da, db, axis = structure["da"], structure["db"], structure["vertex"][:, 2]
    t = da / (da - db) if interpolate else np.full(len(da), F(0.5), F)
    points = structure["base"].copy()
    rows = np.arange(len(da))
    points[rows, axis] = points[rows, axis] + t * F(voxel_length)
    return points


def extract(hv, all_allocated, interpolate, triangles, where=None):
    """(points [n, 3] float32, faces [m, 3] int32, cubes skipped) of vk_extract_mesh. `where`: a dict that receives
    mesh_structure's `entries`, `vertex` and `face`, for a failure message"""
    structure = mesh_structure(hv, all_allocated, triangles)
    if where is not None:
        where.update({key: structure[key] for key in ("entries", "vertex", "face")})
    return place(structure, hv.voxel_length, interpolate), structure["faces"], structure["skipped"]


def state_census(hv, all_allocated=True):
    """[8, 256] how often each state occurs among the valid cubes of the listed blocks, by position class
    (x == 7) | (y == 7) << 1 | (z == 7) << 2"""
    entries = A.listed_entries(hv, all_allocated)
    census = np.zeros((8, 256), dtype=np.int64)
    if entries:
        _, _, _, valid, state = cubes(hv, entries)
        q = (np.arange(8) == 7).astype(np.int64)
        position = (q[None, None, :] | (q[None, :, None] << 1) | (q[:, None, None] << 2))[None].repeat(len(entries), axis=0)
        np.add.at(census, (position[valid], state[valid]), 1)
    return census


# ---- the builder ---------------------------------------------------------------------------------------------------------

def volume_of_blocks(orc, origins, main, excess, voxel_length=0.008, truncation_length=0.04):
    """A HostVolume(main, excess) whose table holds a block at each of `origins`, inserted in order the way the allocator
    links them (volume.cu:304-368): the first block of a bucket in the bucket's main entry, every further one in the next
    entry of the excess range, appended to the end of the bucket's chain; pool slots popped from the free list. The voxels
    stay as initialised: unobserved."""
    hv = orc.HostVolume(main, excess, voxel_length=voxel_length, truncation_length=truncation_length)
    data, link = [-1] * hv.max, [-1] * hv.max
    where = [(0, 0, 0)] * hv.max
    excess_ptr, voxel_ptr = int(hv.counters[T.VK_CTR_EXCESS_PTR]), int(hv.counters[T.VK_CTR_VOXEL_PTR])
    for origin in origins:
        bx, by, bz = (int(c) for c in origin)
        index = ((((bx * A.P1) & A.M32) ^ ((by * A.P2) & A.M32) ^ ((bz * A.P3) & A.M32)) & A.M32) % main
        if data[index] != -1:
            while link[index] != -1:
                index = link[index]
            assert excess_ptr < hv.max, "the excess range is too small for these origins"
            link[index] = excess_ptr
            index, excess_ptr = excess_ptr, excess_ptr + 1
        where[index], data[index] = (bx, by, bz), int(hv.free_voxel_blocks[voxel_ptr])
        voxel_ptr -= 1
    hv.hash_entries["block"]["origin"][:] = np.array(where, dtype=np.int16)
    hv.hash_entries["data"][:], hv.hash_entries["next"][:] = data, link
    hv.counters[T.VK_CTR_EXCESS_PTR], hv.counters[T.VK_CTR_VOXEL_PTR] = excess_ptr, voxel_ptr
    return hv


def set_list(hv, entries):
    """the visible list of `hv` becomes `entries` (hash entry indices)"""
    hv.visible_blocks[:] = 0
    hv.visible_blocks[:len(entries)] = entries
    hv.counters[T.VK_CTR_VISIBLE] = len(entries)
    return hv


def allocated(hv):
    return [int(i) for i in np.nonzero(hv.hash_entries["data"] >= 0)[0]]


def visible_lists(hv, seed=5):
    """{name: entries} of the lists a volume is extracted from: every other block, all of them shuffled, all of them with an
    entry without a block in the middle, none. A list names a block at most once."""
    every = allocated(hv)
    free = [int(i) for i in np.nonzero(hv.hash_entries["data"] < 0)[0]]
    shuffled = [every[i] for i in np.random.default_rng(seed).permutation(len(every))]
    return {"every-other": every[::2], "shuffled": shuffled,
            "with-an-entry-without-a-block": every[:len(every) // 2] + free[:1] + every[len(every) // 2:], "empty": []}


def noise(hv, rng, slots=None, unobserved=0.0):
    """distances uniform in [-1, 1] in every voxel (or those of the pool slots given), observed but for a share"""
    voxels = hv.voxels if slots is None else hv.voxels.reshape(-1, 512)[slots]
    voxels["distance"] = rng.uniform(-1, 1, voxels.shape).astype(F)
    voxels["distance_weight"] = np.where(rng.random(voxels.shape) < unobserved, 0, 1)
    if slots is not None:
        hv.voxels.reshape(-1, 512)[slots] = voxels


# ---- the case volumes: voxel length 0.008, fixed seeds -------------------------------------------------------------------

ATLAS_SIZES = {"long-chains": (257, 512), "mostly-heads": (4093, 128)}
ATLAS_ORIGINS = [(bx - 3, by - 4, bz + 10) for bz in range(8) for by in range(8) for bx in range(8)]
FLT_MIN = F(np.finfo(F).tiny)
_HALF_UP, _ONE_DOWN = np.nextafter(F(0.5), F(1)), np.nextafter(F(1), F(0))
# the values at the ends of the cut edges of `edge-values`: an end is positive or it is not (+0 and -0 are not)
POSITIVE = np.array([1.0, FLT_MIN, 0.5, _HALF_UP, _ONE_DOWN, 0.3], dtype=F)
NOT_POSITIVE = np.array([0.0, -0.0, -1.0, -FLT_MIN, -0.5, -_HALF_UP, -_ONE_DOWN, -0.3], dtype=F)
LONG_LIST_BLOCKS, LONG_LIST_SIZES, TRIP = 8192 + 300, (509, 7990), 8192
INT16_ORIGINS = [(32767, 0, 0), (-32768, 0, 0), (32766, 0, 0), (32767, 0, 0), (-32768, 1, 0), (-32767, 0, -1)]
INT16_GHOST = (32766, 1, 0)
CASES = ("atlas", "atlas-mostly-heads", "atlas-holes", "checkerboard", "edge-values", "int16-edges", "long-list")
STATEMENT_CASES = tuple(name for name in CASES if name != "long-list")
_CASES, _STRUCTURES, _STATEMENTS = {}, {}, {}


def designed_blocks(origins):
    """the blocks whose seven positive neighbours are among `origins`, in the order of `origins`"""
    there = set(origins)
    return [o for o in origins if all((o[0] + cx, o[1] + cy, o[2] + cz) in there for cx, cy, cz in CORNERS)]


def atlas(orc, sizes="long-chains", holes=False, seed=11):
    """8 x 8 x 8 blocks of noise, every voxel observed; the corner cube (7, 7, 7) of the i-th block that has its seven positive
    neighbours gets state 1 + i % 254, by the signs of its eight voxels in eight blocks. `holes`: the second form — about 2 %
    of the voxels unobserved, noise colours and a third of the colour weights zero."""
    hv = volume_of_blocks(orc, ATLAS_ORIGINS, *ATLAS_SIZES[sizes])
    rng = np.random.default_rng(seed)
    slot_of = {tuple(int(c) for c in e["block"]["origin"]): int(e["data"]) for e in hv.hash_entries if e["data"] >= 0}
    noise(hv, rng)
    distance = hv.voxels["distance"]
    distance[distance == 0] = F(0.5)
    for i, (bx, by, bz) in enumerate(designed_blocks(ATLAS_ORIGINS)):
        state = 1 + i % 254
        for c, (cx, cy, cz) in enumerate(CORNERS):
            voxel = slot_of[(bx + cx, by + cy, bz + cz)] * 512 + ((7 + cz) & 7) * 64 + ((7 + cy) & 7) * 8 + ((7 + cx) & 7)
            distance[voxel] = abs(distance[voxel]) if (state >> c) & 1 else -abs(distance[voxel])
    if holes:
        rng = np.random.default_rng(seed + 1)
        hv.voxels["distance_weight"][rng.random(len(hv.voxels)) < 0.02] = 0
        hv.voxels["color"] = rng.random((len(hv.voxels), 3)).astype(F)
        hv.voxels["color_weight"] = np.where(rng.random(len(hv.voxels)) < 1 / 3, 0, rng.integers(1, 17, len(hv.voxels)))
    return hv


def _two_cubed(orc):
    hv = volume_of_blocks(orc, [(bx, by, bz) for bz in range(2) for by in range(2) for bx in range(2)], 3, 8)
    index = np.arange(512)
    even = (((index & 7) + ((index >> 3) & 7) + (index >> 6)) & 1) == 0          # a block is 8 wide: the parity is the voxel's own
    return hv, np.tile(even, hv.max)


def checkerboard(orc):
    """the eight blocks (0..1)^3, +0.5 where x + y + z is even and -0.5 elsewhere, all observed: every edge is cut, block
    (0, 0, 0) holds 3 * 512 vertices and 4 * 512 triangles"""
    hv, even = _two_cubed(orc)
    hv.voxels["distance"] = np.where(even, F(0.5), F(-0.5))
    hv.voxels["distance_weight"] = 1
    return hv


def edge_values(orc, seed=17):
    """the checkerboard's signs, so every edge is cut, with the magnitudes drawn from POSITIVE and NOT_POSITIVE: every pair
    of them ends a cut edge, either way round, along every axis (tests/test_extract_reference.py counts them)"""
    hv, even = _two_cubed(orc)
    rng = np.random.default_rng(seed)
    hv.voxels["distance"] = np.where(even, POSITIVE[rng.integers(0, len(POSITIVE), len(even))],
                                     NOT_POSITIVE[rng.integers(0, len(NOT_POSITIVE), len(even))])
    hv.voxels["distance_weight"] = 1
    return hv


def int16_edges(orc):
    """distance_field_reference.chained: one bucket, blocks at 32767 and -32768 (the far block's neighbour at 32768 truncates
    to -32768 and is found), an origin entered twice, a block that no chain reaches, noise voxels with a third unobserved"""
    return DF.chained(orc, INT16_ORIGINS, ghost=INT16_GHOST)


def long_list_observed(count=LONG_LIST_BLOCKS):
    """the list positions (all allocated, table order) of the 64 observed blocks: both ends of both trips, pairs that are
    neighbours along x, and the rest spread evenly"""
    fixed = [0, 1, TRIP - 2, TRIP - 1, TRIP, TRIP + 1, count - 2, count - 1]
    spread = [int(p) for p in np.linspace(40, count - 40, 64 - len(fixed)).astype(int)]
    positions = sorted(set(fixed + spread))
    assert len(positions) == 64
    return positions


def long_list(orc, seed=23):
    """8192 + 300 blocks, so the two ordered passes of the device take a second trip of 8192 entries; all unobserved but 64
    blocks of noise (a third of their voxels unobserved)"""
    origins = [(i % 22 - 11, (i // 22) % 20 - 7, i // 440 + 3) for i in range(LONG_LIST_BLOCKS)]
    hv = volume_of_blocks(orc, origins, *LONG_LIST_SIZES)
    every = allocated(hv)
    assert len(every) == LONG_LIST_BLOCKS
    slots = hv.hash_entries["data"][[every[p] for p in long_list_observed()]]
    noise(hv, np.random.default_rng(seed), slots=slots, unobserved=1 / 3)
    return hv


def case(orc, name):
    """(volume, {list name: entries}) of a case: built once, only read — but for its visible list, which set_list replaces"""
    if name not in _CASES:
        if name.startswith("atlas"):
            hv = atlas(orc, "mostly-heads" if name == "atlas-mostly-heads" else "long-chains", holes=name == "atlas-holes")
        else:
            hv = {"checkerboard": checkerboard, "edge-values": edge_values, "int16-edges": int16_edges, "long-list": long_list}[name](orc)
        lists = visible_lists(hv) if name in ("atlas", "long-list") else {"backwards": allocated(hv)[::-1]}
        _CASES[name] = (hv, lists)
    return _CASES[name]


def modes(orc, name):
    """the block sources of a case: None (all allocated) and the names of its lists"""
    return [None] + list(case(orc, name)[1])


def statement(orc, name, source, interpolate):
    """(points, faces, skipped, where) of the case from the block source `source` (None: all allocated, or a list's name):
    the numpy statement, the oracle for `long-list`; computed once"""
    key = (name, source, bool(interpolate))
    if key not in _STATEMENTS:
        hv, lists = case(orc, name)
        set_list(hv, lists[source] if source is not None else [])
        if name == "long-list":
            _STATEMENTS[key] = orc.extract_mesh(hv, source is None, interpolate) + ({},)
        else:
            if (name, source) not in _STRUCTURES:
                _STRUCTURES[(name, source)] = mesh_structure(hv, source is None, orc.mc_triangles)
            structure = _STRUCTURES[(name, source)]
            _STATEMENTS[key] = (place(structure, hv.voxel_length, interpolate), structure["faces"], structure["skipped"], structure)
    return _STATEMENTS[key]


def first_difference(got_points, got_faces, want_points, want_faces, where):
    """for a failure message: the first vertex and the first face that differ, with the list position of the block, the cube
    and the axis or state"""
    lines = []
    for what, got, want, names in (("vertex", np.ascontiguousarray(got_points).view(np.uint32), np.ascontiguousarray(want_points).view(np.uint32), "axis"),
                                   ("face", got_faces, want_faces, "state")):
        if got.shape != want.shape:
            lines.append(f"{what}: {len(got)} against {len(want)}")
        rows = min(len(got), len(want))
        different = np.nonzero((got[:rows] != want[:rows]).any(axis=1))[0]
        if len(different):
            i = int(different[0])
            at = where.get(what)
            place = ""
            if at is not None and i < len(at):
                block, cube, last = (int(v) for v in at[i])
                place = f" in listed block {block}, cube {cube} = ({cube & 7}, {(cube >> 3) & 7}, {cube >> 6}), {names} {last}"
            lines.append(f"{what} {i}{place}: {got[i].tolist()} against {want[i].tolist()}; {len(different)} differ")
    return "\n".join(lines) or "equal"
