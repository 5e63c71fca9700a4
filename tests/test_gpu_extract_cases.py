"""vk_extract_mesh and vk_extract_mesh_attributes on the device against the numpy statement of extraction
(tests/extract_reference.py) on its case volumes: every cube state at every position of a block and the five-triangle states
(`atlas`, at two table sizes), a block with the most vertices it can hold (`checkerboard`), the values at which the vertex
arithmetic can differ (`edge-values`), the ends of the int16 block range (`int16-edges`) and a list longer than a trip of the
ordered passes (`long-list`, against the oracle). tests/test_extract_reference.py asserts that the volumes are what they are said
to be and that the statement equals the oracle. The volume is an uploaded oracle state; points are compared as uint32, faces and
counts exactly; every output and the workspace are overwritten before the call and end in a guard tail that has to keep its
pattern."""
import numpy as np
import pytest

import extract_attributes_reference as A
import extract_reference as X
from gpu_support import api, assert_untouched, device_copy, overwrite, sync  # noqa: F401

pytestmark = pytest.mark.gpu

TAIL = 64                         # guard elements behind every output and the workspace
_DEVICE = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def device(api, orc, name):
    """(host volume, its lists, device copy) of a case: uploaded once, only read but for the visible list"""
    if name not in _DEVICE:
        hv, lists = X.case(orc, name)
        _DEVICE[name] = (hv, lists, device_copy(api, hv))
    return _DEVICE[name]


def use(dv, hv, lists, source):
    """the block source of the next calls: None (all allocated) or the name of a list, which becomes the visible list of both"""
    import torch
    X.set_list(hv, lists[source] if source is not None else [])
    dv.visible_blocks.copy_(torch.from_numpy(hv.visible_blocks).to(dv.visible_blocks.device))
    dv.counters.copy_(torch.from_numpy(hv.counters).to(dv.counters.device))
    return source is None


class Buffers:
    """guarded, overwritten outputs of `points` and `faces` rows, counts and a workspace; what they held before the call"""

    def __init__(self, api, dv, points, faces, fill="ones", colors=False, normals=False, workspace=None):
        import torch
        size = int(api.lib().vk_extract_workspace_bytes(dv.main, dv.excess))
        assert size > 0
        self.rows = {"points": points, "faces": faces, "colors": points, "normals": points}
        self.tensors = {"points": torch.empty(3 * points + TAIL, dtype=torch.float32, device="cuda"),
                        "faces": torch.empty(3 * faces + TAIL, dtype=torch.int32, device="cuda"),
                        "counts": torch.empty(4 + TAIL, dtype=torch.int32, device="cuda"),
                        "colors": torch.empty(3 * points + TAIL, dtype=torch.float32, device="cuda") if colors else None,
                        "normals": torch.empty(3 * points + TAIL, dtype=torch.float32, device="cuda") if normals else None,
                        "workspace": workspace if workspace is not None else torch.empty(size + TAIL, dtype=torch.uint8, device="cuda")}
        for seed, (name, tensor) in enumerate(self.tensors.items()):
            if tensor is not None and not (name == "workspace" and workspace is not None):
                overwrite(tensor, fill, 31 + seed)
        self.before = {name: None if t is None else t.clone() for name, t in self.tensors.items()}

    def call(self, api, dv, all_allocated, interpolate, point_capacity=None, face_capacity=None):
        t = self.tensors
        point_capacity = self.rows["points"] if point_capacity is None else point_capacity
        face_capacity = self.rows["faces"] if face_capacity is None else face_capacity
        if t["colors"] is None and t["normals"] is None:
            status = api.lib().vk_extract_mesh(api._ref(dv.desc()), int(all_allocated), int(interpolate), api._ptr(t["points"]), point_capacity,
                                               api._ptr(t["faces"]), face_capacity, api._ptr(t["counts"]), api._ptr(t["workspace"]), api.stream())
        else:
            status = api.lib().vk_extract_mesh_attributes(api._ref(dv.desc()), int(all_allocated), int(interpolate), api._ptr(t["points"]),
                                                          api._ptr(t["colors"]), api._ptr(t["normals"]), point_capacity, api._ptr(t["faces"]),
                                                          face_capacity, api._ptr(t["counts"]), api._ptr(t["workspace"]), api.stream())
        api.check(status, "vk_extract_mesh")
        sync()
        self.capacity = {"points": point_capacity, "faces": face_capacity, "colors": point_capacity, "normals": point_capacity}
        return self.tensors["counts"][:4].cpu().numpy()

    def written(self, name, rows):
        """the first `rows` rows of an output, after asserting that nothing at or past the capacity was written — the rest of
        the buffer and the guard tail hold what they held"""
        import torch
        tensor, before, capacity = self.tensors[name], self.before[name], self.capacity[name]
        kept = min(rows, capacity)
        assert torch.equal(tensor[3 * kept:].view(torch.uint8), before[3 * kept:].view(torch.uint8)), f"{name}: written at or past the capacity or the total"
        return tensor[:3 * kept].cpu().numpy().reshape(kept, 3)

    def assert_tails(self):
        import torch
        for name in ("counts", "workspace"):
            assert torch.equal(self.tensors[name][-TAIL:].view(torch.uint8), self.before[name][-TAIL:].view(torch.uint8)), f"{name}: guard tail written"


def assert_is_statement(b, counts, want, listed, what):
    """counts and the written prefixes of points and faces are the statement's"""
    want_points, want_faces, want_skipped, where = want
    got_points, got_faces = b.written("points", len(want_points)), b.written("faces", len(want_faces))
    b.assert_tails()
    assert counts.tolist() == [len(want_points), len(want_faces), want_skipped, listed], (what, counts.tolist())
    message = f"{what}\n" + X.first_difference(got_points, got_faces, want_points[:len(got_points)], want_faces[:len(got_faces)], where)
    assert np.array_equal(bits(got_points), bits(want_points[:len(got_points)])), message
    assert np.array_equal(got_faces, want_faces[:len(got_faces)]), message


@pytest.mark.parametrize("name", X.CASES)
def test_the_case_volumes_bit_for_bit(api, orc, name):
    """every block source and both vertex rules; `atlas` and `atlas-mostly-heads` are the two table sizes — the vertex order
    follows the table order, so each is held to its own statement"""
    hv, lists, dv = device(api, orc, name)
    for source in X.modes(orc, name):
        for interpolate in (1, 0):
            want = X.statement(orc, name, source, interpolate)
            all_allocated = use(dv, hv, lists, source)
            b = Buffers(api, dv, len(want[0]), len(want[1]))
            counts = b.call(api, dv, all_allocated, interpolate)
            listed = len(A.listed_entries(hv, all_allocated))
            print(name, source, interpolate, counts.tolist())
            assert_is_statement(b, counts, want, listed, f"{name}, list {source}, interpolate {interpolate}")
            assert_untouched(dv, hv)
    assert dv.host_voxels().tobytes() == hv.voxels.tobytes()


def test_the_attributes_of_the_atlas_with_holes(api, orc):
    hv, lists, dv = device(api, orc, "atlas-holes")
    for source, interpolate in ((None, 1), ("backwards", 0)):
        want = X.statement(orc, "atlas-holes", source, interpolate)
        all_allocated = use(dv, hv, lists, source)
        want_colors, want_normals = A.extract_attributes(orc, hv, all_allocated, interpolate)
        n, m = len(want[0]), len(want[1])
        assert len(want_colors) == len(want_normals) == n
        for colors, normals in ((True, True), (False, True), (True, False)):          # and null colours, null normals in turn
            b = Buffers(api, dv, n, m, colors=colors, normals=normals)
            counts = b.call(api, dv, all_allocated, interpolate)
            assert_is_statement(b, counts, want, 512, f"attributes, list {source}, colours {colors}, normals {normals}")
            for given, attribute, expected in ((colors, "colors", want_colors), (normals, "normals", want_normals)):
                if given:
                    got = b.written(attribute, n)
                    different = np.nonzero((bits(got) != bits(expected)).any(axis=1))[0]
                    assert not len(different), (attribute, source, len(different), different[:5], want[3]["vertex"][different[:5]])
    assert_untouched(dv, hv)


CAPACITIES = ("total", "total - 1", "1", "0")


@pytest.mark.parametrize("name", ["checkerboard", "atlas"])
def test_capacities(api, orc, name):
    """each capacity in turn at the exact total, one less, 1 and 0, the other at its total: counts report the full totals, the
    written prefix is the statement's, nothing at or past the capacity is written"""
    hv, lists, dv = device(api, orc, name)
    want = X.statement(orc, name, None, 1)
    use(dv, hv, lists, None)
    n, m = len(want[0]), len(want[1])
    for which in ("points", "faces"):
        for capacity in CAPACITIES:
            total = n if which == "points" else m
            value = {"total": total, "total - 1": total - 1, "1": 1, "0": 0}[capacity]
            b = Buffers(api, dv, n, m)
            counts = b.call(api, dv, 1, 1, point_capacity=value if which == "points" else n, face_capacity=value if which == "faces" else m)
            assert_is_statement(b, counts, want, len(X.allocated(hv)), f"{name}: {which} capacity {capacity}")
            assert len(b.written(which, total)) == value


@pytest.mark.parametrize("fill", ["ones", "noise"])
def test_dirty_buffers_and_a_workspace_used_twice(api, orc, fill):
    """the workspace, counts and the outputs hold 0xFF or noise before the call: the result is the same; a second call on the
    workspace the first one left, from the other block source, is held to its own statement too"""
    hv, lists, dv = device(api, orc, "atlas")
    all_allocated = use(dv, hv, lists, "every-other")
    want = X.statement(orc, "atlas", "every-other", 1)
    first = Buffers(api, dv, len(want[0]), len(want[1]), fill=fill)
    counts = first.call(api, dv, all_allocated, 1)
    assert counts[2] > 0
    assert_is_statement(first, counts, want, len(lists["every-other"]), f"every-other, {fill}")
    want = X.statement(orc, "atlas", None, 1)
    second = Buffers(api, dv, len(want[0]), len(want[1]), fill=fill, workspace=first.tensors["workspace"])
    second.before["workspace"] = first.before["workspace"]
    counts = second.call(api, dv, 1, 1)
    assert_is_statement(second, counts, want, 512, f"all allocated on the workspace of every-other, {fill}")
    want = X.statement(orc, "atlas", "every-other", 0)
    third = Buffers(api, dv, len(want[0]), len(want[1]), fill=fill, workspace=first.tensors["workspace"])
    third.before["workspace"] = first.before["workspace"]
    counts = third.call(api, dv, 0, 0)
    assert_is_statement(third, counts, want, len(lists["every-other"]), f"every-other on the workspace of all allocated, {fill}")
