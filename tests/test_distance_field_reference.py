"""The CPU statement of the clearance field (tests/distance_field_reference.py) against the definition's own words, and the
case grids against the outcomes they are there to reach: the separable passes equal a brute force over all sites, every grid
holds all three classes, finite distances and cells beyond the cap, the signed field is negative exactly on sites."""
import numpy as np
import pytest

import distance_field_reference as DF
import merge_reference as M
import register_reference as RR
from vulcan_amd import api

_STATE = {}


def volume(orc):
    if "hv" not in _STATE:
        hv = M.view_state(orc, "a", 509, 4096)
        _STATE["hv"] = (hv, RR.block_table(hv))
    return _STATE["hv"]


def statement(orc, name):
    if name not in _STATE:
        hv, table = volume(orc)
        origin, dims, stride, max_cells = DF.GRIDS[name]
        _STATE[name] = DF.distance_field(hv, origin, dims, stride, max_cells, table=table)
    return _STATE[name]


@pytest.mark.parametrize("site_mask", [4, 1, 3])
def test_the_passes_equal_the_brute_force(orc, site_mask):
    hv, table = volume(orc)
    origin, dims, stride = DF.SMALL
    classes = DF.classify(hv, origin, dims, stride, table=table)
    sites = int(((classes & site_mask) != 0).sum())
    for max_cells in (3, 7, 256):
        got, want = DF.transform(classes, site_mask, max_cells), DF.brute_force(classes, site_mask, max_cells)
        finite = want != DF.BEYOND
        print("mask", site_mask, "cap", max_cells, "sites", sites, "finite", int(finite.sum()), "beyond", int((~finite).sum()))
        assert np.array_equal(got, want)
    assert sites > 100
    small = DF.brute_force(classes, site_mask, 3)
    # (unknown or free cells are within three cells of every cell of this grid: mask 3 has no cell beyond)
    assert (small != DF.BEYOND).any() and ((small == DF.BEYOND).any() or site_mask == 3)


# what the issue measured on the stride-1 grid, as lower bounds: a case cannot pass empty
LEAST = {"stride-1": (1_000_000, 100_000, 50_000, 500_000, 500_000), "stride-2": (10_000, 1000, 1000, 1000, 1000),
         "stride-4": (1000, 100, 100, 100, 100), "ragged": (1000, 1000, 1000, 1000, 0)}


@pytest.mark.parametrize("name", list(DF.GRIDS))
def test_a_case_grid_reaches_every_outcome(orc, name):
    classes, d2, distance = statement(orc, name)
    counts = [int((classes == c).sum()) for c in (DF.UNKNOWN, DF.FREE, DF.OCCUPIED)]
    finite = int(((d2 != DF.BEYOND) & (d2 != 0)).sum())
    beyond = int((d2 == DF.BEYOND).sum())
    print(name, "unknown, free, occupied", counts, "finite non-zero", finite, "beyond", beyond)
    least = LEAST[name]
    assert sum(counts) == classes.size
    assert counts[0] >= least[0] and counts[1] >= least[1] and counts[2] >= least[2]
    assert finite >= least[3] and beyond >= least[4]
    if name == "ragged":
        assert beyond == 0
    assert np.array_equal(d2 == 0, classes == DF.OCCUPIED)
    assert np.array_equal(np.isinf(distance), d2 == DF.BEYOND) and (distance >= 0).all()
    max_cells = DF.GRIDS[name][3]
    assert d2[d2 != DF.BEYOND].max() <= max_cells * max_cells


def test_the_signed_field_is_negative_exactly_on_sites(orc):
    hv, _ = volume(orc)
    origin, dims, stride, max_cells = DF.GRIDS["stride-2"]
    classes = statement(orc, "stride-2")[0]
    for site_mask in (4, 6):
        _, distance = DF.field(classes, site_mask, max_cells, stride, hv.voxel_length, signed=True)
        sites = (classes & site_mask) != 0
        assert np.array_equal(distance < 0, sites) and sites.any() and not sites.all()
        inside = DF.transform(classes, 7 ^ site_mask, max_cells)
        assert inside[sites].min() >= 1 and (inside[~sites] == 0).all()
        assert (distance[sites] <= -np.float32(stride) * np.float32(hv.voxel_length)).all()


def test_a_coarser_cell_is_the_union_of_its_voxels(orc):
    fine, coarse = statement(orc, "stride-1")[0], statement(orc, "stride-4")[0]
    nz, ny, nx = coarse.shape
    groups = fine.reshape(nz, 4, ny, 4, nx, 4)
    occupied = (groups == DF.OCCUPIED).any(axis=(1, 3, 5))
    observed = (groups != DF.UNKNOWN).any(axis=(1, 3, 5))
    assert np.array_equal(coarse, np.where(occupied, DF.OCCUPIED, np.where(observed, DF.FREE, DF.UNKNOWN)))


@pytest.mark.parametrize("stride", [1, 2, 4, 8])
def test_grid_for_box_covers_its_box_and_is_aligned(stride):
    rng = np.random.default_rng(5)
    voxel = 0.008
    for _ in range(50):
        lo = rng.uniform(-2, 2, 3)
        hi = lo + rng.uniform(0, 1.5, 3)
        origin, dims = api.grid_for_box(lo, hi, stride, voxel)
        assert (origin, dims) == DF.grid_for_box(lo, hi, stride, voxel)
        origin, dims = np.array(origin), np.array(dims)
        assert (origin % stride == 0).all() and (dims >= 1).all()
        cell = stride * voxel
        assert (origin * voxel <= lo + 1e-12).all() and ((origin + stride * dims) * voxel >= hi - 1e-12).all()
        # the smallest: a cell less on either side no longer covers
        assert ((origin + stride) * voxel > lo - 1e-9).all() and ((origin + stride * (dims - 1)) * voxel <= hi + 1e-9).all()
        assert cell > 0
