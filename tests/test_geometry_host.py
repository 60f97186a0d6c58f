"""CPU checks of the geometry metrics (include/ext/geometry.h, freesplat_amd/geometry_metrics.py): the restated grid search of
tests/geometry_ref.py against the brute-force definition on every case, known answers of the metrics, sample_mesh, the C boundary
without a device, and the Python layer's refusals."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import geometry_cases as GC
import geometry_ref as G
from util_abi import declared_names, header_text

HEADER = "ext/geometry.h"
INF, NAN = math.inf, math.nan


# ---- 1. the grid search is the definition ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("cs", [(n, INF) for n in GC.NAMES] + GC.BOUNDED, ids=lambda cs: f"{cs[0]} max_dist={cs[1]}")
def test_the_restated_grid_search_equals_brute_force_bit_for_bit(cs):
    name, max_dist = cs
    c, want = GC.case(name), GC.reference(name, max_dist)
    grid = G.Grid(c["ref"], *GC.grid_params(c["ref"], c["cell"]))
    dist2, index, visited = G.grid_nearest(c["query"], grid, max_dist)
    assert GC.same_bits(dist2, want["dist2"]) and np.array_equal(index, want["index"])
    assert int(visited.max(initial=0)) <= int(G.finite_rows(c["ref"]).sum())


def test_the_case_list_covers_what_the_kernel_branches_on():
    dims = {n: GC.grid_params(GC.case(n)["ref"], GC.case(n)["cell"])[2] for n in GC.NAMES}
    assert dims["one cell 63x257"] == (1, 1, 1) and dims["flat 700x257"][2] == 1 and min(dims["flat 700x257"][:2]) > 1
    assert {GC.case(n)["ref"].shape[0] for n in GC.NAMES} == {1, 63, 700} and {GC.case(n)["query"].shape[0] for n in GC.NAMES} == {1, 257}
    w = GC.reference("walls default cell 700x257")
    assert int((w["dist2"] == 0).sum()) >= 50                                           # queries equal to reference points
    c = GC.case("walls default cell 700x257")
    assert np.unique(c["ref"], axis=0).shape[0] <= 700 - 15                             # duplicated reference points
    far = np.abs(c["query"] - 0.5).max(1)
    assert far.max() > 1.5 and int((far > 0.5).sum()) >= 80                             # queries outside the box, out to 1.6 boxes
    ties = GC.case("lattice ties 63x257")
    d = ((ties["query"][:, None].astype(np.float64) - ties["ref"][None]) ** 2).sum(2)
    assert int(((d == d.min(1, keepdims=True)).sum(1) > 1).sum()) > 100                 # equal minima: the index rule decides
    n = GC.reference("nan and inf rows 63x257")
    assert int(np.isnan(n["dist2"]).sum()) == 5 and (n["index"][np.isnan(n["dist2"])] == -1).all()
    assert not np.isin(n["index"], [0, 7, 20, 41, 62]).any()                            # the dropped reference rows are never named
    e = GC.reference("nothing left 1x257")
    assert np.isinf(e["dist2"]).all() and (e["index"] == -1).all()
    for name, max_dist in GC.BOUNDED:                                                   # a finite bound cuts through every bounded case
        b, u = GC.reference(name, max_dist), GC.reference(name)
        cut = np.isinf(b["dist2"]) & np.isfinite(u["dist2"])
        assert 0 < int(cut.sum()) < int(np.isfinite(u["dist2"]).sum()) and (b["index"][cut] == -1).all(), name
        keep = np.isfinite(b["dist2"])
        assert GC.same_bits(b["dist2"][keep], u["dist2"][keep]) and np.array_equal(b["index"][keep], u["index"][keep])


# ---- 2. known answers of the metrics ----------------------------------------------------------------------------------------------

def _square(n, z, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(0, 1, (n, 2)), np.full((n, 1), z)], 1).astype(np.float32)


def test_two_parallel_squares_are_their_distance_apart():
    """Two parallel unit squares delta apart, the second sampled on the grid the first is sampled on: accuracy = completeness = delta."""
    delta = 0.25
    a = _square(300, 0.0, 0)
    b = a.copy()
    b[:, 2] = np.float32(delta)
    m = G.metrics64(a, b, (0.2, 0.3))
    assert m["accuracy"] == m["completeness"] == m["chamfer"] == delta
    assert m["precision"].tolist() == [0.0, 1.0] and m["recall"].tolist() == [0.0, 1.0] and m["fscore"].tolist() == [0.0, 1.0]
    # independently sampled squares: the in-plane offset to the nearest sample adds at most the sample spacing
    m = G.metrics64(_square(2000, 0.0, 1), _square(2000, delta, 2), (0.3,))
    assert delta <= m["accuracy"] < delta + 0.01 and delta <= m["completeness"] < delta + 0.01


def test_a_cloud_against_itself_and_against_its_half():
    pred, gt = GC.two_clouds()
    m = G.metrics64(gt, gt, (1e-6,))
    assert m["accuracy"] == m["completeness"] == 0.0 and m["precision"][0] == m["recall"][0] == m["fscore"][0] == 1.0
    half = gt[gt[:, 0] < np.median(gt[:, 0])]
    m = G.metrics64(half, gt, (1e-6,))
    assert m["precision"][0] == 1.0 and abs(m["recall"][0] - 0.5) < 0.01 and m["accuracy"] == 0.0 and m["completeness"] > 0.0
    m = G.metrics64(pred, gt, (0.05, 0.2), max_dist=0.5)
    assert m["n_far"][0] == 7 and 0 < m["precision"][0] < m["precision"][1] < 1 and 0 < m["recall"][0] < m["recall"][1] <= 1
    e = G.metrics64(np.zeros((0, 3), np.float32), gt)
    assert math.isnan(e["accuracy"]) and math.isnan(e["completeness"]) and math.isnan(e["chamfer"]) and e["recall"][0] == 0.0


def test_the_fp32_sums_agree_with_the_float64_metrics():
    """What geometry_metrics assembles from the two directions' sums (the fp32 definition) against float64 throughout: 1e-6
    relative, fp32 dist2 being the only fp32 step (its relative error is a few 2^-24), the same integers for the shares."""
    pred, gt = GC.two_clouds()
    th = (0.05, 0.2)
    m = G.metrics64(pred, gt, th, max_dist=0.5)
    a, c = G.sums(G.brute(pred, gt, 0.5)[0], th), G.sums(G.brute(gt, pred, 0.5)[0], th)
    assert abs(a["dist_sum"] / a["n_within"] - m["accuracy"]) <= 1e-6 * m["accuracy"]
    assert abs(c["dist_sum"] / c["n_within"] - m["completeness"]) <= 1e-6 * m["completeness"]
    assert [n / a["n_finite"] for n in a["n_tau"]] == m["precision"].tolist() and [n / c["n_finite"] for n in c["n_tau"]] == m["recall"].tolist()


# ---- 3. sample_mesh on the CPU ----------------------------------------------------------------------------------------------------

def _two_triangles():
    """Areas 1 : 3, apart along x; as an indexed mesh with an unused vertex and a degenerate face."""
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 2, 0], [5, 0, 1], [8, 0, 1], [5, 2, 1], [9, 9, 9]], dtype=torch.float32)
    f = torch.tensor([[0, 1, 2], [3, 3, 4], [3, 4, 5]])
    return v, f


def test_sample_mesh_is_area_weighted_inside_and_reproducible():
    from freesplat_amd.geometry_metrics import sample_mesh
    v, f = _two_triangles()
    n = 20000
    pts, nrm, face = sample_mesh(v, f, n, seed=3, return_normals=True, return_faces=True)
    assert pts.dtype == torch.float32 and tuple(pts.shape) == (n, 3) and tuple(nrm.shape) == (n, 3) and face.dtype == torch.int64
    assert not bool((face == 1).any())                                                  # the degenerate face gets nothing
    k = int((face == 2).sum())
    sigma = math.sqrt(n * 0.75 * 0.25)
    print(f"samples on the larger triangle: {k} of {n}, expected {0.75 * n:.0f} +- {sigma:.1f}")
    assert abs(k - 0.75 * n) <= 5 * sigma                                               # binomial, 5 sigma
    assert bool(((pts[:, 0] > 4) == (face == 2)).all())
    # barycentrics >= 0: the points are float64 combinations rounded to fp32, so a coordinate is off by at most 2^-24 * 9 and a
    # barycentric (a ratio of areas >= 1) by less than 1e-5
    tri = v[f[face]].double()
    p = pts.double()
    area = lambda a, b, c: torch.linalg.cross(b - a, c - a)
    whole = area(tri[:, 0], tri[:, 1], tri[:, 2])
    unit = whole / whole.norm(dim=1, keepdim=True)
    bary = torch.stack([(area(p, tri[:, 1], tri[:, 2]) * unit).sum(1), (area(tri[:, 0], p, tri[:, 2]) * unit).sum(1),
                        (area(tri[:, 0], tri[:, 1], p) * unit).sum(1)], 1) / whole.norm(dim=1, keepdim=True)
    assert float(bary.min()) >= -1e-5 and float((bary.sum(1) - 1).abs().max()) <= 1e-5
    assert float((nrm - torch.tensor([0.0, 0.0, 1.0])).abs().max()) <= 1e-6
    again = sample_mesh(v, f, n, seed=3)
    assert torch.equal(again, pts) and not torch.equal(sample_mesh(v, f, n, seed=4), pts)
    soup = v[f]                                                                         # the soup form gives the same points
    assert torch.equal(sample_mesh(soup, None, n, seed=3), pts)
    assert tuple(sample_mesh(v, f, 0).shape) == (0, 3)


def test_sample_mesh_refusals():
    from freesplat_amd.geometry_metrics import sample_mesh
    v, f = _two_triangles()
    with pytest.raises(ValueError, match="freesplat_amd.geometry_metrics: the mesh has no area"):
        sample_mesh(v, f[1:2], 10)
    with pytest.raises(ValueError, match="freesplat_amd.geometry_metrics: the mesh has no area"):
        sample_mesh(torch.zeros(0, 3, 3), None, 10)
    for bad in (lambda: sample_mesh(v, f.float(), 10), lambda: sample_mesh(v, f[:, :2], 10), lambda: sample_mesh(v[:, :2], f, 10),
                lambda: sample_mesh(v, None, 10), lambda: sample_mesh(v, f + 5, 10), lambda: sample_mesh(v, f, -1),
                lambda: sample_mesh(v.numpy(), f, 10)):
        with pytest.raises(ValueError, match="freesplat_amd.geometry_metrics"):
            bad()


# ---- 4. the C boundary ------------------------------------------------------------------------------------------------------------

P = C.c_void_p(4096)      # a fake non-NULL, 16-byte aligned pointer: nothing may launch with it
GRID = (0.0, 0.0, 0.0, 0.1, 8, 8, 8)


def _tau(*values):
    return (C.c_float * max(len(values), 1))(*values)


def _query(L, Nq=5, query=P, order=None, Nrec=7, rec=P, start=P, grid=GRID, max_d2=INF, n_tau=1, tau=None, out=(P, P, None, None)):
    return L.fs_nn_query(Nq, query, order, Nrec, rec, start, *grid, max_d2, n_tau, _tau(0.01) if tau is None else tau, *out, None)


def _bad_grids():
    g = list(GRID)
    for i in range(3):
        for bad in (NAN, INF, -INF):
            yield tuple(bad if k == i else x for k, x in enumerate(g))
    for bad in (0.0, -1.0, NAN, INF, 1e-31, 1e16):
        yield tuple(bad if k == 3 else x for k, x in enumerate(g))
    for i in (4, 5, 6):
        for bad in (0, -1, 1025):
            yield tuple(bad if k == i else x for k, x in enumerate(g))
    yield (0.0, 0.0, 0.0, 0.1, 1024, 1024, 17)                                          # more than 2^24 cells


def test_geometry_header_is_exported_and_bound():
    from freesplat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    names = declared_names(HEADER)
    assert names == ["fs_geometry_api_version", "fs_nn_grid_gather", "fs_nn_grid_keys", "fs_nn_query", "fs_nn_query_scratch_bytes"]
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/{HEADER} but not exported"
    assert set(_lib.GEOMETRY_SIGNATURES) == set(names)
    assert _lib.lib().fs_geometry_api_version() == _lib.GEOMETRY_API_VERSION
    text = header_text(HEADER)
    for macro, value in (("FS_GEOMETRY_API_VERSION", _lib.GEOMETRY_API_VERSION), ("FS_NN_MAX_SIDE", _lib.NN_MAX_SIDE),
                         ("FS_NN_MAX_THRESHOLDS", _lib.NN_MAX_THRESHOLDS), ("FS_NN_SUM_FINITE", _lib.NN_SUM_FINITE),
                         ("FS_NN_SUM_WITHIN", _lib.NN_SUM_WITHIN), ("FS_NN_SUM_DIST", _lib.NN_SUM_DIST), ("FS_NN_SUM_TAU", _lib.NN_SUM_TAU)):
        assert re.search(rf"#define\s+{macro}\s+{value}\b", text), macro
    assert re.search(r"#define\s+FS_NN_MAX_CELLS\s+\(1 << 24\)", text) and _lib.NN_MAX_CELLS == 1 << 24
    assert _lib.NN_SUM_FIELDS == 3 + _lib.NN_MAX_THRESHOLDS == G_FIELDS
    assert G.MAX_SIDE == _lib.NN_MAX_SIDE and float(G.MARGIN) == 1.0 / 64.0
    # the stream is the last argument of every entry point that launches
    for n in ("fs_nn_grid_keys", "fs_nn_grid_gather", "fs_nn_query"):
        assert re.search(rf"{n}\([^;]*void\* stream\);", re.sub(r"/\*.*?\*/", "", text, flags=re.S)), n


G_FIELDS = 11


def test_the_entry_points_validate_before_touching_a_device():
    """FS_ERR_INVALID_ARG (-1) for every condition the header lists, with fake non-NULL pointers, so nothing may launch; FS_OK (0)
    for an empty job, which launches nothing either."""
    from freesplat_amd import _lib
    L = _lib.lib()
    keys = lambda N=5, pts=P, grid=GRID, out=P: L.fs_nn_grid_keys(N, pts, *grid, out, None)
    assert keys(N=-1) == -1 and keys(pts=None) == -1 and keys(out=None) == -1
    for g in _bad_grids():
        assert keys(grid=g) == -1 and keys(N=0, grid=g) == -1, g
    assert keys(N=0) == 0 and keys(N=0, pts=None, out=None) == 0

    gather = lambda N=5, pts=P, order=P, rec=P: L.fs_nn_grid_gather(N, pts, order, rec, None)
    assert gather(N=-1) == -1 and gather(pts=None) == -1 and gather(order=None) == -1 and gather(rec=None) == -1
    assert gather(rec=C.c_void_p(4100)) == -1                                           # records not 16-byte aligned
    assert gather(N=0) == 0 and gather(N=0, pts=None, order=None, rec=None) == 0

    assert L.fs_nn_query_scratch_bytes(0) == 0 == L.fs_nn_query_scratch_bytes(-4)
    assert L.fs_nn_query_scratch_bytes(1) == L.fs_nn_query_scratch_bytes(256) == 8 * G_FIELDS
    assert L.fs_nn_query_scratch_bytes(257) == 2 * 8 * G_FIELDS and L.fs_nn_query_scratch_bytes(2 ** 31 - 1) == 2 ** 23 * 8 * G_FIELDS

    assert _query(L, Nq=-1) == -1 and _query(L, Nrec=-1) == -1
    assert _query(L, query=None) == -1 and _query(L, start=None) == -1 and _query(L, rec=None) == -1
    assert _query(L, rec=C.c_void_p(4104)) == -1
    for g in _bad_grids():
        assert _query(L, grid=g) == -1 and _query(L, Nq=0, grid=g) == -1, g
    for bad in (NAN, -1.0, -INF):
        assert _query(L, max_d2=bad) == -1, bad
    assert _query(L, n_tau=-1) == -1 and _query(L, n_tau=9, tau=_tau(*[1.0] * 9)) == -1
    assert L.fs_nn_query(5, P, None, 7, P, P, *GRID, INF, 1, None, P, P, None, None, None) == -1      # thresholds without their array
    assert _query(L, n_tau=2, tau=_tau(1.0, NAN)) == -1
    assert _query(L, out=(P, P, P, None)) == -1                                         # sums without scratch
    assert _query(L, out=(None, None, C.c_void_p(4100), P)) == -1 and _query(L, out=(None, None, P, C.c_void_p(4100))) == -1
    assert _query(L, Nq=0) == 0 and _query(L, Nq=0, query=None, start=None, Nrec=0, rec=None, out=(None, None, None, None)) == 0
    assert _query(L, Nq=0, n_tau=0, tau=_tau()) == 0 and _query(L, Nq=0, out=(None, None, P, P)) == 0


# ---- 5. the Python layer ----------------------------------------------------------------------------------------------------------

def test_the_default_cell_and_the_coarsening():
    from freesplat_amd.geometry_metrics import MAX_CELLS, MAX_SIDE, default_cell, grid_dims
    assert default_cell((1.0, 1.0, 1.0), 600) == pytest.approx(0.2) and default_cell((2.0, 3.0, 0.0), 48) == pytest.approx(1.0)
    assert default_cell((4.0, 0.0, 0.0), 8) == pytest.approx(1.0) and default_cell((0.0, 0.0, 0.0), 8) == 1.0
    assert grid_dims((1.0, 1.0, 1.0), 0.25) == (0.25, (5, 5, 5)) and grid_dims((0.0, 0.0, 0.0), 1.0) == (1.0, (1, 1, 1))
    for extent, cell in (((1.0, 1.0, 1.0), 1e-4), ((1000.0, 1.0, 0.0), 0.01), ((1.0, 1.0, 1.0), 1e-30)):
        c, dims = grid_dims(extent, cell)
        assert c >= cell and max(dims) <= MAX_SIDE and dims[0] * dims[1] * dims[2] <= MAX_CELLS
        assert all(d == int(math.floor(e / c)) + 1 for d, e in zip(dims, extent)) and c == float(np.float32(c))


def test_argument_errors_without_a_device():
    from freesplat_amd import geometry_metrics as M
    a, b = torch.rand(10, 3), torch.rand(12, 3)
    for call in (lambda: M.nearest(a, b), lambda: M.NearestGrid(b), lambda: M.geometry_metrics(a, b), lambda: M.nearest_sums(a, b),
                 lambda: M.mesh_metrics(torch.rand(4, 3, 3), None, b, 10)):
        with pytest.raises(ValueError, match="freesplat_amd.geometry_metrics: .*no CPU path"):
            call()
    refused = [(lambda: M.nearest(a, torch.rand(12, 2)), "points must be a point cloud"), (lambda: M.nearest(a[0], b, cell=1.0), "must be a point cloud"),
               (lambda: M.NearestGrid(b, cell=0.0), "cell must be"), (lambda: M.NearestGrid(b, cell=math.inf), "cell must be"),
               (lambda: M.NearestGrid(b, cell=math.nan), "cell must be"), (lambda: M.nearest(a, b, max_dist=-1.0), "max_dist"),
               (lambda: M.nearest(a, b, max_dist=math.nan), "max_dist"), (lambda: M.geometry_metrics(a, b, (0.1, -0.1)), "a threshold"),
               (lambda: M.geometry_metrics(a, b, (math.nan,)), "a threshold"), (lambda: M.geometry_metrics(a, b, 0.1), "thresholds must be"),
               (lambda: M.geometry_metrics(a, b, [0.1] * 9), "at most 8 thresholds"), (lambda: M.geometry_metrics(a, b, cell=-2.0), "cell must be"),
               (lambda: M.nearest(b.numpy(), b), "must be a tensor")]
    for call, what in refused:
        with pytest.raises(ValueError, match=f"freesplat_amd.geometry_metrics: .*{what}"):
            call()
