"""GPU checks of the geometry metrics (include/ext/geometry.h, csrc/nn_grid.hip, freesplat_amd/geometry_metrics.py) against the
brute-force fp32 definition of tests/geometry_ref.py, bit for bit on every query of every case of tests/geometry_cases.py (NaN
compared as "both NaN"): with the queries answered in their own order and in cell order, with a finite max_dist, with and without
the optional outputs, from a misaligned query array, on a side stream, in a captured graph, between guard bands; the sums
against the restatement's integers and math.fsum; geometry_metrics against float64; one fused, extracted, welded and sampled
sphere against analytic points."""
import math

import numpy as np
import pytest
import torch

import geometry_cases as GC
import geometry_ref as G
from guarded_alloc import guarded

pytestmark = pytest.mark.gpu
INF = math.inf
EVERY = [(n, INF) for n in GC.NAMES] + GC.BOUNDED
IDS = lambda cs: f"{cs[0]} max_dist={cs[1]}"


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def _grid(c, dev, place=lambda t: t):
    from freesplat_amd.geometry_metrics import NearestGrid
    return NearestGrid(place(_dev(c["ref"], dev)), c["cell"])


def _assert_nearest(got, want, what):
    dist, index = got
    assert index.dtype == torch.int32 and dist.dtype == torch.float32
    want_dist = np.sqrt(want["dist2"])                                                  # (fp32 sqrt is correctly rounded on both sides)
    assert GC.same_bits(dist.cpu().numpy(), want_dist), f"{what}: dist"
    assert np.array_equal(index.cpu().numpy(), want["index"]), f"{what}: index"


def _assert_sums(got, want, what, rel=1e-12):
    s = want["sums"]
    assert int(got["n_finite"]) == s["n_finite"] and int(got["n_within"]) == s["n_within"], what
    assert got["n_tau"].tolist() == s["n_tau"], what
    err = abs(float(got["dist_sum"]) - s["dist_sum"])
    print(f"{what}: distance sum {float(got['dist_sum'])!r} against fsum {s['dist_sum']!r}")
    assert got["dist_sum"].dtype == torch.float64 and err <= rel * s["dist_sum"], what    # a fixed-order fp64 sum of <= 700 terms


# ---- 1. every case ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sort_queries", [False, True], ids=["query order", "cell order"])
@pytest.mark.parametrize("cs", EVERY, ids=IDS)
def test_nearest_matches_brute_force_bit_for_bit(hip_device, cs, sort_queries):
    from freesplat_amd.geometry_metrics import nearest, nearest_sums
    name, max_dist = cs
    c, want = GC.case(name), GC.reference(name, max_dist)
    grid = _grid(c, hip_device)
    lo, cell, dims = GC.grid_params(c["ref"], c["cell"])
    assert grid.dims == dims and grid.cell == cell and grid.lo == lo
    assert grid.n_points == int(G.finite_rows(c["ref"]).sum()) and grid.n_dropped == c["ref"].shape[0] - grid.n_points
    q = _dev(c["query"], hip_device)
    _assert_nearest(nearest(q, grid, max_dist=max_dist, sort_queries=sort_queries), want, name)
    # dist2 itself, the sums with the outputs ...
    got = nearest_sums(q, grid, GC.THRESHOLDS, max_dist=max_dist, sort_queries=sort_queries, outputs=True)
    assert GC.same_bits(got["dist2"].cpu().numpy(), want["dist2"]) and np.array_equal(got["index"].cpu().numpy(), want["index"])
    _assert_sums(got, want, name)
    # ... and without them: the same bits of the sum
    alone = nearest_sums(q, grid, GC.THRESHOLDS, max_dist=max_dist, sort_queries=sort_queries)
    assert "dist2" not in alone and torch.equal(alone["dist_sum"].view(torch.int64), got["dist_sum"].view(torch.int64))
    assert torch.equal(alone["n_tau"], got["n_tau"]) and int(alone["n_within"]) == int(got["n_within"])


def test_a_reference_tensor_and_a_built_grid_give_the_same(hip_device):
    from freesplat_amd.geometry_metrics import nearest
    name = "walls cell 0.13 700x257"
    c, want = GC.case(name), GC.reference(name)
    q, r = _dev(c["query"], hip_device), _dev(c["ref"], hip_device)
    _assert_nearest(nearest(q, r, cell=c["cell"]), want, "a tensor, the case's cell")
    for cell in (None, 0.05, 0.4, 3.0):                                                 # the grid changes the work, not the result
        _assert_nearest(nearest(q, r, cell=cell), want, f"cell {cell}")
    empty = nearest(q[:0], r)
    assert tuple(empty[0].shape) == (0,) == tuple(empty[1].shape)
    none = nearest(q, r[:0])
    assert bool(torch.isinf(none[0]).all()) and bool((none[1] == -1).all())


# ---- 2. the same bits across conditions -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["walls default cell 700x257", "nan and inf rows 63x257"])
def test_runs_streams_alignments_and_halves_give_the_same_bits(hip_device, name):
    from freesplat_amd.geometry_metrics import nearest, nearest_sums
    c, want = GC.case(name), GC.reference(name)
    grid = _grid(c, hip_device)
    q = _dev(c["query"], hip_device)
    first = nearest_sums(q, grid, GC.THRESHOLDS)
    bits = lambda s: s["dist_sum"].view(torch.int64)
    again = nearest_sums(q, grid, GC.THRESHOLDS)
    assert torch.equal(bits(first), bits(again)) and torch.equal(first["n_tau"], again["n_tau"])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = nearest_sums(q, grid, GC.THRESHOLDS, outputs=True)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(bits(first), bits(on_side)) and GC.same_bits(on_side["dist2"].cpu().numpy(), want["dist2"])
    _assert_sums(on_side, want, "another stream")

    # a misaligned query array: a view that starts one row (12 bytes) into a buffer
    buf = torch.empty(q.shape[0] + 1, 3, device=hip_device)
    view = buf[1:]
    view.copy_(q)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    _assert_nearest(nearest(view, grid), want, "a view offset by one row")
    assert torch.equal(bits(nearest_sums(view, grid, GC.THRESHOLDS)), bits(first))

    # the queries alone against two calls of their halves
    h = q.shape[0] // 2
    a, b = nearest(q[:h], grid), nearest(q[h:], grid)
    _assert_nearest((torch.cat([a[0], b[0]]), torch.cat([a[1], b[1]])), want, "two halves")


# ---- 3. the metrics ----------------------------------------------------------------------------------------------------------------

def _assert_metrics(m, want, rel=1e-6):
    for k in ("accuracy", "completeness", "chamfer"):
        got = float(m[k])
        print(f"{k}: {got!r} against {float(want[k])!r}")
        assert abs(got - want[k]) <= rel * abs(want[k]), k
    for k in ("precision", "recall", "fscore"):
        assert m[k].dtype == torch.float64 and np.allclose(m[k].cpu().numpy(), want[k], rtol=rel, atol=0), k
    assert int(m["n_pred"]) == want["n_pred"] and int(m["n_gt"]) == want["n_gt"] and m["n_far"].tolist() == want["n_far"]


def test_geometry_metrics_match_the_float64_restatement(hip_device):
    from freesplat_amd.geometry_metrics import NearestGrid, geometry_metrics
    pred, gt = GC.two_clouds()
    th = (0.05, 0.2)
    p, g = _dev(pred, hip_device), _dev(gt, hip_device)
    for max_dist in (INF, 0.5):
        want = G.metrics64(pred, gt, th, max_dist)
        assert want["n_far"][0] == (7 if max_dist == 0.5 else 0)
        m = geometry_metrics(p, g, th, max_dist=max_dist)
        assert all(v.device == p.device for k, v in m.items() if k != "thresholds") and m["thresholds"] == th
        _assert_metrics(m, want)
    built = NearestGrid(g)
    _assert_metrics(geometry_metrics(p, built, th, max_dist=0.5), want)               # a prebuilt side
    _assert_metrics(geometry_metrics(NearestGrid(p, 0.3), built, th, max_dist=0.5), want)
    same = geometry_metrics(g, g, (1e-6,))
    assert float(same["accuracy"]) == float(same["completeness"]) == 0.0 and same["fscore"].tolist() == [1.0]
    # rows with NaN take no part; an empty side gives NaN, not an exception
    dirty = torch.cat([p, torch.full((3, 3), math.nan, device=hip_device)])
    _assert_metrics(geometry_metrics(dirty, g, th, max_dist=0.5), want)
    for e in (geometry_metrics(p[:0], g), geometry_metrics(p, g[:0]), geometry_metrics(p[:0], g[:0])):
        assert math.isnan(float(e["accuracy"])) and math.isnan(float(e["completeness"])) and math.isnan(float(e["chamfer"]))


def test_a_fused_sphere_scores_as_the_reference_pipeline_does(hip_device):
    """integrate -> extract_mesh -> weld -> sample_mesh(5000) against 5000 analytic points on the sphere: accuracy and completeness
    below one voxel, F-score at two voxels above 0.95.  (The numpy restatements of the same pipeline give 0.0344 / 0.0342 / 1.0:
    the distances are the sampling density's, sqrt(area / n) = 0.06.)"""
    from freesplat_amd.geometry_metrics import mesh_metrics, sample_mesh
    from freesplat_amd.tsdf import TSDFVolume, weld
    s = GC.sphere_scene()
    vs = s["voxel_size"]
    vol = TSDFVolume(s["origin"], vs, s["dims"], s["trunc"], False, s["max_weight"], device=hip_device)
    vol.integrate(_dev(s["depth"], hip_device), _dev(s["intrinsics"], hip_device), torch.from_numpy(s["c2w"]), near=s["near"], alpha_min=0.0)
    V, F, _ = weld(vol.extract_mesh()[0])
    pts = sample_mesh(V, F, 5000, seed=0)
    assert pts.device == V.device and tuple(pts.shape) == (5000, 3)
    radial = (pts.double() - torch.from_numpy(s["centre"]).to(hip_device)).norm(dim=1) - s["radius"]
    assert float(radial.abs().max()) < vs                                               # the samples lie on the extracted surface
    gt = _dev(GC.sphere_points(5000, s["centre"], s["radius"], 1), hip_device)
    m = mesh_metrics(V, F, gt, 5000, (2 * vs,), seed=0)
    print(f"sphere: accuracy {float(m['accuracy']):.4f}, completeness {float(m['completeness']):.4f}, F-score {float(m['fscore'][0]):.4f}")
    assert float(m["accuracy"]) < vs and float(m["completeness"]) < vs and float(m["fscore"][0]) > 0.95
    want = G.metrics64(pts.cpu().numpy(), gt.cpu().numpy(), (2 * vs,))
    _assert_metrics(m, want)


# ---- 4. guard bands --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fill", ["ff", "garbage"])
@pytest.mark.parametrize("cs", [("walls default cell 700x257", INF), ("nan and inf rows 63x257", 0.5), ("nothing left 1x257", INF), ("single 1x1", INF)], ids=IDS)
def test_nothing_is_written_outside_a_buffer_and_every_element_is_written(hip_device, fill, cs):
    """The grid's arrays, the outputs, the sums and the scratch between guard bands and pre-filled with poison, the clouds between
    NaN guards: no guard byte changes, every output element holds the definition's bits (so none kept its poison and no poison or
    guard was read into a result), the inputs are untouched."""
    from freesplat_amd.geometry_metrics import nearest_sums
    name, max_dist = cs
    c, want = GC.case(name), GC.reference(name, max_dist)
    placed = []
    with guarded(fill) as arena:
        def place(t):
            placed.append((arena.place(t), t))
            return placed[-1][0]
        grid = _grid(c, hip_device, place)
        q = place(_dev(c["query"], hip_device))
        for sort_queries in (False, True):
            got = nearest_sums(q, grid, GC.THRESHOLDS, max_dist=max_dist, sort_queries=sort_queries, outputs=True)
            torch.cuda.synchronize()
            arena.check(f"fs_nn_query, sort_queries={sort_queries}")
            assert GC.same_bits(got["dist2"].cpu().numpy(), want["dist2"]) and np.array_equal(got["index"].cpu().numpy(), want["index"])
            _assert_sums(got, want, f"guarded, fill {fill}")
        for inside, original in placed:
            assert torch.equal(inside.view(torch.int32), original.view(torch.int32))
    assert len(arena.records) >= 6 and len(placed) == 2


# ---- 5. graph capture ------------------------------------------------------------------------------------------------------------

def test_nearest_with_a_built_grid_is_capturable(hip_device):
    """nearest against a prebuilt grid makes no host synchronisation: captured in a graph, the queries replaced, replayed twice."""
    from freesplat_amd.geometry_metrics import nearest
    name = "walls default cell 700x257"
    c, want = GC.case(name), GC.reference(name)
    grid = _grid(c, hip_device)
    q = torch.zeros(257, 3, device=hip_device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for sort_queries in (False, True):
            nearest(q, grid, sort_queries=sort_queries)                                 # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for sort_queries in (False, True):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            got = nearest(q, grid, sort_queries=sort_queries)
        q.copy_(_dev(c["query"], hip_device))
        graph.replay()
        torch.cuda.synchronize()
        _assert_nearest(got, want, "replayed")
        first = got[0].clone()
        graph.replay()
        torch.cuda.synchronize()
        _assert_nearest(got, want, "replayed again")
        assert torch.equal(first.view(torch.int32), got[0].view(torch.int32))
        q.zero_()
