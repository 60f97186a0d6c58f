"""3D geometry metrics between point clouds and meshes on the device: exact nearest neighbours on a uniform grid through
fs_nn_grid_keys / fs_nn_grid_gather / fs_nn_query (libfreesplat_hip.so, include/ext/geometry.h, csrc/nn_grid.hip).  The
definitions are those of DESIGN.md "Geometry metrics":

  nearest   per query q the reference point r with finite coordinates of the smallest d2 = (dx dx + dy dy) + dz dz, d = q - r, in
            fp32 with every operation rounded on its own; of equal ones the smallest index.  The result is that of a loop over the
            whole reference, bit for bit: the grid only decides how much of it a query looks at
  metrics   accuracy = mean distance pred -> gt, completeness = mean distance gt -> pred, chamfer = their mean; per threshold tau
            precision = share of pred points within tau of gt, recall = share of gt points within tau of pred, fscore = their
            harmonic mean (the SimpleRecon / Atlas / TransformerFusion protocol)
  sampling  area-weighted points on a triangle mesh (plain torch, any device): the protocol samples a mesh, it does not measure
            point-to-triangle distances

No autograd: every input is detached, nothing here has a backward.  The nearest-neighbour functions take device tensors only --
there is no CPU / eager path.  Building a NearestGrid reads the cloud's bounds on the host once, the feature's one
synchronisation; a query against a built grid makes none and is capturable in a graph.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch
from torch import Tensor

from . import _args, _lib

MAX_SIDE = _lib.NN_MAX_SIDE
MAX_CELLS = _lib.NN_MAX_CELLS
MAX_THRESHOLDS = _lib.NN_MAX_THRESHOLDS
# nearest(sort_queries=None) sorts the queries by their own cell from this many on.  Measured on an MI355X (bench_geometry.py,
# surface samples in random order): the keys + sort cost 0.085 ms at 200 000 queries and save 0.063 ms of the launch, cost 0.19 ms
# at 1 000 000 and save 0.42 ms; interpolated, the two meet near 270 000.
SORT_QUERIES_FROM = 1 << 18
_NAME = "freesplat_amd.geometry_metrics"


def _shape(t, what: str) -> None:
    if isinstance(t, Tensor):
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{_NAME}: {what} must be a point cloud [N, 3], got {tuple(t.shape)}")
        if t.shape[0] > 2 ** 31 - 1:
            raise ValueError(f"{_NAME}: {what} has {t.shape[0]} points, more than 2^31 - 1")


def _cloud(t, what: str) -> Tensor:
    _shape(t, what)
    return _args.device_f32(t, what, _NAME).detach()


def default_cell(extent, n_points: int) -> float:
    """The cell side NearestGrid picks for `n_points` points in a box of side lengths `extent`: 2 sqrt(S / n) with S the surface
    area of the box.  The clouds this is for are samples of surfaces: n points spread over an area of about S lie about
    sqrt(S / n) apart, so an occupied cell holds a handful of them and the rings 0 and 1 nearly always settle a query.  A box
    without area (a line, one point) takes its longest side / n, one of no size 1."""
    ex, ey, ez = (float(e) for e in extent)
    n = max(int(n_points), 1)
    S = 2.0 * (ex * ey + ey * ez + ez * ex)
    if S > 0.0:
        return 2.0 * math.sqrt(S / n)
    longest = max(ex, ey, ez)
    return 2.0 * longest / n if longest > 0.0 else 1.0


def grid_dims(extent, cell: float):
    """(cell, dims): `cell` coarsened by factors of 1.25 until no side has more than MAX_SIDE cells and there are at most MAX_CELLS
    in all; a side has floor(extent / cell) + 1 cells."""
    cell = float(np.float32(cell))
    while True:
        dims = tuple(int(math.floor(float(e) / cell)) + 1 for e in extent)
        if max(dims) <= MAX_SIDE and dims[0] * dims[1] * dims[2] <= MAX_CELLS:
            return cell, dims
        cell = float(np.float32(cell * 1.25))


class NearestGrid:
    """A reference cloud built for nearest-neighbour queries: NearestGrid(points [N, 3], cell=None).  Reusable across queries.

    n_points  reference points in the grid;  n_dropped  points with a NaN or infinite coordinate, left out
    lo, cell, dims  the grid: cell (ix, iy, iz) covers lo + cell * [i, i + 1) per axis, the outer cells everything beyond
    cell=None takes default_cell() of the cloud's bounding box; either is coarsened by grid_dims()."""

    def __init__(self, points, cell: float | None = None):
        cell = _cell(cell)
        pts = _cloud(points, "points")
        self.device = pts.device
        self.points = pts                                   # (a reference, not a copy: geometry_metrics queries them against the other side)
        N = pts.shape[0]
        self.n_total = N
        lo, hi, dropped = (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0
        if N:
            ok = torch.isfinite(pts).all(1, keepdim=True)
            inf = torch.tensor(math.inf, device=pts.device)
            stats = torch.cat([torch.where(ok, pts, inf).amin(0).double(), torch.where(ok, pts, -inf).amax(0).double(),
                               (~ok).sum().double()[None]]).cpu().tolist()           # the one host synchronisation
            dropped = int(stats[6])
            if dropped < N:
                lo, hi = tuple(stats[0:3]), tuple(stats[3:6])
        self.n_dropped = dropped
        self.n_points = N - dropped
        extent = tuple(h - l for l, h in zip(lo, hi))
        self.lo = lo
        self.cell, self.dims = grid_dims(extent, default_cell(extent, self.n_points) if cell is None else cell)
        if not 1e-30 <= self.cell <= 1e15:
            raise ValueError(f"{_NAME}: a cell of {self.cell!r} is outside [1e-30, 1e15]")
        cells = self.dims[0] * self.dims[1] * self.dims[2]
        self.records = torch.empty(N, 4, device=pts.device)
        if N:
            keys = torch.empty(N, dtype=torch.int32, device=pts.device)
            _lib.launch("fs_nn_grid_keys", N, _lib.ptr(pts), *self.lo, self.cell, *self.dims, _lib.ptr(keys))
            keys, order = torch.sort(keys, stable=True)
            _lib.launch("fs_nn_grid_gather", N, _lib.ptr(pts), _lib.ptr(order), _lib.ptr(self.records))
            self.cell_start = torch.searchsorted(keys, torch.arange(cells + 1, dtype=torch.int32, device=pts.device), out_int32=True)
        else:
            self.cell_start = torch.zeros(cells + 1, dtype=torch.int32, device=pts.device)

    def _grid_args(self):
        return (*self.lo, self.cell, *self.dims)


def _cell(cell):
    if cell is None:
        return None
    cell = float(cell)
    if not (cell > 0.0 and math.isfinite(cell)):
        raise ValueError(f"{_NAME}: cell must be a positive finite number, got {cell!r}")
    return cell


def _scalars(max_dist, thresholds):
    """(max_dist^2, [tau^2]) as the kernel takes them; refuses a negative or NaN value and more than MAX_THRESHOLDS thresholds."""
    try:
        thresholds = tuple(float(t) for t in thresholds)
    except TypeError:
        raise ValueError(f"{_NAME}: thresholds must be a sequence of numbers, got {thresholds!r}") from None
    if len(thresholds) > MAX_THRESHOLDS:
        raise ValueError(f"{_NAME}: at most {MAX_THRESHOLDS} thresholds per call, got {len(thresholds)}")
    return _squares([max_dist], "max_dist")[0], _squares(thresholds, "a threshold")


def _as_grid(ref, cell=None) -> NearestGrid:
    if isinstance(ref, NearestGrid):
        if cell is not None:
            raise ValueError(f"{_NAME}: `cell` belongs to the NearestGrid that was built, not to a query against it")
        return ref
    return NearestGrid(ref, cell)


def _squares(values, what: str):
    """x^2 formed in double and rounded to fp32, for every x."""
    out = []
    for x in values:
        x = float(x)
        if math.isnan(x) or x < 0.0:
            raise ValueError(f"{_NAME}: {what} must not be negative or NaN, got {x!r}")
        with np.errstate(over="ignore"):
            out.append(float(np.float32(x * x)))
    return out


def _query(query: Tensor, grid: NearestGrid, max_dist: float, thresholds, want_dist2: bool, want_index: bool, want_sums: bool,
           sort_queries):
    """One fs_nn_query: (dist2 | None, index | None, sums [NN_SUM_FIELDS] float64 | None)."""
    max_d2, tau2 = _scalars(max_dist, thresholds)
    q = _cloud(query, "query")
    if q.device != grid.device:
        raise ValueError(f"{_NAME}: query lives on {q.device}, the reference on {grid.device}")
    Nq = q.shape[0]
    dist2 = torch.empty(Nq, device=q.device) if want_dist2 else None
    index = torch.empty(Nq, dtype=torch.int32, device=q.device) if want_index else None
    sums = torch.zeros(_lib.NN_SUM_FIELDS, dtype=torch.float64, device=q.device) if want_sums else None
    if Nq == 0:
        return dist2, index, sums
    if sort_queries is None:
        sort_queries = Nq >= SORT_QUERIES_FROM
    order = None
    p = _lib.ptr
    if sort_queries:
        keys = torch.empty(Nq, dtype=torch.int32, device=q.device)
        _lib.launch("fs_nn_grid_keys", Nq, p(q), *grid._grid_args(), p(keys))
        order = torch.sort(keys, stable=True).indices
    scratch = torch.empty(_lib.lib().fs_nn_query_scratch_bytes(Nq) // 8, dtype=torch.float64, device=q.device) if want_sums else None
    tau = (C.c_float * max(len(tau2), 1))(*tau2)
    _lib.launch("fs_nn_query", Nq, p(q), p(order), grid.n_total, p(grid.records), p(grid.cell_start), *grid._grid_args(), max_d2,
                len(tau2), tau, p(dist2), p(index), p(sums), p(scratch))
    return dist2, index, sums


def nearest(query, ref, *, max_dist: float = math.inf, cell: float | None = None, sort_queries: bool | None = None):
    """(dist [Nq] fp32, index [Nq] int32): per query the distance to the nearest point of `ref` (a cloud [Nr, 3] or a NearestGrid)
    and that point's index in the cloud.  dist = sqrt(dist2) of the module docstring's d2.

    A query whose nearest point is farther than max_dist gets (+inf, -1) -- as does every query when the reference has no point
    with finite coordinates --, a query with a NaN or infinite coordinate (NaN, -1).  With max_dist = inf the result is exact for
    every query, at the cost of walking out to the grid's edge for a far outlier; a finite max_dist bounds that walk.
    sort_queries: answer the queries in the order of their own cells (None: from SORT_QUERIES_FROM queries on); the results do not
    depend on it.  No autograd: the inputs are detached."""
    _scalars(max_dist, ())
    _shape(query, "query")
    grid = _as_grid(ref, _cell(cell))
    dist2, index, _ = _query(query, grid, max_dist, (), True, True, False, sort_queries)
    return dist2.sqrt(), index


def nearest_sums(query, ref, thresholds=(), *, max_dist: float = math.inf, cell: float | None = None, sort_queries: bool | None = None,
                 outputs: bool = False):
    """The reduction of one direction: a dict of device scalars n_finite (queries with finite coordinates), n_within (those with a
    neighbour within max_dist), dist_sum (float64 sum of their distances, a fixed association: the same bits on every run and
    stream, with or without `outputs`) and n_tau [len(thresholds)] (those with dist2 <= tau^2, tau^2 formed in double and rounded
    to fp32); with outputs=True also dist2 and index."""
    _scalars(max_dist, thresholds)
    _shape(query, "query")
    grid = _as_grid(ref, _cell(cell))
    dist2, index, s = _query(query, grid, max_dist, thresholds, outputs, outputs, True, sort_queries)
    T = len(tuple(thresholds))
    out = {"n_finite": s[_lib.NN_SUM_FINITE].long(), "n_within": s[_lib.NN_SUM_WITHIN].long(), "dist_sum": s[_lib.NN_SUM_DIST],
           "n_tau": s[_lib.NN_SUM_TAU: _lib.NN_SUM_TAU + T].long()}
    if outputs:
        out["dist2"], out["index"] = dist2, index
    return out


def geometry_metrics(pred, gt, thresholds=(0.05,), *, max_dist: float = math.inf, cell: float | None = None) -> dict:
    """The geometry metrics of a predicted cloud against a ground-truth cloud, as a dict of device scalars (float64):

      accuracy      mean distance from a pred point to the nearest gt point;  completeness  the same from gt to pred
      chamfer       (accuracy + completeness) / 2
      precision, recall, fscore   [len(thresholds)]: the share of pred points within tau of gt, of gt points within tau of pred,
                    and 2 p r / (p + r) (0 when both are 0)
      n_pred, n_gt  points with finite coordinates (the others take no part);  n_far = (pred, gt) points whose nearest
                    neighbour is farther than max_dist

    A point beyond max_dist counts as a miss in precision / recall and is LEFT OUT of the means.  An empty side gives NaN, not an
    exception.  Either side may be a prebuilt NearestGrid (to score many predictions against one ground truth); `cell` applies to
    the sides whose grid is built here.  No autograd: the inputs are detached."""
    _scalars(max_dist, thresholds)
    thresholds, cell = tuple(float(t) for t in thresholds), _cell(cell)
    pred_pts, pred_grid = _side(pred, cell, "pred")
    gt_pts, gt_grid = _side(gt, cell, "gt")
    a = nearest_sums(pred_pts, gt_grid, thresholds, max_dist=max_dist)
    c = nearest_sums(gt_pts, pred_grid, thresholds, max_dist=max_dist)
    accuracy, completeness = a["dist_sum"] / a["n_within"].double(), c["dist_sum"] / c["n_within"].double()
    precision, recall = a["n_tau"].double() / a["n_finite"].double(), c["n_tau"].double() / c["n_finite"].double()
    total = precision + recall
    return {"accuracy": accuracy, "completeness": completeness, "chamfer": 0.5 * (accuracy + completeness),
            "precision": precision, "recall": recall, "fscore": torch.where(total > 0, 2.0 * precision * recall / total, total),
            "n_pred": a["n_finite"], "n_gt": c["n_finite"], "n_far": torch.stack([a["n_finite"] - a["n_within"], c["n_finite"] - c["n_within"]]),
            "thresholds": thresholds}


def _side(x, cell, what: str):
    """A side of geometry_metrics, a cloud or a NearestGrid -> (the points, their grid)."""
    if isinstance(x, NearestGrid):
        return x.points, x
    grid = NearestGrid(x, cell)
    return grid.points, grid


# ---- meshes -------------------------------------------------------------------------------------------------------------------------

def _triangles(vertices, faces) -> Tensor:
    """[T, 3, 3] float64 corner coordinates of an indexed mesh (vertices [V, 3], faces [F, 3]) or of a soup [T, 3, 3] (faces None)."""
    if not isinstance(vertices, Tensor):
        raise ValueError(f"{_NAME}: vertices must be a tensor, got {type(vertices)}")
    v = vertices.detach().to(torch.float64)
    if faces is None:
        if v.dim() != 3 or tuple(v.shape[1:]) != (3, 3):
            raise ValueError(f"{_NAME}: without faces, vertices must be a triangle soup [T, 3, 3], got {tuple(v.shape)}")
        return v
    if not isinstance(faces, Tensor) or faces.dtype.is_floating_point or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{_NAME}: faces must be an integer tensor [F, 3], got {getattr(faces, 'dtype', type(faces))} "
                         f"{tuple(getattr(faces, 'shape', ()))}")
    if v.dim() != 2 or v.shape[1] != 3:
        raise ValueError(f"{_NAME}: vertices must be [V, 3], got {tuple(v.shape)}")
    f = faces.detach().to(device=v.device, dtype=torch.int64)
    if f.numel() and (int(f.min()) < 0 or int(f.max()) >= v.shape[0]):
        raise ValueError(f"{_NAME}: a face names a vertex outside 0 .. {v.shape[0] - 1}")
    return v[f]


def sample_mesh(vertices, faces, n: int, *, seed: int = 0, return_normals: bool = False, return_faces: bool = False):
    """n points [n, 3] fp32 drawn uniformly by area from a triangle mesh: vertices [V, 3] with faces [F, 3] (what tsdf.weld
    returns), or a soup [T, 3, 3] with faces=None (what extract_mesh returns).  A face is drawn by a float64 prefix sum of the
    areas and searchsorted, a point inside it by the square-root map (1 - sqrt(r1), sqrt(r1) (1 - r2), sqrt(r1) r2), from a
    torch.Generator seeded with `seed` on the mesh's device: the same mesh, n, seed and device give the same points.  A face
    without area, or with a NaN or infinite corner, gets weight 0; a mesh whose total area is 0 raises.  Plain torch on any device,
    CPU included; no autograd.  return_normals / return_faces append the unit face normals [n, 3] / the face indices [n]."""
    n = int(n)
    if n < 0:
        raise ValueError(f"{_NAME}: n must not be negative, got {n}")
    tri = _triangles(vertices, faces)
    normal = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    area = 0.5 * normal.norm(dim=1)
    area = torch.where(torch.isfinite(area), area, torch.zeros_like(area))
    cum = area.cumsum(0)
    total = cum[-1] if cum.numel() else cum.new_zeros(())
    if not float(total) > 0.0:
        raise ValueError(f"{_NAME}: the mesh has no area ({tri.shape[0]} faces): nothing to sample")
    g = torch.Generator(device=tri.device).manual_seed(int(seed))
    r = torch.rand(3, n, dtype=torch.float64, device=tri.device, generator=g)
    u = torch.minimum(r[0] * total, torch.nextafter(total, torch.zeros_like(total)))
    face = torch.searchsorted(cum, u, right=True)                       # the first face whose prefix sum exceeds u: never one of area 0
    s = r[1].sqrt()
    b = torch.stack([1.0 - s, s * (1.0 - r[2]), s * r[2]], 1)
    out = [(b[:, :, None] * tri[face]).sum(1).float()]
    if return_normals:
        out.append((normal[face] / (2.0 * area[face])[:, None]).float())
    if return_faces:
        out.append(face)
    return out[0] if len(out) == 1 else tuple(out)


def mesh_metrics(vertices, faces, gt_points, n_samples: int, thresholds=(0.05,), *, seed: int = 0, max_dist: float = math.inf,
                 cell: float | None = None) -> dict:
    """geometry_metrics(sample_mesh(vertices, faces, n_samples, seed=seed), gt_points, ...): the protocol's mesh evaluation."""
    return geometry_metrics(sample_mesh(vertices, faces, n_samples, seed=seed), gt_points, thresholds, max_dist=max_dist, cell=cell)
