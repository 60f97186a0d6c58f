"""numpy restatement of include/ext/geometry.h and freesplat_amd/geometry_metrics.py (test infrastructure only):

  brute(query, ref, max_dist)      the DEFINITION: a loop over the whole reference in fp32, every operation rounded on its own
                                   (numpy float32 arrays round per operation), the smallest index among equal minima
  Grid / grid_nearest              the grid algorithm of the header (cell formula, stable sort by key, Chebyshev rings, the stop
                                   rules), with a counter of the reference points a query visited
  sums / metrics64                 the reductions on the fp32 result, and the metrics in float64 from the coordinates
"""
import math

import numpy as np

F32 = np.float32
MARGIN = F32(1.0 / 64.0)
MAX_SIDE = 1024


def square32(x: float) -> np.float32:
    """x^2 formed in double and rounded to fp32 (how max_dist and the thresholds reach the kernel)."""
    with np.errstate(over="ignore"):
        return F32(float(x) * float(x))


def finite_rows(p):
    return np.isfinite(p).all(1)


def _d2(q, r):
    """(dx dx + dy dy) + dz dz in fp32 for one query against rows r [M, 3]."""
    with np.errstate(over="ignore", invalid="ignore"):
        d = q[None, :] - r
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def brute(query, ref, max_dist=math.inf):
    """(dist2 [Nq] float32, index [Nq] int32) by the definition."""
    query, ref = np.ascontiguousarray(query, F32).reshape(-1, 3), np.ascontiguousarray(ref, F32).reshape(-1, 3)
    md2 = square32(max_dist)
    ids = np.nonzero(finite_rows(ref))[0]
    r = ref[ids]
    dist2 = np.full(query.shape[0], np.inf, F32)
    index = np.full(query.shape[0], -1, np.int32)
    for i, q in enumerate(query):
        if not np.isfinite(q).all():
            dist2[i] = np.nan
            continue
        if r.shape[0] == 0:
            continue
        d2 = _d2(q, r)
        j = int(np.argmin(d2))                                  # the first of equal minima: the smallest index (ids ascend)
        if d2[j] < np.inf and d2[j] <= md2:
            dist2[i], index[i] = d2[j], ids[j]
    return dist2, index


def cell_of(p, lo, cell, dims):
    """[N, 3] int cells of finite points p by the header's formula."""
    inv = F32(1.0) / F32(cell)
    with np.errstate(over="ignore"):
        t = np.floor((np.asarray(p, F32) - np.asarray(lo, F32)[None]) * inv)
    t = np.where(t > 0, t, F32(0))
    m = (np.asarray(dims) - 1).astype(F32)[None]
    t = np.where(t < m, t, m)
    return t.astype(np.int64)


class Grid:
    def __init__(self, ref, lo, cell, dims):
        self.ref = np.ascontiguousarray(ref, F32).reshape(-1, 3)
        self.lo, self.cell, self.dims = tuple(float(x) for x in lo), float(F32(cell)), tuple(int(d) for d in dims)
        nx, ny, nz = self.dims
        cells = nx * ny * nz
        ok = finite_rows(self.ref)
        keys = np.full(self.ref.shape[0], cells, np.int64)
        if ok.any():
            c = cell_of(self.ref[ok], self.lo, self.cell, self.dims)
            keys[ok] = (c[:, 2] * ny + c[:, 1]) * nx + c[:, 0]
        self.keys = keys
        self.order = np.argsort(keys, kind="stable")
        self.start = np.searchsorted(keys[self.order], np.arange(cells + 1), side="left")
        self.sorted = self.ref[self.order]


def grid_nearest(query, grid: Grid, max_dist=math.inf):
    """(dist2, index, visited [Nq]) by the header's ring search."""
    query = np.ascontiguousarray(query, F32).reshape(-1, 3)
    md2 = square32(max_dist)
    nx, ny, nz = grid.dims
    cellf = F32(grid.cell)
    dist2 = np.full(query.shape[0], np.inf, F32)
    index = np.full(query.shape[0], -1, np.int32)
    visited = np.zeros(query.shape[0], np.int64)
    for i, q in enumerate(query):
        if not np.isfinite(q).all():
            dist2[i] = np.nan
            continue
        cx, cy, cz = (int(v) for v in cell_of(q[None], grid.lo, grid.cell, grid.dims)[0])
        best, bi = F32(np.inf), np.iinfo(np.int32).max

        def scan(c0, c1):
            nonlocal best, bi
            s, e = int(grid.start[c0]), int(grid.start[c1 + 1])
            if e <= s:
                return
            visited[i] += e - s
            d2 = _d2(q, grid.sorted[s:e])
            ids = grid.order[s:e]
            m = d2.min()
            if m < best or (m == best and ids[d2 == m].min() < bi):
                best, bi = m, int(ids[d2 == m].min())

        for k in range(MAX_SIDE + 1):
            x0, x1 = max(cx - k, 0), min(cx + k, nx - 1)
            for z in range(max(cz - k, 0), min(cz + k, nz - 1) + 1):
                for y in range(max(cy - k, 0), min(cy + k, ny - 1) + 1):
                    row = (z * ny + y) * nx
                    if abs(z - cz) == k or abs(y - cy) == k:
                        scan(row + x0, row + x1)
                    else:
                        if cx - k >= 0:
                            scan(row + cx - k, row + cx - k)
                        if cx + k <= nx - 1:
                            scan(row + cx + k, row + cx + k)
            b = F32(k) - MARGIN
            if b > 0:
                rb = b * cellf
                rb2 = rb * rb
                if best <= rb2 or rb2 >= md2:
                    break
            if cx - k <= 0 and cx + k >= nx - 1 and cy - k <= 0 and cy + k >= ny - 1 and cz - k <= 0 and cz + k >= nz - 1:
                break
        if best < np.inf and best <= md2:
            dist2[i], index[i] = best, bi
    return dist2, index, visited


def sums(dist2, thresholds=()):
    """The reduction of one direction from the fp32 dist2: n_finite, n_within, dist_sum (math.fsum of sqrt in double), n_tau."""
    d = np.asarray(dist2, F32)
    within = np.isfinite(d)
    return {"n_finite": int((~np.isnan(d)).sum()), "n_within": int(within.sum()),
            "dist_sum": math.fsum(math.sqrt(float(x)) for x in d[within]),
            "n_tau": [int((d[within] <= square32(t)).sum()) for t in thresholds]}


def _nearest64(a, b):
    """float64 distance from every finite row of a to the nearest finite row of b ([0] rows of b: +inf)."""
    a, b = np.asarray(a, np.float64).reshape(-1, 3), np.asarray(b, np.float64).reshape(-1, 3)
    a, b = a[finite_rows(a)], b[finite_rows(b)]
    if b.shape[0] == 0:
        return np.full(a.shape[0], np.inf)
    out = np.empty(a.shape[0])
    for s in range(0, a.shape[0], 256):
        d = a[s: s + 256, None, :] - b[None]
        out[s: s + 256] = np.sqrt((d * d).sum(2).min(1))
    return out


def metrics64(pred, gt, thresholds=(0.05,), max_dist=math.inf):
    """The metrics of geometry_metrics in float64 throughout (the coordinates are the fp32 values)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        a, c = _nearest64(pred, gt), _nearest64(gt, pred)
        wa, wc = (a <= max_dist) & (a < np.inf), (c <= max_dist) & (c < np.inf)     # (no neighbour at all: not within any bound)
        mean = lambda d, w: np.float64(math.fsum(d[w])) / np.float64(int(w.sum()))
        accuracy, completeness = mean(a, wa), mean(c, wc)
        p = np.array([np.float64((a[wa] <= t).sum()) / np.float64(a.size) for t in thresholds])
        r = np.array([np.float64((c[wc] <= t).sum()) / np.float64(c.size) for t in thresholds])
        f = np.where(p + r > 0, 2 * p * r / (p + r), p + r)
    return {"accuracy": accuracy, "completeness": completeness, "chamfer": 0.5 * (accuracy + completeness), "precision": p, "recall": r,
            "fscore": f, "n_pred": a.size, "n_gt": c.size, "n_far": [int((~wa).sum()), int((~wc).sum())]}
