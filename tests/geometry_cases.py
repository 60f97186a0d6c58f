"""The seeded cases the geometry tests share (tests/test_geometry_host.py, tests/test_geometry_hip.py, smoke()): a reference
cloud, queries, the grid's cell (None = the default heuristic) per name; reference(name, max_dist) is the brute-force fp32
definition of tests/geometry_ref.py, computed once per (name, max_dist) and shared -- do not modify what it returns.

Sizes: Nr in {1, 63, 700}, Nq in {1, 257} (no multiple of the wavefront or of the workgroup, more than one workgroup)."""
import functools
import math

import numpy as np

import geometry_ref as G

F32 = np.float32


def grid_params(ref, cell=None):
    """(lo, cell, dims) as NearestGrid forms them: the bounding box of the finite points, default_cell, grid_dims."""
    from freesplat_amd.geometry_metrics import default_cell, grid_dims
    ref = np.asarray(ref, F32).reshape(-1, 3)
    ok = ref[G.finite_rows(ref)]
    if ok.shape[0] == 0:
        lo, extent = (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)
    else:
        lo = tuple(float(v) for v in ok.min(0))
        extent = tuple(float(h) - l for h, l in zip(ok.max(0), lo))
    cell, dims = grid_dims(extent, default_cell(extent, ok.shape[0]) if cell is None else cell)
    return lo, cell, dims


def _walls(rng, lo, cell, dims, n):
    """n points with every coordinate on a cell wall, fp32(lo + i cell): where the cell formula's rounding decides the cell."""
    i = np.stack([rng.integers(0, d + 1, n) for d in dims], 1).astype(F32)
    return (np.asarray(lo, F32)[None] + i * F32(cell)).astype(F32)


def _outside(rng, n, box_lo, box_hi, reach=1.6):
    """n points outside the box, up to `reach` box sizes away from its centre along at least one axis."""
    lo, hi = np.asarray(box_lo, np.float64), np.asarray(box_hi, np.float64)
    centre, half = 0.5 * (lo + hi), 0.5 * np.maximum(hi - lo, 1e-3)
    p = centre + half * rng.uniform(-1, 1, (n, 3))
    axis = rng.integers(0, 3, n)
    p[np.arange(n), axis] = centre[axis] + half[axis] * 2 * rng.uniform(1.0, reach, n) * rng.choice([-1.0, 1.0], n)
    return p.astype(F32)


def _adversarial(seed, cell):
    """700 reference points in the unit box (its corners first, so the grid is known before the rest is made), 100 of them snapped
    onto cell walls and 20 duplicates of earlier points; 257 queries: 50 coincident with reference points, 40 on cell walls, 86
    outside the box up to 1.6 box sizes away, the rest inside."""
    rng = np.random.default_rng(seed)
    ref = rng.uniform(0, 1, (700, 3)).astype(F32)
    ref[0], ref[1] = (0, 0, 0), (1, 1, 1)
    lo, cell_, dims = grid_params(ref[:2], default_cell_for(700) if cell is None else cell)
    ref[2:102] = np.clip(_walls(rng, lo, cell_, dims, 100), 0, 1)
    ref[680:700] = ref[rng.integers(2, 680, 20)]
    q = rng.uniform(0, 1, (257, 3)).astype(F32)
    q[:50] = ref[rng.integers(0, 700, 50)]
    q[50:90] = np.clip(_walls(rng, lo, cell_, dims, 40), 0, 1)
    q[90:176] = _outside(rng, 86, (0, 0, 0), (1, 1, 1))
    return ref, q, cell                                    # (None: NearestGrid's own heuristic arrives at cell_)


def default_cell_for(n):
    from freesplat_amd.geometry_metrics import default_cell
    return default_cell((1.0, 1.0, 1.0), n)


def _make(name):
    rng = np.random.default_rng(abs(hash_name(name)))
    if name == "walls default cell 700x257":
        return _adversarial(1, None)
    if name == "walls cell 0.13 700x257":
        return _adversarial(2, 0.13)
    if name == "walls 1x700":
        ref, q, cell = _adversarial(3, None)
        return ref, q[100:101], cell
    if name == "one cell 63x257":
        ref = rng.normal(0, 1, (63, 3)).astype(F32)
        return ref, np.concatenate([rng.normal(0, 1, (200, 3)), _outside(rng, 57, ref.min(0), ref.max(0))]).astype(F32), 100.0
    if name == "flat 700x257":
        ref = rng.uniform(-2, 3, (700, 3)).astype(F32)
        ref[:, 2] = F32(0.75)
        q = rng.uniform(-2, 3, (257, 3)).astype(F32)
        q[:100, 2] = F32(0.75)
        q[100:130] = ref[rng.integers(0, 700, 30)]
        return ref, q, None
    if name == "lattice ties 63x257":
        # reference points on an integer lattice, each twice: a query at a lattice midpoint is equally far from up to eight of them,
        # and every distance is exact in fp32, so only the index rule decides
        lat = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(2), indexing="ij"), -1).reshape(-1, 3)
        ref = np.concatenate([lat, lat[::-1]])[:63].astype(F32)
        q = (rng.integers(0, 8, (257, 3)) * 0.5).astype(F32)
        return ref, q, 1.0
    if name == "nan and inf rows 63x257":
        ref = rng.uniform(-1, 1, (63, 3)).astype(F32)
        ref[[0, 7, 62]] = np.nan
        ref[20, 1], ref[41, 0] = np.inf, -np.inf
        q = rng.uniform(-1.5, 1.5, (257, 3)).astype(F32)
        q[[0, 100, 256], [0, 1, 2]] = np.nan
        q[5, 2], q[255, 0] = np.inf, -np.inf
        return ref, q, None
    if name == "nothing left 1x257":
        return np.full((1, 3), np.nan, F32), rng.uniform(-1, 1, (257, 3)).astype(F32), None
    if name == "single 1x1":
        return np.array([[0.25, -3.0, 7.5]], F32), np.array([[1.0, 1.0, 1.0]], F32), None
    if name == "single reference 1x257":
        return np.array([[0.25, -3.0, 7.5]], F32), rng.normal(0, 5, (257, 3)).astype(F32), None
    raise KeyError(name)


def hash_name(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


NAMES = ["walls default cell 700x257", "walls cell 0.13 700x257", "walls 1x700", "one cell 63x257", "flat 700x257", "lattice ties 63x257",
         "nan and inf rows 63x257", "nothing left 1x257", "single 1x1", "single reference 1x257"]
# (name, max_dist): the finite bounds cut through the distance distribution of their case
BOUNDED = [("walls default cell 700x257", 0.2), ("walls cell 0.13 700x257", 0.05), ("nan and inf rows 63x257", 0.5),
           ("lattice ties 63x257", 0.5), ("single reference 1x257", 6.0)]
THRESHOLDS = (0.02, 0.05, 0.1, 0.25, 0.5, 1.0, 2.0, 1e30)        # eight: the most one call takes


@functools.lru_cache(maxsize=None)
def case(name):
    ref, q, cell = _make(name)
    ref, q = np.ascontiguousarray(ref, F32), np.ascontiguousarray(q, F32)
    ref.setflags(write=False)
    q.setflags(write=False)
    return {"ref": ref, "query": q, "cell": cell}


@functools.lru_cache(maxsize=None)
def reference(name, max_dist=math.inf):
    c = case(name)
    dist2, index = G.brute(c["query"], c["ref"], max_dist)
    dist2.setflags(write=False)
    index.setflags(write=False)
    return {"dist2": dist2, "index": index, "sums": G.sums(dist2, THRESHOLDS)}


def same_bits(got, want):
    """The same fp32 bits, a NaN in `want` matching any NaN."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan])


# ---- metric scenes ------------------------------------------------------------------------------------------------------------------

def two_clouds(seed=0, n_pred=257, n_gt=700):
    """A noisy cloud against a clean one on the same surface patch (a paraboloid z = 0.3 r^2 >= 0), with seven stray points more
    than 0.9 below it: every metric is strictly between its extremes."""
    rng = np.random.default_rng(seed)
    uv = rng.uniform(-1, 1, (n_gt, 2))
    gt = np.stack([uv[:, 0], uv[:, 1], 0.3 * (uv ** 2).sum(1)], 1).astype(F32)
    uv = rng.uniform(-0.8, 1, (n_pred, 2))
    pred = np.stack([uv[:, 0], uv[:, 1], 0.3 * (uv ** 2).sum(1)], 1) + rng.normal(0, 0.03, (n_pred, 3))
    pred[:7, 2] = -rng.uniform(1.0, 1.5, 7)
    return pred.astype(F32), gt


def sphere_points(n, centre, radius, seed=0):
    """n points on a sphere (normalised Gaussians), float32."""
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (np.asarray(centre, np.float64)[None] + radius * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


# ---- the end-to-end scene ------------------------------------------------------------------------------------------------------------

def sphere_scene():
    """The sphere of tests/tsdf_raycast_cases.py (radius 12 voxels of 0.1 in a 34^3 volume, a far wall behind it) as the inputs of
    TSDFVolume.integrate: fourteen 128 x 128 analytic depth maps from the six axes and the eight diagonals."""
    import itertools
    import tsdf_raycast_cases as RC
    S = RC.SPHERE
    vs, n = S["vs"], S["n"]
    origin = tuple(float(F32(o)) for o in S["origin"])
    centre = np.array(origin) + vs * np.array(S["centre_vox"])
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)] + list(itertools.product((-1, 1), repeat=3))
    c2w = np.stack([RC.look_at(centre + 4.0 * np.array(d, np.float64) / np.linalg.norm(d), centre, up=(0.3, 0.5 + 0.1 * i, -0.8))
                    for i, d in enumerate(dirs)])
    intr = np.tile(np.array([150.0, 150.0, 63.5, 63.5], F32), (len(dirs), 1))
    radius = S["radius_vox"] * vs
    depth = np.stack([RC.sphere_depth(c2w[v], intr[v], 128, 128, centre, radius, 0.0)[0] for v in range(len(dirs))])
    depth = np.where(np.isnan(depth), 10.0, depth).astype(F32)
    return dict(origin=origin, voxel_size=vs, dims=(n, n, n), trunc=S["trunc_vox"] * vs, max_weight=64.0, c2w=c2w, intrinsics=intr,
                depth=depth, near=0.05, centre=centre, radius=radius)
