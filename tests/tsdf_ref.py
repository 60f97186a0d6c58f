"""Restatement of TSDF fusion and marching-tetrahedra extraction (include/freesplat_amd_tsdf.h) in vectorised numpy: the oracle of
tests/test_tsdf_host.py, tests/test_tsdf_hip.py and smoke().

Two modes, chosen by `dtype`:
  np.float32   every operation of the header in the header's association order, each rounded on its own (numpy neither fuses
               nor reassociates; np.rint rounds half to even): the bits the kernels must give.
  np.float64   the same formulas in double from the same fp32 inputs: the value the fp32 result is bounded against.

A volume is a dict: origin (3 floats), voxel_size, dims (X, Y, Z), trunc, max_weight, tsdf [Z, Y, X], weight [Z, Y, X],
color [3, Z, Y, X] | None.  No Python loop runs over grid points or cubes (loops run over views, tetrahedra and cases)."""
import itertools

import numpy as np

PERMS = list(itertools.permutations(range(3)))


# ---- the 6 x 16 table from its geometric definition ----------------------------------------------------------------------------

def tet_corners(t):
    """Cube corners of Kuhn tetrahedron t: {c0, c0 + e_a, c0 + e_a + e_b, c7} for the t-th permutation (a, b, .) of the axes."""
    a, b, _ = PERMS[t]
    return (0, 1 << a, (1 << a) | (1 << b), 7)


def corner_offset(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1])


def mt_table():
    """uint8 [6, 16, 7]: entry (tet, case) = (number of triangles, 6 edge codes); bit m of `case` is set iff tet vertex m is inside
    (tsdf < 0); an edge code is (A << 3) | B for the cube corners A < B of the cut edge.  Triangles as the header states them:
    one vertex o against three p < q < r gives (op, oq, or); inside {a, b}, outside {c, d} gives (ac, ad, bd), (ac, bd, bc); a
    triangle whose normal, with every cut at the edge midpoint, points from free space to the inside has its last two swapped."""
    tab = np.zeros((6, 16, 7), np.uint8)
    for t in range(6):
        tc = tet_corners(t)
        P = [corner_offset(c).astype(np.float64) for c in tc]
        for case in range(1, 15):
            ins = [m for m in range(4) if (case >> m) & 1]
            out = [m for m in range(4) if not (case >> m) & 1]
            if len(ins) == 1 or len(out) == 1:
                o = ins[0] if len(ins) == 1 else out[0]
                p, q, r = [m for m in range(4) if m != o]
                tris = [[(o, p), (o, q), (o, r)]]
            else:
                (a, b), (c, d) = ins, out
                tris = [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]
            n = np.mean([P[m] for m in out], 0) - np.mean([P[m] for m in ins], 0)
            tab[t, case, 0] = len(tris)
            for k, tri in enumerate(tris):
                A, B, C = [(P[i] + P[j]) / 2 for i, j in tri]
                s = float(np.dot(np.cross(B - A, C - A), n))
                assert abs(s) > 1e-9
                if s < 0:
                    tri = [tri[0], tri[2], tri[1]]
                for e, (i, j) in enumerate(tri):
                    lo, hi = sorted((tc[i], tc[j]))
                    tab[t, case, 1 + 3 * k + e] = (lo << 3) | hi
    return tab


# ---- the volume ----------------------------------------------------------------------------------------------------------------

def new_volume(origin, voxel_size, dims, trunc, max_weight, color):
    X, Y, Z = dims
    return dict(origin=tuple(float(np.float32(o)) for o in origin), voxel_size=float(np.float32(voxel_size)), dims=(X, Y, Z),
                trunc=float(np.float32(trunc)), max_weight=float(np.float32(max_weight)),
                tsdf=np.ones((Z, Y, X), np.float32), weight=np.zeros((Z, Y, X), np.float32),
                color=np.zeros((3, Z, Y, X), np.float32) if color else None)


def copy_volume(vol):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in vol.items()}


def grid_axes(vol, dtype):
    """The coordinates of the grid points along x, y, z: origin[c] + voxel_size * idx, one product and one sum in `dtype`."""
    vs = dtype(vol["voxel_size"])
    return [dtype(vol["origin"][c]) + vs * np.arange(vol["dims"][c]).astype(dtype) for c in range(3)]


# decisions of a (grid point, view) pair
BEHIND, OUTSIDE, INVALID, CUT, UPDATED = 0, 1, 2, 3, 4


def integrate(vol, views, dtype=np.float32, decisions=False):
    """Fuses the views into `vol` in place, in the order v = 0 .. V - 1.  views: world_to_cam [V, 3, 4], intrinsics [V, 4], depth
    [V, H, W], alpha [V, H, W] | None, image [V, 3, H, W] | None (fp32 arrays) and the scalars near, min_depth, max_depth,
    alpha_min, alpha_floor.  In float64 mode the volume's arrays must be float64 already (to_f64).

    decisions = True: also returns (code int8 [V, Z, Y, X], pixel int64 [V, Z, Y, X]) -- which of the five outcomes every pair
    had and, where it got as far as a pixel, the pixel's index."""
    f = dtype
    X, Y, Z = vol["dims"]
    gx, gy, gz = grid_axes(vol, f)
    x, y, z = gx[None, None, :], gy[None, :, None], gz[:, None, None]
    w2c, intr = views["world_to_cam"].astype(f), views["intrinsics"].astype(f)
    depth = views["depth"].astype(f)
    alpha = None if views.get("alpha") is None else views["alpha"]
    image = None if views.get("image") is None else views["image"].astype(f)
    assert (image is None) == (vol["color"] is None)
    V, H, W = depth.shape
    near, lo, hi = f(views["near"]), f(views["min_depth"]), f(views["max_depth"])
    trunc, max_w = f(vol["trunc"]), f(vol["max_weight"])
    codes = np.zeros((V, Z, Y, X), np.int8) if decisions else None
    pixels = np.full((V, Z, Y, X), -1, np.int64) if decisions else None
    T, Wt, Cl = vol["tsdf"], vol["weight"], vol["color"]
    assert T.dtype == f
    with np.errstate(all="ignore"):
        for v in range(V):
            m, k = w2c[v], intr[v]
            p = [((m[c, 0] * x + m[c, 1] * y) + m[c, 2] * z) + m[c, 3] for c in range(3)]
            front = p[2] > near
            u = k[0] * (p[0] / p[2]) + k[2]
            w_ = k[1] * (p[1] / p[2]) + k[3]
            fx, fy = np.rint(u), np.rint(w_)
            inside = front & (fx >= 0) & (fx < f(W)) & (fy >= 0) & (fy < f(H))
            ix = np.where(inside, fx, 0).astype(np.int64)
            iy = np.where(inside, fy, 0).astype(np.int64)
            pix = iy * W + ix
            d = depth[v].reshape(-1)[pix]
            ok = inside
            if alpha is not None:
                a32 = alpha[v].reshape(-1)[pix]                                      # (the two alpha tests are made on the fp32 values)
                ok = ok & ~(a32 < np.float32(views["alpha_min"]))
                d = d / np.fmax(a32, np.float32(views["alpha_floor"])).astype(f)      # (fmaxf: a NaN alpha gives the floor)
            valid = ok & (np.abs(d) < np.inf) & (d > lo) & (d < hi)
            sdf = d - p[2]
            upd = valid & ~(sdf < -trunc)
            s = np.minimum(f(1), sdf / trunc)
            W1 = Wt + f(1)
            T[...] = np.where(upd, (T * Wt + s) / W1, T)
            if Cl is not None:
                for ch in range(3):
                    c = image[v, ch].reshape(-1)[pix]
                    Cl[ch] = np.where(upd, (Cl[ch] * Wt + c) / W1, Cl[ch])
            Wt[...] = np.where(upd, np.minimum(W1, max_w), Wt)
            if decisions:
                codes[v] = np.where(~front, BEHIND, np.where(~inside, OUTSIDE, np.where(~valid, INVALID, np.where(~upd, CUT, UPDATED))))
                pixels[v] = np.where(inside, pix, -1)
    return (codes, pixels) if decisions else None


def to_f64(vol):
    out = copy_volume(vol)
    for k in ("tsdf", "weight", "color"):
        if out[k] is not None:
            out[k] = out[k].astype(np.float64)
    return out


# ---- extraction ----------------------------------------------------------------------------------------------------------------

def extract(vol, min_weight=1.0, dtype=np.float32, table=None):
    """The triangle soup (vertices [T, 3, 3], colors [T, 3, 3] | None) in the header's order: linear cube index (x fastest), then
    tetrahedron, then triangle."""
    f = dtype
    tab = mt_table() if table is None else table
    X, Y, Z = vol["dims"]
    T, Wt, Cl = vol["tsdf"].astype(f), vol["weight"], vol["color"]
    empty = (np.zeros((0, 3, 3), f), None if Cl is None else np.zeros((0, 3, 3), f))
    if min(X, Y, Z) < 2:
        return empty
    sub = lambda a, c: a[..., (c >> 2) & 1: Z - 1 + ((c >> 2) & 1), (c >> 1) & 1: Y - 1 + ((c >> 1) & 1), (c & 1): X - 1 + (c & 1)]
    live = np.ones((Z - 1, Y - 1, X - 1), bool)
    for c in range(8):
        live &= sub(Wt, c) >= np.float32(min_weight)
    fc = [sub(T, c) for c in range(8)]
    ins = [(fc[c] < 0) & live for c in range(8)]
    axes = grid_axes(vol, f)
    kk, jj, ii = np.meshgrid(np.arange(Z - 1), np.arange(Y - 1), np.arange(X - 1), indexing="ij")
    lin = (kk * (Y - 1) + jj) * (X - 1) + ii
    keys, verts, cols = [], [], []
    with np.errstate(all="ignore"):
        for t in range(6):
            tc = tet_corners(t)
            case = sum(ins[tc[m]].astype(np.int64) << m for m in range(4))
            case = np.where(live, case, 0)
            for cs in range(1, 15):
                sel = case == cs
                if not sel.any():
                    continue
                ci, cj, ck = ii[sel], jj[sel], kk[sel]
                for k in range(int(tab[t, cs, 0])):
                    tri_v, tri_c = [], []
                    for e in range(3):
                        code = int(tab[t, cs, 1 + 3 * k + e])
                        A, B = code >> 3, code & 7
                        f0, f1 = fc[A][sel], fc[B][sel]
                        tt = f0 / (f0 - f1)
                        P = []
                        for ax, idx in enumerate((ci, cj, ck)):
                            P0 = axes[ax][idx + ((A >> ax) & 1)]
                            P1 = axes[ax][idx + ((B >> ax) & 1)]
                            P.append(P0 + tt * (P1 - P0))
                        tri_v.append(np.stack(P, -1))
                        if Cl is not None:
                            c0, c1 = sub(Cl.astype(f), A)[:, sel], sub(Cl.astype(f), B)[:, sel]
                            tri_c.append((c0 + tt * (c1 - c0)).T)
                    keys.append((lin[sel] * 6 + t) * 2 + k)
                    verts.append(np.stack(tri_v, 1))
                    if Cl is not None:
                        cols.append(np.stack(tri_c, 1))
    if not keys:
        return empty
    order = np.argsort(np.concatenate(keys), kind="stable")
    vertices = np.concatenate(verts)[order].astype(f)
    return vertices, (None if Cl is None else np.concatenate(cols)[order].astype(f))


# ---- mesh helpers ----------------------------------------------------------------------------------------------------------------

def weld(vertices, drop_degenerate=True):
    """Exact-bits weld: (V [n, 3], F [m, 3])."""
    flat = np.ascontiguousarray(vertices.reshape(-1, 3))
    bits = flat.view(np.uint32 if flat.dtype == np.float32 else np.uint64)
    _, first, inv = np.unique(bits, axis=0, return_index=True, return_inverse=True)
    F = inv.reshape(-1, 3)
    if drop_degenerate:
        F = F[(F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 0] != F[:, 2])]
    return flat[first], F


def mesh_report(V, F):
    """Closedness and orientation (every directed edge once, its reverse once), Euler characteristic, signed volume, area."""
    e = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]])
    n = int(V.shape[0]) + 1
    key, rev = e[:, 0].astype(np.int64) * n + e[:, 1], e[:, 1].astype(np.int64) * n + e[:, 0]
    uniq, counts = np.unique(key, return_counts=True)
    bad = int((counts != 1).sum()) + int((~np.isin(rev, uniq)).sum())
    used = np.unique(F)
    a, b, c = (V[F[:, i]].astype(np.float64) for i in range(3))
    cr = np.cross(b - a, c - a)
    return dict(bad_edges=bad, euler=int(used.size) - int(uniq.size) // 2 + int(F.shape[0]),
                volume=float((a * cr).sum() / 6.0), area=float(np.linalg.norm(cr, axis=1).sum() / 2.0))
