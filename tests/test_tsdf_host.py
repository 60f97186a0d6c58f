"""Host checks of TSDF fusion and mesh extraction (no GPU): the fp32 restatement (tests/tsdf_ref.py) against its float64 mode at a
bound derived from the operation count, known answers in float64 (a plane, a sphere: fused values, a closed and consistently
oriented mesh, Euler characteristic, volume, area), the 6 x 16 table that ships with the library against the regenerated one,
the C boundary of include/freesplat_amd_tsdf.h without a device, the Python layer's argument errors and the PLY round trip."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

import tsdf_cases as TC
import tsdf_ref as R
from util_abi import declared_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = ["fs_tsdf_api_version", "fs_tsdf_integrate", "fs_tsdf_mt_table", "fs_tsdf_mesh_scratch_bytes", "fs_tsdf_mesh_plan",
            "fs_tsdf_mesh_emit"]
U = 2.0 ** -24


# ---- 1. fp32 mode against float64 mode ----------------------------------------------------------------------------------------

def _value_bound(c):
    """|tsdf32 - tsdf64| where every decision agrees, u = 2^-24, Cm the largest |grid coordinate|, A = max over views of
    sum_i |R_zi| Cm + |t_z|, dm the largest valid depth a gather can return, n the number of views:
      grid coordinate: 2 roundings, <= 2 u Cm;  p_z: that through |R_z.| plus 4 roundings of partial sums <= A: <= 6 u A
      d: exact, or one quotient: <= u dm;  sdf = d - p_z: <= u dm + 6 u A + u |sdf| <= u (2 dm + 7 A)
      s = min(1, sdf / trunc): min is 1-Lipschitz, one quotient with |s| <= 1: <= u (2 dm + 7 A) / trunc + u
      running mean: e' <= (e W + e_s) / W' + 3 u (product, sum, quotient on values <= 1 after the division) <= max(e, e_s) + 3 u
    so after n views <= u ((2 dm + 7 A) / trunc + 1 + 3 n); colours (exact inputs in [0, 1]): <= 3 u n."""
    vol, views = c["vol"], c["views"]
    Cm = max(float(np.abs(a).max()) for a in R.grid_axes(vol, np.float64))
    m = views["world_to_cam"].astype(np.float64)
    A = float((np.abs(m[:, 2, :3]).sum(1) * Cm + np.abs(m[:, 2, 3])).max())
    d = views["depth"].astype(np.float64)
    if views["alpha"] is not None:
        d = d / np.fmax(views["alpha"], np.float32(views["alpha_floor"])).astype(np.float64)
    dm = float(d[np.isfinite(d) & (d > views["min_depth"]) & (d < views["max_depth"])].max())
    n = m.shape[0]
    return U * ((2 * dm + 7 * A) / vol["trunc"] + 1 + 3 * n), 3 * U * n


@pytest.mark.parametrize("cs", TC.CASES + [TC.BIG], ids=lambda cs: TC.case(*cs)["name"])
def test_fp32_restatement_against_float64(cs):
    c = TC.case(*cs)
    v32, codes32, pix32 = TC.fused(cs)
    v64 = R.to_f64(c["vol"])
    codes64, pix64 = R.integrate(v64, c["views"], np.float64, decisions=True)
    agree = ((codes32 == codes64) & (pix32 == pix64)).all(0)
    touched = (v32["weight"] > 0) | (v64["weight"] > 0)
    left_out = int((touched & ~agree).sum())
    assert int(touched.sum()) > 0
    assert left_out <= 0.01 * int(touched.sum()), f"{left_out} of {int(touched.sum())} touched grid points differ in a decision"
    assert np.array_equal(v32["weight"][agree], v64["weight"][agree].astype(np.float32))
    b_t, b_c = _value_bound(c)
    e_t = float(np.abs(v32["tsdf"].astype(np.float64) - v64["tsdf"])[agree].max())
    e_c = 0.0 if v32["color"] is None else float(np.abs(v32["color"].astype(np.float64) - v64["color"])[:, agree].max())
    print(f"{c['name']}: {left_out} / {int(touched.sum())} touched points left out; tsdf error {e_t:.3e} (bound {b_t:.3e}), "
          f"colour error {e_c:.3e} (bound {b_c:.3e})")
    assert e_t <= b_t and e_c <= b_c


def test_the_case_list_covers_what_the_kernels_branch_on():
    from freesplat_amd import tsdf as T
    assert (T.MAX_VIEWS, T.BRICK, T.MESH_RUN, T.SCAN_THREADS) == (TC.MAX_VIEWS, TC.BRICK, TC.MESH_RUN, TC.SCAN_THREADS)
    bx, by, bz = T.BRICK
    dims = {c[0] for c in TC.CASES}
    assert {(1, 1, 1), (5, 3, 2), (bx - 1, by - 1, bz - 1), (bx + 1, by + 1, bz + 1)} <= dims
    assert any(X > 2 * bx and Y > 2 * by and Z > 2 * bz and X % 4 for X, Y, Z in dims)
    X, Y, Z = TC.BIG[0]
    assert (X - 1) * (Y - 1) * (Z - 1) > T.SCAN_THREADS * T.MESH_RUN and X % 4 and X > bx and Y > by and Z > bz
    assert {c[1] for c in TC.CASES} == {(1, 1), (5, 7), (30, 40)}
    assert {c[2] for c in TC.CASES} == {1, 3, T.MAX_VIEWS, T.MAX_VIEWS + 1}
    assert {(c[3], c[4]) for c in TC.CASES} == {(False, False), (True, False), (True, True), (False, True)}
    seen, behind, cut_bricks, capped = set(), False, False, False
    for cs in TC.CASES:
        c = TC.case(*cs)
        vol, codes, pixels = TC.fused(cs)
        d = c["views"]["depth"]
        for v in range(d.shape[0]):
            hit = np.unique(pixels[v][codes[v] == R.INVALID])
            vals = d[v].reshape(-1)[hit]
            seen |= {"nan" for x in vals if np.isnan(x)} | {"+inf" for x in vals if x == np.inf} | {"-inf" for x in vals if x == -np.inf}
            seen |= {"zero" for x in vals if x == 0} | {"negative" for x in vals if x < 0 and np.isfinite(x)}
            behind |= bool((codes[v] == R.BEHIND).all())
            # a view whose frustum edge cuts a brick: inside the brick some points project into the map and some beside it
            X, Y, Z = c["vol"]["dims"]
            if X >= bx and Y >= by and Z >= bz:
                blk = codes[v][:bz, :by, :bx]
                cut_bricks |= bool((blk == R.OUTSIDE).any() and (blk >= R.INVALID).any())
        capped |= bool((vol["weight"] == vol["max_weight"]).any()) and d.shape[0] > vol["max_weight"]
    assert seen == {"nan", "+inf", "-inf", "zero", "negative"} and behind and cut_bricks and capped
    exact = TC.CASES[-1]
    assert exact[5] == "exact"
    c, (vol, codes, pixels) = TC.case(*exact), TC.fused(exact)
    gx, gy, gz = R.grid_axes(c["vol"], np.float32)
    k = c["views"]["intrinsics"][0]
    u = k[0] * (gx[None, :] / gz[:, None]) + k[2]                            # (identity camera: p = x)
    on_boundary = (u - np.floor(u) == 0.5) & (u > 0) & (u < 6)
    assert bool(on_boundary.any())
    kz, ix = np.argwhere(on_boundary)[0]
    assert int(pixels[0][kz, 4, ix]) % 7 == int(np.rint(u[kz, ix])) and np.rint(np.float32(4.5)) == 4      # half to even
    assert bool(((vol["tsdf"] == 0) & (vol["weight"] == 2)).any()) and float(vol["weight"].max()) == 2.0


# ---- 2. known answers in float64 ----------------------------------------------------------------------------------------------

def _axis_camera(direction, dist, centre, roll):
    z = -np.asarray(direction, np.float64)
    a = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(a, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    x, y = math.cos(roll) * x + math.sin(roll) * y, -math.sin(roll) * x + math.cos(roll) * y
    E = np.eye(4)
    E[:3, 0], E[:3, 1], E[:3, 2], E[:3, 3] = x, y, z, centre - dist * z
    return E


def _views64(c2w, intr, depth):
    return dict(world_to_cam=np.linalg.inv(c2w)[:, :3], intrinsics=intr, depth=depth, alpha=None, image=None, near=0.05,
                min_depth=0.0, max_depth=np.inf, alpha_min=0.0, alpha_floor=1e-3)


def _vol64(origin, vs, dims, trunc):
    vol = R.to_f64(R.new_volume(origin, vs, dims, trunc, 64.0, False))
    vol.update(origin=tuple(origin), voxel_size=vs, trunc=trunc)
    return vol


def test_a_plane_under_fronto_parallel_cameras_gives_the_signed_distance():
    """The plane z = 0.4 seen from six cameras above it that look straight down, at different heights, offsets and rolls: each
    depth map is its camera's height above the plane, so the projective value IS the signed distance: where at least one camera
    sees a grid point within trunc of the plane, tsdf = distance / trunc."""
    vs, dims, trunc, plane = 0.05, (20, 18, 16), 0.2, 0.4
    vol = _vol64((-0.5, -0.45, 0.03), vs, dims, trunc)
    rng = np.random.default_rng(1)
    c2w = np.stack([_axis_camera((0, 0, 1), 2.0 + 0.3 * v, np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), plane]), 0.7 * v)
                    for v in range(6)])
    H, W = 24, 32
    intr = np.tile(np.array([40.0, 40.0, 15.5, 11.5]), (6, 1))
    depth = np.stack([np.full((H, W), c2w[v, 2, 3] - plane) for v in range(6)])
    codes, _ = R.integrate(vol, _views64(c2w, intr, depth), np.float64, decisions=True)
    gz = R.grid_axes(vol, np.float64)[2]
    dist = np.broadcast_to((gz - plane)[:, None, None], vol["tsdf"].shape)
    near = (np.abs(dist) < trunc) & (vol["weight"] > 0)
    assert int(near.sum()) > 500 and bool((codes == R.OUTSIDE).any())
    err = float(np.abs(vol["tsdf"] - dist / trunc)[near].max())
    print(f"plane: {int(near.sum())} grid points within trunc and seen, max |tsdf - distance / trunc| = {err:.2e}")
    assert err <= 1e-12
    assert bool((vol["tsdf"][(dist >= trunc) & (vol["weight"] > 0)] == 1.0).all())
    assert not bool(vol["weight"][dist < -trunc - 1e-9].any())               # beyond the truncation behind the surface: never updated


GRAZING = 0.6    # cosine of the largest incidence angle the ray-caster keeps


def _sphere_depth(c2w, k, H, W, centre, radius, px=None, py=None):
    """Analytic z-depth of the sphere along the rays through the pixel centres (px, py) (default: the whole map); NaN on a miss
    and where the ray meets the surface at more than acos(GRAZING) from the normal, as a sensor drops grazing samples."""
    if px is None:
        py, px = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.stack([(px - k[2]) / k[0], (py - k[3]) / k[1], np.ones_like(px)], -1) @ c2w[:3, :3].T
    oc = c2w[:3, 3] - centre
    a, b, cc = (ray * ray).sum(-1), (ray * oc).sum(-1), float(oc @ oc) - radius * radius
    disc = b * b - a * cc
    with np.errstate(invalid="ignore"):
        s = (-b - np.sqrt(disc)) / a
        cosine = -((oc + s[..., None] * ray) * ray).sum(-1) / (radius * np.sqrt(a))
        return np.where((disc > 0) & (cosine >= GRAZING), s, np.nan)


def test_a_sphere_fuses_to_the_projective_value_and_extracts_closed():
    """A sphere of radius 8.3 voxels ray-cast analytically from fourteen directions (the six axes and the eight diagonals),
    grazing samples dropped.  Six axis cameras with every hit kept do not give a closed surface under these rules: a grid point
    outside the sphere but behind a camera's silhouette receives that camera's negative projective value (284 bad edges, area
    +16 %); with the grazing samples dropped six cameras leave holes at the diagonals.  (a) at grid points within trunc of the
    surface that a camera updated, tsdf equals the mean over the updating cameras of min(1, (D(pixel) - p_z) / trunc) with D the
    analytic depth along the ray through the chosen pixel's centre (formed here per grid point, not gathered from a map);
    (b) the extracted mesh, welded and without its degenerate faces, is closed and consistently oriented (every directed edge
    once, its reverse once), has Euler characteristic 2, a positive signed volume, and volume and area within 2 % of the
    sphere's.  (A CPU prototype of the rules on the analytic distance field gave 7 728 triangles, 64 of zero area, volume
    -0.73 %, area -0.37 %; the figures of this fused field are printed.)"""
    vs, n, trunc_vox, radius_vox = 0.1, 24, 3.0, 8.3
    origin = (-1.13, -1.21, -1.17)
    vol = _vol64(origin, vs, (n, n, n), trunc_vox * vs)
    centre = np.array(origin) + vs * np.array([11.37, 11.62, 11.45])
    radius = radius_vox * vs
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)] + list(itertools.product((-1, 1), repeat=3))
    nv = len(dirs)
    c2w = np.stack([_axis_camera(np.array(d, np.float64) / np.linalg.norm(d), 4.0, centre, 0.3 * i) for i, d in enumerate(dirs)])
    H = W = 96
    intr = np.tile(np.array([120.0, 120.0, 47.5, 47.5]), (nv, 1))
    depth = np.stack([_sphere_depth(c2w[v], intr[v], H, W, centre, radius) for v in range(nv)])
    views = _views64(c2w, intr, depth)
    codes, pixels = R.integrate(vol, views, np.float64, decisions=True)
    # (a)
    gx, gy, gz = R.grid_axes(vol, np.float64)
    pts = np.stack(np.broadcast_arrays(gx[None, None, :], gy[None, :, None], gz[:, None, None]), -1)
    acc, cnt = np.zeros(vol["tsdf"].shape), np.zeros(vol["tsdf"].shape)
    for v in range(nv):
        m = views["world_to_cam"][v]
        p = pts @ m[:, :3].T + m[:, 3]
        upd = codes[v] == R.UPDATED
        D = _sphere_depth(c2w[v], intr[v], H, W, centre, radius, (pixels[v] % W).astype(np.float64), (pixels[v] // W).astype(np.float64))
        s = np.minimum(1.0, (D - p[..., 2]) / vol["trunc"])
        acc += np.where(upd, s, 0.0)
        cnt += upd
    dist = np.linalg.norm(pts - centre, axis=-1) - radius
    near = (np.abs(dist) < vol["trunc"]) & (cnt > 0)
    assert np.array_equal(cnt, vol["weight"]) and int(near.sum()) > 5000
    err = float(np.abs(vol["tsdf"] - acc / np.maximum(cnt, 1))[near].max())
    print(f"sphere: {int(near.sum())} grid points within trunc and seen, max |tsdf - analytic projective value| = {err:.2e}")
    assert err <= 1e-12
    # (b)
    verts, _ = R.extract(vol, 1.0, np.float64)
    Vw, F = R.weld(verts)
    rep = R.mesh_report(Vw, F)
    a, b, c = verts[:, 0], verts[:, 1], verts[:, 2]
    zero_area = int((np.linalg.norm(np.cross(b - a, c - a), axis=1) == 0).sum())
    vol_rel = rep["volume"] / (4 / 3 * math.pi * radius ** 3) - 1
    area_rel = rep["area"] / (4 * math.pi * radius ** 2) - 1
    print(f"sphere mesh: {verts.shape[0]} triangles, {zero_area} of zero area, {rep['bad_edges']} bad edges, Euler characteristic "
          f"{rep['euler']}, volume {100 * vol_rel:+.2f} %, area {100 * area_rel:+.2f} %")
    assert rep["bad_edges"] == 0 and rep["euler"] == 2 and rep["volume"] > 0
    assert abs(vol_rel) <= 0.02 and abs(area_rel) <= 0.02


# ---- 3. the table ---------------------------------------------------------------------------------------------------------------

def test_the_shipped_table_equals_the_regenerated_one():
    from freesplat_amd import tsdf as T
    shipped, want = T.mt_table(), R.mt_table()
    assert shipped.shape == (6, 16, 7) and shipped.dtype == np.uint8
    for t in range(6):
        for case in range(16):
            assert np.array_equal(shipped[t, case], want[t, case]), (t, case, shipped[t, case], want[t, case])
    assert [int(want[t, c, 0]) for t in range(1) for c in range(16)] == [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0]
    assert [R.tet_corners(t) for t in range(6)] == [(0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7)]


def test_neighbouring_cubes_split_their_shared_face_by_the_same_diagonal():
    """The Kuhn split is translation-invariant: the face diagonals of the cube at x = 1 are those at x = 0 shifted, per axis."""
    diag = set()
    for t in range(6):
        tc = R.tet_corners(t)
        diag |= {(a, b) for a in tc for b in tc if a < b and bin(a ^ b).count("1") == 2}
    for ax in range(3):
        bit = 1 << ax
        lo = {(a, b) for a, b in diag if not a & bit and not b & bit}
        hi = {(a ^ bit, b ^ bit) for a, b in diag if a & bit and b & bit}
        assert lo == hi and len(lo) == 1


# ---- 4. the C boundary ----------------------------------------------------------------------------------------------------------

def test_tsdf_header_is_exported_and_bound():
    from freesplat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    names = declared_names("freesplat_amd_tsdf.h")
    assert names == sorted(EXPECTED)
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/freesplat_amd_tsdf.h but not exported"
    assert set(_lib.TSDF_SIGNATURES) == set(names)
    assert _lib.lib().fs_tsdf_api_version() == 1 == _lib.TSDF_API_VERSION
    text = open(os.path.join(ROOT, "include", "freesplat_amd_tsdf.h")).read()
    assert re.search(r"#define\s+FS_TSDF_API_VERSION\s+1\b", text)
    assert re.search(r"#define\s+FS_TSDF_MAX_VIEWS\s+64\b", text) and _lib.TSDF_MAX_VIEWS == 64
    got = tuple(int(re.search(rf"#define\s+FS_TSDF_BRICK_{ax}\s+(\d+)", text).group(1)) for ax in "XYZ")
    assert got == _lib.TSDF_BRICK and int(re.search(r"#define\s+FS_TSDF_MESH_RUN\s+(\d+)", text).group(1)) == _lib.TSDF_MESH_RUN


P = C.c_void_p(4096)      # a fake non-NULL pointer: nothing may launch with it
INF = math.inf


def _integrate(L, dims=(8, 8, 8), origin=(0.0, 0.0, 0.0), vs=0.1, trunc=0.3, max_weight=64.0, vol=(P, P, None), V=2, H=16, W=16,
               maps=(P, P, P, None, None), sc=(0.05, 0.0, INF, 0.5, 1e-3), flags=0):
    """vol = (tsdf, weight, color); maps = (world_to_cam, intrinsics, depth, alpha, image); sc = (near, min_depth, max_depth,
    alpha_min, alpha_floor)."""
    return L.fs_tsdf_integrate(*dims, *origin, vs, trunc, max_weight, *vol, V, H, W, *maps, *sc, flags, None)


def _plan(L, dims=(8, 8, 8), ptrs=(P, P), min_weight=1.0, out=(P, P)):
    return L.fs_tsdf_mesh_plan(*dims, *ptrs, min_weight, *out, None)


def _emit(L, dims=(8, 8, 8), origin=(0.0, 0.0, 0.0), vs=0.1, ptrs=(P, P, None), min_weight=1.0, scratch=P, T=5, out=(P, None)):
    return L.fs_tsdf_mesh_emit(*dims, *origin, vs, *ptrs, min_weight, scratch, T, *out, None)


def test_entry_points_validate_before_touching_a_device():
    """FS_ERR_INVALID_ARG (-1) and FS_ERR_UNSUPPORTED (-3) for every condition the header lists -- with fake non-NULL pointers,
    so nothing may launch."""
    from freesplat_amd import _lib
    L = _lib.lib()
    nan = math.nan
    for i in range(3):
        for bad in (0, -1):
            dims = tuple(bad if k == i else 8 for k in range(3))
            assert _integrate(L, dims=dims) == -1 and _plan(L, dims=dims) == -1 and _emit(L, dims=dims) == -1, dims
            assert L.fs_tsdf_mesh_scratch_bytes(*dims) == 0
    for bad in (dict(V=0), dict(V=-1), dict(H=0), dict(W=-2)):
        assert _integrate(L, **bad) == -1, bad
    assert _integrate(L, vol=(None, P, None)) == -1 and _integrate(L, vol=(P, None, None)) == -1
    for i in range(3):
        assert _integrate(L, maps=tuple(None if k == i else v for k, v in enumerate((P, P, P, None, None)))) == -1, i
    assert _integrate(L, vol=(P, P, P)) == -1 and _integrate(L, maps=(P, P, P, None, P)) == -1        # colour without image, image without colour
    for i in range(3):
        for bad in (nan, INF, -INF):
            assert _integrate(L, origin=tuple(bad if k == i else 0.0 for k in range(3))) == -1
            assert _emit(L, origin=tuple(bad if k == i else 0.0 for k in range(3))) == -1
    for i in range(4):
        assert _integrate(L, sc=tuple(nan if k == i else v for k, v in enumerate((0.05, 0.0, INF, 0.5, 1e-3)))) == -1, i
    for bad in (0.0, -1.0, INF, nan):
        assert _integrate(L, vs=bad) == -1 and _integrate(L, trunc=bad) == -1 and _integrate(L, max_weight=bad) == -1, bad
        assert _integrate(L, sc=(0.05, 0.0, INF, 0.5, bad)) == -1 and _emit(L, vs=bad) == -1, bad
    assert _integrate(L, flags=2) == -1 and _integrate(L, flags=-1) == -1
    assert _integrate(L, V=65) == -3 and _integrate(L, V=2 ** 20) == -3
    big = (2048, 1024, 1024)                                                 # 2^31 grid points
    assert _integrate(L, dims=big) == -3 and _plan(L, dims=big) == -3 and _emit(L, dims=big) == -3
    assert L.fs_tsdf_mesh_scratch_bytes(*big) == 0 and _integrate(L, dims=(2 ** 20, 2 ** 20, 1)) == -3
    assert _integrate(L, H=46341, W=46341) == -3
    for i in range(2):
        assert _plan(L, ptrs=tuple(None if k == i else P for k in range(2))) == -1
        assert _plan(L, out=tuple(None if k == i else P for k in range(2))) == -1
        assert _emit(L, ptrs=tuple(None if k == i else v for k, v in enumerate((P, P, None)))) == -1
    for bad in (0.0, -1.0, nan):
        assert _plan(L, min_weight=bad) == -1 and _emit(L, min_weight=bad) == -1, bad
    assert _emit(L, scratch=None) == -1 and _emit(L, T=-1) == -1 and _emit(L, out=(None, None)) == -1
    assert _emit(L, ptrs=(P, P, P)) == -1 and _emit(L, out=(P, P)) == -1      # colour planes without a colour output, and the reverse
    assert _emit(L, T=(2 ** 31 - 1) // 9 + 1) == -3
    assert _emit(L, T=0, out=(None, None)) == 0                              # an empty soup: nothing to do, nothing launched
    assert _emit(L, dims=(1, 8, 8), T=1) == -1                               # a volume without a cube has no triangle
    assert L.fs_tsdf_mt_table(None) == -1


def test_mesh_scratch_bytes():
    """One uint32 count and one uint64 offset per workgroup of MESH_RUN cubes, each run rounded up to 256 bytes."""
    from freesplat_amd import _lib, tsdf as T
    L = _lib.lib()
    al = lambda x: (x + 255) // 256 * 256
    for X, Y, Z in ((1, 1, 1), (2, 2, 2), (5, 3, 2), (33, 9, 5), (67, 66, 65), (256, 256, 256), (1, 70, 9)):
        nb = max(1, -(-(X - 1) * (Y - 1) * (Z - 1) // T.MESH_RUN))
        assert L.fs_tsdf_mesh_scratch_bytes(X, Y, Z) == al(4 * nb) + al(8 * nb) > 0


# ---- the Python layer's argument errors that need no device --------------------------------------------------------------------

def test_argument_errors_without_a_device():
    from freesplat_amd import tsdf as T
    with pytest.raises(ValueError, match="freesplat_amd.tsdf.*no CPU path"):
        T.TSDFVolume((0, 0, 0), 0.1, (4, 4, 4), device="cpu")
    for kw in (dict(voxel_size=0.0), dict(voxel_size=math.nan), dict(trunc=-1.0), dict(max_weight=math.inf), dict(dims=(4, 0, 4)),
               dict(dims=(4, 4)), dict(origin=(0.0, math.nan, 0.0)), dict(dims=(2048, 1024, 1024))):
        args = dict(origin=(0, 0, 0), voxel_size=0.1, dims=(4, 4, 4), device="cpu")
        args.update(kw)
        with pytest.raises(ValueError, match="freesplat_amd.tsdf"):
            T.TSDFVolume(**args)
    f = torch.ones(3, 4, 5)
    with pytest.raises(ValueError, match="freesplat_amd.tsdf.*no CPU path"):
        T.extract_mesh(f, f, None, (0, 0, 0), 0.1)
    for bad in (0.0, -1.0, math.nan):
        with pytest.raises(ValueError, match="min_weight"):
            T.extract_mesh(f, f, None, (0, 0, 0), 0.1, min_weight=bad)
    E = torch.eye(4, dtype=torch.float64).repeat(2, 1, 1)
    E[1, :3, 3] = torch.tensor([1.0, -2.0, 0.5])
    w2c = T.world_to_cam(E, "cpu")
    assert w2c.dtype == torch.float32 and tuple(w2c.shape) == (2, 3, 4) and torch.equal(w2c[1, :, 3], torch.tensor([-1.0, 2.0, -0.5]))
    rot = torch.tensor(TC.case(*TC.CASES[4])["c2w"])
    back = T.world_to_cam(rot, "cpu").double()
    assert float((back @ rot - torch.eye(4, dtype=torch.float64)[:3]).abs().max()) <= 1e-6
    for bad in (E[0], E[:, :3], torch.zeros(0, 4, 4)):
        with pytest.raises(ValueError, match=r"camera-to-world \[V, 4, 4\]"):
            T.world_to_cam(bad, "cpu")
    nanE, rowE, singE = E.clone(), E.clone(), E.clone()
    nanE[0, 0, 0], rowE[0, 3, 0], singE[0, :3, 0] = math.nan, 1.0, 0.0
    for bad in (nanE, rowE):
        with pytest.raises(ValueError, match="last row"):
            T.world_to_cam(bad, "cpu")
    with pytest.raises(ValueError, match="not invertible"):
        T.world_to_cam(singE, "cpu")
    with pytest.raises(RuntimeError, match="extrinsics gets no gradient"):
        T.world_to_cam(E.clone().requires_grad_(True), "cpu")
    for bad in (torch.zeros(4, 3), torch.zeros(4, 3, 3, dtype=torch.float64)):
        with pytest.raises(ValueError, match="triangle soup"):
            T.weld(bad)
    with pytest.raises(ValueError, match="colors"):
        T.weld(torch.zeros(4, 3, 3), torch.zeros(3, 3, 3))


def test_weld_on_the_host_matches_the_restatement():
    """torch.unique on the bits (here on CPU tensors: weld runs where the soup lives) against the numpy weld: the same vertex
    set, the same faces up to the numbering, colours of the first occurrence; -0.0 and 0.0 are different bits."""
    from freesplat_amd import tsdf as T
    vol, _, _ = TC.fused(TC.CASES[-1])
    verts, cols = R.extract(vol)
    assert verts.shape[0] > 0 and cols is not None
    V, F, Cc = T.weld(torch.from_numpy(verts), torch.from_numpy(cols))
    Vr, Fr = R.weld(verts)
    assert V.shape[0] == Vr.shape[0] and F.shape[0] == Fr.shape[0] < verts.shape[0]      # (zero-area faces were dropped)
    assert np.array_equal(V.numpy()[F.numpy()], Vr[Fr])
    soup = torch.from_numpy(verts).reshape(-1, 3)
    first = {tuple(p.tolist()): i for i, p in reversed(list(enumerate(soup)))}
    assert all(torch.equal(Cc[i], torch.from_numpy(cols).reshape(-1, 3)[first[tuple(V[i].tolist())]]) for i in range(0, V.shape[0], 7))
    z = torch.tensor([[[0.0, 0.0, 0.0], [-0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]])
    assert T.weld(z)[0].shape[0] == 3 and T.weld(z, drop_degenerate=False)[1].shape[0] == 1


# ---- 5. PLY -----------------------------------------------------------------------------------------------------------------------

def test_mesh_ply_round_trip(tmp_path):
    from freesplat_amd import tsdf as T
    vol, _, _ = TC.fused(TC.CASES[-1])
    verts, cols = R.extract(vol)
    V, F, Cc = T.weld(torch.from_numpy(verts), torch.from_numpy(cols))
    for name, colours in (("plain.ply", None), ("colour.ply", Cc)):
        path = str(tmp_path / name)
        T.export_mesh_ply(path, V, F, colours)
        v2, f2, c2 = T.read_mesh_ply(path)
        assert v2.dtype == np.float32 and f2.dtype == np.int32
        assert np.array_equal(v2.view(np.uint32), V.numpy().view(np.uint32)) and np.array_equal(f2, F.numpy())
        if colours is None:
            assert c2 is None
        else:
            assert c2.dtype == np.uint8 and np.array_equal(c2, np.rint(np.clip(Cc.numpy().astype(np.float64), 0, 1) * 255).astype(np.uint8))
        head = open(path, "rb").read(400).split(b"end_header")[0].decode()
        assert head.startswith("ply\nformat binary_little_endian 1.0\n") and f"element vertex {V.shape[0]}" in head
        assert f"element face {F.shape[0]}" in head and "property list uchar int vertex_indices" in head
    path = str(tmp_path / "empty.ply")
    T.export_mesh_ply(path, torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64))
    v2, f2, c2 = T.read_mesh_ply(path)
    assert v2.shape == (0, 3) and f2.shape == (0, 3) and c2 is None
    with pytest.raises(ValueError, match="outside"):
        T.export_mesh_ply(path, torch.zeros(2, 3), torch.tensor([[0, 1, 2]]))
