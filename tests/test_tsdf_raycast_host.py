"""CPU checks of TSDF ray casting (include/freesplat_ext_raycast.h, freesplat_amd/tsdf.py): the restatement
tests/tsdf_raycast_ref.py against known answers (a plane, a sphere) and against its own float64 run on every case of
tests/tsdf_raycast_cases.py, the C boundary's status codes with fake pointers (nothing launches), and the Python layer's
refusals that need no device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import tsdf_raycast_cases as RC
import tsdf_raycast_ref as RR
from util_abi import declared_names, header_text

HEADER = "freesplat_ext_raycast.h"


# ---- 1. known answers ------------------------------------------------------------------------------------------------------------

# max |depth - analytic| / max |normal component - analytic| over the valid pixels of the plane scene, as this restatement
# measured them (float64 run: 2.0e-8 / 1.1e-16 -- the depth figure is what the fp32 rounding of the fused values leaves;
# fp32 run: 2.9e-7 / 2.7e-8).  The bounds are 10 x the fp32 figures, for other sample positions.
PLANE_DEPTH_BOUND, PLANE_NORMAL_BOUND = 2.9e-6, 2.7e-7


def plane_answer():
    """(analytic z-depth [H, W], analytic camera-space normal [3]) of the plane scene from the 25-degree camera, in float64 from
    the fp32 camera rows the ray cast receives."""
    E, k, (H, W) = RC.plane_camera()
    A, kk = E[0, :3].astype(np.float32).astype(np.float64), k[0].astype(np.float64)
    py, px = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depth = (RC.PLANE_Z - A[2, 3]) / (A[2, 0] * (px - kk[2]) / kk[0] + A[2, 1] * (py - kk[3]) / kk[1] + A[2, 2])
    n = A[:, :3].T @ np.array([0.0, 0.0, 1.0])              # the world normal (0, 0, -1) towards the camera, sign convention flipped
    return depth, n / np.linalg.norm(n)


def plane_errors(out):
    depth, n = plane_answer()
    ok = out["valid"][0]
    return (float(ok.mean()), float(np.abs(out["depth"][0].astype(np.float64) - depth)[ok].max()),
            max(float(np.abs(out["normals"][0, j].astype(np.float64) - n[j])[ok].max()) for j in range(3)))


def test_a_plane_seen_at_25_degrees_gives_the_analytic_depth_and_normal():
    """40^3 grid points, the plane z = 2.5 fused from three identity-rotation cameras (the projective value is the signed distance,
    so the field is exactly linear within trunc), ray cast with the defaults from a 48 x 64 camera turned 25 degrees about y."""
    E, k, hw = RC.plane_camera()
    vol = RC.volume(("plane",))
    rows = E[:, :3].astype(np.float32)
    res = {}
    for dtype in (np.float64, np.float32):
        out = RR.raycast(vol, rows, k, hw, dtype)
        res[dtype] = plane_errors(out)
        print(f"plane, {dtype.__name__}: valid share {res[dtype][0]:.3f}, max |depth - analytic| = {res[dtype][1]:.2e}, "
              f"max |normal - analytic| = {res[dtype][2]:.2e}, at most {int(out['steps'].max())} samples")
        assert np.array_equal(out["valid"], out["hit"]) and bool((out["depth"][~out["hit"]] == 0).all())
        assert bool(np.isnan(out["normals"][0][:, ~out["valid"][0]]).all())
    share, d_err, n_err = res[np.float32]
    assert share > 0.5
    assert d_err <= PLANE_DEPTH_BOUND and n_err <= PLANE_NORMAL_BOUND
    assert res[np.float64][1] <= PLANE_DEPTH_BOUND / 10 and res[np.float64][2] <= PLANE_NORMAL_BOUND / 10


def test_a_fused_sphere_is_hit_everywhere_away_from_its_silhouette():
    """A sphere of radius 12 voxels fused from fourteen views, seen from a new 96 x 128 camera: every ray that meets the analytic
    sphere at an incidence cosine above 0.3 is a hit, and the median depth error is below one voxel.  The error that remains (this
    restatement: median 0.20, 95th percentile 0.64, maximum 2.8 voxels, the maximum at the silhouette) is a property of
    nearest-pixel projective fusion -- a grid point behind a fusing camera's silhouette takes that camera's projective value --,
    not of the march: on the plane scene above, where the fused value is the distance, the same march is exact to 3e-7."""
    E, k, hw, centre, radius = RC.sphere_camera()
    vol = RC.volume(("sphere",))
    out = RR.raycast(vol, E[:, :3].astype(np.float32), k, hw)
    D, cosine = RC.sphere_depth(E[0], k[0].astype(np.float64), hw[0], hw[1], centre, radius)
    hit, ana = out["hit"][0], np.isfinite(D)
    err = (np.abs(out["depth"][0] - D) / vol["voxel_size"])[hit & ana]
    print(f"sphere: hit share {hit.mean():.3f}, analytic {ana.mean():.3f}; depth error in voxels: median {np.median(err):.2f}, 95th percentile "
          f"{np.percentile(err, 95):.2f}, maximum {err.max():.2f}; {out['steps'].mean():.1f} samples per ray, at most {out['steps'].max()}")
    assert int(ana.sum()) > 5000 and not bool((ana & (cosine > 0.3) & ~hit).any())
    assert float(np.median(err)) < 1.0
    n = out["normals"][0][:, out["valid"][0]]
    assert bool(np.allclose((n.astype(np.float64) ** 2).sum(0), 1.0, atol=1e-6)) and float(np.median(n[2])) > 0.5     # towards the camera


# ---- 2. fp32 against float64 -----------------------------------------------------------------------------------------------------

# max |depth_fp32 - depth_float64| over the pixels of a case on which both runs take the same decisions, as measured with this
# restatement; the test allows 10 x as much.  (The cases with noisy fused fields are the ill-conditioned ones: a flat
# crossing moves far for a small change of the values.)
DEPTH_ERR_MEASURED = {
    "one cell 1x1": 2.4e-8, "(5,3,2) 5x7 V=3 fusing/inside/away": 3.7e-8, "(33,9,5) 17x33 V=3 refine=0": 3.8e-7,
    "(70,17,9) 17x33 V=3 fusing/between/away": 8.3e-7, "(70,17,9) 5x7 max_steps=3": 8.6e-8, "no cell (5,1,4) 5x7": 0.0,
    "holes 17x33 axis-parallel": 1.3e-7, "plane 5x7 axis-parallel": 1.5e-8, "plane 48x64 turned 25 degrees": 3.0e-7,
    "sphere 17x33": 8.0e-7,
}


@pytest.mark.parametrize("name", RC.NAMES)
def test_fp32_restatement_against_float64(name):
    """At most 1 % of a case's pixels may be left out because the two precisions decide differently (hit, march samples, a
    refinement branch, validity); on the others depth agrees within 10 x the measured figure, normals and colour within 1e-4
    (their conditioning is the field's, not the march's: a sanity bound), and the NaN / 0 patterns are the same."""
    a, b = RC.reference(name), RC.reference(name, np.float64)
    agree = RR.decisions_agree(a, b)
    left_out = int((~agree).sum())
    both = agree & a["hit"]
    with np.errstate(invalid="ignore"):
        d = np.abs(a["depth"].astype(np.float64) - b["depth"])[both]
    nan_a, nan_b = np.isnan(a["depth"][both]), np.isnan(b["depth"][both])
    assert np.array_equal(nan_a, nan_b)                                       # (a NaN value in the bracket: both runs give NaN)
    err = float(d[~nan_a].max()) if (~nan_a).any() else 0.0
    print(f"{name}: {left_out} of {agree.size} pixels left out, {int(both.sum())} hits compared, max |depth - float64| = {err:.2e}")
    assert left_out <= 0.01 * agree.size
    assert err <= 10 * DEPTH_ERR_MEASURED[name]
    assert bool((a["depth"][~a["hit"]] == 0).all())
    ok = agree & a["valid"]
    for key in ("normals", "color"):
        if a[key] is None:
            assert b[key] is None
            continue
        sel = np.broadcast_to(ok[:, None], a[key].shape)
        if sel.any():
            assert float(np.abs(a[key].astype(np.float64) - b[key])[sel].max()) <= 1e-4, key
    assert bool(np.isnan(a["normals"][np.broadcast_to(~a["valid"][:, None], a["normals"].shape)]).all())
    if a["color"] is not None:
        assert bool((a["color"][np.broadcast_to(~a["valid"][:, None], a["color"].shape)] == 0).all())


def test_the_case_list_covers_what_the_kernel_branches_on():
    cases = [RC.case(n) for n in RC.NAMES]
    refs = [RC.reference(n) for n in RC.NAMES]
    hws = {c["hw"] for c in cases}
    assert (1, 1) in hws and any(h % RC.TILE and w % RC.TILE and h < RC.TILE and w < RC.TILE for h, w in hws)
    assert any(h > RC.TILE and w > 2 * RC.TILE and h % 8 and w % 8 for h, w in hws)
    dims = {c["vol"]["dims"] for c in cases}
    assert {(2, 2, 2), (5, 3, 2), (33, 9, 5), (70, 17, 9)} <= dims and any(min(d) == 1 for d in dims)
    assert any(c["rows"].shape[0] == 3 and len({tuple(k) for k in c["intrinsics"]}) == 3 for c in cases)
    assert {0, 1, 2, 4} <= {c["params"].get("refine", 4) for c in cases}
    assert any(c["vol"]["color"] is not None for c in cases) and any(c["vol"]["color"] is None for c in cases)
    for c, r in zip(cases, refs):
        if min(c["vol"]["dims"]) == 1:
            assert not r["hit"].any() and not r["steps"].any() and np.isnan(r["normals"]).all() and not r["color"].any()
        if c["params"].get("max_steps") == 3:
            full = RR.raycast(c["vol"], c["rows"], c["intrinsics"], c["hw"], **dict(c["params"], max_steps=None))
            cut = (full["steps"] > 3) & full["hit"]
            assert cut.any() and not r["hit"][cut].any() and (r["steps"][cut] == 3).all() and int(r["steps"].max()) == 3
        if "away" in c["name"]:
            assert not r["steps"][2].any() and not r["hit"][2].any()           # the view that looks away: no ray alive
        if "inside" in c["name"]:
            v = 1 if "fusing/inside" in c["name"] else 2
            assert r["steps"][v].all()                                         # the camera inside the box: every ray alive
        if "axis-parallel" in c["name"]:
            k = c["intrinsics"][0]
            assert float(k[2]) == int(k[2]) and float(k[3]) == int(k[3]) and np.array_equal(c["c2w"][0, :3, :3], np.eye(3))
    holes = RC.volume(("holes",))
    assert np.isnan(holes["tsdf"]).any() and np.isnan(holes["weight"]).any() and (holes["weight"] == 0).any()
    r = RC.reference("holes 17x33 axis-parallel")
    assert r["hit"].any() and (r["hit"] & ~r["valid"]).any() and (~r["hit"] & (r["steps"] > 0)).any()
    assert sum(int(x["hit"].sum()) for x in refs) > 3000


# ---- 3. the C boundary -----------------------------------------------------------------------------------------------------------

P = C.c_void_p(4096)      # a fake non-NULL pointer: nothing may launch with it
INF, NAN = math.inf, math.nan


def _cast(L, dims=(8, 8, 8), origin=(0.0, 0.0, 0.0), vs=0.1, trunc=0.3, vol=(P, P, None), V=2, H=16, W=16, cams=(P, P),
          sc=(0.0, INF, 1.0, 0.5, 0.8), refine=4, max_steps=96, out=(P, None, None, None)):
    """vol = (tsdf, weight, color); cams = (cam_to_world, intrinsics); sc = (min_depth, max_depth, min_weight, step_min, relax);
    out = (depth, normals, color, steps)."""
    return L.fs_tsdf_raycast(*dims, *origin, vs, trunc, *vol, V, H, W, *cams, *sc, refine, max_steps, *out, None)


def test_raycast_header_is_exported_and_bound():
    from freesplat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    names = declared_names(HEADER)
    assert names == ["fs_raycast_api_version", "fs_tsdf_raycast"]
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/{HEADER} but not exported"
    assert set(_lib.RAYCAST_SIGNATURES) == set(names)
    assert _lib.lib().fs_raycast_api_version() == 1 == _lib.RAYCAST_API_VERSION
    text = header_text(HEADER)
    for macro, value in (("FS_RAYCAST_API_VERSION", 1), ("FS_RAYCAST_TILE", _lib.RAYCAST_TILE), ("FS_RAYCAST_MAX_REFINE", _lib.RAYCAST_MAX_REFINE)):
        assert re.search(rf"#define\s+{macro}\s+{value}\b", text), macro
    assert re.search(r"#define\s+FS_RAYCAST_MAX_STEPS\s+\(1 << 20\)", text) and _lib.RAYCAST_MAX_STEPS == 1 << 20
    assert RC.TILE == _lib.RAYCAST_TILE


def test_the_entry_point_validates_before_touching_a_device():
    """FS_ERR_INVALID_ARG (-1) and FS_ERR_UNSUPPORTED (-3) for every condition the header lists, with fake non-NULL pointers, so
    nothing may launch; an invalid argument is answered before an unsupported size."""
    from freesplat_amd import _lib
    L = _lib.lib()
    for i in range(3):
        for bad in (0, -1):
            assert _cast(L, dims=tuple(bad if k == i else 8 for k in range(3))) == -1
    for bad in (dict(V=0), dict(V=-1), dict(H=0), dict(H=-3), dict(W=0), dict(W=-2)):
        assert _cast(L, **bad) == -1, bad
    assert _cast(L, vol=(None, P, None)) == -1 and _cast(L, vol=(P, None, None)) == -1
    assert _cast(L, cams=(None, P)) == -1 and _cast(L, cams=(P, None)) == -1
    assert _cast(L, out=(None, P, None, P)) == -1                              # depth is required
    assert _cast(L, out=(P, None, P, None)) == -1                              # a colour map without colour planes
    for i in range(3):
        for bad in (NAN, INF, -INF):
            assert _cast(L, origin=tuple(bad if k == i else 0.0 for k in range(3))) == -1
    for bad in (0.0, -1.0, INF, NAN):
        assert _cast(L, vs=bad) == -1 and _cast(L, trunc=bad) == -1, bad
        assert _cast(L, sc=(0.0, INF, 1.0, bad, 0.8)) == -1 and _cast(L, sc=(0.0, INF, 1.0, 0.5, bad)) == -1, bad
    for bad in (NAN, -1e-3, -INF):
        assert _cast(L, sc=(bad, INF, 1.0, 0.5, 0.8)) == -1, bad
    assert _cast(L, sc=(0.0, NAN, 1.0, 0.5, 0.8)) == -1
    for bad in (NAN, 0.0, -1.0):
        assert _cast(L, sc=(0.0, INF, bad, 0.5, 0.8)) == -1, bad
    for bad in (-1, 33):
        assert _cast(L, refine=bad) == -1
    for bad in (0, -1, (1 << 20) + 1):
        assert _cast(L, max_steps=bad) == -1
    big = (2048, 1024, 1024)                                                   # 2^31 grid points
    assert _cast(L, dims=big) == -3 and _cast(L, dims=(2 ** 20, 2 ** 20, 1)) == -3
    assert _cast(L, H=46341, W=46341) == -3
    assert _cast(L, V=2 ** 31 - 1, H=17, W=17) == -3                           # more than 2^31 - 1 workgroups
    for bad in (dict(vs=NAN), dict(refine=33), dict(max_steps=0), dict(out=(None, None, None, None)), dict(cams=(None, P)),
                dict(sc=(-1.0, INF, 1.0, 0.5, 0.8))):
        assert _cast(L, dims=big, **bad) == -1 and _cast(L, H=46341, W=46341, **bad) == -1, bad


# ---- 4. the Python layer's refusals that need no device -----------------------------------------------------------------------

def test_argument_errors_without_a_device():
    from freesplat_amd import tsdf as T
    f = torch.ones(3, 4, 5)
    col = torch.ones(3, 3, 4, 5)
    k, E = (8.0, 8.0, 3.5, 2.5), torch.eye(4, dtype=torch.float64).repeat(2, 1, 1)
    cast = lambda *a, **kw: T.raycast(*a, **kw)
    with pytest.raises(ValueError, match="freesplat_amd.tsdf.*no CPU path"):
        cast(f, f, None, (0, 0, 0), 0.1, 0.3, k, E, (6, 8))                  # a CPU volume
    refused = [(dict(hw=(6,)), "hw must"), (dict(hw=(0, 8)), "hw must"), (dict(hw=(6, -1)), "hw must"), (dict(hw=6), "hw must"),
               (dict(hw=(46341, 46341)), "hw must"), (dict(tsdf=f[0]), "tsdf and weight"), (dict(weight=torch.ones(3, 4, 6)), "tsdf and weight"),
               (dict(tsdf=torch.ones(0, 4, 5), weight=torch.ones(0, 4, 5)), "tsdf and weight"),
               (dict(color=torch.ones(3, 3, 4, 6)), "color must be"), (dict(color=torch.ones(3, 4, 5)), "color must be"),
               (dict(origin=(0.0, math.nan, 0.0)), "origin"), (dict(origin=(0.0, 0.0)), "origin"), (dict(voxel_size=0.0), "voxel_size"),
               (dict(trunc=math.inf), "trunc"), (dict(step_min=0.0), "step_min"), (dict(relax=-1.0), "relax"), (dict(relax=math.nan), "relax"),
               (dict(min_depth=-1.0), "min_depth"), (dict(min_depth=math.nan), "min_depth"), (dict(max_depth=math.nan), "max_depth"),
               (dict(min_weight=0.0), "min_weight"), (dict(min_weight=math.nan), "min_weight"), (dict(refine=-1), "refine"),
               (dict(refine=33), "refine"), (dict(max_steps=0), "max_steps"), (dict(max_steps=(1 << 20) + 1), "max_steps"),
               (dict(color_out=True), "colour map")]
    for bad, what in refused:
        args = dict(tsdf=f, weight=f, color=None, origin=(0, 0, 0), voxel_size=0.1, trunc=0.3, intrinsics=k, extrinsics=E, hw=(6, 8))
        args.update(bad)
        with pytest.raises(ValueError, match=f"freesplat_amd.tsdf: .*{what}"):
            cast(**args)
    with pytest.raises(ValueError, match="colour map needs a volume with colour"):
        cast(f, f, None, (0, 0, 0), 0.1, 0.3, k, E, (6, 8), color_out=True)
    for t, what in ((dict(tsdf=f.clone().requires_grad_(True)), "tsdf"), (dict(weight=f.clone().requires_grad_(True)), "weight"),
                    (dict(color=col.clone().requires_grad_(True)), "color"),
                    (dict(intrinsics=torch.tensor(k).requires_grad_(True)), "intrinsics")):
        args = dict(tsdf=f, weight=f, color=col, origin=(0, 0, 0), voxel_size=0.1, trunc=0.3, intrinsics=k, extrinsics=E, hw=(6, 8))
        args.update(t)
        with pytest.raises(RuntimeError, match=f"{what} gets no gradient"):
            cast(**args)
    # the camera rows: as given, validated on the host only
    E[1, :3, 3] = torch.tensor([1.0, -2.0, 0.5])
    rows = T.cam_rows(E, "cpu")
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (2, 3, 4) and torch.equal(rows, E[:, :3].float())
    for bad in (E[0], E[:, :3], torch.zeros(0, 4, 4)):
        with pytest.raises(ValueError, match=r"camera-to-world \[V, 4, 4\]"):
            T.cam_rows(bad, "cpu")
    nanE, rowE = E.clone(), E.clone()
    nanE[0, 0, 0], rowE[0, 3, 0] = math.nan, 1.0
    for bad in (nanE, rowE):
        with pytest.raises(ValueError, match="last row"):
            T.cam_rows(bad, "cpu")
    with pytest.raises(RuntimeError, match="extrinsics gets no gradient"):
        T.cam_rows(E.clone().requires_grad_(True), "cpu")
