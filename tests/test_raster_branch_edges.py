"""The rasterizer's backward at its branch edges, judged per Gaussian (GPU).

The other rasterizer tests draw a wall 1 - 5 m in front of the cameras with colours in 0.22 - 0.78: no colour channel is ever
clamped, the Jacobian's frustum clamp never acts, nothing comes near the near plane, and every gradient comparison divides by
the largest entry of the whole tensor.  These tests render util_raster.edge_scene (clamped SH colours, the frustum clamp on
+-x and +-y, view-space z exactly at / one ulp above / below the near cull and behind the camera, zero covariances, opacities
below 1/255 and above 0.99; 320 Gaussians = one full and one ragged block of preprocess_bwd, 40 x 56 pixels) and compare with
util_raster.per_gaussian_err, which scales every Gaussian's error by that Gaussian's own gradient.

Bounds (util_raster.EDGE_TOL_GPU): 4 x what the C oracle's fp32 backward measures against float64 autograd of the dense
restatement on the same scene on the CPU (util_raster.EDGE_ORACLE_VS_F64: means3D 5.64e-5, cov3D 2.29e-5, opacities 4.00e-4,
colour 1.08e-4, scales 1.64e-5, rotations 2.57e-5) -- the kernels share the oracle's fp32 arithmetic (the forward is
bit-equal) and differ in the order of the sums.  The same bound holds against the oracle and against float64 directly.  With
one convention of the original wrong for the Gaussians it touches the metric reads 5e-3 - 1
(test_raster_oracle.py::test_edge_scene_and_metric_see_each_convention).
"""
import numpy as np
import pytest
import torch

from util_raster import (EDGE_H, EDGE_N, EDGE_SEED, EDGE_TOL_GPU, EDGE_W, assert_edge_cases_present, chain_scale_rot,
                         colour_key, dead_rows, dense_reference, edge_dense_reference, edge_oracle_backward, edge_scale_rot,
                         edge_scene, edge_view, max_abs_err, oracle_forward, per_gaussian_err)

pytestmark = pytest.mark.gpu

H, W, N = EDGE_H, EDGE_W, EDGE_N


def _mode(monkeypatch, deterministic):
    from freesplat_amd import rasterizer as R
    monkeypatch.setattr(R, "DETERMINISTIC", deterministic)


def _judge(got: dict, ref: dict, names, what, figures):
    """per_gaussian_err of every tensor in `names` (pairs of bound name, key) within EDGE_TOL_GPU; figures are printed first."""
    fig = {n: per_gaussian_err(got[k], ref[k]) + (max_abs_err(got[k], ref[k]),) for n, k in names}
    figures[what] = {n: f"{e:.2e} @{g} ({m:.1e} of max-abs)" for n, (e, g, m) in fig.items()}
    print(f"{what}: {figures[what]}")
    for n, (e, g, _) in fig.items():
        assert e <= EDGE_TOL_GPU[n], f"{what}, {n}: per-Gaussian error {e:.3e} at Gaussian {g} (bound {EDGE_TOL_GPU[n]:.2e})"


def _single_view(dev, sh_degree, precomp, opacity, scale_rot):
    """One forward + backward of GaussianRasterizer on the edge scene; every assertion of the single-view tests."""
    import test_raster_scale_rot_alpha as sra
    from oracle import raster_oracle as ro
    vi, st, g_color, g_depth = edge_view(sh_degree, precomp, opacity)
    ck = colour_key(vi)
    names = [("means3D", "means3D"), ("opacities", "opacities"), ("colour", ck)]
    if scale_rot:
        sc, rq = edge_scale_rot(vi["cov3D"], vi["edge_rows"]["zero_cov"])
        vi = dict(vi, cov3D=sra._native_cov(torch.cat([sc, rq], 1).to(dev)).cpu())   # the covariance the kernels form
        st = oracle_forward(vi)
        ref = ro.backward(st, g_color, g_depth)
        ref.update(chain_scale_rot(sc, rq, ref["cov3D"]))
        form = dict(scales=sc, rotations=rq)
        names += [("scales", "scales"), ("rotations", "rotations")]
    else:
        ref = edge_oracle_backward(sh_degree, precomp, opacity)
        form = dict(cov3D_precomp=vi["cov3D"])
        names += [("cov3D", "cov3D")]
    full = opacity == "full"
    counts = assert_edge_cases_present(vi, st, colours_clamp=not precomp, low_opacity_visible=2 if full else 0,
                                       high_opacity_visible=2 if full else 0)
    (color, radii, depth, alpha), leaves = sra._render(vi, dev, requires_grad=True, **form)
    for x, key in ((color, "color"), (depth, "depth"), (alpha, "alpha"), (radii, "radii")):
        np.testing.assert_array_equal(x.detach().cpu().numpy(), st[key], err_msg=key)
    ((color * torch.from_numpy(g_color).to(dev)).sum() + (depth * torch.from_numpy(g_depth).to(dev)).sum()).backward()
    got = {k: t.grad.cpu().numpy() for k, t in leaves.items() if t is not None}
    got["cov3D"] = got.pop("cov3D_precomp", None)
    got["opacities"] = got["opacities"].reshape(N)
    figures = {}
    for k, g in got.items():
        if g is not None:
            assert np.isfinite(g).all(), k
    assert not got["means2D"][:, 2].any()
    _judge(got, ref, names, f"GPU vs oracle (degree {sh_degree}, precomp {precomp}, opacity {opacity}, scale_rot {scale_rot})", figures)
    assert max_abs_err(got["means2D"][:, :2], ref["means2D"]) <= 2e-4
    # exact: nothing reaches a culled Gaussian, one below 1/255, or the SH coefficients of a clamped channel
    dead = dead_rows(vi, st)
    assert dead.sum() >= 3
    for k, g in got.items():
        if g is not None:
            assert not g[dead].any(), f"{k}: a culled / transparent Gaussian has a gradient"
    if not precomp:
        cl = st["clamped"].astype(bool)
        assert not got["shs"][np.broadcast_to(cl[:, None, :], got["shs"].shape)].any()
        assert got["shs"][:, 0, :][~cl & ~dead[:, None]].any()
    if opacity == "dense":
        f64 = dense_reference(vi, st, g_color, g_depth) if scale_rot else edge_dense_reference(sh_degree, precomp, opacity)
        if scale_rot:
            f64.update(chain_scale_rot(sc, rq, f64["cov3D"]))
        _judge(got, f64, names, f"GPU vs float64 (degree {sh_degree}, precomp {precomp}, scale_rot {scale_rot})", figures)
    return counts, figures


@pytest.mark.parametrize("sh_degree,precomp,deterministic,scale_rot",
                         [(0, False, False, False), (1, False, False, False), (2, False, False, False),
                          (3, False, False, False), (2, True, False, False), (2, False, True, False),
                          (2, False, False, True)],
                         ids=["sh0", "sh1", "sh2", "sh3", "precomp", "sh2-deterministic", "sh2-scale_rot"])
def test_single_view_branch_edges(hip_device, monkeypatch, sh_degree, precomp, deterministic, scale_rot):
    """GaussianRasterizer on the edge scene.  Full opacity range: forward bit-equal to the oracle (colour, depth, alpha, radii),
    gradients per Gaussian against the oracle's backward, exact zeros for culled / transparent Gaussians and clamped channels,
    means2D.grad[:, 2] == 0, everything finite.  Opacities in 0.05 - 0.9: the same, and per Gaussian against float64 autograd
    of the dense restatement directly."""
    _mode(monkeypatch, deterministic)
    counts, _ = _single_view(hip_device, sh_degree, precomp, "full", scale_rot)
    print("edge scene, full opacity range:", counts)
    _single_view(hip_device, sh_degree, precomp, "dense", scale_rot)


# ------------------------------------------------------------------------------------------------------- three views
def _views_scene(form, dev):
    """The three-view edge scene (nears 0.5 / 1 / 0.25), its per-view oracle states with the presence conditions asserted, and
    the reference: the oracle's single-view backward of each view's framed inputs, summed over the views in float64 and
    mapped back to render_views' layouts.  The views are framed by frame_views on the device, as render_views frames them
    (test_raster_hip.py::test_render_views_equals_render_cuda_and_reference_framing): the oracle then sees the matrices the
    kernels see, bit for bit, and not the ulp-different ones of the CPU's fp32 chain.
    Returns (scene, cams, rows7 | None, cotangents, reference, per-view parts)."""
    from freesplat_amd.decoder import frame_views
    from freesplat_amd.rasterizer import build_cov3d
    from oracle import raster_oracle as ro
    scene, cams = edge_scene(N, H, W, EDGE_SEED, 3, 2, "full")
    rows = scene["edge_rows"]
    r_, c_ = torch.triu_indices(3, 3)
    sc = rq = None
    if form == "scale_rot":
        sc, rq = edge_scale_rot(scene["covariances"][:, r_, c_], rows["zero_cov"])
        S = torch.zeros(N, 3, 3)
        S[:, r_, c_] = build_cov3d(sc.double(), rq.double(), 1.0).float()
        scene["covariances"] = S + S.transpose(1, 2) - torch.diag_embed(torch.diagonal(S, dim1=1, dim2=2))
    campos, scale32, tanfov, view, full = (t.cpu() for t in frame_views(*(cams[k].to(dev) for k in
                                                                        ("extrinsics", "intrinsics", "near", "far"))))
    scale = scale32.double().numpy()
    g_color, g_depth, parts = [], [], []
    g_cull, g_clamp = rows["per_view_cull"][0], rows["per_view_clamp"][0]
    for i in range(3):
        vi = dict(H=H, W=W, tanfovx=float(tanfov[i, 0]), tanfovy=float(tanfov[i, 1]), bg=torch.full((3,), 0.2),
                  viewmatrix=view[i].contiguous(), projmatrix=full[i].contiguous(), campos=campos[i].contiguous(), sh_degree=2,
                  means3D=scene["means"] * scale32[i], cov3D=(scene["covariances"] * (scale32[i] * scale32[i]))[:, r_, c_].contiguous(),
                  shs=scene["harmonics"].transpose(-1, -2).contiguous(), opacities=scene["opacities"])
        st = oracle_forward(vi)
        n = assert_edge_cases_present(vi, st, **({} if i == 0 else dict(z_exactly_02_culled=0, z_one_ulp_above_02_drawn=0,
                                                                      z_below_02=0, behind=0, just_inside=0, just_outside=0)))
        V, m = vi["viewmatrix"].numpy(), vi["means3D"].numpy()[g_cull]
        pv = m[0] * V[0, :3] + m[1] * V[1, :3] + m[2] * V[2, :3] + V[3, :3]
        if i == 0:      # drawn, inside the clamp
            assert st["radii"][g_cull] > 0 and abs(pv[0] / pv[2]) < 1.3 * vi["tanfovx"] and st["clamped"][g_clamp, 0]
        elif i == 1:    # in front of the camera, inside the near cull
            assert st["radii"][g_cull] == 0 and 0 < pv[2] <= 0.2 and st["radii"][g_clamp] > 0
        else:           # drawn, frustum-clamped; the red channel of the other row is no longer clamped
            assert st["radii"][g_cull] > 0 and abs(pv[0] / pv[2]) > 1.3 * vi["tanfovx"]
            assert st["radii"][g_clamp] > 0 and not st["clamped"][g_clamp, 0]
        rng = np.random.default_rng(EDGE_SEED + 10 * i)
        g_color.append(rng.normal(size=(3, H, W)).astype(np.float32))
        g_depth.append(rng.normal(size=(H, W)).astype(np.float32))
        b = ro.backward(st, g_color[i], g_depth[i])
        cov33 = np.zeros((N, 3, 3))
        cov33[:, r_.numpy(), c_.numpy()] = b["cov3D"].astype(np.float64) * scale[i] ** 2
        parts.append(dict(means=b["means3D"].astype(np.float64) * scale[i], covariances=cov33, cov6=b["cov3D"].astype(np.float64) * scale[i] ** 2,
                          harmonics=b["shs"].astype(np.float64).transpose(0, 2, 1), opacities=b["opacities"].astype(np.float64)))
        print(f"edge scene view {i}:", n)
    ref = {k: sum(p[k] for p in parts) for k in parts[0]}
    if form == "scale_rot":
        ref.update(chain_scale_rot(sc, rq, ref["cov6"]))
        for p in parts:
            p.update(chain_scale_rot(sc, rq, p["cov6"]))
    rows7 = None if sc is None else torch.cat([sc, rq], 1)
    return scene, cams, rows7, (np.stack(g_color), np.stack(g_depth)), ref, parts


def _views_cov(dev, scene, cams, cot):
    """render_views (3x3 covariances) forward + backward: gradients in render_views' layouts."""
    from freesplat_amd.decoder import render_views
    g = {k: scene[k].to(dev).requires_grad_(True) for k in ("means", "covariances", "harmonics", "opacities")}
    cam = {k: t.to(dev) for k, t in cams.items()}
    color, depth = render_views(cam["extrinsics"], cam["intrinsics"], cam["near"], cam["far"], (H, W),
                                torch.full((3, 3), 0.2, device=dev), g["means"], g["covariances"], g["harmonics"], g["opacities"])
    loss = (color * torch.from_numpy(cot[0]).to(dev)).sum() + (depth[:, 0] * torch.from_numpy(cot[1]).to(dev)).sum()
    grads = torch.autograd.grad(loss, list(g.values()))
    return {k: t.detach().clone() for k, t in zip(g, grads)}


def _views_scale_rot(dev, scene, cams, rows7, cot):
    """rasterizer.rasterize_forward_views + rasterize_backward_views with FS_RASTER_SCALE_ROT rows [N,7] and shs [N,M,3], the
    launches decoder._RenderViews makes for the 3x3 form (render_views itself has no (scales, rotations) argument)."""
    from freesplat_amd import rasterizer as R
    from freesplat_amd.decoder import frame_views
    d = lambda t: t.to(dev).contiguous()
    means, rows7, opac = d(scene["means"]), d(rows7), d(scene["opacities"])
    shs = d(scene["harmonics"].transpose(1, 2))
    campos, scale, tanfov, view, full = frame_views(d(cams["extrinsics"]), d(cams["intrinsics"]), d(cams["near"]), d(cams["far"]))
    s0 = R.GaussianRasterizationSettings(H, W, 0.0, 0.0, None, 1.0, None, None, 2, None, False, False)
    dims = R.make_dims(N, shs.shape[1], s0, scale_rot=True)
    buf, _, _, _ = R.rasterize_forward_views(dims, means, rows7, shs, None, opac, torch.full((3, 3), 0.2, device=dev), view, full,
                                             campos, tanfov, scale, R.default_capacity(N, R._state(dev), H, W))
    assert not any(o for _, o in buf.counters.tolist()), "instance capacity overflow"
    out = R.rasterize_backward_views(buf, means, rows7, shs, None, opac, torch.from_numpy(cot[0]).to(dev),
                                     torch.from_numpy(cot[1]).to(dev))
    torch.cuda.synchronize()
    return dict(means=out["means3D"], scales=out["cov3D"][:, :3], rotations=out["cov3D"][:, 3:],
                harmonics=out["shs"].transpose(1, 2), opacities=out["opacities"], radii=buf.radii)


_VIEW_NAMES = dict(cov3D=[("means3D", "means"), ("cov3D", "covariances"), ("opacities", "opacities"), ("colour", "harmonics")],
                   scale_rot=[("means3D", "means"), ("scales", "scales"), ("rotations", "rotations"), ("opacities", "opacities"),
                              ("colour", "harmonics")])


@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("form", ["cov3D", "scale_rot"])
def test_three_views_branch_edges(hip_device, monkeypatch, form, deterministic):
    """The views entry points with three different 1/near rescales: gradients per Gaussian against the sum over the views of
    the oracle's single-view backwards.  The Gaussian that is drawn in view 0, near-culled in view 1 and frustum-clamped in
    view 2 gets the oracle's view-0 and view-2 contributions and nothing else; the lower triangle of the 3x3 covariance
    gradient is exactly zero."""
    _mode(monkeypatch, deterministic)
    scene, cams, rows7, cot, ref, parts = _views_scene(form, hip_device)
    g_cull = scene["edge_rows"]["per_view_cull"][0]
    if form == "cov3D":
        got = _views_cov(hip_device, scene, cams, cot)
        low = got["covariances"][:, [1, 2, 2], [0, 0, 1]]
        assert not low.any() and got["covariances"].any()
    else:
        got = _views_scale_rot(hip_device, scene, cams, rows7, cot)
        assert (got["radii"][1, g_cull] == 0) and (got["radii"][0, g_cull] > 0) and (got["radii"][2, g_cull] > 0)
    got = {k: t.cpu().numpy() for k, t in got.items()}
    for k, g in got.items():
        assert np.isfinite(g).all(), k
    _judge(got, ref, _VIEW_NAMES[form], f"three views, {form}, deterministic {deterministic}: GPU vs oracle summed", {})
    # view 1 gives that Gaussian exactly nothing; what it has is views 0 and 2
    only = np.zeros(N, bool)
    only[g_cull] = True
    for n, k in _VIEW_NAMES[form]:
        assert not parts[1][k][g_cull].any() and parts[0][k][g_cull].any() and parts[2][k][g_cull].any(), k
        e, _ = per_gaussian_err(got[k], parts[0][k] + parts[2][k], rows=only)
        assert e <= EDGE_TOL_GPU[n], f"{k} of the per-view Gaussian: {e:.3e}"
        e1, _ = per_gaussian_err(got[k], parts[0][k], rows=only)
        assert e1 > 10 * EDGE_TOL_GPU[n], f"{k}: view 2 adds nothing to tell apart ({e1:.3e})"


def test_three_views_chunked_rows_bit_equal(hip_device, monkeypatch):
    """The row-chunked per-Gaussian pass (fs_raster_backward_views_rows, through decoder.GRAD_EXCHANGE_HOOK as
    test_raster_deterministic.py::test_chunked_rows_and_view_by_view_paths reaches it) on the edge scene: the bits of the
    one-call deterministic backward.  Chunk borders fall inside both blocks of preprocess_bwd."""
    from freesplat_amd import decoder as D
    _mode(monkeypatch, True)
    scene, cams, _, cot, _, _ = _views_scene("cov3D", hip_device)
    want = _views_cov(hip_device, scene, cams, cot)

    class Hook:
        chunks = []

        def begin(self, n):
            pass

        def chunk_rows(self, n):
            b = [0, n // 3, 2 * n // 3, n]
            return list(zip(b[:-1], b[1:]))

        def chunk_ready(self, c0, c1, tensors):
            self.chunks.append((c0, c1))

    monkeypatch.setattr(D, "GRAD_EXCHANGE_HOOK", Hook())
    got = _views_cov(hip_device, scene, cams, cot)
    assert Hook.chunks == [(0, N // 3), (N // 3, 2 * N // 3), (2 * N // 3, N)]      # the chunked path was the one taken
    for k in want:
        assert torch.equal(want[k], got[k]), f"{k}: chunked rows differ (max {float((want[k] - got[k]).abs().max()):.3e})"
    assert any(bool(t.any()) for t in want.values())
