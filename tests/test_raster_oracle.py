"""CPU tests that pin the rasterizer ORACLE itself (the reference has no golden vectors for this
boundary -- SURVEY.md 8(c)): closed-form known answers, an independent float64 torch restatement,
and autograd for the hand-derived backward.

The test_edge_* tests ask the oracle about the branches the wall scene never takes (util_raster.edge_scene: clamped SH
colours, the Jacobian's frustum clamp, the near cull, zero covariances, opacities below 1/255 and above 0.99), judged per
Gaussian (util_raster.per_gaussian_err) against float64 autograd of the dense restatement.  Bounds: twice the figures measured
on the CPU (util_raster.EDGE_ORACLE_VS_F64)."""
import math

import numpy as np
import pytest
import torch

from oracle import raster_oracle as ro
from oracle.raster_dense_torch import render_dense
from util_framing import _frame
from util_raster import (EDGE_ORACLE_VS_F64, EDGE_TOL_CPU, assert_edge_cases_present, colour_key, dead_rows,
                         chain_scale_rot, dense_reference, edge_dense_reference, edge_scale_rot, edge_oracle_backward, edge_view, max_abs_err, oracle_forward,
                         per_gaussian_err, small_scene, view_inputs)

C0 = 0.28209479177387814


def test_exp_accuracy():
    L = ro.lib()
    xs = np.concatenate([np.linspace(-80, 0, 4001), -np.logspace(-8, 1.5, 500)]).astype(np.float32)
    got = np.array([L.fso_exp_public(float(x)) for x in xs], np.float64)
    ref = np.exp(xs.astype(np.float64))
    rel = np.abs(got - ref) / ref
    # alpha = opacity * exp(power) can reach the 1/255 threshold only for power >= -5.55: that is where the accuracy
    # matters (one-fma reduction: 1.7e-7 there; the |n| > 8 of the far tail add up to 2e-7 more, on alphas < 1e-3 / 255)
    assert rel[xs >= -6.0].max() < 2e-7
    assert rel.max() < 4e-7
    assert L.fso_exp_public(-100.0) == 0.0
    assert L.fso_exp_public(0.0) == 1.0


def _axis_camera(H, W, near=0.5, far=15.0):
    """Identity pose, normalised fx=fy=1 (tan(fov/2) = 0.5), framed like render_cuda does."""
    extr = torch.eye(4)[None]
    K = torch.tensor([[[1.0, 0, 0.5], [0, 1.0, 0.5], [0, 0, 1]]])
    e, scale, tx, ty, view, full = _frame(extr, K, torch.tensor([near]), torch.tensor([far]), True)
    return dict(H=H, W=W, tanfovx=float(tx[0]), tanfovy=float(ty[0]), viewmatrix=view[0], projmatrix=full[0],
                campos=e[0, :3, 3], scale=float(scale[0]))


def _iso(vi, pos, sigma, opacity, dc, bg=(0.0, 0.0, 0.0)):
    """Isotropic Gaussians at world `pos` (pre-scale), world sigma, DC-only SH."""
    s = vi["scale"]
    pos = torch.tensor(pos, dtype=torch.float32).reshape(-1, 3) * s
    n = pos.shape[0]
    sig = torch.tensor(sigma, dtype=torch.float32).reshape(n) * s
    cov = torch.zeros(n, 6)
    cov[:, 0] = cov[:, 3] = cov[:, 5] = sig ** 2
    shs = torch.zeros(n, 9, 3)
    shs[:, 0, :] = torch.tensor(dc, dtype=torch.float32).reshape(n, 3)
    d = dict(vi)
    d.update(bg=torch.tensor(bg), sh_degree=2, means3D=pos, cov3D=cov, shs=shs,
             opacities=torch.tensor(opacity, dtype=torch.float32).reshape(n))
    return d


def test_kat_single_isotropic_gaussian():
    H = W = 32
    vi = _iso(_axis_camera(H, W), [[0, 0, 2.0]], [0.08], [0.8], [[0.5, -0.2, 1.0]], bg=(0.1, 0.2, 0.3))
    st = oracle_forward(vi)
    fx = W / (2 * vi["tanfovx"])
    z = 2.0 * vi["scale"]
    var = (fx / z) ** 2 * (0.08 * vi["scale"]) ** 2 + 0.3
    ys, xs = np.mgrid[0:H, 0:W]
    d2 = (xs - 15.5) ** 2 + (ys - 15.5) ** 2
    alpha = np.minimum(0.99, 0.8 * np.exp(-0.5 * d2 / var))
    alpha[alpha < 1 / 255] = 0
    col = np.maximum(np.array([0.5, -0.2, 1.0]) * C0 + 0.5, 0)
    bg = np.array([0.1, 0.2, 0.3])
    exp_color = col[:, None, None] * alpha[None] + (1 - alpha)[None] * bg[:, None, None]
    assert st["radii"][0] == math.ceil(3 * math.sqrt(var))
    assert st["num_rendered"] == 4
    np.testing.assert_allclose(st["means2D"][0], [15.5, 15.5], atol=1e-4)
    np.testing.assert_allclose(st["color"], exp_color, atol=2e-6)
    np.testing.assert_allclose(st["depth"], z * alpha, atol=1e-5)
    np.testing.assert_allclose(st["alpha"], alpha, atol=2e-6)
    np.testing.assert_array_equal(st["n_contrib"], (alpha > 0).astype(np.int32))


def test_kat_two_gaussians_order_and_depth():
    H = W = 32
    vi = _iso(_axis_camera(H, W), [[0, 0, 3.0], [0.0, 0.0, 1.5]], [0.15, 0.06], [0.7, 0.6],
              [[1.0, 0, 0], [0, 1.0, 0]])
    st = oracle_forward(vi)
    # gaussian 1 (id 1) is nearer -> drawn first in every tile
    for t in range(4):
        a, b = st["ranges"][t]
        assert list(st["point_list"][a:b]) == [1, 0]
    s = vi["scale"]
    fx = W / (2 * vi["tanfovx"])
    ys, xs = np.mgrid[0:H, 0:W]

    def alpha_of(pos, sig, op):
        z = pos[2] * s
        var = (fx / z) ** 2 * (sig * s) ** 2 + 0.3
        cx = fx * pos[0] / pos[2] + 15.5
        cy = fx * pos[1] / pos[2] + 15.5
        a = np.minimum(0.99, op * np.exp(-0.5 * ((xs - cx) ** 2 + (ys - cy) ** 2) / var))
        a[a < 1 / 255] = 0
        return a, z

    a_near, z_near = alpha_of([0.0, 0, 1.5], 0.06, 0.6)
    a_far, z_far = alpha_of([0, 0, 3.0], 0.15, 0.7)
    c_near = np.maximum(np.array([0, 1.0, 0]) * C0 + 0.5, 0)
    c_far = np.maximum(np.array([1.0, 0, 0]) * C0 + 0.5, 0)
    exp = c_near[:, None, None] * a_near + c_far[:, None, None] * (a_far * (1 - a_near))
    np.testing.assert_allclose(st["color"], exp, atol=3e-6)
    np.testing.assert_allclose(st["depth"], z_near * a_near + z_far * a_far * (1 - a_near), atol=2e-5)
    # swapping the draw order would give a different image (order-dependent blend)
    wrong = c_far[:, None, None] * a_far + c_near[:, None, None] * (a_near * (1 - a_far))
    assert np.abs(wrong - exp).max() > 1e-2


def test_kat_near_cull_and_empty():
    H = W = 32
    cam = _axis_camera(H, W)
    # view-space z (after the 1/near rescale) <= 0.2 is culled: world z = 0.1 -> 0.2 exactly
    vi = _iso(cam, [[0, 0, 0.1], [0, 0, -1.0]], [0.05, 0.05], [0.9, 0.9], [[1, 1, 1], [1, 1, 1]], bg=(0.3, 0.1, 0.2))
    st = oracle_forward(vi)
    assert st["num_rendered"] == 0 and (st["radii"] == 0).all()
    np.testing.assert_array_equal(st["color"], np.broadcast_to(np.array([0.3, 0.1, 0.2], np.float32)[:, None, None], (3, H, W)))
    assert (st["depth"] == 0).all() and (st["n_contrib"] == 0).all() and (st["final_T"] == 1).all()


def test_transmittance_cutoff_and_alpha_cap():
    H = W = 16
    cam = _axis_camera(H, W)
    n = 12
    pos = [[0, 0, 1.0 + 0.1 * i] for i in range(n)]
    vi = _iso(cam, pos, [0.5] * n, [5.0] * n, [[1, 1, 1]] * n)  # opacity 5 -> alpha capped at 0.99
    st = oracle_forward(vi)
    # alpha = 0.99f for every Gaussian; T after the first = 1 - 0.99f = 0.00999999; the second would
    # give 0.00999999^2 = 9.99998e-5 < 1e-4 -> the pixel stops BEFORE applying it (App. A.4)
    assert (st["n_contrib"] == 1).all()
    np.testing.assert_allclose(st["final_T"], 1.0 - np.float32(0.99), rtol=1e-6)
    np.testing.assert_allclose(st["alpha"], 0.99, rtol=1e-6)


@pytest.mark.parametrize("sh_degree,precomp", [(2, False), (3, False), (0, False), (1, True)])
def test_dense_float64_restatement_matches(sh_degree, precomp):
    H, W = 40, 56
    scene, cams = small_scene(N=300, H=H, W=W, seed=11 + sh_degree, sh_degree=max(sh_degree, 0))
    vi = view_inputs(scene, cams, 1, H, W, bg=(0.2, 0.4, 0.6))
    if precomp:
        vi["colors_precomp"] = vi["shs"][:, 0, :].abs().contiguous()
        vi["shs"] = None
    st = oracle_forward(vi)
    assert st["num_rendered"] > 300
    f64 = lambda t: None if t is None else t.double()
    order = torch.from_numpy(np.lexsort((np.arange(st["N"]), st["depths"].view(np.uint32))).astype(np.int64))
    color, depth, _ = render_dense(H, W, vi["tanfovx"], vi["tanfovy"], vi["bg"], vi["viewmatrix"], vi["projmatrix"],
                                   vi["sh_degree"], vi["campos"], f64(vi["means3D"]), f64(vi["cov3D"]),
                                   f64(vi["opacities"]), shs=f64(vi.get("shs")),
                                   colors_precomp=f64(vi.get("colors_precomp")),
                                   rect=torch.from_numpy(st["rect"]), radii=torch.from_numpy(st["radii"]), order=order)
    np.testing.assert_allclose(st["color"], color.numpy(), atol=2e-5)
    np.testing.assert_allclose(st["depth"], depth.numpy(), atol=1e-4)


def test_binning_invariants():
    H, W = 72, 100  # ragged: not multiples of 16
    scene, cams = small_scene(N=2000, H=H, W=W, seed=3)
    vi = view_inputs(scene, cams, 0, H, W)
    st = oracle_forward(vi)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    assert st["ranges"].shape == (gx * gy, 2)
    assert st["ranges"][0, 0] == 0 and st["ranges"][-1, 1] == st["num_rendered"] == st["tiles_touched"].sum()
    assert (st["ranges"][1:, 0] == st["ranges"][:-1, 1]).all()
    dbits = st["depths"].view(np.uint32)
    for t in range(gx * gy):
        a, b = st["ranges"][t]
        ids = st["point_list"][a:b].astype(np.int64)
        key = dbits[ids].astype(np.int64) << 32 | ids
        assert (np.diff(key) > 0).all()
        tx, ty = t % gx, t // gx
        r = st["rect"][ids]
        assert ((r[:, 0] <= tx) & (tx < r[:, 2]) & (r[:, 1] <= ty) & (ty < r[:, 3])).all()


@pytest.mark.parametrize("sh_degree,precomp,with_depth", [(2, False, True), (3, False, False), (1, True, True)])
def test_backward_matches_autograd_of_dense(sh_degree, precomp, with_depth):
    H, W = 32, 48
    scene, cams = small_scene(N=60, H=H, W=W, seed=21 + sh_degree, sh_degree=sh_degree)
    scene["opacities"] = scene["opacities"].clamp(0.05, 0.9)
    vi = view_inputs(scene, cams, 0, H, W, bg=(0.3, 0.5, 0.1))
    if precomp:
        vi["colors_precomp"] = (vi["shs"][:, 0, :] * 0.5 + 0.5).contiguous()
        vi["shs"] = None
    st = oracle_forward(vi)
    rng = np.random.default_rng(0)
    g_color = rng.normal(size=(3, H, W)).astype(np.float32)
    g_depth = rng.normal(size=(H, W)).astype(np.float32) if with_depth else None
    got = ro.backward(st, g_color, g_depth)

    leaf = lambda t: None if t is None else t.double().clone().requires_grad_(True)
    m, c, o = leaf(vi["means3D"]), leaf(vi["cov3D"]), leaf(vi["opacities"])
    s, cp = leaf(vi.get("shs")), leaf(vi.get("colors_precomp"))
    order = torch.from_numpy(np.lexsort((np.arange(st["N"]), st["depths"].view(np.uint32))).astype(np.int64))
    color, depth, (px, py) = render_dense(H, W, vi["tanfovx"], vi["tanfovy"], vi["bg"], vi["viewmatrix"],
                                           vi["projmatrix"], vi["sh_degree"], vi["campos"], m, c, o, shs=s,
                                           colors_precomp=cp, rect=torch.from_numpy(st["rect"]),
                                           radii=torch.from_numpy(st["radii"]), order=order)
    np.testing.assert_allclose(st["color"], color.detach().numpy(), atol=2e-5)
    px.retain_grad(); py.retain_grad()
    loss = (color * torch.from_numpy(g_color).double()).sum()
    if with_depth:
        loss = loss + (depth * torch.from_numpy(g_depth).double()).sum()
    loss.backward()

    def close(a, b, name):
        b = b.numpy()
        scale = np.abs(b).max() + 1e-12
        err = np.abs(a - b).max() / scale
        assert err < 2e-4, f"{name}: rel-to-max err {err}"

    close(got["means3D"], m.grad, "means3D")
    close(got["cov3D"], c.grad, "cov3D")
    close(got["opacities"], o.grad, "opacities")
    if precomp:
        close(got["colors_precomp"], cp.grad, "colors")
    else:
        close(got["shs"], s.grad, "shs")


def test_backward_matches_finite_differences_of_dense():
    """the hand-derived backward of the C oracle against central finite differences of the
    float64 dense restatement (the discrete pieces -- tile rects, radii, depth order -- held fixed), on a scene small
    enough to perturb parameter by parameter."""
    H, W = 24, 32
    scene, cams = small_scene(N=12, H=H, W=W, seed=77, sh_degree=1)
    scene["opacities"] = scene["opacities"].clamp(0.1, 0.8)
    vi = view_inputs(scene, cams, 0, H, W, bg=(0.2, 0.1, 0.3))
    st = oracle_forward(vi)
    rng = np.random.default_rng(3)
    g_color = rng.normal(size=(3, H, W)).astype(np.float32)
    got = ro.backward(st, g_color)
    order = torch.from_numpy(np.lexsort((np.arange(st["N"]), st["depths"].view(np.uint32))).astype(np.int64))
    gc = torch.from_numpy(g_color).double()

    def loss(m, c, o, s):
        color, _, _ = render_dense(H, W, vi["tanfovx"], vi["tanfovy"], vi["bg"], vi["viewmatrix"], vi["projmatrix"],
                                   vi["sh_degree"], vi["campos"], m, c, o, shs=s, rect=torch.from_numpy(st["rect"]),
                                   radii=torch.from_numpy(st["radii"]), order=order)
        return float((color * gc).sum())

    base = [vi[k].double().clone() for k in ("means3D", "cov3D", "opacities", "shs")]
    names = ("means3D", "cov3D", "opacities", "shs")
    for which, name in enumerate(names):
        flat = base[which].reshape(-1)
        ana = np.asarray(got[name], np.float64).reshape(-1)
        idx = rng.choice(flat.numel(), size=min(12, flat.numel()), replace=False)
        fd = np.zeros(len(idx))
        for j, i in enumerate(idx):
            h = 1e-5 * max(1.0, abs(float(flat[i])))
            args_p, args_m = [t.clone() for t in base], [t.clone() for t in base]
            args_p[which].reshape(-1)[i] += h
            args_m[which].reshape(-1)[i] -= h
            fd[j] = (loss(*args_p) - loss(*args_m)) / (2 * h)
        scale = np.abs(ana).max() + 1e-12
        assert np.abs(fd - ana[idx]).max() / scale < 2e-3, (name, fd, ana[idx])


EDGE_CASES = [(0, False), (1, False), (2, False), (3, False), (2, True)]


@pytest.mark.parametrize("sh_degree,precomp", EDGE_CASES)
def test_edge_backward_matches_float64_per_gaussian(sh_degree, precomp):
    """The oracle's fp32 backward on the edge scene (colour and depth cotangents) against float64 autograd of the dense
    restatement, per Gaussian.  Opacities in 0.05 - 0.9 so that fp32 and float64 take the same 1/255 and T < 1e-4
    decisions; at this seed no pixel flips and no Gaussian is excluded."""
    vi, st, g_color, g_depth = edge_view(sh_degree, precomp, "dense")
    counts = assert_edge_cases_present(vi, st, colours_clamp=not precomp)
    got, ref = edge_oracle_backward(sh_degree, precomp, "dense"), edge_dense_reference(sh_degree, precomp, "dense")
    np.testing.assert_allclose(st["color"], ref["color"], atol=2e-5)
    np.testing.assert_allclose(st["depth"], ref["depth"], atol=1e-4)
    ck = colour_key(vi)
    fig = {}
    for name, key in (("means3D", "means3D"), ("cov3D", "cov3D"), ("opacities", "opacities"), ("colour", ck)):
        assert np.isfinite(got[key]).all() and np.isfinite(ref[key]).all(), name
        fig[name] = per_gaussian_err(got[key], ref[key]) + (max_abs_err(got[key], ref[key]),)
    print(f"edge scene degree {sh_degree} precomp {precomp}: {counts}")
    print("oracle vs float64 (per-Gaussian error, worst Gaussian, error / tensor max-abs):",
          {k: f"{e:.2e} @{g} {m:.1e}" for k, (e, g, m) in fig.items()})
    for name, (e, g, _) in fig.items():
        assert e <= EDGE_TOL_CPU[name], f"{name}: per-Gaussian error {e:.3e} at Gaussian {g} (bound {EDGE_TOL_CPU[name]:.2e})"


def test_edge_backward_scale_rot_form_matches_float64_per_gaussian():
    """The (scales, rotations) form of the edge scene: covariances rebuilt from edge_scale_rot's rows (the zero rows stay
    zero), the oracle's dL/dcov3D and the float64 restatement's both chained through float64 build_cov3d."""
    from freesplat_amd.rasterizer import build_cov3d
    vi, _, g_color, g_depth = edge_view(2, False, "dense")
    sc, rq = edge_scale_rot(vi["cov3D"], vi["edge_rows"]["zero_cov"])
    vi = dict(vi, cov3D=build_cov3d(sc.double(), rq.double(), 1.0).float())
    st = oracle_forward(vi)
    assert_edge_cases_present(vi, st)
    got, ref = ro.backward(st, g_color, g_depth), dense_reference(vi, st, g_color, g_depth)
    got.update(chain_scale_rot(sc, rq, got["cov3D"]))
    ref.update(chain_scale_rot(sc, rq, ref["cov3D"]))
    fig = {name: per_gaussian_err(got[key], ref[key]) for name, key in (("means3D", "means3D"), ("cov3D", "cov3D"),
           ("opacities", "opacities"), ("colour", "shs"), ("scales", "scales"), ("rotations", "rotations"))}
    print("oracle vs float64, (scales, rotations) form:", {k: f"{e:.2e} @{g}" for k, (e, g) in fig.items()})
    for name, (e, g) in fig.items():
        assert e <= EDGE_TOL_CPU[name], f"{name}: per-Gaussian error {e:.3e} at Gaussian {g} (bound {EDGE_TOL_CPU[name]:.2e})"


@pytest.mark.parametrize("sh_degree,precomp", EDGE_CASES)
def test_edge_exact_zero_gradients(sh_degree, precomp):
    """No tolerance: a clamped colour channel gives every one of its SH coefficients gradient 0; a culled Gaussian and one
    whose opacity is below 1/255 get gradient 0 in every tensor; everything is finite.  Full opacity range."""
    vi, st, _, _ = edge_view(sh_degree, precomp, "full")
    assert_edge_cases_present(vi, st, colours_clamp=not precomp, low_opacity_visible=2, high_opacity_visible=2)
    got = edge_oracle_backward(sh_degree, precomp, "full")
    dead = dead_rows(vi, st)
    assert (st["radii"][dead] == 0).sum() >= 2 and (st["radii"][dead] > 0).sum() >= 2
    for key in ("means3D", "cov3D", "opacities", colour_key(vi), "means2D"):
        assert np.isfinite(got[key]).all(), key
        assert not got[key][dead].any(), key
        assert got[key][~dead].any(), key
    if not precomp:
        cl = st["clamped"].astype(bool)                                   # [N,3]
        assert not got["shs"][np.broadcast_to(cl[:, None, :], got["shs"].shape)].any()
        assert got["shs"][:, 0, :][~cl & ~dead[:, None]].any()


@pytest.mark.parametrize("switch,opacity,seen_in", [("sh_clamp_convention", "dense", ("colour", "means3D")),
                                                    ("jacobian_clamp", "dense", ("means3D", "cov3D", "opacities", "colour")),
                                                    ("alpha_cap_convention", "capped", ("opacities", "means3D", "cov3D"))])
def test_edge_scene_and_metric_see_each_convention(switch, opacity, seen_in):
    """Sensitivity, on the reference side so that nothing broken ever runs: with ONE emulated convention of the original
    switched off in the float64 restatement, the per-Gaussian error of the (unchanged) oracle exceeds the bound by 10x and
    more in the tensors the convention reaches -- a kernel that took that branch wrongly would be as far off.  The alpha
    cap needs o * G > 0.99, so its check runs on the "capped" scene (the dense one plus the three rows above 0.99), on
    which the unaltered reference is checked first.  Prints the tensor-wide max-abs figure (the older tests' metric, bar
    2e-4) of the same alteration beside it."""
    vi, st, g_color, g_depth = edge_view(2, False, opacity)
    assert_edge_cases_present(vi, st, high_opacity_visible=3 if opacity == "capped" else 0)
    got = edge_oracle_backward(2, False, opacity)
    plain = edge_dense_reference(2, False, opacity)
    altered = dense_reference(vi, st, g_color, g_depth, **{switch: False})
    for name in ("means3D", "cov3D", "opacities", "colour"):
        key = "shs" if name == "colour" else name
        base, _ = per_gaussian_err(got[key], plain[key])
        assert base <= EDGE_TOL_CPU[name], f"{name}: {base:.3e} against the unaltered reference"
        e, g = per_gaussian_err(got[key], altered[key])
        m = max_abs_err(got[key], altered[key])
        print(f"{switch} off, {name}: per-Gaussian {e:.2e} (Gaussian {g}) = {e / EDGE_TOL_CPU[name]:.0f}x the bound; "
              f"tensor-wide max-abs {m:.1e} ({'seen' if m >= 2e-4 else 'NOT seen'} at the 2e-4 bar)")
        if name in seen_in:
            assert e >= 10.0 * EDGE_TOL_CPU[name], f"{switch} off is invisible in {name}: {e:.3e}"
