"""(scales, rotations) covariances (FS_RASTER_SCALE_ROT) and the gradient of the accumulated alpha (fs_raster_backward*_alpha).

CPU: the header and the binding declare the flag and the four entry points; they refuse NULL arguments, and the flag combined
with FS_RASTER_COV_FULL is refused before anything is launched.
GPU: fs_raster_cov3d_from_scale_rot against float64 build_cov3d; a (scales, rotations) render is bit-identical to the
cov3D_precomp render of that covariance and to the oracle's; its gradients match float64 autograd of build_cov3d chained with
the oracle's dL/dcov3D.  The alpha gradient matches the oracle's colour-0 backward with colors_precomp = 1 and bg = 0 (colour 0
then IS alpha); cotangents combine linearly; the views entry point equals the single-view one summed over the views; both new
paths are bitwise repeatable in the deterministic mode.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from freesplat_amd import _lib, synthetic
from util_raster import oracle_forward, small_scene, view_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fs_raster_backward_alpha", "fs_raster_backward_views_alpha", "fs_raster_backward_views_rows_alpha",
       "fs_raster_cov3d_from_scale_rot")
GRAD_TOL = 2e-4     # the rasterizer's gradient bar (tests/test_raster_hip.py): 2e-4 of each gradient's max-abs


def _dims(N, H, W, flags):
    d = _lib.RasterDims()
    d.N, d.M, d.H, d.W, d.sh_degree, d.tanfovx, d.tanfovy, d.flags = N, 0, H, W, 0, 0.5, 0.5, flags
    return d


def test_header_declares_the_flag_and_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "freesplat_amd.h")).read()
    assert re.search(r"#define FS_RASTER_SCALE_ROT 128\b", hdr)
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", hdr), name
    assert re.search(r"#define FS_ABI_VERSION 9\b", hdr)     # additive: the revision stays
    assert _lib.RASTER_SCALE_ROT == 128


def test_binding_lists_the_new_symbols_and_they_refuse_null_arguments():
    for name in NEW:
        assert name in _lib.SIGNATURES, name
    L = _lib.lib()
    for name in NEW:
        _, at = _lib.SIGNATURES[name]
        args = [1 if a in (C.c_int32, C.c_int64, C.c_int) else None for a in at]
        assert getattr(L, name)(*args) == -1, name
    d = _dims(100, 32, 32, _lib.RASTER_SCALE_ROT)
    strides = (C.c_size_t * 3)(1 << 20, 1 << 20, 1 << 20)
    assert L.fs_raster_backward_alpha(C.byref(d), *([None] * 25), 0, None) == -1
    assert L.fs_raster_backward_views_alpha(C.byref(d), 2, *([None] * 15), strides, *([None] * 10), 0, 0, None, None) == -1
    assert L.fs_raster_backward_views_rows_alpha(C.byref(d), 2, *([None] * 15), strides, *([None] * 10), 0, 0, None, None,
                                                 0, 100, 1) == -1
    assert L.fs_raster_cov3d_from_scale_rot(-1, None, None, None) == -1
    assert L.fs_raster_cov3d_from_scale_rot(0, None, None, None) == 0     # an empty job


def test_scale_rot_with_cov_full_is_refused_before_any_launch():
    """The two row layouts exclude each other: -1 before anything is launched, so fake non-NULL pointers are enough (as in
    tests/test_abi.py::test_cost_volume_rejects_maps_of_4GB_and_more)."""
    assert "fs_raster_cov3d_from_scale_rot" in _lib.SIGNATURES    # (a library without the check would launch on them)
    L = _lib.lib()
    p = C.c_void_p(4096)
    d = _dims(100, 32, 32, _lib.RASTER_SCALE_ROT | _lib.RASTER_COV_FULL | _lib.RASTER_TILE_CULL)
    s3, s4 = (C.c_size_t * 3)(1 << 20, 1 << 20, 1 << 20), (C.c_size_t * 4)(1 << 20, 1 << 20, 1 << 20, 1 << 20)
    # inputs: means3D, cov3D, shs = NULL, colors_precomp, opacities, bg, view, proj, campos, tanfov = NULL, scale = NULL
    ins = [p, p, None, p, p, p, p, p, p, None, None]
    assert L.fs_raster_forward(C.byref(d), *ins, p, p, p, p, 1 << 20, *([p] * 5), None) == -1
    assert L.fs_raster_forward_views(C.byref(d), 2, *ins, p, p, p, p, s4, 1 << 20, *([p] * 5), 0, None, None) == -1
    # outputs: dL_dmeans3D, dL_dmeans2D, dL_dcov3D, dL_dshs = NULL, dL_dcolors, dL_dopacities
    outs = [p, p, p, None, p, p]
    bwd = [p, p, p, p]                      # geom, binning, image, counters
    assert L.fs_raster_backward(C.byref(d), *ins, *bwd, p, p, p, *outs, 0, None) == -1
    assert L.fs_raster_backward_alpha(C.byref(d), *ins, *bwd, p, p, p, p, *outs, 0, None) == -1
    for fn, alpha in ((L.fs_raster_backward_views, []), (L.fs_raster_backward_views_alpha, [p])):
        assert fn(C.byref(d), 2, *ins, *bwd[:3], p, s3, p, p, *alpha, p, *outs, 0, 0, None, None) == -1
    for fn, alpha in ((L.fs_raster_backward_views_rows, []), (L.fs_raster_backward_views_rows_alpha, [p])):
        assert fn(C.byref(d), 2, *ins, *bwd[:3], p, s3, p, p, *alpha, p, *outs, 0, 0, None, None, 0, 100, 1) == -1


# ---------------------------------------------------------------------------------------------------------------- GPU
def _scale_rot_for(vi, seed):
    """(scales [N,3], rotations [N,4]) of the size of the view's covariances; quaternion norms in 0.5 - 2, random signs."""
    rng = np.random.default_rng(seed)
    cov = vi["cov3D"].numpy().astype(np.float64)
    N = cov.shape[0]
    size = np.sqrt(np.maximum((cov[:, 0] + cov[:, 3] + cov[:, 5]) / 3.0, 1e-12))
    scales = size[:, None] * rng.uniform(0.3, 1.7, (N, 3))
    q = rng.normal(size=(N, 4))
    q *= (rng.uniform(0.5, 2.0, N) / np.linalg.norm(q, axis=1))[:, None]
    return torch.from_numpy(scales.astype(np.float32)), torch.from_numpy(q.astype(np.float32))


def _native_cov(rows7: torch.Tensor) -> torch.Tensor:
    rows7 = rows7.contiguous()
    out = torch.empty(rows7.shape[0], 6, dtype=torch.float32, device=rows7.device)
    _lib.check(_lib.lib().fs_raster_cov3d_from_scale_rot(rows7.shape[0], _lib.ptr(rows7), _lib.ptr(out), _lib.current_stream()),
               "fs_raster_cov3d_from_scale_rot")
    return out


def _render(vi, dev, scale_modifier=1.0, requires_grad=False, **form):
    """GaussianRasterizer on `dev` with vi's means / colours / opacities and the covariance form in `form` (cov3D_precomp=, or
    scales= and rotations=); returns (outputs, leaves)."""
    from freesplat_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    d = lambda t: t.to(dev)
    leaf = lambda t: None if t is None else t.to(dev).clone().requires_grad_(requires_grad)
    leaves = {k: leaf(vi.get(k)) for k in ("means3D", "shs", "colors_precomp", "opacities")}
    leaves.update({k: leaf(v) for k, v in form.items()})
    leaves["means2D"] = torch.zeros(vi["means3D"].shape[0], 3, device=dev, requires_grad=requires_grad)
    s = GaussianRasterizationSettings(vi["H"], vi["W"], vi["tanfovx"], vi["tanfovy"], d(vi["bg"]), scale_modifier,
                                      d(vi["viewmatrix"]), d(vi["projmatrix"]), vi["sh_degree"], d(vi["campos"]), False, False)
    out = GaussianRasterizer(s)(means3D=leaves["means3D"], means2D=leaves["means2D"], opacities=leaves["opacities"][:, None],
                                shs=leaves["shs"], colors_precomp=leaves["colors_precomp"], **{k: leaves[k] for k in form})
    return out, leaves


def _rel(got, want):
    got = got.detach().cpu().numpy().reshape(want.shape) if isinstance(got, torch.Tensor) else got
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-30))


@pytest.mark.gpu
def test_cov3d_from_scale_rot_matches_float64_build_cov3d(hip_device):
    from freesplat_amd.rasterizer import build_cov3d
    scene, cams = small_scene(N=20000, H=64, W=80, seed=3)
    vi = view_inputs(scene, cams, 0, 64, 80)
    sc, rq = _scale_rot_for(vi, 1)
    got = _native_cov(torch.cat([sc, rq], 1).to(hip_device)).cpu().numpy()
    want = build_cov3d(sc.double(), rq.double(), 1.0).numpy()
    assert _rel(got, want) <= 1e-6
    assert np.isfinite(got).all()


@pytest.mark.gpu
@pytest.mark.parametrize("scale_modifier", [1.0, 0.7])
def test_scale_rot_render_is_bit_identical_and_never_builds_cov3d_in_torch(hip_device, monkeypatch, scale_modifier):
    from freesplat_amd import rasterizer as R
    H, W = 72, 100
    scene, cams = small_scene(N=3000, H=H, W=W, seed=5)
    vi = view_inputs(scene, cams, 1, H, W, bg=(0.1, 0.2, 0.3))
    sc, rq = _scale_rot_for(vi, 2)
    folded = sc * scale_modifier if scale_modifier != 1.0 else sc      # what the Python layer folds into the scales
    cov = _native_cov(torch.cat([folded, rq], 1).to(hip_device))

    def boom(*a, **k):
        raise AssertionError("build_cov3d reached on the (scales, rotations) path")
    monkeypatch.setattr(R, "build_cov3d", boom)
    (c1, r1, d1, a1), _ = _render(vi, hip_device, scale_modifier, requires_grad=True, scales=sc, rotations=rq)
    (c2, r2, d2, a2), _ = _render(vi, hip_device, scale_modifier, requires_grad=True, cov3D_precomp=cov.cpu())
    for x, y in ((c1, c2), (r1, r2), (d1, d2), (a1, a2)):
        assert torch.equal(x, y)
    s1, s2 = R.debug_state(c1.grad_fn.rs), R.debug_state(c2.grad_fn.rs)
    for k in ("offsets", "point_list", "quad", "rec", "rect", "final_T", "n_contrib"):
        np.testing.assert_array_equal(s1[k], s2[k], err_msg=k)
    st = oracle_forward(dict(vi, cov3D=cov.cpu()))
    np.testing.assert_array_equal(c1.detach().cpu().numpy(), st["color"])
    np.testing.assert_array_equal(d1.detach().cpu().numpy(), st["depth"])
    np.testing.assert_array_equal(a1.detach().cpu().numpy(), st["alpha"])
    np.testing.assert_array_equal(r1.cpu().numpy(), st["radii"])
    with torch.no_grad():   # the inference forward (FS_RASTER_NO_BACKWARD_STATE) of the same rows
        c3 = _render(vi, hip_device, scale_modifier, scales=sc, rotations=rq)[0][0]
    assert torch.equal(c1.detach(), c3)


def _scale_rot_grads_vs_oracle(vi, dev, seed, scale_modifier):
    from oracle import raster_oracle as ro
    from freesplat_amd.rasterizer import build_cov3d
    H, W = vi["H"], vi["W"]
    sc, rq = _scale_rot_for(vi, seed)
    folded = sc * scale_modifier if scale_modifier != 1.0 else sc
    cov = _native_cov(torch.cat([folded, rq], 1).to(dev)).cpu()
    st = oracle_forward(dict(vi, cov3D=cov))
    rng = np.random.default_rng(seed)
    g_color = rng.normal(size=(3, H, W)).astype(np.float32)
    g_depth = (0.25 * rng.normal(size=(H, W))).astype(np.float32)
    ref = ro.backward(st, g_color, g_depth)
    (color, _, depth, _), leaves = _render(vi, dev, scale_modifier, requires_grad=True, scales=sc, rotations=rq)
    ((color * torch.from_numpy(g_color).to(dev)).sum() + (depth * torch.from_numpy(g_depth).to(dev)).sum()).backward()
    s64, r64 = sc.double().requires_grad_(True), rq.double().requires_grad_(True)
    (build_cov3d(s64, r64, scale_modifier) * torch.from_numpy(ref["cov3D"]).double()).sum().backward()
    worst = dict(scales=_rel(leaves["scales"].grad, s64.grad.numpy()), rotations=_rel(leaves["rotations"].grad, r64.grad.numpy()),
                 means3D=_rel(leaves["means3D"].grad, ref["means3D"]), opacities=_rel(leaves["opacities"].grad, ref["opacities"]),
                 shs=_rel(leaves["shs"].grad, ref["shs"]), means2D=_rel(leaves["means2D"].grad[:, :2], ref["means2D"]))
    print(f"(scales, rotations) gradient error / max-abs = {worst}")
    assert max(worst.values()) < GRAD_TOL, worst
    assert np.isfinite(leaves["rotations"].grad.cpu().numpy()).all()


@pytest.mark.gpu
@pytest.mark.parametrize("scale_modifier", [1.0, 1.3])
def test_scale_rot_gradients_match_float64_chain_through_the_oracle(hip_device, scale_modifier):
    scene, cams = small_scene(N=4000, H=96, W=128, seed=11)
    vi = view_inputs(scene, cams, 1, 96, 128, bg=(0.3, 0.5, 0.1))
    _scale_rot_grads_vs_oracle(vi, hip_device, 4, scale_modifier)


def _alpha_grads_vs_oracle(vi, dev, seed, tol=GRAD_TOL):
    """HIP gradients of sum(gA * alpha) against the oracle's backward of colour channel 0 for the same geometry with
    colors_precomp = 1, bg = 0, dL/dcolour = [gA, 0, 0]: with those inputs colour 0 equals alpha."""
    from oracle import raster_oracle as ro
    H, W, N = vi["H"], vi["W"], vi["means3D"].shape[0]
    ones = dict(vi, shs=None, colors_precomp=torch.ones(N, 3), bg=torch.zeros(3))
    st = oracle_forward(ones)
    gA = np.random.default_rng(seed).normal(size=(H, W)).astype(np.float32)
    ref = ro.backward(st, np.stack([gA, np.zeros_like(gA), np.zeros_like(gA)]))
    (color, _, depth, alpha), leaves = _render(vi, dev, requires_grad=True, cov3D_precomp=vi["cov3D"])
    np.testing.assert_array_equal(alpha.detach().cpu().numpy(), st["alpha"])
    (alpha * torch.from_numpy(gA).to(dev)).sum().backward()
    worst = dict(means3D=_rel(leaves["means3D"].grad, ref["means3D"]), cov3D=_rel(leaves["cov3D_precomp"].grad, ref["cov3D"]),
                 opacities=_rel(leaves["opacities"].grad, ref["opacities"]),
                 means2D=_rel(leaves["means2D"].grad[:, :2], ref["means2D"]))
    print(f"alpha gradient error / max-abs = {worst}")
    assert max(worst.values()) < tol, worst
    assert (leaves["means2D"].grad[:, 2] == 0).all()
    # an alpha-only loss leaves the colours alone: their gradients are exactly zero
    assert not leaves["shs"].grad.any()


@pytest.mark.gpu
def test_alpha_sum_backward_and_zero_colour_gradients(hip_device):
    H, W = 64, 80
    scene, cams = small_scene(N=600, H=H, W=W, seed=7)
    vi = view_inputs(scene, cams, 1, H, W, bg=(0.4, 0.4, 0.4))
    (_, _, _, alpha), leaves = _render(vi, hip_device, requires_grad=True, cov3D_precomp=vi["cov3D"])
    alpha.sum().backward()
    assert leaves["means3D"].grad.abs().sum() > 0 and leaves["opacities"].grad.abs().sum() > 0
    assert not leaves["shs"].grad.any()
    N = vi["means3D"].shape[0]
    vc = dict(vi, shs=None, colors_precomp=torch.rand(N, 3, generator=torch.Generator().manual_seed(0)))
    (_, _, _, alpha), leaves = _render(vc, hip_device, requires_grad=True, cov3D_precomp=vi["cov3D"])
    alpha.sum().backward()
    assert not leaves["colors_precomp"].grad.any() and leaves["opacities"].grad.abs().sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,N,seed", [(64, 80, 600, 7), (128, 160, 8000, 13)])
def test_alpha_gradients_match_the_oracle_colour_channel(hip_device, H, W, N, seed):
    scene, cams = small_scene(N=N, H=H, W=W, seed=seed)
    _alpha_grads_vs_oracle(view_inputs(scene, cams, 1, H, W, bg=(0.3, 0.5, 0.1)), hip_device, seed)


@pytest.mark.gpu
@pytest.mark.slow
def test_alpha_gradients_match_the_oracle_at_config_3_size(hip_device):
    H, W, N = synthetic.WORKLOADS["c3_968x1296_1M"]
    scene = synthetic.make_scene(N)
    cams = synthetic.target_cameras(2)
    _alpha_grads_vs_oracle(view_inputs(scene, cams, 1, H, W), hip_device, 5)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["cov3D", "scale_rot"])
def test_combined_loss_is_the_sum_of_the_separate_backwards(hip_device, form):
    H, W = 96, 128
    scene, cams = small_scene(N=5000, H=H, W=W, seed=21)
    vi = view_inputs(scene, cams, 1, H, W, bg=(0.2, 0.1, 0.3))
    if form == "cov3D":
        kw = dict(cov3D_precomp=vi["cov3D"])
    else:
        sc, rq = _scale_rot_for(vi, 3)
        kw = dict(scales=sc, rotations=rq)
    (color, _, depth, alpha), leaves = _render(vi, hip_device, requires_grad=True, **kw)
    rng = np.random.default_rng(2)
    t = lambda *shape: torch.from_numpy(rng.normal(size=shape).astype(np.float32)).to(hip_device)
    terms = [(color * t(3, H, W)).sum(), (depth * t(H, W)).sum(), (alpha * t(H, W)).sum()]
    names = [k for k in ("means3D", "means2D", "shs", "opacities", *kw) if leaves.get(k) is not None]
    grad = lambda loss: torch.autograd.grad(loss, [leaves[k] for k in names], retain_graph=True)
    parts = [grad(x) for x in terms]
    whole = grad(terms[0] + terms[1] + terms[2])
    for i, k in enumerate(names):
        want = whole[i]
        got = parts[0][i] + parts[1][i] + parts[2][i]
        err = float((got - want).abs().max()) / (float(want.abs().max()) + 1e-30)
        assert err < 2e-5, f"{k}: {err:.3e} of max-abs"


def _views_call(color, dims, g_color, g_alpha, n_streams):
    """rasterizer.rasterize_backward_views (fs_raster_backward_views_alpha; fs_raster_backward_views without g_alpha) on the
    buffers a render_views forward left behind (its autograd node's batch)."""
    from freesplat_amd import rasterizer as R
    ctx = color.grad_fn
    means, cov6, shs, opac = ctx.saved_tensors
    out = R.rasterize_backward_views(ctx.batch, means, cov6, shs, None, opac, g_color, None, g_alpha=g_alpha, n_streams=n_streams,
                                     dims=dims)
    return {k: t for k, t in out.items() if t is not None}


def _views_setup(dev, seed):
    from freesplat_amd.decoder import render_views
    H, W, v = 96, 128, 4
    scene, cams = small_scene(N=6000, H=H, W=W, seed=seed, n_views=v)
    g = {k: scene[k].to(dev).requires_grad_(True) for k in ("means", "covariances", "harmonics", "opacities")}
    cam = {k: t.to(dev) for k, t in cams.items()}
    color, _ = render_views(cam["extrinsics"], cam["intrinsics"], cam["near"], cam["far"], (H, W),
                            torch.full((v, 3), 0.2, device=dev), g["means"], g["covariances"], g["harmonics"], g["opacities"])
    rng = np.random.default_rng(seed)
    g_color = torch.from_numpy(rng.normal(size=(v, 3, H, W)).astype(np.float32)).to(dev)
    g_alpha = torch.from_numpy(rng.normal(size=(v, H, W)).astype(np.float32)).to(dev)
    return color, g_color, g_alpha


@pytest.mark.gpu
def test_views_alpha_equals_the_single_view_backwards_summed(hip_device):
    from freesplat_amd import rasterizer as R
    color, g_color, g_alpha = _views_setup(hip_device, 51)
    ctx = color.grad_fn
    means, cov6, shs, opac = ctx.saved_tensors
    got = _views_call(color, ctx.batch.dims, g_color, g_alpha, 2)
    want = None
    for i, rs in enumerate(ctx.states):
        want = R.rasterize_backward(rs, means, cov6, shs, None, opac, g_color[i], None, out=want, accumulate=i > 0,
                                    g_alpha=g_alpha[i])
    for k in got:
        err = float((got[k] - want[k]).abs().max()) / (float(want[k].abs().max()) + 1e-30)
        assert err < 1e-5, f"{k}: {err:.3e} of max-abs"
    # and the alpha term changed something: the same call without it differs
    plain = _views_call(color, ctx.batch.dims, g_color, None, 2)
    assert not torch.equal(plain["opacities"], got["opacities"])


@pytest.mark.gpu
def test_deterministic_mode_repeats_both_paths_bitwise(hip_device, monkeypatch):
    from freesplat_amd import rasterizer as R
    monkeypatch.setattr(R, "DETERMINISTIC", True)
    # alpha through the views entry point: two runs, one and two streams
    color, g_color, g_alpha = _views_setup(hip_device, 52)
    dims = R.backward_dims(color.grad_fn.batch.dims)
    runs = [_views_call(color, dims, g_color, g_alpha, ns) for ns in (2, 2, 1)]
    for r in runs[1:]:
        for k in r:
            assert torch.equal(runs[0][k], r[k]), k
    # (scales, rotations) with colour + alpha cotangents through GaussianRasterizer: two backward runs of one forward
    H, W = 96, 128
    scene, cams = small_scene(N=6000, H=H, W=W, seed=53)
    vi = view_inputs(scene, cams, 1, H, W)
    sc, rq = _scale_rot_for(vi, 5)
    (c, _, _, a), leaves = _render(vi, hip_device, requires_grad=True, scales=sc, rotations=rq)
    rng = np.random.default_rng(5)
    loss = (c * torch.from_numpy(rng.normal(size=(3, H, W)).astype(np.float32)).to(hip_device)).sum() + \
        (a * torch.from_numpy(rng.normal(size=(H, W)).astype(np.float32)).to(hip_device)).sum()
    names = ["means3D", "shs", "opacities", "scales", "rotations"]
    g1 = torch.autograd.grad(loss, [leaves[k] for k in names], retain_graph=True)
    g2 = torch.autograd.grad(loss, [leaves[k] for k in names])
    for k, x, y in zip(names, g1, g2):
        assert torch.equal(x, y), k
