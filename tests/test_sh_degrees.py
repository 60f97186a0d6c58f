"""sh_degree 0 - 3 end to end: the Gaussian head at d_sh = 1 / 4 / 9 / 16 (C ABI fs_gaussian_head_forward_sh / _backward_sh,
GaussianAdapter.forward(fusion=False, coords=...)) and the decoder paths fed [G, 3, d_sh] harmonics.

CPU: argument checks and refused degrees of the two entry points; sh_degree 4 names the rasterizer's limit.
GPU: the head against the reference's own outputs (tests/golden/adapter_sh{0,1,3}.npz, make_golden_sh.py) and its backward
against a float64 restatement; render_views bit-exact against the C oracle with gradients within the existing bound, the
unbatched decoder, the deterministic backward, fp16 harmonics; and latents -> head -> render_views -> MSE against a float64
chain."""
import ctypes as C
import os
from math import isqrt

import numpy as np
import pytest
import torch

from adapter_ref import head64
from util_raster import oracle_forward, small_scene

HERE = os.path.dirname(os.path.abspath(__file__))
ATOL_PIXEL = 1e-4          # the north_star tolerance, fp32 (tests/test_raster_hip.py)
FS_ERR_UNSUPPORTED = -3


def _load(name):
    z = np.load(os.path.join(HERE, "golden", name))
    return {k: torch.from_numpy(z[k]) if z[k].ndim else z[k].item() for k in z.files}


def _adapter(degree):
    from freesplat_amd.gaussian_adapter import GaussianAdapter, GaussianAdapterCfg
    return GaussianAdapter(GaussianAdapterCfg(0.5, 15.0, degree))


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_head_sh_entry_points_check_arguments_then_degree():
    from freesplat_amd import _lib
    L = _lib.lib()
    fwd, bwd = L.fs_gaussian_head_forward_sh, L.fs_gaussian_head_backward_sh
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)     # host memory: every call below returns before anything is launched
    for d_sh in (1, 4, 9, 16, 0, 2, 25):
        assert fwd(1, d_sh, *[None] * 4, 0, None, 0.5, 15.0, *[None] * 5, None) == -1, d_sh
        assert bwd(1, d_sh, *[None] * 4, 0, None, 0.5, 15.0, *[None] * 8, None) == -1, d_sh
        assert fwd(-1, d_sh, p, p, p, p, 0, p, 0.5, 15.0, p, p, p, p, None) == -1, d_sh
    for d_sh in (0, 2, 25, 3, -9):
        for M in (0, 1, 1000):
            assert fwd(M, d_sh, p, p, p, p, 0, p, 0.5, 15.0, p, p, p, p, None) == FS_ERR_UNSUPPORTED, (M, d_sh)
            assert bwd(M, d_sh, p, p, p, p, 0, p, 0.5, 15.0, None, None, None, None, p, p, p, None) == FS_ERR_UNSUPPORTED
    for d_sh in (1, 4, 9, 16):
        assert fwd(0, d_sh, None, None, None, p, 0, p, 0.5, 15.0, None, None, None, None, None) == 0      # empty job
        assert bwd(0, d_sh, None, None, None, p, 0, p, 0.5, 15.0, *[None] * 7, None) == 0
        assert fwd(1, d_sh, None, p, p, p, 0, p, 0.5, 15.0, p, p, p, p, None) == -1                        # raw missing
        assert bwd(1, d_sh, p, p, p, p, 0, p, 0.5, 15.0, None, None, None, None, p, p, None, None) == -1   # g_extrinsics


def test_adapter_sizes_follow_sh_degree_and_degree_4_names_the_rasterizer_limit():
    for degree, d_sh in ((0, 1), (1, 4), (2, 9), (3, 16)):
        ad = _adapter(degree)
        assert ad.d_sh == d_sh and ad.d_in == 7 + 3 * d_sh and ad.sh_mask.shape == (d_sh,)
    ad = _adapter(4)
    M = 5
    with pytest.raises(NotImplementedError, match="degree 0 - 3"):
        ad(torch.eye(4).repeat(M, 1, 1).view(1, 1, M, 1, 1, 4, 4), torch.eye(3).view(1, 1, 1, 1, 1, 3, 3), None,
           torch.ones(1, 1, M, 1, 1), torch.ones(1, 1, M, 1, 1), torch.zeros(1, 1, M, 1, 1, ad.d_in), (8, 12),
           fusion=False, coords=torch.zeros(1, 1, M, 1, 1, 3))


def test_sh_goldens_hold_the_reference_masks():
    for degree in (0, 1, 3):
        g = _load(f"adapter_sh{degree}.npz")
        d_sh = (degree + 1) ** 2
        assert g["sh_degree"] == degree and g["raw"].shape[-1] == 7 + 3 * d_sh
        assert g["out_harmonics"].shape[-2:] == (3, d_sh)
        assert torch.equal(g["sh_mask"], _adapter(degree).sh_mask)


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("degree", [0, 1, 3])
def test_gaussian_head_matches_reference_golden_at_degree(hip_device, degree):
    g = _load(f"adapter_sh{degree}.npz")
    h, w = int(g["h"]), int(g["w"])
    M = g["extrinsics"].shape[0]
    d = lambda t: t.to(hip_device)
    ad = _adapter(degree).to(hip_device)
    out = ad(d(g["extrinsics"]).view(1, 1, M, 1, 1, 4, 4), d(g["intrinsics"]).view(1, 1, 1, 1, 1, 3, 3).expand(1, 1, M, 1, 1, 3, 3),
             None, d(g["depths"]).view(1, 1, M, 1, 1), d(g["opacities"]).view(1, 1, M, 1, 1),
             d(g["raw"]).view(1, 1, M, 1, 1, ad.d_in), (h, w), fusion=False, coords=d(g["coords"]).view(1, 1, M, 1, 1, 3))
    for got, key, rtol in ((out.covariances, "out_cov", 2e-5), (out.harmonics, "out_harmonics", 1e-6),
                           (out.scales, "out_scales", 2e-6), (out.rotations, "out_rotations", 2e-6),
                           (out.means, "out_means", 0), (out.opacities, "out_opacities", 0)):
        want = g[key]
        assert got.shape == want.shape, key
        assert (got.cpu() - want).abs().max().item() <= rtol * want.abs().max().item() + 1e-12, key


@pytest.mark.gpu
@pytest.mark.parametrize("degree", [0, 1, 3])
def test_gaussian_head_backward_vs_float64_autograd(hip_device, degree):
    """M = 2000 rows: full and partial workgroups of 256 (d_sh 1, 4) and 128 rows (d_sh 16); raw is a view one row into its
    buffer, so its rows start off the 16-byte grid (the scalar staging path)."""
    from freesplat_amd.gaussian_adapter import _Head
    d_sh = (degree + 1) ** 2
    gen = torch.Generator().manual_seed(3 + degree)
    M = 2000
    rawbuf = torch.randn(M + 1, 7 + 3 * d_sh, generator=gen)
    dep = 1.0 + torch.rand(M, generator=gen)
    E = torch.eye(4).repeat(M, 1, 1) + 0.1 * torch.randn(M, 4, 4, generator=gen)
    mult = torch.tensor([0.0123])
    mask = _adapter(degree).sh_mask
    gcov, gsh = torch.randn(M, 3, 3, generator=gen), torch.randn(M, 3, d_sh, generator=gen)
    gsc, grot = torch.randn(M, 3, generator=gen), torch.randn(M, 4, generator=gen)
    leaf = lambda t: t.double().clone().requires_grad_(True)
    r64, d64, e64 = leaf(rawbuf[1:]), leaf(dep), leaf(E)
    ref = head64(r64, d64, e64, mult.double()[0], mask.double())
    ((ref[0] * gcov).sum() + (ref[1] * gsh).sum() + (ref[2] * gsc).sum() + (ref[3] * grot).sum()).backward()
    dv = lambda t: t.to(hip_device)
    rb, dg, eg = dv(rawbuf).requires_grad_(True), dv(dep).requires_grad_(True), dv(E).requires_grad_(True)
    o = _Head.apply(rb[1:], dg, eg, dv(mult), dv(mask), 0.5, 15.0)
    assert o[1].shape == (M, 3, d_sh)
    for a, b in zip(o, ref):
        assert (a.detach().cpu().double() - b.detach()).abs().max().item() <= 2e-5 * (b.abs().max().item() + 1e-12)
    ((o[0] * dv(gcov)).sum() + (o[1] * dv(gsh)).sum() + (o[2] * dv(gsc)).sum() + (o[3] * dv(grot)).sum()).backward()
    assert bool((rb.grad[0] == 0).all())
    for got, want, name in ((rb.grad[1:], r64.grad, "raw"), (dg.grad, d64.grad, "depths"), (eg.grad, e64.grad, "extrinsics")):
        s = want.abs().max().item()
        assert (got.cpu().double() - want).abs().max().item() <= 2e-4 * s, name
    # only the covariance carries a gradient (g_harmonics / g_scales / g_rotations NULL): the SH channels get exact zeros
    r2 = dv(rawbuf[1:]).requires_grad_(True)
    (_Head.apply(r2, dv(dep), dv(E), dv(mult), dv(mask), 0.5, 15.0)[0] * dv(gcov)).sum().backward()
    r64b = leaf(rawbuf[1:])
    (head64(r64b, dep.double(), E.double(), mult.double()[0], mask.double())[0] * gcov).sum().backward()
    assert bool((r2.grad[:, 7:] == 0).all())
    assert (r2.grad.cpu().double() - r64b.grad).abs().max().item() <= 2e-4 * r64b.grad.abs().max().item()


def _frames(cam):
    from freesplat_amd.decoder import frame_views
    return [t.cpu() for t in frame_views(cam["extrinsics"], cam["intrinsics"], cam["near"], cam["far"])]


def _api_view(fr, i, H, W, bg, means, cov, harm, opac):
    """The rasterizer API inputs of view i, framed by the SAME matrices render_views uses (fs_frame_views): transposed
    harmonics [G, d_sh, 3], upper-triangle covariances [G, 6], means and covariances rescaled by 1/near."""
    campos, scale, tanfov, view, full = fr
    r, c = torch.triu_indices(3, 3)
    s = scale[i]
    return dict(H=H, W=W, tanfovx=float(tanfov[i, 0]), tanfovy=float(tanfov[i, 1]), bg=bg, viewmatrix=view[i].contiguous(),
                projmatrix=full[i].contiguous(), campos=campos[i].contiguous(), sh_degree=isqrt(harm.shape[-1]) - 1,
                means3D=(means * s).contiguous(), cov3D=(cov * s ** 2)[:, r, c].contiguous(),
                shs=harm.transpose(-1, -2).contiguous(), opacities=opac.contiguous())


def _oracle_grads(fr, H, W, bg, scene, weights, states):
    """Oracle backward of every view, carried back to render_views' inputs (means, covariances [G,3,3], harmonics [G,3,d_sh],
    opacities) through the same layout changes, summed over the views."""
    from oracle import raster_oracle as ro
    leaves = {k: scene[k].detach().clone().requires_grad_(True) for k in ("means", "covariances", "harmonics", "opacities")}
    for i, st in enumerate(states):
        g = ro.backward(st, weights[i])
        vi = _api_view(fr, i, H, W, bg, leaves["means"], leaves["covariances"], leaves["harmonics"], leaves["opacities"])
        torch.autograd.backward([vi["means3D"], vi["cov3D"], vi["shs"], vi["opacities"]],
                                [torch.from_numpy(g[k]).reshape(vi[k].shape) for k in ("means3D", "cov3D", "shs", "opacities")])
    return {k: t.grad for k, t in leaves.items()}


def _render_views_grads(scene, cam, H, W, bg, dev, weights, harm=None):
    from freesplat_amd.decoder import render_views
    g = {k: scene[k].to(dev).requires_grad_(True) for k in ("means", "covariances", "harmonics", "opacities")}
    if harm is not None:
        g["harmonics"] = harm.to(dev).requires_grad_(True)
    v = cam["extrinsics"].shape[0]
    color, depth = render_views(cam["extrinsics"], cam["intrinsics"], cam["near"], cam["far"], (H, W),
                                bg.to(dev)[None].expand(v, 3), g["means"], g["covariances"], g["harmonics"], g["opacities"])
    (color * weights.to(dev)).sum().backward()
    return color.detach().cpu(), depth.detach().cpu(), {k: t.grad.detach().cpu() for k, t in g.items()}


def _scene(degree, H, W, v=3, N=900, seed=17):
    scene, cams = small_scene(N=N, H=H, W=W, seed=seed + degree, n_views=v, sh_degree=degree)
    assert scene["harmonics"].shape[-1] == (degree + 1) ** 2
    return scene, cams


def _assert_grads_close(got, want, tol=2e-4, what=""):
    for k in want:
        s = want[k].abs().max().item() + 1e-20
        err = (got[k].double() - want[k].double()).abs().max().item()
        assert err <= tol * s, (what, k, err / s)


@pytest.mark.gpu
@pytest.mark.parametrize("degree", [0, 1, 3])
def test_render_views_at_degree_matches_the_oracle(hip_device, degree):
    H, W, v = 48, 64, 3
    scene, cams = _scene(degree, H, W, v)
    cam = {k: t.to(hip_device) for k, t in cams.items()}
    bg = torch.tensor([0.2, 0.3, 0.4])
    weights = torch.randn(v, 3, H, W, generator=torch.Generator().manual_seed(degree))
    color, depth, grads = _render_views_grads(scene, cam, H, W, bg, hip_device, weights)
    fr = _frames(cam)
    states = []
    for i in range(v):
        st = oracle_forward(_api_view(fr, i, H, W, bg, scene["means"], scene["covariances"], scene["harmonics"],
                                      scene["opacities"]))
        assert st["num_rendered"] > 500
        np.testing.assert_array_equal(color[i].numpy(), st["color"])
        np.testing.assert_array_equal(depth[i, 0].numpy(), st["depth"])
        states.append(st)
    _assert_grads_close(grads, _oracle_grads(fr, H, W, bg, scene, weights.numpy(), states), what=f"degree {degree}")


@pytest.mark.gpu
@pytest.mark.parametrize("degree", [0, 1, 3])
def test_decoder_batched_and_unbatched_at_degree(hip_device, degree):
    from freesplat_amd.decoder import DecoderSplattingCUDA, Gaussians, render_views
    H, W, v = 48, 64, 3
    scene, cams = _scene(degree, H, W, v, seed=40)
    dev = hip_device
    cam = {k: t.to(dev)[None] for k, t in cams.items()}
    wts = torch.randn(1, v, 3, H, W, generator=torch.Generator().manual_seed(7)).to(dev)
    wd = torch.randn(1, v, H, W, generator=torch.Generator().manual_seed(8)).to(dev)
    outs = {}
    for batched in (True, False):
        g = {k: scene[k].to(dev)[None].requires_grad_(True) for k in ("means", "covariances", "harmonics", "opacities")}
        dec = DecoderSplattingCUDA(background_color=(0.2, 0.3, 0.4), batched=batched).to(dev)
        out = dec(Gaussians(g["means"], g["covariances"], g["harmonics"], g["opacities"]), cam["extrinsics"],
                  cam["intrinsics"], cam["near"], cam["far"], (H, W), depth_mode="depth")
        assert out.color.shape == (1, v, 3, H, W) and out.depth.shape == (1, v, H, W)
        ((out.color * wts).sum() + (out.depth * wd).sum()).backward()
        outs[batched] = (out.color.detach(), out.depth.detach(), {k: t.grad[0].cpu() for k, t in g.items()})
    (c1, d1, g1), (c2, d2, g2) = outs[True], outs[False]
    # the unbatched path frames with the reference's fp32 torch ops: ulp-level different matrices (as at d_sh = 9)
    assert (c1 - c2).abs().max() <= ATOL_PIXEL and (d1 - d2).abs().max() <= 1e-3 * d2.abs().max()
    _assert_grads_close(g2, g1, what="unbatched vs batched")
    with torch.no_grad():
        c3, d3 = render_views(cam["extrinsics"][0], cam["intrinsics"][0], cam["near"][0], cam["far"][0], (H, W),
                              torch.tensor([0.2, 0.3, 0.4], device=dev)[None].expand(v, 3), *(scene[k].to(dev) for k in
                              ("means", "covariances", "harmonics", "opacities")))
    assert torch.equal(c1[0], c3) and torch.equal(d1[0], d3[:, 0] / 2)


@pytest.mark.gpu
def test_deterministic_backward_at_d_sh_16(hip_device, monkeypatch):
    from freesplat_amd import rasterizer as R
    H, W, v = 48, 64, 3
    scene, cams = _scene(3, H, W, v, seed=60)
    cam = {k: t.to(hip_device) for k, t in cams.items()}
    bg = torch.tensor([0.2, 0.3, 0.4])
    weights = torch.randn(v, 3, H, W, generator=torch.Generator().manual_seed(61))
    _, _, atomic = _render_views_grads(scene, cam, H, W, bg, hip_device, weights)
    monkeypatch.setattr(R, "DETERMINISTIC", True)
    runs = [_render_views_grads(scene, cam, H, W, bg, hip_device, weights)[2] for _ in range(2)]
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
    _assert_grads_close(runs[0], atomic, what="deterministic vs atomic")


@pytest.mark.gpu
def test_fp16_harmonics_at_d_sh_16(hip_device):
    """fp16 SH is storage only: the image equals the fp32 render of the fp16-rounded coefficients bit for bit."""
    H, W, v = 48, 64, 3
    scene, cams = _scene(3, H, W, v, seed=70)
    cam = {k: t.to(hip_device) for k, t in cams.items()}
    bg = torch.tensor([0.2, 0.3, 0.4])
    weights = torch.randn(v, 3, H, W, generator=torch.Generator().manual_seed(71))
    h16 = scene["harmonics"].half()
    c16, d16, g16 = _render_views_grads(scene, cam, H, W, bg, hip_device, weights, harm=h16)
    c32, d32, g32 = _render_views_grads(scene, cam, H, W, bg, hip_device, weights, harm=h16.float())
    assert torch.equal(c16, c32) and torch.equal(d16, d32)
    assert g16["harmonics"].dtype == torch.float16
    s = g32["harmonics"].abs().max().item()
    assert (g16["harmonics"].float() - g32["harmonics"]).abs().max().item() <= 2e-3 * s     # fp16 rounding of the gradient
    _assert_grads_close({k: g16[k] for k in ("means", "covariances", "opacities")},
                        {k: g32[k] for k in ("means", "covariances", "opacities")}, what="fp16 vs fp32 storage")


@pytest.mark.gpu
@pytest.mark.parametrize("degree", [0, 3])
def test_composed_latents_head_render_chain_vs_float64(hip_device, degree):
    """latents -> to_gaussians stand-in Linear(64, 2 + d_in) -> GaussianAdapter (HIP head) -> render_views -> MSE -> backward,
    against the same chain in float64 torch ops (head64 + oracle/raster_dense_torch.render_dense, whose discrete choices --
    tile rectangles and draw order -- come from the C oracle on the HIP chain's Gaussians)."""
    from oracle.raster_dense_torch import render_dense
    from freesplat_amd.decoder import render_views
    dev = hip_device
    H, W, v, M = 32, 40, 2, 64
    ad = _adapter(degree)
    d_in = ad.d_in
    gen = torch.Generator().manual_seed(80 + degree)
    _, cams = small_scene(N=10, H=H, W=W, seed=81, n_views=v, sh_degree=degree)
    lin = torch.nn.Linear(64, 2 + d_in)
    with torch.no_grad():
        lin.weight.mul_(0.5)
    lat = torch.randn(M, 64, generator=gen)
    K = cams["intrinsics"][0]
    # Gaussians in front of the first target camera, blended extrinsics near it
    c2w = cams["extrinsics"][0]
    local = torch.cat([0.6 * (torch.rand(M, 2, generator=gen) - 0.5), 1.5 + torch.rand(M, 1, generator=gen)], -1)
    means = local @ c2w[:3, :3].T + c2w[:3, 3]
    dep = local[:, 2].clone()
    E = c2w.repeat(M, 1, 1) + 0.02 * torch.randn(M, 4, 4, generator=gen)
    target = torch.rand(v, 3, H, W, generator=gen)
    bg = torch.tensor([0.1, 0.2, 0.3])

    def chain(lin_, lat_, means_, dev_, adapter_call):
        raw = lin_(lat_)
        opac = torch.sigmoid(raw[:, 0])
        cov, sh = adapter_call(raw[:, 2:])
        return means_, cov, sh, opac

    # ---- HIP chain ----
    lin_h = torch.nn.Linear(64, 2 + d_in).to(dev)
    lin_h.load_state_dict(lin.state_dict())
    lat_h, means_h = lat.to(dev).requires_grad_(True), means.to(dev).requires_grad_(True)
    ad_h = ad.to(dev)

    def hip_head(raw):
        g = ad_h(E.to(dev).view(1, 1, M, 1, 1, 4, 4), K.to(dev).view(1, 1, 1, 1, 1, 3, 3).expand(1, 1, M, 1, 1, 3, 3), None,
                 dep.to(dev).view(1, 1, M, 1, 1), torch.ones(1, 1, M, 1, 1, device=dev), raw.view(1, 1, M, 1, 1, d_in), (H, W),
                 fusion=False, coords=means_h.view(1, 1, M, 1, 1, 3))
        return g.covariances.reshape(M, 3, 3), g.harmonics.reshape(M, 3, ad.d_sh)

    m_, cov_h, sh_h, op_h = chain(lin_h, lat_h, means_h, dev, hip_head)
    cam = {k: t.to(dev) for k, t in cams.items()}
    img, _ = render_views(cam["extrinsics"], cam["intrinsics"], cam["near"], cam["far"], (H, W), bg.to(dev)[None].expand(v, 3),
                          m_, cov_h, sh_h, op_h)
    loss = ((img - target.to(dev)) ** 2).mean()
    loss.backward()
    # ---- float64 chain ----
    lin_d = torch.nn.Linear(64, 2 + d_in).double()
    lin_d.load_state_dict({k: t.double() for k, t in lin.state_dict().items()})
    lat_d, means_d = lat.double().requires_grad_(True), means.double().requires_grad_(True)
    mult = ad.get_scale_multiplier(K.view(1, 3, 3), 1 / torch.tensor((W, H), dtype=torch.float32)).reshape(()).double()

    def ref_head(raw):
        cov, sh, _, _ = head64(raw, dep.double(), E.double(), mult, ad.sh_mask.cpu().double())
        return cov, sh

    m_d, cov_d, sh_d, op_d = chain(lin_d, lat_d, means_d, None, ref_head)
    fr = _frames(cam)
    r, c = torch.triu_indices(3, 3)
    imgs = []
    for i in range(v):
        st = oracle_forward(_api_view(fr, i, H, W, bg, means, cov_h.detach().cpu(), sh_h.detach().cpu(), op_h.detach().cpu()))
        assert st["num_rendered"] > 50
        s = fr[1][i].double()
        order = torch.from_numpy(np.lexsort((np.arange(st["N"]), st["depths"].view(np.uint32))).astype(np.int64))
        color, _, _ = render_dense(H, W, float(fr[2][i, 0]), float(fr[2][i, 1]), bg.double(), fr[3][i], fr[4][i], degree,
                                   fr[0][i].double(), m_d * s, (cov_d * s * s)[:, r, c], op_d,
                                   shs=sh_d.transpose(-1, -2), rect=torch.from_numpy(st["rect"]),
                                   radii=torch.from_numpy(st["radii"]), order=order)
        imgs.append(color)
    ref_img = torch.stack(imgs)
    ref_loss = ((ref_img - target.double()) ** 2).mean()
    ref_loss.backward()
    err = (img.detach().cpu().double() - ref_img.detach()).abs().max().item()
    assert err <= ATOL_PIXEL, err
    assert abs(loss.item() - ref_loss.item()) <= 1e-5 * max(1.0, abs(ref_loss.item()))
    for name, got, want in (("latents", lat_h.grad, lat_d.grad), ("means", means_h.grad, means_d.grad),
                            ("weight", lin_h.weight.grad, lin_d.weight.grad), ("bias", lin_h.bias.grad, lin_d.bias.grad)):
        g_, w_ = got.cpu().double().flatten(), want.flatten()
        rel = ((g_ - w_).abs().max() / (w_.abs().max() + 1e-300)).item()
        cos = float((g_ @ w_) / (g_.norm() * w_.norm() + 1e-300))
        assert rel <= 1e-3 and cos >= 0.9999, (name, rel, cos)
