"""GPU checks of the evaluation metrics (freesplat_amd/metrics.py on fs_image_metrics / fs_depth_metrics) against the
float64 restatement (tests/metrics_ref.py) and the reference's outputs (tests/golden/depth_metrics.npz)."""
import os

import numpy as np
import pytest
import torch

import metrics_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_metrics.npz")


def _smooth(rng, B, C, H, W, noise=0.002):
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([0.5 + 0.4 * np.sin(xx / (17.0 + 5 * c)) * np.cos(yy / (13.0 + 3 * c)) for c in range(C)])
    gt = np.broadcast_to(base, (B, C, H, W)) + 0.02 * rng.standard_normal((B, 1, 1, 1))
    return gt.astype(np.float32), (gt + noise * rng.standard_normal(gt.shape)).astype(np.float32)


def _inputs(kind, B, C, H, W, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.random((B, C, H, W), np.float32), rng.random((B, C, H, W), np.float32)
    if kind == "smooth":
        return _smooth(rng, B, C, H, W)
    if kind == "outside":
        a = rng.random((B, C, H, W), np.float32)
        return (a * 1.8 - 0.4).astype(np.float32), (a * 1.5 - 0.2 + 0.3 * rng.random(a.shape)).astype(np.float32)
    raise ValueError(kind)


def _check(gt, pred, dev, with_map=True):
    from freesplat_amd import metrics as M
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    psnr, ssim, smap = M.image_metrics(t(gt), t(pred), return_map=True)
    want = R.ssim_batch(gt, pred)
    got = ssim.cpu().numpy()
    assert np.abs(got - want).max() <= 1e-5, (got, want)
    if with_map:
        m = smap.cpu().numpy()
        for b in range(gt.shape[0]):
            assert np.abs(m[b] - R.ssim_map(gt[b], pred[b])).max() <= 5e-4
    with np.errstate(divide="ignore"):
        want_psnr = -10 * np.log10(R.mse(gt, pred))
    assert np.abs(psnr.cpu().numpy() - want_psnr).max() <= 1e-4
    return float(np.abs(got - want).max())


@pytest.mark.parametrize("H,W", [(11, 11), (11, 40), (13, 300), (96, 128)])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("kind", ["noise", "smooth", "outside"])
def test_ssim_small_shapes_vs_restatement(hip_device, kind, C, H, W):
    gt, pred = _inputs(kind, 5, C, H, W, seed=H * W + C)
    _check(gt, pred, hip_device)


@pytest.mark.parametrize("B,H,W", [(1, 384, 512), (5, 480, 640), (16, 96, 128)])
@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_ssim_batches_vs_restatement(hip_device, kind, B, H, W):
    gt, pred = _inputs(kind, B, 3, H, W, seed=B)
    _check(gt, pred, hip_device, with_map=B == 1)


@pytest.mark.slow
def test_ssim_full_size_vs_restatement(hip_device):
    gt, pred = _inputs("smooth", 1, 3, 968, 1296, seed=3)
    _check(gt, pred, hip_device)


def test_ssim_of_rendered_views(hip_device):
    """A pair rendered by the library's own rasterizer: a seeded synthetic scene and a perturbed copy."""
    from freesplat_amd import synthetic
    from freesplat_amd.decoder import render_views
    H, W = 96, 128
    scene = synthetic.make_scene(6000, seed=5)
    cams = {k: t.to(hip_device) for k, t in synthetic.target_cameras(2, seed=5).items()}
    g = {k: scene[k].to(hip_device) for k in ("means", "covariances", "harmonics", "opacities")}
    bg = torch.zeros(2, 3, device=hip_device)
    render = lambda means: render_views(cams["extrinsics"], cams["intrinsics"], cams["near"], cams["far"], (H, W), bg, means,
                                        g["covariances"], g["harmonics"], g["opacities"])[0]
    a = render(g["means"])
    noise = torch.randn(g["means"].shape, generator=torch.Generator().manual_seed(1)).to(hip_device)
    b = render(g["means"] + 0.003 * noise)
    assert a.shape == (2, 3, H, W) and float((a - b).abs().max()) > 0
    _check(a.float().cpu().numpy(), b.float().cpu().numpy(), hip_device)


def test_identical_and_constant_images(hip_device):
    from freesplat_amd import metrics as M
    x = torch.from_numpy(_inputs("smooth", 3, 3, 40, 57)[0]).to(hip_device)
    psnr, ssim = M.image_metrics(x, x.clone())
    assert torch.all(ssim == 1.0) and torch.all(torch.isinf(psnr)) and torch.all(psnr > 0)
    for a, b in ((0.2, 0.7), (0.5, 0.5), (1.3, -0.4)):
        s = M.compute_ssim(torch.full((2, 3, 20, 30), a, device=hip_device), torch.full((2, 3, 20, 30), b, device=hip_device))
        want = (2 * a * b + R.C1) / (a * a + b * b + R.C1)
        assert torch.allclose(s.double().cpu(), torch.full((2,), want, dtype=torch.float64), atol=1e-6, rtol=0)


def test_psnr_matches_torch_formula(hip_device):
    from freesplat_amd import metrics as M
    z = np.load(GOLD)
    gt, pred = torch.from_numpy(z["psnr__gt"]).to(hip_device), torch.from_numpy(z["psnr__pred"]).to(hip_device)
    mse = ((gt.clip(0, 1) - pred.clip(0, 1)) ** 2).mean(dim=(1, 2, 3))
    want = -10 * mse.log10()
    got = M.compute_psnr(gt, pred)
    assert got.dtype == torch.float32 and got.shape == (4,) and got.device == gt.device
    assert torch.isinf(got[3]) and torch.isinf(want[3])
    assert (got[:3] - want[:3]).abs().max().item() <= 1e-4
    assert np.abs(got[:3].cpu().numpy() - z["psnr__out"][:3]).max() <= 1e-4


def test_determinism_batch_and_stream(hip_device):
    from freesplat_amd import metrics as M
    gt, pred = _inputs("noise", 16, 3, 200, 300, seed=9)
    gt, pred = torch.from_numpy(gt).to(hip_device), torch.from_numpy(pred).to(hip_device)
    p1, s1 = M.image_metrics(gt, pred)
    p2, s2 = M.image_metrics(gt, pred)
    assert torch.equal(s1, s2) and torch.equal(p1, p2)
    for k in (0, 7, 15):
        pk, sk = M.image_metrics(gt[k:k + 1], pred[k:k + 1])
        assert torch.equal(sk[0], s1[k]) and torch.equal(pk[0], p1[k])
    side = torch.cuda.Stream(device=hip_device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        p3, s3 = M.image_metrics(gt, pred)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(s3, s1) and torch.equal(p3, p1)


@pytest.mark.parametrize("case", ["mixed", "single", "empty", "inf_pred"])
def test_depth_metrics_vs_reference_and_restatement(hip_device, case):
    from types import SimpleNamespace
    from freesplat_amd import metrics as M
    z = np.load(GOLD)
    gt, pred = z[f"{case}__gt"], z[f"{case}__pred"]
    b, v = gt.shape[:2]
    batch = {"target": {"depth": torch.from_numpy(gt).unsqueeze(2).to(hip_device)}}
    out = M.depth_render_metrics(SimpleNamespace(depth=torch.from_numpy(pred).to(hip_device)), batch)
    per_view = M.depth_metrics(torch.from_numpy(gt).to(hip_device), torch.from_numpy(pred).to(hip_device))
    ref = R.depth(gt.reshape(b * v, -1), pred.reshape(b * v, -1))
    for k, o in zip(("abs_diff", "abs_rel", "delta_25", "delta_10"), out):
        assert o.shape == () and o.dtype == torch.float32 and o.device.type == "cuda"
        want = z[f"{case}__{k}"]
        got = o.cpu().numpy()
        assert np.isnan(got) == np.isnan(want) and np.isinf(got) == np.isinf(want), (k, got, want)
        if np.isfinite(want):
            assert abs(got - want) <= 1e-6 * abs(want) + 1e-7, (k, got, want)
        pv = per_view[k].cpu().numpy()
        assert np.array_equal(np.isnan(pv), np.isnan(ref[k])) and np.array_equal(np.isinf(pv), np.isinf(ref[k]))
        f = np.isfinite(ref[k])
        assert np.allclose(pv[f], ref[k][f], rtol=1e-6, atol=0), (k, pv, ref[k])


def test_depth_render_metrics_without_depth(hip_device):
    from freesplat_amd import metrics as M
    out = M.depth_render_metrics(None, {"target": {}})
    assert len(out) == 4 and all(torch.equal(o, torch.tensor(0.0)) for o in out)


def test_mirror_shapes_dtypes_slices_and_errors(hip_device):
    from freesplat_amd import metrics as M
    gt, pred = _inputs("noise", 6, 3, 30, 44, seed=4)
    g, p = torch.from_numpy(gt).to(hip_device), torch.from_numpy(pred).to(hip_device)
    s = M.compute_ssim(g, p)
    assert s.shape == (6,) and s.dtype == torch.float32 and s.device == p.device
    assert M.compute_ssim(g.double(), p.double()).dtype == torch.float64
    ps = M.compute_psnr(g, p)
    assert ps.shape == (6,) and ps.dtype == torch.float32 and ps.device == p.device
    # non-contiguous slices: every other view, and a channels-last view of the same data
    s2 = M.compute_ssim(g[::2], p[::2])
    assert torch.allclose(s2.double().cpu(), torch.from_numpy(R.ssim_batch(gt[::2], pred[::2])), atol=1e-5, rtol=0)
    gl = g.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not gl.is_contiguous()
    assert torch.equal(M.compute_ssim(gl, p), s)
    assert torch.equal(M.compute_ssim(g[:4], p[:4]), s[:4])
    with pytest.raises(ValueError):
        M.compute_ssim(g[:, :, :10], p[:, :, :10])
    with pytest.raises(ValueError):
        M.compute_psnr(g[..., :10], p[..., :10])
    with pytest.raises(ValueError):
        M.compute_ssim(g.cpu(), p.cpu())
    with pytest.raises(ValueError):
        M.depth_metrics(g.cpu(), p.cpu())
