"""GPU checks of the fused SSIM / photometric loss (freesplat_amd/ssim_loss.py on fs_ssim_loss_forward / _backward) against
the float64 restatement (tests/ssim_loss_ref.py): values, gradients (bounded by the eager fp32 run's own error, the rule of
tests/test_lpips_hip.py), exact cases, determinism, what is held for the backward, the error cases, and guard bands."""
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

import metrics_ref as R
import ssim_loss_ref as SR
from freesplat_amd.ssim_loss import TILE_H, TILE_W          # the kernels' tile extents

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO_TILES = (TILE_H + 1, TILE_W + 1)          # two tiles meet in both axes; W = 247 is no multiple of 4 either
SHAPES = [(11, 11), (11, 40), (13, 300), (96, 128), TWO_TILES, (17, 43)]
BELOW_WINDOW = [(1, 1), (3, 7), (10, 10)]     # "3dgs" only: the window exceeds the image
CASES = [(c, H, W) for c in SR.CONVENTIONS for H, W in SHAPES] + [("3dgs", H, W) for H, W in BELOW_WINDOW]
KINDS = ["noise", "smooth", "outside"]
B = 3


def _smooth(rng, B_, C, H, W, noise=0.002):
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([0.5 + 0.4 * np.sin(xx / (17.0 + 5 * c)) * np.cos(yy / (13.0 + 3 * c)) for c in range(C)])
    gt = np.broadcast_to(base, (B_, C, H, W)) + 0.02 * rng.standard_normal((B_, 1, 1, 1))
    return gt.astype(np.float32), (gt + noise * rng.standard_normal(gt.shape)).astype(np.float32)


def _inputs(kind, B_, C, H, W, seed=0):
    """(gt, pred) float32, the three kinds of tests/test_metrics_hip.py."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.random((B_, C, H, W), np.float32), rng.random((B_, C, H, W), np.float32)
    if kind == "smooth":
        return _smooth(rng, B_, C, H, W)
    if kind == "outside":
        a = rng.random((B_, C, H, W), np.float32)
        return (a * 1.8 - 0.4).astype(np.float32), (a * 1.5 - 0.2 + 0.3 * rng.random(a.shape)).astype(np.float32)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def _case(convention, kind, C, H, W):
    """Inputs, cotangents and every float64 reference of one case, computed once and shared (never modified)."""
    gt, pred = (torch.from_numpy(a) for a in _inputs(kind, B, C, H, W, seed=H * W + C))
    g = torch.Generator().manual_seed(H + W)
    cs, cl = torch.randn(B, generator=g), torch.randn(B, generator=g)
    ssim64, l164 = SR.values(pred, gt, convention)
    grads = {"both": SR.grad(pred, gt, convention, cs, cl), "ssim": SR.grad(pred, gt, convention, cs, None),
             "l1": SR.grad(pred, gt, convention, None, cl)}
    loss64, grads["photometric"] = SR.photometric_grad(pred, gt, 0.2, convention)
    return dict(gt=gt, pred=pred, cs=cs, cl=cl, ssim=ssim64, l1=l164, grads=grads, loss=loss64)


def _err(got, want):
    want = want.double()
    return float((got.double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300))


def _bound(eager_err):
    return max(4.0 * eager_err, 1e-6)


@gpu
@pytest.mark.parametrize("convention,H,W", CASES)
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_values_vs_float64(hip_device, kind, C, convention, H, W):
    from freesplat_amd import metrics as M, ssim_loss as S
    c = _case(convention, kind, C, H, W)
    pred, gt = c["pred"].to(hip_device), c["gt"].to(hip_device)
    s, l1 = S.ssim_and_l1(pred, gt, convention)
    assert s.shape == (B,) and s.dtype == torch.float32 and l1.shape == (B,) and s.device == pred.device and s.grad_fn is None
    e_s = float((s.double().cpu() - c["ssim"]).abs().max())
    e_l = float(((l1.double().cpu() - c["l1"]).abs() / c["l1"]).max())
    print(f"ssim err {e_s:.2e} (bound 1e-5), l1 rel err {e_l:.2e} (bound 1e-6)")
    assert e_s <= 1e-5 and e_l <= 1e-6
    assert torch.equal(S.ssim(pred, gt, convention), s)
    want_loss = 0.8 * c["l1"].mean() + 0.2 * (1 - c["ssim"].mean())
    assert abs(float(S.photometric_loss(pred, gt, 0.2, convention)) - float(want_loss)) <= 1e-5
    assert abs(float(S.dssim_loss(pred, gt, convention)) - float(1 - c["ssim"].mean())) <= 1e-5
    if convention == "skimage":
        m = M.image_metrics(gt, pred)[1]
        assert float((m.cpu() - s.double().cpu()).abs().max()) <= 2e-5


@gpu
@pytest.mark.parametrize("convention,H,W", CASES)
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_gradients_vs_float64_autograd(hip_device, kind, C, convention, H, W):
    """Error relative to the gradient's max-abs at most max(4 x the eager fp32 run's error, 1e-6), for random per-view
    cotangents of both terms, each term alone (the other cotangent NULL) and through photometric_loss.
    Largest kernel / eager ratio observed on the MI355X: DESIGN.md "SSIM / photometric loss"."""
    from freesplat_amd import ssim_loss as S
    c = _case(convention, kind, C, H, W)
    gt = c["gt"].to(hip_device)
    cs, cl = c["cs"].to(hip_device), c["cl"].to(hip_device)
    failures = []
    for mode in ("both", "ssim", "l1", "photometric"):
        pred = c["pred"].to(hip_device).requires_grad_(True)
        if mode == "photometric":
            loss = S.photometric_loss(pred, gt, 0.2, convention)
            assert abs(float(loss.detach()) - float(c["loss"])) <= 1e-5
            (got,) = torch.autograd.grad(loss, pred)
            eager = SR.photometric_grad(c["pred"], c["gt"], 0.2, convention, torch.float32, hip_device)[1]
        else:
            s, l1 = S.ssim_and_l1(pred, gt, convention)
            total = {"both": (s * cs).sum() + (l1 * cl).sum(), "ssim": (s * cs).sum(), "l1": (l1 * cl).sum()}[mode]
            (got,) = torch.autograd.grad(total, pred)
            eager = SR.grad(c["pred"], c["gt"], convention, cs if mode != "l1" else None, cl if mode != "ssim" else None,
                            torch.float32, hip_device)
        want = c["grads"][mode]
        assert got.shape == want.shape and got.dtype == torch.float32 and bool(got.isfinite().all())
        e_k, e_e = _err(got, want), _err(eager, want)
        print(f"{mode}: kernel err {e_k:.3e}, eager fp32 err {e_e:.3e}, bound {_bound(e_e):.3e}, ratio {e_k / max(e_e, 1e-30):.2f}")
        if e_k > _bound(e_e):
            failures.append((mode, e_k, e_e))
    assert not failures, failures


@gpu
@pytest.mark.parametrize("convention", SR.CONVENTIONS)
def test_identical_images(hip_device, convention):
    from freesplat_amd import ssim_loss as S
    x = torch.from_numpy(_inputs("smooth", B, 3, 40, 57)[0])
    pred = x.to(hip_device).requires_grad_(True)
    s = S.ssim(pred, x.to(hip_device), convention)
    assert float((s - 1).abs().max()) <= 1e-6
    (got,) = torch.autograd.grad(s.sum(), pred)
    ones = torch.ones(B)
    want = SR.grad(x, x, convention, ones, None)                          # (zero up to float64 rounding: S is at its maximum)
    eager = SR.grad(x, x, convention, ones, None, torch.float32, hip_device)
    e_k = float((got.double().cpu() - want).abs().max())
    e_e = float((eager.double().cpu() - want).abs().max())
    print(f"identical images: kernel abs err {e_k:.3e}, eager fp32 abs err {e_e:.3e}")
    assert e_k <= max(4 * e_e, 1e-9)


@gpu
@pytest.mark.parametrize("convention", SR.CONVENTIONS)
def test_constant_images_are_finite(hip_device, convention):
    from freesplat_amd import ssim_loss as S
    for a, b in ((0.2, 0.7), (0.5, 0.5), (1.3, -0.4), (0.0, 0.0)):
        pred = torch.full((2, 3, 20, 30), b, device=hip_device, requires_grad=True)
        gt = torch.full((2, 3, 20, 30), a, device=hip_device)
        loss = S.photometric_loss(pred, gt, 0.2, convention)
        (g,) = torch.autograd.grad(loss, pred)
        assert bool(loss.isfinite()) and bool(g.isfinite().all())
        if convention == "skimage":
            s = S.ssim(pred, gt, convention)
            want = (2 * a * b + R.C1) / (a * a + b * b + R.C1)
            assert torch.allclose(s.double().cpu(), torch.full((2,), want, dtype=torch.float64), atol=1e-6, rtol=0)


@gpu
@pytest.mark.parametrize("convention", SR.CONVENTIONS)
def test_determinism_runs_streams_and_batches(hip_device, convention):
    from freesplat_amd import ssim_loss as S
    gt, pred = (torch.from_numpy(a).to(hip_device) for a in _inputs("noise", 5, 3, 70, 300, seed=9))
    cs = torch.randn(5, generator=torch.Generator().manual_seed(2)).to(hip_device)
    cl = torch.randn(5, generator=torch.Generator().manual_seed(3)).to(hip_device)

    def run(p, g, a, b):
        p = p.clone().requires_grad_(True)
        s, l1 = S.ssim_and_l1(p, g, convention)
        return s.detach(), l1.detach(), torch.autograd.grad((s * a).sum() + (l1 * b).sum(), p)[0]

    first = run(pred, gt, cs, cl)
    for a, b in zip(first, run(pred, gt, cs, cl)):
        assert torch.equal(a, b)
    side = torch.cuda.Stream(device=hip_device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = run(pred, gt, cs, cl)
    torch.cuda.current_stream().wait_stream(side)
    for a, b in zip(first, third):
        assert torch.equal(a, b)
    for k in (0, 2, 4):
        alone = run(pred[k:k + 1], gt[k:k + 1], cs[k:k + 1], cl[k:k + 1])
        for a, b in zip(first, alone):
            assert torch.equal(a[k:k + 1], b)


@gpu
def test_nothing_is_held_without_a_pending_backward(hip_device, monkeypatch):
    from freesplat_amd import _lib, ssim_loss as S
    L = _lib.lib()
    real, calls = L.fs_ssim_loss_saved_bytes, []
    monkeypatch.setattr(L, "fs_ssim_loss_saved_bytes", lambda *a: calls.append(a) or real(*a))
    gt, pred = (torch.from_numpy(a).to(hip_device) for a in _inputs("noise", 2, 3, 64, 96))
    held = S.saved_bytes(2, 3, 64, 96, "3dgs")
    calls.clear()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(hip_device)
    out = S.photometric_loss(pred, gt)                                     # no input requires a gradient
    with torch.no_grad():
        out2 = S.photometric_loss(pred.clone().requires_grad_(True), gt)  # grad mode off
    torch.cuda.synchronize()
    assert not calls and out.grad_fn is None and out2.grad_fn is None and not out2.requires_grad
    assert torch.cuda.memory_allocated(hip_device) - before < held // 4
    p = pred.clone().requires_grad_(True)
    before = torch.cuda.memory_allocated(hip_device)
    out3 = S.photometric_loss(p, gt)
    assert len(calls) == 1 and out3.grad_fn is not None
    assert torch.cuda.memory_allocated(hip_device) - before >= held        # the three maps, until the backward has run
    out3.backward()
    assert p.grad is not None and bool(p.grad.isfinite().all())


@gpu
def test_error_cases(hip_device):
    from freesplat_amd import ssim_loss as S
    a = torch.rand(2, 3, 16, 20, device=hip_device)
    for fn in (S.ssim, S.dssim_loss, S.photometric_loss):
        with pytest.raises(ValueError):
            fn(a.cpu(), a)
        with pytest.raises(ValueError):
            fn(a, a.cpu())
        with pytest.raises(ValueError):
            fn(a, a[:, :, :15])
        with pytest.raises(ValueError):
            fn(a[0], a[0])
        with pytest.raises(ValueError):
            fn(a[:0], a[:0])
        with pytest.raises(ValueError):
            fn(a, a, convention="other")
        with pytest.raises(RuntimeError):
            fn(a, a.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="win_size"):
        S.ssim(a[:, :, :10], a[:, :, :10], "skimage")
    with pytest.raises(ValueError, match="win_size"):
        S.photometric_loss(a[..., :10], a[..., :10], convention="skimage")
    assert S.ssim(a[:, :, :10], a[:, :, :10], "3dgs").shape == (2,)
    # what the inputs go through: other dtypes and non-contiguous views
    s = S.ssim(a, a * 0.9, "skimage")
    assert torch.equal(S.ssim(a.double(), (a * 0.9).double(), "skimage"), s)
    al = a.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not al.is_contiguous() and torch.equal(S.ssim(al, a * 0.9, "skimage"), s)
    p = al.clone().requires_grad_(True)
    S.dssim_loss(p, a * 0.9).backward()
    assert p.grad.shape == p.shape and bool(p.grad.isfinite().all())


# ---- guard bands (tests/guarded_alloc.py, the harness of tests/test_memory_guards.py) ----

GUARDED = {
    "fs_ssim_loss_forward": "test_guard_bands_photometric_loss",
    "fs_ssim_loss_backward": "test_guard_bands_photometric_loss",
}


@gpu
@pytest.mark.parametrize("H,W", [(13, 300), TWO_TILES])
@pytest.mark.parametrize("convention", SR.CONVENTIONS)
def test_guard_bands_photometric_loss(hip_device, convention, H, W):
    """Forward and backward unguarded and under the three fills: no guard byte changes, nothing non-finite, the same bits."""
    from freesplat_amd import ssim_loss as S
    from test_memory_guards import _four
    gt, pred = (torch.from_numpy(a) for a in _inputs("noise", 2, 3, H, W, seed=H))

    def op(place):
        p = place(pred, True)
        loss = S.photometric_loss(p, place(gt), 0.2, convention)
        return [loss], lambda: torch.autograd.grad([loss], [p])
    _four(op, hip_device, f"photometric loss {convention} {H}x{W}")

    def ssim_alone(place):                       # g_l1 = NULL
        p = place(pred, True)
        s = S.ssim(p, place(gt), convention)
        g = place(torch.tensor([0.5, -1.5]))
        return [s], lambda: torch.autograd.grad([s], [p], [g])
    _four(ssim_alone, hip_device, f"ssim {convention} {H}x{W}")


def test_every_loss_entry_point_with_a_device_buffer_has_a_guarded_case():
    text = open(os.path.join(ROOT, "include", "freesplat_amd_loss.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    with_buffers = sorted(n for n, args in re.findall(r"\b(fs_\w+)\s*\(([^)]*)\)", text) if "*" in args)
    assert with_buffers == sorted(GUARDED) and len(with_buffers) == 2
    me = sys.modules[__name__]
    for n, t in GUARDED.items():
        fn = getattr(me, t, None)
        assert callable(fn), (n, t)
        assert "gpu" in [m.name for m in getattr(fn, "pytestmark", [])], f"{n}: {t} is not a GPU case"
