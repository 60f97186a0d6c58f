"""CPU checks of the SSIM / photometric loss: the float64 restatement (tests/ssim_loss_ref.py) against the metric's restatement
and against its own closed-form gradient (the gather csrc/ssim_loss.hip implements), and the C boundary of
include/freesplat_amd_loss.h (exports, binding table, argument validation, size queries).  No GPU."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest
import torch

import metrics_ref as R
import ssim_loss_ref as SR
from util_abi import declared_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(11, 11), (13, 40), (70, 300)]


def _pair(B, C_, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(B, C_, H, W, generator=g, dtype=torch.float64)
    pred = (gt + 0.1 * torch.randn(B, C_, H, W, generator=g, dtype=torch.float64)).clamp(-0.2, 1.2)
    return pred, gt


@pytest.mark.parametrize("H,W", SHAPES)
def test_skimage_map_equals_the_metric_restatement(H, W):
    pred, gt = _pair(2, 3, H, W, seed=H + W)
    got = SR.ssim_map(pred, gt, "skimage").numpy()
    for b in range(2):
        assert np.abs(got[b] - R.ssim_map(gt[b].numpy(), pred[b].numpy())).max() <= 1e-12
    s, l1 = SR.values(pred, gt, "skimage")
    assert np.abs(s.numpy() - R.ssim_batch(gt.numpy(), pred.numpy())).max() <= 1e-12
    assert torch.allclose(l1, (pred - gt).abs().flatten(1).mean(1), rtol=1e-14, atol=0)


def test_3dgs_map_is_the_zero_padded_population_form():
    """Written out without conv2d: pad by 5 with zeros, the 'valid' filter of metrics_ref, covariance factor 1."""
    pred, gt = _pair(1, 2, 9, 14, seed=3)             # smaller than the window in one axis
    got = SR.ssim_map(pred, gt, "3dgs").numpy()[0]
    assert got.shape == (2, 9, 14)
    pad = lambda a: np.pad(a, R.RAD)
    for c in range(2):
        x, y = pad(gt[0, c].numpy()), pad(pred[0, c].numpy())
        f = R._valid_filter
        ux, uy = f(x), f(y)
        vx, vy, vxy = f(x * x) - ux * ux, f(y * y) - uy * uy, f(x * y) - ux * uy
        want = (2 * ux * uy + R.C1) * (2 * vxy + R.C2) / ((ux * ux + uy * uy + R.C1) * (vx + vy + R.C2))
        assert np.abs(got[c] - want).max() <= 1e-12


@pytest.mark.parametrize("convention,H,W", [(c, H, W) for c in SR.CONVENTIONS for H, W in SHAPES] + [("3dgs", 3, 7)])
def test_closed_form_gradient_equals_autograd(convention, H, W):
    pred, gt = _pair(3, 2, H, W, seed=7 * H + W)
    pred[0, 0, 0, :3] = gt[0, 0, 0, :3]                # sign(0) = 0
    g = torch.Generator().manual_seed(1)
    gs, gl = torch.randn(3, generator=g, dtype=torch.float64), torch.randn(3, generator=g, dtype=torch.float64)
    for a, b in ((gs, gl), (gs, None), (None, gl)):
        want = SR.grad(pred, gt, convention, a, b)
        got = SR.closed_form_grad(pred, gt, convention, a, b)
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert torch.all(SR.closed_form_grad(pred, gt, convention, None, gl)[0, 0, 0, :3] == 0)


def test_loss_header_is_exported_and_bound():
    from freesplat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    names = declared_names("freesplat_amd_loss.h")
    assert "fs_ssim_loss_forward" in names and "fs_ssim_loss_backward" in names and len(names) == 5
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/freesplat_amd_loss.h but not exported"
        assert n in _lib.LOSS_SIGNATURES, f"{n} has no ctypes signature in freesplat_amd/_lib.py"
    assert set(_lib.LOSS_SIGNATURES) == set(names)
    assert not set(_lib.LOSS_SIGNATURES) & set(_lib.SIGNATURES)
    assert _lib.lib().fs_loss_api_version() == 1 == _lib.LOSS_API_VERSION
    text = open(os.path.join(ROOT, "include", "freesplat_amd_loss.h")).read()
    assert re.search(r"#define\s+FS_LOSS_API_VERSION\s+1\b", text)
    assert re.search(r"#define\s+FS_SSIM_SKIMAGE\s+%d\b" % _lib.SSIM_SKIMAGE, text)
    assert re.search(r"#define\s+FS_SSIM_3DGS\s+%d\b" % _lib.SSIM_3DGS, text)


def test_main_header_keeps_its_symbol_set():
    """The new entry points live in their own header: include/freesplat_amd.h declares the names it declared before
    (their count and the digest of the sorted list), and FS_ABI_VERSION stays 9."""
    from freesplat_amd import _lib
    names = declared_names("freesplat_amd.h")
    assert set(names) == set(_lib.SIGNATURES) and not any("ssim_loss" in n or "loss_api" in n for n in names)
    assert len(names) == 93
    assert hashlib.sha256("\n".join(names).encode()).hexdigest() == "590e07f0e577c48904722252d8732a99cfa85cacaed1070a8f78789024ebb521"
    assert _lib.ABI_VERSION == 9 and _lib.lib().fs_abi_version() == 9


def test_entry_points_validate_before_touching_a_device():
    """NULL pointers with positive sizes: FS_ERR_INVALID_ARG (-1) from every int-returning entry point, as are an unknown
    flag, non-positive sizes, an image below the window under the skimage flag, and a backward without any cotangent or with
    an SSIM cotangent but no saved maps -- all with fake non-NULL pointers, so nothing may launch."""
    from freesplat_amd import _lib
    L = _lib.lib()
    for name, (rt, at) in _lib.LOSS_SIGNATURES.items():
        if rt is not C.c_int or not at:
            continue
        for size in (1, 16):
            assert getattr(L, name)(*[size if a is C.c_int32 else None for a in at]) == -1, name
    p = C.c_void_p(4096)
    fwd = lambda B=1, C_=3, H=16, W=16, flags=1, ptrs=(p,) * 6: L.fs_ssim_loss_forward(B, C_, H, W, flags, *ptrs, None)
    bwd = lambda B=1, C_=3, H=16, W=16, flags=1, ptrs=(p,) * 7: L.fs_ssim_loss_backward(B, C_, H, W, flags, *ptrs, None)
    for bad in (dict(B=0), dict(C_=0), dict(H=0), dict(W=-3), dict(flags=0), dict(flags=3), dict(flags=4), dict(H=10), dict(W=10)):
        assert fwd(**bad) == -1 and bwd(**bad) == -1, bad
    assert fwd(flags=2, H=0) == -1 and bwd(flags=2, W=0) == -1
    for i in (0, 1, 2, 3, 5):                          # pred, gt, ssim, l1_mean, scratch (saved is optional)
        assert fwd(ptrs=tuple(None if k == i else p for k in range(6))) == -1, i
    for i in (0, 1, 5):                                # pred, gt, g_pred (the reserved scratch is optional)
        assert bwd(ptrs=tuple(None if k == i else p for k in range(7))) == -1, i
    assert bwd(ptrs=(p, p, None, None, p, p, p)) == -1             # no cotangent at all
    assert bwd(ptrs=(p, p, p, None, None, p, p)) == -1             # an SSIM cotangent without the saved maps


def test_size_queries_and_tile_constants():
    from freesplat_amd import _lib
    from freesplat_amd import ssim_loss as S
    L = _lib.lib()
    al = lambda x: (x + 255) // 256 * 256
    for flags, crop in ((_lib.SSIM_SKIMAGE, 10), (_lib.SSIM_3DGS, 0)):
        for C_, H, W in ((3, 968, 1296), (1, 11, 11), (3, 65, 247)):
            prev_saved = prev_scratch = 0
            for B in (1, 2, 5, 16, 64):
                saved, scratch = L.fs_ssim_loss_saved_bytes(B, C_, H, W, flags), L.fs_ssim_loss_scratch_bytes(B, C_, H, W, flags)
                assert saved == al(12 * B * C_ * (H - crop) * (W - crop)) > 0 and saved >= prev_saved
                tiles = -(-W // S.TILE_W) * -(-H // S.TILE_H)
                assert scratch == al(16 * B * C_ * tiles) > 0 and scratch >= prev_scratch
                prev_saved, prev_scratch = saved, scratch
            assert L.fs_ssim_loss_saved_bytes(64, C_, H, W, flags) > L.fs_ssim_loss_saved_bytes(1, C_, H, W, flags)
            assert S.saved_bytes(2, C_, H, W, "skimage" if crop else "3dgs") == L.fs_ssim_loss_saved_bytes(2, C_, H, W, flags)
        for bad in ((0, 3, 16, 16), (1, 0, 16, 16), (1, 3, 0, 16), (1, 3, 16, -1)):
            assert L.fs_ssim_loss_saved_bytes(*bad, flags) == 0 and L.fs_ssim_loss_scratch_bytes(*bad, flags) == 0
    assert L.fs_ssim_loss_saved_bytes(1, 3, 10, 16, _lib.SSIM_SKIMAGE) == 0 and L.fs_ssim_loss_saved_bytes(1, 3, 10, 16, _lib.SSIM_3DGS) > 0
    assert L.fs_ssim_loss_saved_bytes(1, 3, 16, 16, 0) == 0 and L.fs_ssim_loss_scratch_bytes(1, 3, 16, 16, 3) == 0
    # the module's tile constants are the kernel's: one more row or column is one more tile
    one = L.fs_ssim_loss_scratch_bytes(16, 1, S.TILE_H, S.TILE_W, _lib.SSIM_3DGS)
    assert one == 256 and L.fs_ssim_loss_scratch_bytes(16, 1, S.TILE_H + 1, S.TILE_W, _lib.SSIM_3DGS) == 512
    assert L.fs_ssim_loss_scratch_bytes(16, 1, S.TILE_H, S.TILE_W + 1, _lib.SSIM_3DGS) == 512


def test_python_layer_refuses_what_it_cannot_run():
    """The error cases that need no device: CPU tensors, an unknown convention."""
    from freesplat_amd import ssim_loss as S
    a = torch.rand(1, 3, 16, 16)
    for fn in (S.ssim, S.dssim_loss, S.photometric_loss, S.ssim_and_l1):
        with pytest.raises(ValueError, match="HIP device"):
            fn(a, a)
    with pytest.raises(ValueError, match="convention"):
        S.ssim(a, a, convention="ms-ssim")
