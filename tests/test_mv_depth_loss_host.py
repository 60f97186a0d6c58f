"""Host checks of the multi-view / scale-invariant depth losses (no GPU): the case generator's decidability condition over every
case the GPU tests use, the float64 restatement (tests/mv_depth_ref.py) against its own fp32 evaluation, against finite
differences and against the reference's MVDepthLoss / ScaleInvariantLoss (tests/golden/mv_depth_small.npz, written by
tests/golden/make_mv_depth_golden.py), pair_transforms, the C boundary of include/freesplat_amd_mvdepth.h without a device and
the Python layer's argument errors."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import mv_depth_cases as MC
import mv_depth_ref as MR
from util_abi import declared_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = ["fs_mvdepth_api_version", "fs_mvdepth_scratch_bytes", "fs_mv_depth_forward", "fs_mv_depth_backward",
            "fs_si_depth_forward", "fs_si_depth_backward"]
GOLDEN = {"a": (9, 11, 3, 2), "b": (16, 20, 1, 1)}          # name -> (H, W, K, views)


# ---- the cases ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cs", MC.CASES)
def test_every_case_is_decidable_and_fp32_selects_what_float64_selects(cs):
    """No decision of a case can flip in fp32, at most 1 % of its pixels were made holes for that, and an fp32 evaluation of the
    restatement on the CPU makes float64's selection on every pixel (the multi-view term's and the scale-invariant term's)."""
    c = MC.case(*cs)
    MC.assert_decidable(c)
    print(f"{cs}: {c['holed']:.4f} of the pixels made holes")
    total, cnt, res = c["vals"]
    t32, c32, r32 = MR.mv_values(c, torch.float32)
    assert torch.equal(torch.isnan(r32), torch.isnan(res)) and torch.equal(c32.double(), cnt)
    assert torch.equal(MR.si_values(c, torch.float32)[2].double(), c["si_vals"][2])
    live = cnt[:-1] if c["invalid_view"] else cnt
    assert bool((live.sum(1) > 0).all()), "every view with a valid pixel has a selected one"
    if c["invalid_view"]:
        assert not bool(cnt[-1].any()) and not bool(total[-1].any()) and float(c["si_vals"][2][-1]) == 0.0
    if c["src_index"] is not None:                       # the pairs whose index is out of range contribute nothing
        off = (c["src_index"] < 0) | (c["src_index"] >= c["src"].shape[0])
        assert bool(off.any()) and not bool(cnt[off].any()) and bool(torch.isnan(res[off]).all())
        assert torch.equal(cnt[0, 0], cnt[0, 2]) and float(cnt[0, 0]) > 0          # the repeated index


def test_the_case_list_covers_what_the_kernels_branch_on():
    from freesplat_amd import mv_depth_loss as M
    shapes = {c[:4] for c in MC.CASES}
    assert {(1, 1, 1, 1), (1, 67, 1, 67), (37, 53, 37, 53), (33, 130, 33, 130), (5, 130, 7, 96)} == shapes
    assert {c[4] for c in MC.CASES if not c[6]} == {1, 3, M.MAX_SOURCES}
    assert {c[5] for c in MC.CASES} == {True, False} and any(c[6] for c in MC.CASES) and any(c[7] for c in MC.CASES)
    assert 33 * 130 > 4 * M.CHUNK > 37 * 53 > M.CHUNK and 53 % 4 and 130 % M.CHUNK and M.CHUNK % 130


# ---- the restatement against known answers, finite differences and the reference ----------------------------------------------

def test_an_identity_pair_compares_the_prediction_with_the_source_pixel_for_pixel():
    g = torch.Generator().manual_seed(0)
    gt = 1.0 + 2.0 * torch.rand(1, 6, 7, generator=g, dtype=torch.float64)
    src = (gt * (1.0 + 0.2 * torch.rand(1, 6, 7, generator=g, dtype=torch.float64)))[:, None]
    pred = gt * 1.1
    pairs = torch.eye(3, 4, dtype=torch.float64).view(1, 1, 3, 4)
    total, cnt = MR.terms(pred, gt, src, pairs)
    assert float(cnt) == 42.0
    assert abs(float(total) - float((torch.log(pred + MR.EPS) - torch.log(src[:, 0])).abs().sum())) <= 1e-12
    occluded = src.clone()
    occluded[0, 0, 2, 3] = gt[0, 2, 3] / 1.06                               # the point lies behind what the source measured
    assert float(MR.terms(pred, gt, occluded, pairs)[1]) == 41.0
    shifted = pairs.clone()
    shifted[..., 0, 3] = 1.0                                                # u = x + 1 / gt: at gt < 2 the next column
    r = MR.residuals(pred, gt, src, shifted)
    assert bool(torch.isnan(r[0, 0, :, -1][gt[0, :, -1] < 2.0]).all())      # ... which the last column does not have


def test_scale_invariance():
    c = MC.case(*MC.CASES[4])
    d, g, a = c["depth"].double(), c["gt"].double(), c["alpha"].double()
    one = MR.scale_invariant_loss(d, g, a, 1.0)
    assert float(one) > 0 and abs(float(MR.scale_invariant_loss(3.0 * d, g, a, 1.0)) - float(one)) <= 1e-12
    assert abs(float(MR.scale_invariant_loss(3.0 * d, g, a, 0.85)) - float(MR.scale_invariant_loss(d, g, a, 0.85))) > 1e-3
    nothing = torch.full_like(g, float("nan"))
    assert float(MR.scale_invariant_loss(d, nothing, a)) == 0.0 and float(MR.mv_depth_loss(d, nothing, c["src"].double(), c["pairs"].double(), a)) == 0.0


@pytest.mark.parametrize("cs", [MC.CASES[4], MC.CASES[12]])
def test_restatement_gradients_against_finite_differences(cs):
    """Central differences in float64 at spot pixels, for the multi-view sum with a random cotangent and for both scalar losses."""
    c = MC.case(*cs)
    d0, a0 = c["depth"].double(), c["alpha"].double()
    gt, src, pairs = c["gt"].double(), c["src"].double(), c["pairs"].double()
    kw = dict(c["kw"], src_index=c["src_index"])
    si_kw = MR._si_kw(c)
    fns = {
        "mv terms": (lambda d, a: (MR.terms(d, gt, src, pairs, a, **kw)[0] * c["g_sum"]).sum(), c["grads"]["terms"]),
        "mv loss": (lambda d, a: MR.mv_depth_loss(d, gt, src, pairs, a, **kw), c["grads"]["loss"]),
        "si loss": (lambda d, a: MR.scale_invariant_loss(d, gt, a, **si_kw), c["si_grads"]["loss"]),
    }
    sel = (~torch.isnan(c["vals"][2])).any(1) & (a0 > 2 * MC.FLOOR)
    spots = sel.nonzero()[:: max(1, int(sel.sum()) // 6)][:6]
    assert len(spots) >= 4
    for name, (fn, (g_d, g_a)) in fns.items():
        for b, y, x in spots.tolist():
            for which, base, grad in (("depth", d0, g_d), ("alpha", a0, g_a)):
                h = 1e-6 * float(base[b, y, x])
                lo, hi = base.clone(), base.clone()
                lo[b, y, x] -= h
                hi[b, y, x] += h
                fd = (float(fn(hi, a0) - fn(lo, a0)) if which == "depth" else float(fn(d0, hi) - fn(d0, lo))) / (2 * h)
                assert abs(fd - float(grad[b, y, x])) <= 1e-5 * max(1.0, abs(fd)), (name, which, (b, y, x), fd, float(grad[b, y, x]))


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_restatement_against_the_reference(name):
    """The reference's MVDepthLoss and ScaleInvariantLoss in float64 (values and autograd's gradients with respect to the
    prediction) against the restatement given cx - 0.5 (the cases' integer-pixel intrinsics are that already) and pooled over
    the batch: 1e-10 relative, both float64, only the association of the matrix products differs."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "mv_depth_small.npz"))
    g = {k[len(name) + 1:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(name + "_")}
    H, W, K, views = GOLDEN[name]
    assert tuple(g["src"].shape) == (views, K, H, W) and float(g["holed"]) <= MC.MAX_HOLED
    pairs = MR.pair_transforms(g["intr"], g["cam_to_world"], g["src_intr"], g["src_world_to_cam"])
    assert float((pairs - g["pairs"].double()).abs().max()) <= 1e-6 * float(pairs.abs().max())
    d = g["depth"].double().requires_grad_(True)
    gt, src = g["gt"].double(), g["src"].double()
    total, cnt = MR.terms(d, gt, src, pairs)
    assert bool((cnt.sum(0) > 0).all()), "no source column is empty"
    loss = MR.combine(total, cnt)
    grad, = torch.autograd.grad(loss, d)
    assert abs(float(loss.detach()) - float(g["mv_loss"])) <= 1e-10 * float(g["mv_loss"])
    assert float((grad - g["mv_grad"]).abs().max()) <= 1e-10 * float(g["mv_grad"].abs().max()) and bool(g["mv_grad"].any())
    si = MR.scale_invariant_loss(d, gt)
    grad, = torch.autograd.grad(si, d)
    assert abs(float(si.detach()) - float(g["si_loss"])) <= 1e-10 * float(g["si_loss"])
    assert float((grad - g["si_grad"]).abs().max()) <= 1e-10 * float(g["si_grad"].abs().max()) and bool(g["si_grad"].any())


def test_pair_transforms_against_the_restatement():
    """The module's batched float64 matmuls (it runs where cam_to_world lives: here the CPU) against the restatement's loops,
    for [B, K] sources and for the pool form; q(D) of a pixel is the source camera's projection of the lifted point."""
    from freesplat_amd.mv_depth_loss import pair_transforms
    for cs in (MC.CASES[10], MC.CASES[12]):
        c = MC.case(*cs)
        cams = c["cams"]
        got = pair_transforms(cams["intr"], cams["cam_to_world"], cams["src_intr"], cams["src_world_to_cam"], c["src_index"])
        assert got.dtype == torch.float32 and got.shape == c["pairs"].shape
        on = torch.ones(got.shape[:2], dtype=torch.bool) if c["src_index"] is None else \
            (c["src_index"] >= 0) & (c["src_index"] < c["src"].shape[0])
        assert float((got - c["pairs"])[on].abs().max()) <= 2e-7 * float(c["pairs"].abs().max())
        per_view = cams["intr"].expand(MC.B, 4).contiguous()
        assert torch.equal(pair_transforms(per_view, cams["cam_to_world"], cams["src_intr"], cams["src_world_to_cam"], c["src_index"]), got)
    c = MC.case(*MC.CASES[10])
    cams, (x, y, D) = c["cams"], (17.0, 3.0, 2.5)
    fx, fy, cx, cy = cams["intr"].tolist()
    world = cams["cam_to_world"][1] @ torch.tensor([D * (x - cx) / fx, D * (y - cy) / fy, D, 1.0], dtype=torch.float64)
    cam = cams["src_world_to_cam"][1, 2] @ world
    sx, sy, scx, scy = cams["src_intr"].tolist()
    want = torch.stack([sx * cam[0] + scx * cam[2], sy * cam[1] + scy * cam[2], cam[2]])
    q = D * (c["pairs"][1, 2, :, :3].double() @ torch.tensor([x, y, 1.0], dtype=torch.float64)) + c["pairs"][1, 2, :, 3].double()
    assert float((q - want).abs().max()) <= 1e-4


# ---- the C boundary ------------------------------------------------------------------------------------------------------------

def test_mvdepth_header_is_exported_and_bound():
    from freesplat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    names = declared_names("freesplat_amd_mvdepth.h")
    assert names == sorted(EXPECTED)
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/freesplat_amd_mvdepth.h but not exported"
    assert set(_lib.MVDEPTH_SIGNATURES) == set(names)
    assert _lib.lib().fs_mvdepth_api_version() == 1 == _lib.MVDEPTH_API_VERSION
    text = open(os.path.join(ROOT, "include", "freesplat_amd_mvdepth.h")).read()
    assert re.search(r"#define\s+FS_MVDEPTH_API_VERSION\s+1\b", text)
    assert re.search(r"#define\s+FS_MVDEPTH_MAX_SOURCES\s+16\b", text) and _lib.MVDEPTH_MAX_SOURCES == 16


P = C.c_void_p(4096)      # a fake non-NULL pointer: nothing may launch with it
SC = (1.05, 0.0, math.inf, 1e-3)


def _mv_fwd(L, B=2, K=3, H=16, W=16, Hs=16, Ws=16, S=0, ptrs=None, sc=SC):
    ptrs = [P, P, P, P, None, P, P, P, None, P] if ptrs is None else ptrs   # depth gt alpha src index pairs | sum cnt residual scratch
    return L.fs_mv_depth_forward(B, K, H, W, Hs, Ws, S, *ptrs[:6], *sc, *ptrs[6:], None)


def _mv_bwd(L, B=2, K=3, H=16, W=16, Hs=16, Ws=16, S=0, ptrs=None, sc=SC):
    ptrs = [P, P, P, P, None, P, P, P, P] if ptrs is None else ptrs          # depth gt alpha src index pairs | g_sum g_depth g_alpha
    return L.fs_mv_depth_backward(B, K, H, W, Hs, Ws, S, *ptrs[:6], *sc, *ptrs[6:], None)


def _si_fwd(L, B=2, H=16, W=16, ptrs=None, sc=SC[1:]):
    ptrs = [P, P, P, P, P, P, P] if ptrs is None else ptrs                   # depth gt alpha | s1 s2 n scratch
    return L.fs_si_depth_forward(B, H, W, *ptrs[:3], *sc, *ptrs[3:], None)


def _si_bwd(L, B=2, H=16, W=16, ptrs=None, sc=SC[1:]):
    ptrs = [P, P, P, P, P, P, P] if ptrs is None else ptrs                   # depth gt alpha | g_s1 g_s2 g_depth g_alpha
    return L.fs_si_depth_backward(B, H, W, *ptrs[:3], *sc, *ptrs[3:], None)


def test_entry_points_validate_before_touching_a_device():
    """FS_ERR_INVALID_ARG (-1) for NULL required pointers, non-positive sizes, a pool without a size, alpha and g_alpha not given
    together, bad scalars; FS_ERR_UNSUPPORTED (-3) for K > 16 and for sizes beyond the 32-bit indices -- with fake non-NULL
    pointers, so nothing may launch."""
    from freesplat_amd import _lib
    L = _lib.lib()
    checked = 0
    for name, (rt, at) in _lib.MVDEPTH_SIGNATURES.items():
        if rt is not C.c_int or not at:
            continue
        for size in (1, 16):
            args = [size if a is C.c_int32 else (1.0 if a is C.c_float else None) for a in at]
            assert getattr(L, name)(*args) == -1, name
        zero = [0 if a is C.c_int32 else (1.0 if a is C.c_float else P) for a in at]
        assert getattr(L, name)(*zero) == -1, name
        checked += 1
    assert checked == 4
    for call in (_mv_fwd, _mv_bwd):
        for bad in (dict(B=0), dict(B=-1), dict(K=0), dict(K=-2), dict(H=0), dict(W=-3), dict(Hs=0), dict(Ws=0)):
            assert call(L, **bad) == -1, (call.__name__, bad)
        assert call(L, K=17) == -3, call.__name__
        assert call(L, H=46341, W=46341) == -3 and call(L, Hs=46341, Ws=46341) == -3, call.__name__
        assert call(L, B=2 ** 30, H=128, W=128) == -3, call.__name__
        for sc in ((math.nan,) + SC[1:], (1.05, math.nan, 1.0, 1e-3), (1.05, 0.0, math.nan, 1e-3), (1.05, 0.0, 1.0, 0.0),
                   (1.05, 0.0, 1.0, -1.0), (1.05, 0.0, 1.0, math.inf), (1.05, 0.0, 1.0, math.nan)):
            assert call(L, sc=sc) == -1, (call.__name__, sc)
    base = [P, P, P, P, None, P, P, P, None, P]
    for i in (0, 1, 3, 5, 6, 7, 9):                                          # every required pointer of the forward
        assert _mv_fwd(L, ptrs=[None if k == i else v for k, v in enumerate(base)]) == -1, i
    with_index = [P, P, P, P, P, P, P, P, None, P]
    assert _mv_fwd(L, ptrs=with_index, S=0) == -1 and _mv_fwd(L, ptrs=with_index, S=-1) == -1        # a pool without a size
    base = [P, P, P, P, None, P, P, P, P]
    for i in (0, 1, 3, 5, 6, 7):
        assert _mv_bwd(L, ptrs=[None if k == i else v for k, v in enumerate(base)]) == -1, i
    assert _mv_bwd(L, ptrs=[P, P, None, P, None, P, P, P, P]) == -1          # g_alpha without alpha
    assert _mv_bwd(L, ptrs=[P, P, P, P, None, P, P, P, None]) == -1          # alpha without g_alpha
    for call in (_si_fwd, _si_bwd):
        for bad in (dict(B=0), dict(H=-1), dict(W=0)):
            assert call(L, **bad) == -1, (call.__name__, bad)
        assert call(L, H=46341, W=46341) == -3 and call(L, B=2 ** 30, H=128, W=128) == -3, call.__name__
        for sc in ((math.nan, 1.0, 1e-3), (0.0, math.nan, 1e-3), (0.0, 1.0, 0.0), (0.0, 1.0, math.inf)):
            assert call(L, sc=sc) == -1, (call.__name__, sc)
    for i in (0, 1, 3, 4, 5, 6):
        assert _si_fwd(L, ptrs=[None if k == i else P for k in range(7)]) == -1, i
    for i in (0, 1, 3, 4, 5):
        assert _si_bwd(L, ptrs=[None if k == i else P for k in range(7)]) == -1, i
    assert _si_bwd(L, ptrs=[P, P, None, P, P, P, P]) == -1 and _si_bwd(L, ptrs=[P, P, P, P, P, P, None]) == -1


def test_scratch_bytes():
    """max(2 K, 3) doubles per workgroup of CHUNK pixels, rounded up to 256; 0 for what the entry points refuse."""
    from freesplat_amd import _lib, mv_depth_loss as M
    L = _lib.lib()
    al = lambda x: (x + 255) // 256 * 256
    for B, K, H, W in ((1, 1, 1, 1), (2, 3, 13, 9), (4, 4, 968, 1296), (8, 7, 384, 512), (2, 16, 33, 130), (3, 0, 64, 65)):
        assert L.fs_mvdepth_scratch_bytes(B, K, H, W) == al(8 * max(2 * K, 3) * B * -(-H * W // M.CHUNK)) > 0
    for K in range(2, 17):                                # the size for K >= 2 serves the scale-invariant forward too
        assert L.fs_mvdepth_scratch_bytes(2, K, 37, 53) >= L.fs_mvdepth_scratch_bytes(2, 0, 37, 53)
    for bad in ((0, 1, 4, 4), (1, -1, 4, 4), (1, 17, 4, 4), (1, 1, 0, 4), (1, 1, 4, -1), (1, 1, 46341, 46341), (2 ** 30, 1, 128, 128)):
        assert L.fs_mvdepth_scratch_bytes(*bad) == 0, bad


# ---- the Python layer's argument errors that need no device ------------------------------------------------------------------

def test_argument_errors_without_a_device():
    from freesplat_amd import mv_depth_loss as M
    d = 1.0 + torch.rand(2, 8, 9)
    src, pairs = 1.0 + torch.rand(2, 3, 8, 9), torch.eye(3, 4).expand(2, 3, 3, 4)
    for fn in (M.mv_depth_loss, M.mv_depth_terms, M.mv_depth_residuals):
        with pytest.raises(ValueError, match="freesplat_amd.mv_depth_loss.*no CPU path"):
            fn(d, d, src, pairs)
    for fn in (M.scale_invariant_loss, M.si_depth_terms):
        with pytest.raises(ValueError, match="freesplat_amd.mv_depth_loss.*no CPU path"):
            fn(d, d)
        with pytest.raises(ValueError, match="alpha_floor"):
            fn(d, d, alpha_floor=0.0)
        with pytest.raises(ValueError, match="NaN"):
            fn(d, d, max_depth=math.nan)
        with pytest.raises(RuntimeError, match="gt gets no gradient"):
            fn(d, d.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="occlusion"):
        M.mv_depth_loss(d, d, src, pairs, occlusion=0.0)
    with pytest.raises(ValueError, match="si_lambda"):
        M.scale_invariant_loss(d, d, si_lambda=math.inf)
    with pytest.raises(RuntimeError, match="gt gets no gradient"):
        M.mv_depth_loss(d, d.clone().requires_grad_(True), src, pairs)
    T = torch.eye(4).expand(2, 4, 4)
    k = (9.0, 9.0, 4.0, 3.5)
    assert tuple(M.pair_transforms(k, T, k, T[:, None].expand(2, 3, 4, 4)).shape) == (2, 3, 3, 4)
    for bad in (lambda: M.pair_transforms(k, T[0], k, T[:, None]), lambda: M.pair_transforms(k, T, k, T),
                lambda: M.pair_transforms((9.0, 9.0, 4.0), T, k, T[:, None]), lambda: M.pair_transforms(k, T, torch.ones(2, 2, 4), T[:, None]),
                lambda: M.pair_transforms(k, T, k, T[:, None], torch.zeros(2, 1, dtype=torch.int32)),
                lambda: M.pair_transforms(k, T, k, T, torch.zeros(2, 1))):
        with pytest.raises(ValueError, match="freesplat_amd.mv_depth_loss"):
            bad()
    ident = M.pair_transforms(k, T, k, T, torch.tensor([[0, 1, -1], [5, 1, 0]]))         # an index out of range stays on the device
    assert tuple(ident.shape) == (2, 3, 3, 4) and float((ident - torch.eye(3, 4)).abs().max()) <= 1e-6
