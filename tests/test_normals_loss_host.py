"""CPU checks of the normals loss: the float64 restatement (tests/normals_loss_ref.py, NaN propagation) against known answers and
against an explicit mask formulation of the definitions, the backward gather csrc/normals_loss.hip implements against autograd,
the C boundary of include/freesplat_amd_normals.h (exports, binding table, revision, argument validation), the Python layer's
error cases, and the GPU cases' input generator (tests/normals_loss_cases.py) run over every case.  No GPU."""
import ctypes as C
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import normals_loss_cases as NC
import normals_loss_ref as NR
from util_abi import declared_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = ["fs_depth_normals_backward", "fs_depth_normals_forward", "fs_normals_api_version", "fs_normals_loss_backward",
            "fs_normals_loss_forward", "fs_normals_scratch_bytes"]
HOLES = (float("nan"), float("inf"), 0.0, -1.0)


def _inputs(B, H, W, seed, holes=0.25, with_alpha=True):
    """float64 (depth, gt_depth, alpha | None, intr): holes of the four kinds in both maps, alpha below the floor, exact zeros."""
    g = torch.Generator().manual_seed(seed)
    gt = NC.surface(H, W, B, g)
    depth = gt * (1.0 + 0.05 * torch.randn(B, H, W, generator=g, dtype=torch.float64))
    kinds = torch.tensor(HOLES, dtype=torch.float64)
    if holes:
        gt = torch.where(NC.blocky(H, W, B, g, holes), kinds[torch.randint(0, 4, (B, H, W), generator=g)], gt)
        depth = torch.where(NC.blocky(H, W, B, g, holes / 3), kinds[torch.randint(0, 4, (B, H, W), generator=g)], depth)
    alpha = None
    if with_alpha:
        alpha = 0.3 + 0.7 * torch.rand(B, H, W, generator=g, dtype=torch.float64)
        alpha = torch.where(torch.rand(B, H, W, generator=g) < 0.1, torch.full_like(alpha, 2e-4), alpha)
        depth = depth * alpha.clamp_min(1e-3)
        zero = torch.rand(B, H, W, generator=g) < 0.05
        alpha, depth = torch.where(zero, torch.zeros_like(alpha), alpha), torch.where(zero, torch.zeros_like(depth), depth)
    return depth, gt, alpha, NC.intrinsics(H, W, B).double()


# ---- known answers ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [(0.0, 0.0, 1.0), (0.3, -0.2, 0.9), (-0.5, 0.4, 0.7), (0.1, 0.6, 0.5)])
def test_a_plane_gives_its_own_normal(m):
    """m . X = d through arbitrary intrinsics, smoothing=None: every pixel whose nine taps are interior gives m / |m| (m_z > 0:
    the side that faces away from the camera, (0, 0, +1) for a fronto-parallel plane) to 1e-12."""
    H, W = 11, 14
    m = torch.tensor(m, dtype=torch.float64)
    m = m / m.norm()
    intr = torch.tensor([[13.7, 12.1, 6.3, 4.9], [9.2, 15.5, 7.7, 5.2]], dtype=torch.float64)
    rx, ry = NR.rays(intr, H, W, torch.float64, "cpu")
    depth = 2.3 / (m[0] * rx + m[1] * ry + m[2])
    assert bool((depth > 0).all())
    n = NR.depth_normals(depth, intr, smoothing=None)
    assert bool(torch.isfinite(n).all())
    err = (n - m.view(1, 3, 1, 1)).abs()[:, :, 1:-1, 1:-1].max()
    assert float(err) <= 1e-12
    # ... and the loss against itself is 0, against the mirrored normal 1
    total, cnt = NR.terms(depth, intr, gt_normals=m.view(1, 3, 1, 1).expand(2, 3, H, W), smoothing=None)
    assert torch.equal(cnt, torch.full((2,), float(H * W), dtype=torch.float64))
    inner = NR.pixel_terms(depth, intr, gt_normals=-m.view(1, 3, 1, 1).expand(2, 3, H, W), smoothing=None)[0][:, 1:-1, 1:-1]
    assert float((inner - 1.0).abs().max()) <= 1e-12


def test_a_constant_depth_gives_plus_z_with_smoothing():
    depth = torch.full((2, 9, 12), 1.75, dtype=torch.float64)
    intr = NC.intrinsics(9, 12).double()
    n = NR.depth_normals(depth, intr, smoothing=2.0)
    want = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).view(1, 3, 1, 1)
    assert float((n - want).abs()[:, :, 1:-1, 1:-1].max()) <= 1e-12
    w = NR.blur_weights(2.0)
    assert abs(float(w.sum()) - 1.0) <= 1e-7 and torch.equal(w, w.flip(0)) and bool((w > 0).all())
    assert torch.equal(w, w.float().double())                                  # rounded once to fp32
    # a single hole takes out the 7 x 7 window around it with smoothing, the 3 x 3 window without
    depth[0, 4, 6] = float("nan")
    bad = ~torch.isfinite(NR.depth_normals(depth, intr, smoothing=2.0)[0, 0])
    assert int(bad.sum()) == 49 and bool(bad[1:8, 3:10].all())
    bad = ~torch.isfinite(NR.depth_normals(depth, intr, smoothing=None)[0, 0])
    assert int(bad.sum()) == 9 and bool(bad[3:6, 5:8].all())


def test_pixel_centre_conventions():
    """The rasterizer's pixel p sees NDC (2 p + 1) / W - 1: intrinsics_from_fov's cx = (W - 1) / 2 is the half-pixel convention's
    W / 2 shifted by exactly 0.5, and its rays are the rasterizer's."""
    from freesplat_amd.normals_loss import intrinsics_from_fov
    H, W, tx, ty = 24, 40, 0.7, 0.45
    fx, fy, cx, cy = intrinsics_from_fov(tx, ty, H, W)
    assert (fx, fy) == (W / (2 * tx), H / (2 * ty)) and cx == W / 2 - 0.5 and cy == H / 2 - 0.5
    intr = torch.tensor([[fx, fy, cx, cy]], dtype=torch.float64)
    rx, ry = NR.rays(intr, H, W, torch.float64, "cpu")
    px, py = torch.arange(W, dtype=torch.float64), torch.arange(H, dtype=torch.float64)
    assert float((rx.flatten() - ((2 * px + 1) / W - 1) * tx).abs().max()) <= 1e-15
    assert float((ry.flatten() - ((2 * py + 1) / H - 1) * ty).abs().max()) <= 1e-15
    # integer pixel coordinates with a principal point at W / 2 (the adapter's unprojection with the dataset's K) are the same
    # rays moved by half a pixel: the normals of one depth map differ, and agree again once cx, cy carry the shift
    g = torch.Generator().manual_seed(0)
    depth = NC.surface(H, W, 1, g)
    a = NR.depth_normals(depth, intr, smoothing=None)
    b = NR.depth_normals(depth, torch.tensor([[fx, fy, W / 2, H / 2]], dtype=torch.float64), smoothing=None)
    assert float((a - b).abs().max()) > 1e-4
    px_half = NR.depth_normals(depth, torch.tensor([[fx, fy, W / 2 - 0.5, H / 2 - 0.5]], dtype=torch.float64), smoothing=None)
    assert torch.equal(a, px_half)


# ---- the mask formulation of the definitions, written out with loops over taps (no NaN) -------------------------------------

def _mask_map(x, V, sigma):
    """x [B, H, W] (0 where invalid), V bool -> (S, valid): the 25-tap sum; valid iff all 25 clamped taps are."""
    if sigma is None:
        return x, V
    w = NR.blur_weights(sigma)
    S, ok = torch.zeros_like(x), torch.ones_like(V)
    for a in range(-2, 3):
        for b in range(-2, 3):
            S = S + w[a + 2] * w[b + 2] * NR.taps(x, a, b)
            ok = ok & NR.taps(V, a, b)
    return S, ok


def _mask_normals(x, V, sigma, intr):
    S, ok = _mask_map(x, V, sigma)
    M = torch.ones_like(ok)
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            M = M & NR.taps(ok, a, b)
    Gx, Gy = NR.sobel_vectors(torch.where(ok, S, torch.ones_like(S)), intr)
    raw = torch.cross(Gx, Gy, dim=1)
    return raw / raw.norm(dim=1, keepdim=True).clamp_min(NR.EPS), M


def mask_terms(depth, intr, *, gt_depth=None, gt_normals=None, alpha=None, smoothing=2.0, min_depth=0.0, max_depth=math.inf,
               alpha_floor=1e-3):
    E = depth if alpha is None else depth / torch.maximum(alpha, torch.tensor(alpha_floor, dtype=depth.dtype))
    V = torch.isfinite(E) & (E > 0)
    n, M = _mask_normals(torch.where(V, E, torch.zeros_like(E)), V, smoothing, intr)
    if gt_depth is not None:
        Vg = torch.isfinite(gt_depth) & (gt_depth > min_depth) & (gt_depth < max_depth)
        t, Mt = _mask_normals(torch.where(Vg, gt_depth, torch.zeros_like(gt_depth)), Vg, smoothing, intr)
    else:
        Mt = torch.isfinite(gt_normals).all(1)
        t = torch.where(Mt[:, None], gt_normals, torch.zeros_like(gt_normals))
    M = M & Mt
    term = torch.where(M, 0.5 * (1.0 - (n * t).sum(1)), torch.zeros_like(E))
    return term.flatten(1).sum(1), M.flatten(1).sum(1).double(), M


@pytest.mark.parametrize("smoothing", NC.SMOOTHINGS)
@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (5, 7), (13, 9), (21, 34), (4, 40)])
def test_nan_propagation_equals_the_mask_formulation(H, W, smoothing):
    for with_alpha in (False, True):
        for holes in (0.0, 0.25):
            depth, gt, alpha, intr = _inputs(2, H, W, seed=H * W + 3, holes=holes, with_alpha=with_alpha)
            tn = NR.depth_normals(NC.surface(H, W, 2, torch.Generator().manual_seed(1)), intr, smoothing=None)
            if holes:
                tn[:, 1] = torch.where(NC.blocky(H, W, 2, torch.Generator().manual_seed(2), 0.2), torch.full_like(tn[:, 1], float("inf")), tn[:, 1])
            for target in (dict(gt_depth=gt), dict(gt_normals=tn)):
                kw = dict(alpha=alpha, smoothing=smoothing, min_depth=1.7, max_depth=2.9, **target)
                want_sum, want_cnt, M = mask_terms(depth, intr, **kw)
                term, sel = NR.pixel_terms(depth, intr, **kw)
                got_sum, got_cnt = NR.terms(depth, intr, **kw)
                assert torch.equal(sel, M) and torch.equal(got_cnt, want_cnt)
                assert float((got_sum - want_sum).abs().max()) <= 1e-12 * max(1.0, float(want_sum.abs().max()))
                if holes and H * W > 500 and smoothing is None:
                    assert 0 < float(want_cnt.min()) and float(want_cnt.max()) < H * W
            # the normal map's NaN pattern is the mask form's set, thresholds applied to the depth itself
            E = depth if alpha is None else depth / alpha.clamp_min(1e-3)
            V = torch.isfinite(E) & (E > 1.7) & (E < 2.9)
            n, M = _mask_normals(torch.where(V, E, torch.zeros_like(E)), V, smoothing, intr)
            got = NR.depth_normals(depth, intr, alpha, smoothing=smoothing, min_depth=1.7, max_depth=2.9)
            assert torch.equal(torch.isfinite(got).all(1), M) and torch.equal(torch.isfinite(got).any(1), M)
            if bool(M.any()):
                assert float((got - n)[M[:, None].expand_as(n)].abs().max()) <= 1e-12


# ---- the backward as the gather of csrc/normals_loss.hip, float64, no autograd ------------------------------------------------

def _fold(n, w=None):
    """[n, 5] (or [n, 3] for the Sobel pair): weight of output p + d on element p with the replicate clamp folded in."""
    p = torch.arange(n)
    if w is None:                                             # the Sobel's smoothing (1, 2, 1) and difference (-1, 0, 1) taps
        lo, hi = (p == 0).double(), (p == n - 1).double()
        one = torch.ones(n, dtype=torch.float64)
        return torch.stack([one, 2 + lo + hi, one], 1), torch.stack([one, hi - lo, -one], 1)
    out = torch.zeros(n, 5, dtype=torch.float64)
    for d in range(-2, 3):
        s = p + d
        inside = (s >= 0) & (s < n)
        for b in range(-2, 3):
            out[:, d + 2] += torch.where(inside & ((s + b).clamp(0, n - 1) == p), w[b + 2], torch.zeros((), dtype=torch.float64))
    return out


def gather_grad(depth, intr, alpha, cot, *, gt_depth=None, gt_normals=None, smoothing=2.0, min_depth=0.0, max_depth=math.inf,
                alpha_floor=1e-3, for_map=False):
    """cot: g_sum [B] (loss) or g [B, 3, H, W] (normal map).  The stages of the kernel: cotangents of the Sobel vectors per output,
    gathered onto S with folded 1-D weights and dotted with the pixel's own ray, gathered through the blur, then dE."""
    B, H, W = depth.shape
    E0 = NR.expected_depth(depth, alpha, alpha_floor)
    E = NR.with_nans(E0, max(min_depth, 0.0) if for_map else 0.0, max_depth if for_map else math.inf)
    S = NR.smooth(E, smoothing)
    n, M = NR.normals_of(S, intr)
    Gx, Gy = NR.sobel_vectors(torch.where(torch.isfinite(S), S, torch.ones_like(S)), intr)
    raw = torch.cross(Gx, Gy, dim=1)
    nr = raw.norm(dim=1, keepdim=True)
    if for_map:
        c = cot
    else:
        if gt_depth is not None:
            t, Mt = NR.normals_of(NR.smooth(NR.with_nans(gt_depth, min_depth, max_depth), smoothing), intr)
        else:
            Mt = torch.isfinite(gt_normals).all(1)
            t = torch.where(Mt[:, None], gt_normals, torch.zeros_like(gt_normals))
        M = M & Mt
        c = -0.5 * cot.view(B, 1, 1, 1) * t
    inv = 1.0 / nr.clamp_min(NR.EPS)
    dr = torch.where(nr >= NR.EPS, (c - n * (n * c).sum(1, keepdim=True)) * inv, c * inv)
    dr = torch.where(M[:, None], dr, torch.zeros_like(dr))
    dGx = F.pad(0.125 * torch.cross(Gy, dr, dim=1), (1, 1, 1, 1))
    dGy = F.pad(0.125 * torch.cross(dr, Gx, dim=1), (1, 1, 1, 1))
    (wsy, wdy), (wsx, wdx) = _fold(H), _fold(W)
    acc = torch.zeros(B, 3, H, W, dtype=torch.float64)
    for a in range(3):
        for b in range(3):
            acc = acc + (wsy[:, a, None] * wdx[None, :, b]) * dGx[:, :, a:a + H, b:b + W] \
                      + (wdy[:, a, None] * wsx[None, :, b]) * dGy[:, :, a:a + H, b:b + W]
    rx, ry = NR.rays(intr, H, W, torch.float64, "cpu")
    dS = rx * acc[:, 0] + ry * acc[:, 1] + acc[:, 2]
    if smoothing is None:
        dE = dS
    else:
        w = NR.blur_weights(smoothing)
        wy, wx = _fold(H, w), _fold(W, w)
        pad = F.pad(dS, (2, 2, 2, 2))
        dE = torch.zeros_like(dS)
        for a in range(5):
            for b in range(5):
                dE = dE + (wy[:, a, None] * wx[None, :, b]) * pad[:, a:a + H, b:b + W]
    dE = torch.where(torch.isfinite(E), dE, torch.zeros_like(dE))
    if alpha is None:
        return dE, None
    fl = torch.tensor(alpha_floor, dtype=torch.float64)
    gd = dE / torch.maximum(alpha, fl)
    return gd, torch.where(alpha > fl, -gd * torch.nan_to_num(E), torch.zeros_like(dE))


@pytest.mark.parametrize("smoothing", NC.SMOOTHINGS)
@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (5, 7), (13, 9), (21, 34), (3, 12)])
def test_the_backward_gather_equals_autograd(H, W, smoothing):
    for with_alpha in (False, True):
        depth, gt, alpha, intr = _inputs(2, H, W, seed=3 * H + W, holes=0.15, with_alpha=with_alpha)
        g = torch.Generator().manual_seed(H)
        g_sum = torch.randn(2, generator=g, dtype=torch.float64)
        tn = NR.depth_normals(NC.surface(H, W, 2, g), intr, smoothing=None)
        tn[0, 2, 0, 0] = float("nan")
        for target in (dict(gt_depth=gt), dict(gt_normals=tn)):
            kw = dict(smoothing=smoothing, min_depth=1.6, max_depth=3.0, **target)
            want = NR.grad(depth, intr, alpha, g_sum, **kw)
            got = gather_grad(depth, intr, alpha, g_sum, **kw)
            for x, y in zip(got, want):
                assert (x is None) == (y is None)
                if x is not None:
                    assert float((x - y).abs().max()) <= 1e-12 * max(1.0, float(y.abs().max()))
            E = NR.with_nans(NR.expected_depth(depth, alpha, 1e-3), 0.0, math.inf)
            assert not bool(got[0][~torch.isfinite(E)].any())                    # an invalid pixel receives exactly 0
        cot = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64)
        kw = dict(smoothing=smoothing, min_depth=1.6, max_depth=3.0)
        want = NR.normals_grad(depth, intr, alpha, cot, **kw)
        got = gather_grad(depth, intr, alpha, cot, for_map=True, **kw)
        for x, y in zip(got, want):
            if x is not None:
                assert float((x - y).abs().max()) <= 1e-12 * max(1.0, float(y.abs().max()))
        if H * W > 100:
            assert bool(got[0].any())


# ---- the C boundary --------------------------------------------------------------------------------------------------------

def test_normals_header_is_exported_and_bound():
    from freesplat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    names = declared_names("freesplat_amd_normals.h")
    assert names == EXPECTED
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/freesplat_amd_normals.h but not exported"
        assert n in _lib.NORMALS_SIGNATURES, f"{n} has no ctypes signature in freesplat_amd/_lib.py"
    assert set(_lib.NORMALS_SIGNATURES) == set(names)
    assert _lib.lib().fs_normals_api_version() == 1 == _lib.NORMALS_API_VERSION
    text = open(os.path.join(ROOT, "include", "freesplat_amd_normals.h")).read()
    assert re.search(r"#define\s+FS_NORMALS_API_VERSION\s+1\b", text)


P = C.c_void_p(4096)      # a fake non-NULL pointer: nothing may launch with it
OK_SCALARS = (2.0, 0.0, math.inf, 1e-3)      # sigma, min_depth, max_depth, alpha_floor


def _map_fwd(L, B=1, H=16, W=16, ptrs=None, scalars=OK_SCALARS):
    ptrs = [P] * 4 if ptrs is None else ptrs          # depth, alpha, intrinsics | normals
    return L.fs_depth_normals_forward(B, H, W, *ptrs[:3], *scalars, *ptrs[3:], None)


def _map_bwd(L, B=1, H=16, W=16, ptrs=None, scalars=OK_SCALARS):
    ptrs = [P] * 6 if ptrs is None else ptrs          # depth, alpha, intrinsics | g_normals, g_depth, g_alpha
    return L.fs_depth_normals_backward(B, H, W, *ptrs[:3], *scalars, *ptrs[3:], None)


def _loss_fwd(L, B=1, H=16, W=16, ptrs=None, scalars=OK_SCALARS):
    ptrs = [P, P, P, P, None, P, P, P] if ptrs is None else ptrs   # depth, alpha, intr, gt_depth, gt_normals | sum, cnt, scratch
    return L.fs_normals_loss_forward(B, H, W, *ptrs[:5], *scalars, *ptrs[5:], None)


def _loss_bwd(L, B=1, H=16, W=16, ptrs=None, scalars=OK_SCALARS):
    ptrs = [P, P, P, P, None, P, P, P] if ptrs is None else ptrs   # depth, alpha, intr, gt_depth, gt_normals | g_sum, g_depth, g_alpha
    return L.fs_normals_loss_backward(B, H, W, *ptrs[:5], *scalars, *ptrs[5:], None)


def test_entry_points_validate_before_touching_a_device():
    """FS_ERR_INVALID_ARG (-1) from every int-returning entry point for NULL pointers with positive sizes, non-positive sizes, an
    H * W that overflows, bad scalars, both or neither target and alpha without g_alpha -- all but the first with fake non-NULL
    pointers, so nothing may launch.  sigma == 0 is not among them: it is the "no smoothing" encoding."""
    from freesplat_amd import _lib
    L = _lib.lib()
    checked = 0
    for name, (rt, at) in _lib.NORMALS_SIGNATURES.items():
        if rt is not C.c_int or not at:
            continue
        for size in (1, 16):
            args = [size if a is C.c_int32 else (1e-3 if a is C.c_float else None) for a in at]
            assert getattr(L, name)(*args) == -1, name
        checked += 1
    assert checked == 4
    nan, inf = float("nan"), float("inf")
    bad_scalars = [(-1.0, 0.0, inf, 1e-3), (nan, 0.0, inf, 1e-3), (inf, 0.0, inf, 1e-3), (2.0, nan, inf, 1e-3), (2.0, 0.0, nan, 1e-3),
                   (2.0, 0.0, inf, 0.0), (2.0, 0.0, inf, -1.0), (2.0, 0.0, inf, nan), (2.0, 0.0, inf, inf), (0.0, 0.0, inf, 0.0)]
    for call in (_map_fwd, _map_bwd, _loss_fwd, _loss_bwd):
        for bad in [dict(B=0), dict(B=-1), dict(H=0), dict(W=-3), dict(H=46341, W=46341), dict(B=2 ** 30, H=64, W=64)] + \
                   [dict(scalars=s) for s in bad_scalars]:
            assert call(L, **bad) == -1, (call.__name__, bad)
    for i in (0, 2, 3):                                # depth, intrinsics, normals (alpha is optional)
        assert _map_fwd(L, ptrs=[None if k == i else P for k in range(4)]) == -1, i
    for i in (0, 2, 3, 4):                             # depth, intrinsics, g_normals, g_depth
        assert _map_bwd(L, ptrs=[None if k == i else P for k in range(6)]) == -1, i
    assert _map_bwd(L, ptrs=[P, P, P, P, P, None]) == -1                      # alpha without g_alpha
    for call, required in ((_loss_fwd, (0, 2, 5, 6, 7)), (_loss_bwd, (0, 2, 5, 6))):
        base = [P, P, P, P, None, P, P, P]
        for i in required:
            assert call(L, ptrs=[None if k == i else v for k, v in enumerate(base)]) == -1, (call.__name__, i)
        assert call(L, ptrs=[P, P, P, P, P, P, P, P]) == -1                   # both targets
        assert call(L, ptrs=[P, P, P, None, None, P, P, P]) == -1             # neither
    assert _loss_bwd(L, ptrs=[P, P, P, None, P, P, P, None]) == -1            # alpha without g_alpha
    # the size query: one 16-byte row per workgroup, rounded up to 256; 0 for what the entry points refuse
    from freesplat_amd import normals_loss as N
    al = lambda x: (x + 255) // 256 * 256
    for B, H, W in ((1, 1, 1), (2, 13, 9), (4, 968, 1296), (3, N.TILE_H + 1, N.TILE_W + 1)):
        assert L.fs_normals_scratch_bytes(B, H, W) == al(16 * B * -(-H // N.TILE_H) * -(-W // N.TILE_W)) > 0
    for bad in ((0, 16, 16), (1, 0, 16), (1, 16, -1), (1, 46341, 46341), (2 ** 30, 64, 64)):
        assert L.fs_normals_scratch_bytes(*bad) == 0


def test_python_layer_refuses_what_it_cannot_run():
    """The error cases that need no device: CPU tensors, both targets or none, a target that requires grad, bad scalars, bad host
    intrinsics."""
    from freesplat_amd import normals_loss as N
    a = 1.0 + torch.rand(1, 16, 16)
    k = (12.0, 12.0, 7.5, 7.5)
    for fn in (N.normals_loss, N.normals_loss_terms):
        with pytest.raises(ValueError, match="HIP device"):
            fn(a, k, gt_depth=a)
        with pytest.raises(ValueError, match="exactly one"):
            fn(a, k)
        with pytest.raises(ValueError, match="exactly one"):
            fn(a, k, gt_depth=a, gt_normals=a[:, None].expand(1, 3, 16, 16))
        with pytest.raises(RuntimeError, match="no gradient"):
            fn(a, k, gt_depth=a.clone().requires_grad_(True))
        for s in (0.0, -1.0, float("nan"), float("inf"), True):
            with pytest.raises(ValueError, match="smoothing"):
                fn(a, k, gt_depth=a, smoothing=s)
        with pytest.raises(ValueError, match="alpha_floor"):
            fn(a, k, gt_depth=a, alpha_floor=0.0)
        with pytest.raises(ValueError, match="NaN"):
            fn(a, k, gt_depth=a, min_depth=float("nan"))
    with pytest.raises(ValueError, match="HIP device"):
        N.depth_normals(a, k)
    with pytest.raises(ValueError, match="smoothing"):
        N.depth_normals(a, k, smoothing=0.0)
    cpu = torch.device("cpu")
    for bad in ((12.0, 12.0, 7.5), (0.0, 12.0, 7.5, 7.5), (12.0, -1.0, 7.5, 7.5), (12.0, 12.0, float("nan"), 7.5),
                (float("inf"), 12.0, 7.5, 7.5), [[12.0, 12.0, 7.5, 7.5]] * 3, [[[12.0, 12.0, 7.5, 7.5]]]):
        with pytest.raises(ValueError, match="intrinsics"):
            N._intrinsics(bad, 2, cpu)
    got = N._intrinsics(k, 2, cpu)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 4) and got.is_contiguous()
    assert torch.equal(N._intrinsics(torch.tensor([k, k], dtype=torch.float64), 2, cpu), got)
    assert (N.TILE_W, N.TILE_H, N.HALO) == (32, 16, 6)


# ---- the GPU cases' inputs ---------------------------------------------------------------------------------------------------

def test_case_grid():
    assert len(NC.CASES) == len(set(NC.CASES)) == 6 * 2 * 2 * (4 + 3) and len(NC.MAP_CASES) == 6 * 2 * (3 + 2)
    from freesplat_amd.normals_loss import HALO, TILE_H, TILE_W
    assert sum(1 for H, W in NC.SHAPES if H <= 2 * HALO + 1 and W <= 2 * HALO + 1) == 4
    (h0, w0), (h1, w1) = NC.STRADDLING
    assert (h0, w0) == (TILE_H + 1, TILE_W + 1) and (h1, w1) == (2 * TILE_H - 1, 2 * TILE_W + 1)


@pytest.mark.parametrize("H,W", NC.SHAPES)
def test_every_gpu_case_is_decidable(H, W):
    """The generator over every GPU case of one shape: the conditions the GPU comparisons rely on hold in float64, the masks do
    what their names say, and the eager fp32 restatement itself stays near float64 (the inputs are well conditioned)."""
    for case in [c for c in NC.CASES if c[:2] == (H, W)]:
        _, _, smoothing, with_alpha, target, mask = case
        c = NC.case(*case)
        NC.assert_decidable(c, smoothing, mask)
        assert (c["alpha"] is not None) == with_alpha and target in c and tuple(c["depth"].shape) == (NC.B, H, W)
        total, cnt = c["vals"]
        assert bool(torch.isfinite(total).all()) and all(bool(torch.isfinite(t).all()) for t in c["grads"]["terms"] if t is not None)
        if mask == "valid":
            assert float(cnt.min()) == H * W
        if mask == "view_invalid":
            assert float(cnt[-1]) == 0 and float(total[-1]) == 0 and not bool(c["grads"]["terms"][0][-1].any())
            assert not bool(c["grads"]["loss"][0][-1].any())
        if mask == "low_alpha":
            assert bool((c["alpha"] == 0).any()) and bool(((c["alpha"] > 0) & (c["alpha"] < NC.FLOOR)).any())
            assert bool(((c["alpha"] == 0) == (c["depth"] == 0)).all())
        if mask == "holes" and H * W > 500 and smoothing is None:
            assert 0 < float(cnt.min()) and float(cnt.max()) < H * W
        if H * W > 100 and mask != "holes":
            e32 = NR.values(c["depth"], c["intr"], c["alpha"], torch.float32, **c["kw"])[0].double()
            assert float((e32 - total).abs().max()) <= 1e-3 * float(total.abs().max())
    for case in [c for c in NC.MAP_CASES if c[:2] == (H, W)]:
        c = NC.map_case(*case)
        NC.assert_decidable(c, case[2], case[4], for_map=True)
        ok = torch.isfinite(c["normals"])
        assert torch.equal(ok.all(1), ok.any(1))
        if case[4] == "valid":
            assert bool(ok.all())
        E = NR.with_nans(NR.expected_depth(c["depth"].double(), None if c["alpha"] is None else c["alpha"].double(), NC.FLOOR), 0.0, math.inf)
        assert not bool(c["grads"][0][~torch.isfinite(E)].any())
