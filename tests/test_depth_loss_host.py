"""CPU checks of the depth loss: the float64 restatement (tests/depth_loss_ref.py, NaN propagation) against the mask
formulation of the definitions and against known answers, the backward gather csrc/depth_loss.hip implements against autograd,
and the C boundary of include/freesplat_amd_depthloss.h (exports, binding table, revision, argument validation, size queries).
No GPU."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import depth_loss_ref as DR
from util_abi import declared_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = ["fs_depth_loss_backward", "fs_depth_loss_forward", "fs_depth_loss_saved_bytes", "fs_depth_loss_scratch_bytes",
            "fs_depthloss_api_version"]
HOLES = (float("nan"), float("inf"), 0.0, -1.0)


def _inputs(B, H, W, seed, holes=0.3, with_alpha=True):
    g = torch.Generator().manual_seed(seed)
    gt = 0.5 + 4.0 * torch.rand(B, H, W, generator=g, dtype=torch.float64)
    depth = gt * torch.exp(0.2 * torch.randn(B, H, W, generator=g, dtype=torch.float64))
    alpha = None
    if with_alpha:
        alpha = 0.3 + 0.7 * torch.rand(B, H, W, generator=g, dtype=torch.float64)
        low = torch.rand(B, H, W, generator=g) < 0.1
        alpha = torch.where(low, torch.full_like(alpha, 2e-4), alpha)
        depth = depth * alpha.clamp_min(1e-3)
        zero = torch.rand(B, H, W, generator=g) < 0.05
        alpha, depth = torch.where(zero, torch.zeros_like(alpha), alpha), torch.where(zero, torch.zeros_like(depth), depth)
    if holes:
        kind = torch.randint(0, len(HOLES), (B, H, W), generator=g)
        hole = torch.rand(B, H, W, generator=g) < holes
        gt = torch.where(hole, torch.tensor(HOLES, dtype=torch.float64)[kind], gt)
    return depth, gt, alpha


# ---- the mask formulation of the definitions, written out with loops over taps (no conv2d, no NaN) -------------------------

def _level_sizes(H, W, S):
    out = [(H, W)]
    for _ in range(S - 1):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def _blur_pool(x, valid):
    """x [B, H, W] float64 (0 where invalid), valid bool -> the next level: zero padding, stride 2; valid iff every in-range
    tap is valid."""
    B, H, W = x.shape
    Hn, Wn = (H + 1) // 2, (W + 1) // 2
    out, ok = torch.zeros(B, Hn, Wn, dtype=x.dtype), torch.ones(B, Hn, Wn, dtype=torch.bool)
    k = (1.0, 2.0, 1.0)
    iy, ix = 2 * torch.arange(Hn), 2 * torch.arange(Wn)
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            yy, xx = iy + a, ix + b
            my, mx = (yy >= 0) & (yy < H), (xx >= 0) & (xx < W)
            tap = x[:, yy.clamp(0, H - 1)][:, :, xx.clamp(0, W - 1)]
            tv = valid[:, yy.clamp(0, H - 1)][:, :, xx.clamp(0, W - 1)]
            inside = (my[:, None] & mx[None, :])[None]
            out = out + torch.where(inside, k[a + 1] * k[b + 1] / 16.0 * tap, torch.zeros_like(tap))
            ok = ok & (tv | ~inside)
    return out, ok


SX = ((-1.0, 0.0, 1.0), (-2.0, 0.0, 2.0), (-1.0, 0.0, 1.0))


def _sobel(x, valid):
    """-> (g_x, g_y, M): replicate clamping, M iff all nine clamped taps are valid."""
    B, H, W = x.shape
    gx, gy, M = torch.zeros_like(x), torch.zeros_like(x), torch.ones(B, H, W, dtype=torch.bool)
    iy, ix = torch.arange(H), torch.arange(W)
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            yy, xx = (iy + a).clamp(0, H - 1), (ix + b).clamp(0, W - 1)
            tap = x[:, yy][:, :, xx]
            gx = gx + SX[a + 1][b + 1] / 8.0 * tap
            gy = gy + SX[b + 1][a + 1] / 8.0 * tap
            M = M & valid[:, yy][:, :, xx]
    return gx, gy, M


def mask_terms(depth, gt, alpha=None, *, mode="log_l1", num_scales=4, min_depth=0.0, max_depth=math.inf, alpha_floor=1e-3):
    """The definitions as masks: the four term tensors and, per level, the selected set M_s."""
    E = depth if alpha is None else depth / torch.maximum(alpha, torch.tensor(alpha_floor, dtype=depth.dtype))
    V = torch.isfinite(gt) & (gt > min_depth) & (gt < max_depth)
    g = torch.where(V, gt, torch.zeros_like(gt))
    if mode == "log_l1":
        P = V & (E > 0)
        err = (torch.log(torch.where(P, E, torch.ones_like(E))) - torch.log(torch.where(P, g, torch.ones_like(g)))).abs()
    else:
        P = V
        err = (E - g).abs()
    point_sum, point_cnt = torch.where(P, err, torch.zeros_like(err)).flatten(1).sum(1), P.flatten(1).sum(1).double()
    xe, xg, v = E, g, V
    sums, cnts, sets = [], [], []
    for s in range(num_scales):
        if s:
            (xe, _), (xg, v) = _blur_pool(xe, v), _blur_pool(xg, v)
        ex, ey, _ = _sobel(xe, v)
        tx, ty, M = _sobel(xg, v)
        d = (ex - tx).abs() + (ey - ty).abs()
        sums.append(torch.where(M, d, torch.zeros_like(d)).flatten(1).sum(1))
        cnts.append(2.0 * M.flatten(1).sum(1).double())
        sets.append(M)
    return (point_sum, point_cnt, torch.stack(sums, 1), torch.stack(cnts, 1)), sets


# ---- the backward as the gather of csrc/depth_loss.hip, float64, no autograd --------------------------------------------------

def gather_grad(depth, gt, alpha, g_point, g_grad, *, mode="log_l1", num_scales=4, min_depth=0.0, max_depth=math.inf,
                alpha_floor=1e-3):
    """One residual pyramid (NaN = invalid); from the top level down every element collects the Sobel outputs of its 3 x 3
    neighbourhood with the 1-D weights (1, 2 + [p = 0] + [p = n - 1], 1) and (1, [p = n - 1] - [p = 0], -1) of the outputs
    p - 1, p, p + 1, and the elements q of the level above with 2 q + a = p."""
    B, H, W = depth.shape
    fl = torch.tensor(alpha_floor, dtype=depth.dtype)
    E = depth if alpha is None else depth / torch.maximum(alpha, fl)
    V = torch.isfinite(gt) & (gt > min_depth) & (gt < max_depth)
    g = torch.where(V, gt, torch.zeros_like(gt))
    nan = torch.full_like(E, float("nan"))
    levels = [torch.where(V, E - g, nan)]
    for _ in range(num_scales - 1):
        levels.append(DR.pyramid(levels[-1], 2)[1][:, 0])
    G_up = None
    for s in range(num_scales - 1, -1, -1):
        R = levels[s]
        Hs, Ws = R.shape[1:]
        G = torch.zeros_like(R)
        if g_grad is not None:
            sg = DR.spatial_gradient(R[:, None]) * 8.0
            ok = torch.isfinite(sg).all(1)
            cx = torch.where(ok, torch.sign(torch.nan_to_num(sg[:, 0])), torch.zeros_like(R))
            cy = torch.where(ok, torch.sign(torch.nan_to_num(sg[:, 1])), torch.zeros_like(R))
            cxp, cyp = torch.nn.functional.pad(cx, (1, 1, 1, 1)), torch.nn.functional.pad(cy, (1, 1, 1, 1))
            ys, xs = torch.arange(Hs), torch.arange(Ws)
            lo_y, hi_y = (ys == 0).double(), (ys == Hs - 1).double()
            lo_x, hi_x = (xs == 0).double(), (xs == Ws - 1).double()
            one_y, one_x = torch.ones(Hs, dtype=torch.float64), torch.ones(Ws, dtype=torch.float64)
            wsy, wdy = (one_y, 2 + lo_y + hi_y, one_y), (one_y, hi_y - lo_y, -one_y)
            wsx, wdx = (one_x, 2 + lo_x + hi_x, one_x), (one_x, hi_x - lo_x, -one_x)
            acc = torch.zeros_like(R)
            for a in range(3):
                for b in range(3):
                    acc = acc + (wsy[a][:, None] * wdx[b][None, :]) * cxp[:, a:a + Hs, b:b + Ws] \
                              + (wdy[a][:, None] * wsx[b][None, :]) * cyp[:, a:a + Hs, b:b + Ws]
            G = 0.125 * g_grad[:, s].view(B, 1, 1) * acc
            if G_up is not None:
                Hn, Wn = G_up.shape[1:]
                k = (1.0, 2.0, 1.0)
                for a in (-1, 0, 1):
                    for b in (-1, 0, 1):
                        ty, tx = ys - a, xs - b
                        my = (ty >= 0) & (ty % 2 == 0) & (ty // 2 < Hn)
                        mx = (tx >= 0) & (tx % 2 == 0) & (tx // 2 < Wn)
                        v = G_up[:, (ty // 2).clamp(0, Hn - 1)][:, :, (tx // 2).clamp(0, Wn - 1)]
                        G = G + torch.where((my[:, None] & mx[None, :])[None], k[a + 1] * k[b + 1] / 16.0 * v, torch.zeros_like(v))
        G_up = G
    dE = G_up
    if g_point is not None:
        gp = g_point.view(B, 1, 1)
        if mode == "log_l1":
            pos = E > 0
            safe_E, safe_g = torch.where(pos & V, E, torch.ones_like(E)), torch.where(pos & V, g, torch.ones_like(g))
            dE = dE + torch.where(pos, gp * torch.sign(torch.log(safe_E) - torch.log(safe_g)) / safe_E, torch.zeros_like(E))
        else:
            dE = dE + gp * torch.sign(E - g)
    dE = torch.where(V, dE, torch.zeros_like(dE))
    if alpha is None:
        return dE, None
    return dE / torch.maximum(alpha, fl), torch.where(alpha > fl, -dE * E / alpha.clamp_min(alpha_floor), torch.zeros_like(dE))


# ---- the restatement checks itself ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", DR.MODES)
@pytest.mark.parametrize("H,W,S", [(1, 1, 4), (2, 3, 4), (5, 7, 4), (37, 53, 4), (37, 53, 1), (33, 65, 6), (16, 24, 3)])
def test_nan_propagation_equals_the_mask_formulation(mode, H, W, S):
    for with_alpha in (False, True):
        for holes in (0.0, 0.3):
            depth, gt, alpha = _inputs(2, H, W, seed=H * W + S, holes=holes, with_alpha=with_alpha)
            kw = dict(mode=mode, num_scales=S, min_depth=0.6, max_depth=4.3)
            want, sets = mask_terms(depth, gt, alpha, **kw)
            got = DR.terms(depth, gt, alpha, **kw)
            assert [tuple(m.shape[1:]) for m in sets] == _level_sizes(H, W, S)
            # the same selected sets: NaN propagation through conv2d against the explicit masks
            g = DR.gt_with_nans(gt, 0.6, 4.3)
            for M, level in zip(sets, DR.pyramid(g, S)):
                sel = torch.isfinite(DR.spatial_gradient(level))
                assert torch.equal(sel[:, 0], M) and torch.equal(sel[:, 1], M)
            assert torch.equal(got[1], want[1]) and torch.equal(got[3], want[3])
            for a, b in ((got[0], want[0]), (got[2], want[2])):
                assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
            if holes and H * W > 100:
                assert 0 < float(want[3][:, 0].min()) and float(want[3][:, 0].max()) < 2 * H * W


def test_known_answers():
    g = torch.Generator().manual_seed(4)
    gt = 0.5 + 3.0 * torch.rand(2, 21, 30, generator=g, dtype=torch.float64)
    gt[0, 3:6, 4:9] = float("nan")
    gt[1, 10, :] = 0.0
    c = 0.37
    ps, pc, gs, gc = DR.terms(gt.nan_to_num(1.0) + c, gt, mode="l1", num_scales=4)
    assert float(gc[:, 0].min()) > 0 and abs(float(ps.sum() / pc.sum()) - c) <= 1e-13
    assert float(gs[:, 0].abs().max()) <= 1e-13                                 # a constant offset has no gradient at level 0
    assert abs(float(DR.depth_loss(gt.nan_to_num(1.0) + c, gt, mode="l1", num_scales=1)) - c) <= 1e-13
    ps, pc, _, _ = DR.terms(gt.nan_to_num(1.0) * math.exp(c), gt, mode="log_l1")
    assert abs(float(ps.sum() / pc.sum()) - c) <= 1e-13
    assert int(pc[0]) == 21 * 30 - 15 and int(pc[1]) == 21 * 30 - 30
    # E <= 0 leaves the point term in log mode, not in l1 mode, and never the pyramid
    d = gt.nan_to_num(1.0).clone()
    d[0, 0, 0] = -1.0
    assert int(DR.terms(d, gt, mode="log_l1")[1][0]) == int(pc[0]) - 1 and int(DR.terms(d, gt, mode="l1")[1][0]) == int(pc[0])
    # a view with no valid pixel contributes 0, not NaN; all views invalid: the loss is exactly 0
    bad = gt.clone()
    bad[1] = torch.tensor(HOLES, dtype=torch.float64)[torch.arange(21 * 30) % 4].view(21, 30)
    terms = DR.terms(gt.nan_to_num(1.0) + c, bad, mode="l1")
    assert float(terms[0][1]) == 0 and float(terms[1][1]) == 0 and not bool(terms[2][1].any()) and not bool(terms[3][1].any())
    assert all(bool(t.isfinite().all()) for t in terms)
    loss, g_depth, _ = DR.loss_grad(gt.nan_to_num(1.0) + c, bad, mode="l1")
    assert bool(loss.isfinite()) and not bool(g_depth[1].any()) and bool(g_depth[0].any())
    bad[0] = bad[1]
    loss, g_depth, _ = DR.loss_grad(gt.nan_to_num(1.0) + c, bad)
    assert float(loss) == 0.0 and not bool(g_depth.any())
    # thresholds
    ps, pc, _, _ = DR.terms(gt.nan_to_num(1.0), gt, mode="l1", min_depth=1.0, max_depth=3.0)
    assert torch.equal(pc, ((gt > 1.0) & (gt < 3.0)).flatten(1).sum(1).double())


@pytest.mark.parametrize("mode", DR.MODES)
@pytest.mark.parametrize("H,W,S", [(1, 1, 4), (2, 3, 4), (5, 7, 4), (37, 53, 4), (33, 65, 6), (12, 9, 1)])
def test_the_backward_gather_equals_autograd(mode, H, W, S):
    for with_alpha in (False, True):
        depth, gt, alpha = _inputs(2, H, W, seed=3 * H + W, holes=0.2, with_alpha=with_alpha)
        gt[1] = float("nan") if H * W > 30 else gt[1]
        g = torch.Generator().manual_seed(S)
        gp, gg = torch.randn(2, generator=g, dtype=torch.float64), torch.randn(2, S, generator=g, dtype=torch.float64)
        kw = dict(mode=mode, num_scales=S)
        for a, b in ((gp, gg), (gp, None), (None, gg)):
            want = DR.grad(depth, gt, alpha, a, b, **kw)
            got = gather_grad(depth, gt, alpha, a, b, **kw)
            for x, y in zip(got, want):
                assert (x is None) == (y is None)
                if x is not None:
                    assert float((x - y).abs().max()) <= 1e-12 * max(1.0, float(y.abs().max()))
        if H * W > 30:
            assert not bool(got[0][1].any())


# ---- the C boundary --------------------------------------------------------------------------------------------------------

def test_depthloss_header_is_exported_and_bound():
    from freesplat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    names = declared_names("freesplat_amd_depthloss.h")
    assert names == EXPECTED
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/freesplat_amd_depthloss.h but not exported"
        assert n in _lib.DEPTHLOSS_SIGNATURES, f"{n} has no ctypes signature in freesplat_amd/_lib.py"
    assert set(_lib.DEPTHLOSS_SIGNATURES) == set(names)
    assert _lib.lib().fs_depthloss_api_version() == 1 == _lib.DEPTHLOSS_API_VERSION
    text = open(os.path.join(ROOT, "include", "freesplat_amd_depthloss.h")).read()
    assert re.search(r"#define\s+FS_DEPTHLOSS_API_VERSION\s+1\b", text)
    assert re.search(r"#define\s+FS_DEPTH_LOSS_LOG_L1\s+%d\b" % _lib.DEPTH_LOSS_LOG_L1, text)
    assert re.search(r"#define\s+FS_DEPTH_LOSS_L1\s+%d\b" % _lib.DEPTH_LOSS_L1, text)
    assert re.search(r"#define\s+FS_DEPTH_LOSS_MAX_SCALES\s+%d\b" % _lib.DEPTH_LOSS_MAX_SCALES, text)


P = C.c_void_p(4096)      # a fake non-NULL pointer: nothing may launch with it


def _fwd(L, B=1, H=16, W=16, S=4, mode=1, ptrs=None, scalars=(0.0, math.inf, 1e-3)):
    ptrs = [P] * 9 if ptrs is None else ptrs          # depth, gt, alpha | point_sum, point_cnt, grad_sum, grad_cnt, saved, scratch
    return L.fs_depth_loss_forward(B, H, W, S, mode, *ptrs[:3], *scalars, *ptrs[3:], None)


def _bwd(L, B=1, H=16, W=16, S=4, mode=1, ptrs=None, scalars=(0.0, math.inf, 1e-3)):
    ptrs = [P] * 9 if ptrs is None else ptrs          # depth, gt, alpha | g_point, g_grad, saved, g_depth, g_alpha, scratch
    return L.fs_depth_loss_backward(B, H, W, S, mode, *ptrs[:3], *scalars, *ptrs[3:], None)


def test_entry_points_validate_before_touching_a_device():
    """FS_ERR_INVALID_ARG (-1) from every int-returning entry point for NULL pointers with positive sizes, non-positive sizes,
    an unknown mode, S = 0 or 7, bad scalars and a backward without any cotangent -- all but the first with fake non-NULL
    pointers, so nothing may launch."""
    from freesplat_amd import _lib
    L = _lib.lib()
    checked = 0
    for name, (rt, at) in _lib.DEPTHLOSS_SIGNATURES.items():
        if rt is not C.c_int or not at:
            continue
        for size in (1, 16):
            args = [size if a is C.c_int32 else (1e-3 if a is C.c_float else None) for a in at]
            args[3], args[4] = 4, 1                                  # a valid S and mode: the NULL pointers are what is refused
            assert getattr(L, name)(*args) == -1, name
        checked += 1
    assert checked == 2
    nan, inf = float("nan"), float("inf")
    for call in (_fwd, _bwd):
        for bad in (dict(B=0), dict(B=-1), dict(H=0), dict(W=-3), dict(S=0), dict(S=7), dict(S=-1), dict(mode=0), dict(mode=3),
                    dict(mode=-1), dict(H=46341, W=46341), dict(scalars=(nan, inf, 1e-3)), dict(scalars=(0.0, nan, 1e-3)),
                    dict(scalars=(0.0, inf, 0.0)), dict(scalars=(0.0, inf, -1.0)), dict(scalars=(0.0, inf, nan)),
                    dict(scalars=(0.0, inf, inf))):
            assert call(L, **bad) == -1, (call.__name__, bad)
    for i in (0, 1, 3, 4, 5, 6, 8):                    # depth, gt, the four outputs, scratch (alpha and saved are optional)
        assert _fwd(L, ptrs=[None if k == i else P for k in range(9)]) == -1, i
    for i in (0, 1, 6):                                # depth, gt, g_depth
        assert _bwd(L, ptrs=[None if k == i else P for k in range(9)]) == -1, i
    assert _bwd(L, ptrs=[P, P, P, None, None, P, P, P, P]) == -1          # no cotangent at all
    assert _bwd(L, ptrs=[P, P, P, P, P, None, P, P, P]) == -1             # a gradient-term cotangent without the saved pyramid
    assert _bwd(L, ptrs=[P, P, P, P, P, P, P, P, None]) == -1             # ... or without scratch
    assert _bwd(L, ptrs=[P, P, P, P, P, P, P, None, P]) == -1             # alpha without g_alpha


def test_size_queries_are_monotone_and_zero_free():
    from freesplat_amd import _lib
    from freesplat_amd import depth_loss as D
    L = _lib.lib()
    al = lambda x: (x + 255) // 256 * 256
    for H, W in ((968, 1296), (1, 1), (33, 65), (37, 53)):
        for S in range(1, 7):
            sizes = _level_sizes(H, W, S)
            pyr = sum(h * w for h, w in sizes[1:])
            tiles = sum(-(-h // (D.UPPER_TILE_H if s else D.TILE_H)) * -(-w // D.TILE_W) for s, (h, w) in enumerate(sizes))
            prev = (0, 0)
            for B in (1, 2, 5, 16, 64):
                saved, scratch = L.fs_depth_loss_saved_bytes(B, H, W, S), L.fs_depth_loss_scratch_bytes(B, H, W, S)
                assert saved == al(4 * max(B * pyr, 1)) > 0 and scratch == al(32 * B * tiles) + saved > 0
                assert saved >= prev[0] and scratch >= prev[1]
                prev = (saved, scratch)
                assert D.saved_bytes(B, H, W, S) == saved
            if S > 1:
                assert L.fs_depth_loss_saved_bytes(1, H, W, S) >= L.fs_depth_loss_saved_bytes(1, H, W, S - 1)
                assert L.fs_depth_loss_scratch_bytes(1, H, W, S) >= L.fs_depth_loss_scratch_bytes(1, H, W, S - 1)
    for bad in ((0, 16, 16, 4), (1, 0, 16, 4), (1, 16, -1, 4), (1, 16, 16, 0), (1, 16, 16, 7), (1, 46341, 46341, 4)):
        assert L.fs_depth_loss_saved_bytes(*bad) == 0 and L.fs_depth_loss_scratch_bytes(*bad) == 0
    # the module's tile constants are the kernel's: one more row or column is one more tile (8 tiles of 32 bytes = 256)
    base = L.fs_depth_loss_scratch_bytes(8, D.TILE_H, D.TILE_W, 1)
    assert base == 256 + 256
    assert L.fs_depth_loss_scratch_bytes(8, D.TILE_H + 1, D.TILE_W, 1) == 512 + 256
    assert L.fs_depth_loss_scratch_bytes(8, D.TILE_H, D.TILE_W + 1, 1) == 512 + 256


def test_python_layer_refuses_what_it_cannot_run():
    """The error cases that need no device: CPU tensors, an unknown mode, num_scales out of range, bad scalars."""
    from freesplat_amd import depth_loss as D
    a = 1.0 + torch.rand(1, 16, 16)
    for fn in (D.depth_loss, D.depth_loss_terms):
        with pytest.raises(ValueError, match="HIP device"):
            fn(a, a)
        with pytest.raises(ValueError, match="mode"):
            fn(a, a, mode="l2")
        for S in (0, 7, -1, 2.0, True):
            with pytest.raises(ValueError, match="num_scales"):
                fn(a, a, num_scales=S)
        with pytest.raises(ValueError, match="alpha_floor"):
            fn(a, a, alpha_floor=0.0)
        with pytest.raises(ValueError, match="NaN"):
            fn(a, a, min_depth=float("nan"))
    assert D.MODES == {"log_l1": 1, "l1": 2} and D.MAX_SCALES == 6
