"""GPU checks of the fused depth loss (freesplat_amd/depth_loss.py on fs_depth_loss_forward / _backward) against the float64
restatement (tests/depth_loss_ref.py): values, gradients for random per-view, per-level cotangents (bounded by the eager fp32
run's own error, the rule of tests/test_ssim_loss_hip.py), determinism, what is held for the backward, guard bands, the path
through the rasterizer and the error cases.

No element is left out of a comparison.  Instead every case asserts on its own inputs, in float64 on the CPU, that no sign and
no threshold decision can flip in fp32 (`_assert_decidable`); the inputs are built so that this holds (`_settle`)."""
import functools
import math
import sys

import pytest
import torch
import torch.nn.functional as F

import depth_loss_ref as DR
from freesplat_amd.depth_loss import TILE_H, TILE_W          # the kernels' tile extents

gpu = pytest.mark.gpu
B = 2
STRADDLING = [(TILE_H + 1, TILE_W + 1), (2 * TILE_H - 1, TILE_W + 3)]
SHAPES = [(1, 1), (2, 3), (5, 7), (37, 53)] + STRADDLING      # 37 x 53 is odd at every level: 37 19 10 5, 53 27 14 7
MASKS = ["valid", "holes", "view_invalid", "low_alpha"]      # low_alpha: only with alpha
HOLES = (float("nan"), float("inf"), 0.0, -1.0)
FLOOR = 1e-3
# a float64 reference value below this is rounding residue of a structural zero (1 x 1: the Sobel taps are one clamped element,
# conv2d's float64 sum of w * x - w * x leaves 1e-16): the kernels give an exact 0 there, and no relative error is formed
ZERO = 1e-12
CASES = [(H, W, mode, S, with_alpha, mask) for H, W in SHAPES for mode in DR.MODES for S in (1, 4) for with_alpha in (False, True)
         for mask in MASKS if with_alpha or mask != "low_alpha"]


def _kw(mode, S, mask):
    kw = dict(mode=mode, num_scales=S, alpha_floor=FLOOR)
    if mask == "holes":
        kw.update(min_depth=0.6, max_depth=4.3)          # some finite, positive values are holes too
    return kw


def _raw_inputs(H, W, with_alpha, mask, seed, views=B):
    """float32 (depth, gt, alpha | None): gt in 0.5 .. 4.5, E = gt e^noise with a few negative values, alpha in 0.3 .. 1."""
    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.rand(views, H, W, generator=g, dtype=torch.float64)
    gt = 0.5 + 4.0 * r()
    for edge in (0.6, 4.3):
        gt = torch.where((gt - edge).abs() < 0.01, torch.full_like(gt, edge + 0.02), gt)
    E = gt * torch.exp(0.15 * torch.randn(views, H, W, generator=g, dtype=torch.float64))
    E = torch.where(r() < 0.02, -0.5 - r(), E)
    alpha = None
    if with_alpha:
        alpha = 0.3 + 0.7 * r()
        if mask == "low_alpha":
            alpha = torch.where(r() < 0.15, 2e-4 + 6e-4 * r(), alpha)             # below the floor: E = depth / floor
            zero = r() < 0.1                                                      # nothing rendered: depth = alpha = 0
            alpha, E = torch.where(zero, torch.zeros_like(alpha), alpha), torch.where(zero, torch.zeros_like(E), E)
        depth = E * alpha.clamp_min(FLOOR)
    else:
        depth = E
    holes = torch.tensor(HOLES, dtype=torch.float64)
    if mask == "holes":
        kind = torch.randint(0, len(HOLES), (views, H, W), generator=g)
        gt = torch.where(r() < 0.3, holes[kind], gt)
    if mask == "view_invalid":
        gt[-1] = holes[torch.arange(H * W) % len(HOLES)].view(H, W)
    f = lambda t: None if t is None else t.float()
    return f(depth), f(gt), f(alpha)


def _undecided(depth, gt, alpha, kw):
    """Level-0 pixels next to an abs() argument that is consumed and smaller than 1e-4 x the largest of its term (the point
    term, each pyramid level), float64 on the CPU.  Arguments that are zero by construction (differences of one clamped tap
    with itself, below 1e-12 of the inputs' magnitude in float64) are exact zeros in the kernel too and are not counted."""
    d, g, a = depth.double(), gt.double(), None if alpha is None else alpha.double()
    H, W = d.shape[1:]
    scale = float(d.abs().max()) / (FLOOR if a is not None else 1.0) + 10.0
    bad = torch.zeros(d.shape, dtype=torch.bool)
    for k, (arg, sel) in enumerate(DR.abs_arguments(d, g, a, **kw)):
        if not bool(sel.any()):
            continue
        mag = arg.abs()
        small = sel & (mag < 1e-4 * mag[sel].max()) & (mag > 1e-12 * scale)
        if k == 0:
            bad |= small
        elif bool(small.any()):
            near = F.max_pool2d(small.any(1, keepdim=True).float(), 3, 1, 1)[:, 0] > 0
            f = 2 ** (k - 1)
            bad |= near.repeat_interleave(f, 1).repeat_interleave(f, 2)[:, :H, :W]
    return bad


def _settle(depth, gt, alpha, kw, seed):
    """Nudges the depth of the pixels `_undecided` names until it names none."""
    g = torch.Generator().manual_seed(seed + 1000)
    for _ in range(200):
        bad = _undecided(depth, gt, alpha, kw)
        if not bool(bad.any()):
            return depth
        depth = torch.where(bad, depth * (1.0 + 0.1 * torch.randn(depth.shape, generator=g)).float(), depth)
    raise AssertionError("the inputs did not settle: choose another seed")


def _assert_decidable(depth, gt, alpha, kw):
    """What the comparisons below rely on, asserted on the inputs themselves."""
    assert not bool(_undecided(depth, gt, alpha, kw).any()), "an abs() argument is within 1e-4 of zero relative to its term"
    g = gt.double()
    fin = g[torch.isfinite(g)]
    for edge in (kw.get("min_depth", 0.0), kw.get("max_depth", math.inf)):
        if math.isfinite(edge):
            near = (fin - edge).abs() < 1e-3 * max(abs(edge), 1.0)
            assert not bool((near & (fin != edge)).any()) and not (edge != 0.0 and bool((fin == edge).any())), edge
    d = depth.double()
    if alpha is not None:
        a = alpha.double()
        assert not bool(((a - FLOOR).abs() < 1e-3 * FLOOR).any())
        d = d / a.clamp_min(FLOOR)
    assert not bool(((d != 0) & (d.abs() < 1e-3 * d.abs().max())).any())          # E is an exact 0 or well away from it


@functools.lru_cache(maxsize=None)
def _case(H, W, mode, S, with_alpha, mask):
    """Inputs, cotangents and every float64 reference of one case, computed once and shared (never modified)."""
    seed = 1000 * H + 10 * W + S + (5 if with_alpha else 0) + MASKS.index(mask) * 100000 + (mode == "l1") * 50000
    kw = _kw(mode, S, mask)
    depth, gt, alpha = _raw_inputs(H, W, with_alpha, mask, seed)
    depth = _settle(depth, gt, alpha, kw, seed)
    g = torch.Generator().manual_seed(seed + 1)
    gp, gg = torch.randn(B, generator=g), torch.randn(B, S, generator=g)
    vals = DR.values(depth, gt, alpha, **kw)
    grads = {"both": DR.grad(depth, gt, alpha, gp, gg, **kw), "point": DR.grad(depth, gt, alpha, gp, None, **kw),
             "grad": DR.grad(depth, gt, alpha, None, gg, **kw)}
    loss64, ld, la = DR.loss_grad(depth, gt, alpha, point_weight=0.7, grad_weight=1.3, **kw)
    grads["loss"] = (ld, la)
    return dict(depth=depth, gt=gt, alpha=alpha, kw=kw, gp=gp, gg=gg, vals=vals, grads=grads, loss=loss64)


def _err(got, want):
    want = want.double()
    return float((got.detach().double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300))


def _bound(eager_err):
    return max(4.0 * eager_err, 1e-6)


def _dev(c, dev, requires_grad=False):
    d = c["depth"].to(dev).requires_grad_(requires_grad)
    a = None if c["alpha"] is None else c["alpha"].to(dev).requires_grad_(requires_grad)
    return d, c["gt"].to(dev), a


@gpu
@pytest.mark.parametrize("H,W,mode,S,with_alpha,mask", CASES)
def test_values_and_gradients_vs_float64(hip_device, H, W, mode, S, with_alpha, mask):
    """Sums: error relative to the tensor's max-abs at most max(4 x the eager fp32 run's error on the same device, 1e-6);
    counts exact.  Gradients to depth and alpha: the same bound, for random per-view and per-level cotangents of both sums,
    each sum alone (the other cotangent NULL) and through the scalar loss."""
    from freesplat_amd import depth_loss as D
    c = _case(H, W, mode, S, with_alpha, mask)
    kw = c["kw"]
    _assert_decidable(c["depth"], c["gt"], c["alpha"], kw)
    depth, gt, alpha = _dev(c, hip_device)
    got = D.depth_loss_terms(depth, gt, alpha, **kw)
    eager = DR.values(c["depth"], c["gt"], c["alpha"], torch.float32, hip_device, **kw)
    assert [tuple(t.shape) for t in got] == [(B,), (B,), (B, S), (B, S)] and all(t.dtype == torch.float64 for t in got)
    assert all(t.grad_fn is None and t.device == depth.device for t in got)
    assert torch.equal(got[1].cpu(), c["vals"][1]) and torch.equal(got[3].cpu(), c["vals"][3])
    failures = []
    for name, k in (("point_sum", 0), ("grad_sum", 2)):
        want = c["vals"][k]
        assert bool(got[k].isfinite().all())
        if float(want.abs().max()) <= ZERO:
            assert float(got[k].abs().max()) <= ZERO, name
            continue
        e_k, e_e = _err(got[k], want), _err(eager[k], want)
        print(f"{name}: kernel err {e_k:.3e}, eager fp32 err {e_e:.3e}, bound {_bound(e_e):.3e}, ratio {e_k / max(e_e, 1e-30):.2f}")
        if e_k > _bound(e_e):
            failures.append((name, e_k, e_e))
    if mask == "view_invalid":
        assert not any(bool(t[-1].any()) for t in got)
    gp, gg = c["gp"].to(hip_device), c["gg"].to(hip_device)
    for which in ("both", "point", "grad", "loss"):
        depth, gt, alpha = _dev(c, hip_device, True)
        leaves = [depth] if alpha is None else [depth, alpha]
        if which == "loss":
            loss = D.depth_loss(depth, gt, alpha, point_weight=0.7, grad_weight=1.3, **kw)
            assert loss.dtype == torch.float32 and loss.dim() == 0
            assert abs(float(loss.detach()) - float(c["loss"])) <= 1e-5 * max(1.0, abs(float(c["loss"])))
            grads = torch.autograd.grad(loss, leaves)
            eager_g = DR.loss_grad(c["depth"], c["gt"], c["alpha"], torch.float32, hip_device, 0.7, 1.3, **kw)[1:]
        else:
            ps, _, gs, _ = D.depth_loss_terms(depth, gt, alpha, **kw)
            total = {"both": (ps * gp).sum() + (gs * gg).sum(), "point": (ps * gp).sum(), "grad": (gs * gg).sum()}[which]
            grads = torch.autograd.grad(total, leaves)
            eager_g = DR.grad(c["depth"], c["gt"], c["alpha"], gp if which != "grad" else None, gg if which != "point" else None,
                              torch.float32, hip_device, **kw)
        for name, g_k, g_e, want in zip(("g_depth", "g_alpha"), grads, eager_g, c["grads"][which]):
            assert g_k.shape == want.shape and g_k.dtype == torch.float32 and bool(g_k.isfinite().all())
            if mask == "view_invalid":
                assert not bool(g_k[-1].any()), f"{which} {name}: a view without a valid pixel must get exactly zero"
            if float(want.abs().max()) <= ZERO:
                assert float(g_k.abs().max()) <= ZERO, (which, name)
                continue
            e_k, e_e = _err(g_k, want), _err(g_e, want)
            print(f"{which} {name}: kernel err {e_k:.3e}, eager fp32 err {e_e:.3e}, bound {_bound(e_e):.3e}, "
                  f"ratio {e_k / max(e_e, 1e-30):.2f}")
            if e_k > _bound(e_e):
                failures.append((which, name, e_k, e_e))
    assert not failures, failures


@gpu
def test_all_six_scales(hip_device):
    """S = 6 on a shape whose top level is a single row: the same bound for the sums and the gradients."""
    from freesplat_amd import depth_loss as D
    H, W = 33, 70
    kw = dict(mode="log_l1", num_scales=6, alpha_floor=FLOOR)
    depth, gt, alpha = _raw_inputs(H, W, True, "valid", 77)
    depth = _settle(depth, gt, alpha, kw, 77)
    _assert_decidable(depth, gt, alpha, kw)
    gg = torch.randn(B, 6, generator=torch.Generator().manual_seed(5))
    want_v, want_g = DR.values(depth, gt, alpha, **kw), DR.grad(depth, gt, alpha, None, gg, **kw)
    eager_v = DR.values(depth, gt, alpha, torch.float32, hip_device, **kw)
    eager_g = DR.grad(depth, gt, alpha, None, gg, torch.float32, hip_device, **kw)
    d, a = depth.to(hip_device).requires_grad_(True), alpha.to(hip_device).requires_grad_(True)
    got = D.depth_loss_terms(d, gt.to(hip_device), a, **kw)
    assert torch.equal(got[3].cpu(), want_v[3]) and tuple(got[2].shape) == (B, 6)
    assert _err(got[2], want_v[2]) <= _bound(_err(eager_v[2], want_v[2]))
    for g_k, g_e, want in zip(torch.autograd.grad((got[2] * gg.to(hip_device)).sum(), [d, a]), eager_g, want_g):
        e_k, e_e = _err(g_k, want), _err(g_e, want)
        print(f"S = 6: kernel err {e_k:.3e}, eager fp32 err {e_e:.3e}")
        assert e_k <= _bound(e_e)


@gpu
@pytest.mark.parametrize("mode", DR.MODES)
def test_determinism_runs_streams_and_batches(hip_device, mode):
    from freesplat_amd import depth_loss as D
    V, H, W = 5, 70, 150
    depth, gt, alpha = (t.to(hip_device) for t in _raw_inputs(H, W, True, "holes", 9, views=V))
    kw = _kw(mode, 4, "holes")
    gp = torch.randn(V, generator=torch.Generator().manual_seed(2)).to(hip_device)
    gg = torch.randn(V, 4, generator=torch.Generator().manual_seed(3)).to(hip_device)

    def run(d, g, a, cp, cg):
        d, a = d.clone().requires_grad_(True), a.clone().requires_grad_(True)
        out = D.depth_loss_terms(d, g, a, **kw)
        return tuple(t.detach() for t in out) + torch.autograd.grad((out[0] * cp).sum() + (out[2] * cg).sum(), [d, a])

    first = run(depth, gt, alpha, gp, gg)
    for x, y in zip(first, run(depth, gt, alpha, gp, gg)):
        assert torch.equal(x, y)
    side = torch.cuda.Stream(device=hip_device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = run(depth, gt, alpha, gp, gg)
    torch.cuda.current_stream().wait_stream(side)
    for x, y in zip(first, third):
        assert torch.equal(x, y)
    for k in (0, 2, 4):
        alone = run(depth[k:k + 1], gt[k:k + 1], alpha[k:k + 1], gp[k:k + 1], gg[k:k + 1])
        for x, y in zip(first, alone):
            assert torch.equal(x[k:k + 1], y)


@gpu
def test_nothing_is_held_without_a_pending_backward(hip_device, monkeypatch):
    from freesplat_amd import _lib, depth_loss as D
    L = _lib.lib()
    real, calls = L.fs_depth_loss_saved_bytes, []
    monkeypatch.setattr(L, "fs_depth_loss_saved_bytes", lambda *a: calls.append(a) or real(*a))
    H, W = 256, 384
    depth, gt, alpha = (t.to(hip_device) for t in _raw_inputs(H, W, True, "holes", 3))
    held = D.saved_bytes(B, H, W, 4)
    assert held >= 4 * B * (H * W // 4)
    calls.clear()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(hip_device)
    out = D.depth_loss(depth, gt, alpha)                                          # no input requires a gradient
    with torch.no_grad():
        out2 = D.depth_loss(depth.clone().requires_grad_(True), gt, alpha)       # grad mode off
    torch.cuda.synchronize()
    assert not calls and out.grad_fn is None and out2.grad_fn is None and not out2.requires_grad
    assert torch.cuda.memory_allocated(hip_device) - before < held // 4
    d = depth.clone().requires_grad_(True)
    before = torch.cuda.memory_allocated(hip_device)
    out3 = D.depth_loss(d, gt, alpha)
    assert len(calls) == 1 and out3.grad_fn is not None
    assert torch.cuda.memory_allocated(hip_device) - before >= held             # the pyramid, until the backward has run
    out3.backward()
    assert d.grad is not None and bool(d.grad.isfinite().all())
    a = alpha.clone().requires_grad_(True)                                        # alpha alone asks for a backward too
    out4 = D.depth_loss(depth, gt, a)
    assert len(calls) == 2 and out4.grad_fn is not None
    out4.backward()
    assert a.grad is not None and bool(a.grad.any())


@gpu
def test_error_cases(hip_device):
    from freesplat_amd import depth_loss as D
    a = 1.0 + torch.rand(2, 16, 20, device=hip_device)
    for fn in (D.depth_loss, D.depth_loss_terms):
        with pytest.raises(ValueError):
            fn(a.cpu(), a)
        with pytest.raises(ValueError):
            fn(a, a.cpu())
        with pytest.raises(ValueError):
            fn(a, a, a.cpu())
        with pytest.raises(ValueError):
            fn(a, a[:, :15])
        with pytest.raises(ValueError):
            fn(a, a, a[:, :, :19])
        with pytest.raises(ValueError):
            fn(a[0], a[0])
        with pytest.raises(ValueError):
            fn(a[:, None], a[:, None])
        with pytest.raises(ValueError):
            fn(a[:0], a[:0])
        with pytest.raises(ValueError):
            fn(a, a, mode="other")
        for S in (0, 7):
            with pytest.raises(ValueError):
                fn(a, a, num_scales=S)
        with pytest.raises(RuntimeError):
            fn(a, a.clone().requires_grad_(True))
    # what the inputs go through: other dtypes and non-contiguous views
    want = D.depth_loss(a, a * 0.9)
    assert torch.equal(D.depth_loss(a.double(), (a * 0.9).double()), want)
    at = a.transpose(1, 2).contiguous().transpose(1, 2)
    assert not at.is_contiguous() and torch.equal(D.depth_loss(at, a * 0.9), want)
    d = at.clone().requires_grad_(True)
    D.depth_loss(d, a * 0.9).backward()
    assert d.grad.shape == d.shape and bool(d.grad.isfinite().all())
    assert float(D.depth_loss(a, torch.full_like(a, float("nan")))) == 0.0         # no valid pixel anywhere: exactly 0


# ---- through the rasterizer --------------------------------------------------------------------------------------------------

@gpu
def test_through_the_rasterizer(hip_device, monkeypatch):
    """A 64-Gaussian scene at 32 x 32 in the (scales, rotations) form: the gradients the fused loss sends to means3D and
    opacities through the rasterizer's depth and alpha outputs, against those of the float64 restatement's cotangents sent
    through the same backward, bounded by the eager fp32 restatement's error."""
    from freesplat_amd import depth_loss as D, rasterizer as R
    from test_raster_scale_rot_alpha import _render, _scale_rot_for
    from util_raster import small_scene, view_inputs
    monkeypatch.setattr(R, "DETERMINISTIC", True)
    H = W = 32
    scene, cams = small_scene(N=64, H=H, W=W, seed=11)
    vi = view_inputs(scene, cams, 0, H, W)
    sc, rq = _scale_rot_for(vi, 4)
    (_, _, depth, alpha), leaves = _render(vi, hip_device, requires_grad=True, scales=sc, rotations=rq)
    assert tuple(depth.shape) == (H, W) and tuple(alpha.shape) == (H, W)
    E = (depth / alpha.clamp_min(FLOOR)).detach().cpu()
    g = torch.Generator().manual_seed(1)
    gt = (E * torch.exp(0.1 * torch.randn(H, W, generator=g))).clamp_min(0.05)
    gt = torch.where(torch.rand(H, W, generator=g) < 0.1, torch.full_like(gt, float("nan")), gt)
    wrt = [leaves["means3D"], leaves["opacities"]]

    def through(g_depth, g_alpha):
        return torch.autograd.grad([depth, alpha], wrt, [g_depth.to(hip_device).float(), g_alpha.to(hip_device).float()],
                                   retain_graph=True)

    loss = D.depth_loss(depth[None], gt[None].to(hip_device), alpha[None])
    got = torch.autograd.grad(loss, wrt, retain_graph=True)
    d0, a0 = depth.detach()[None], alpha.detach()[None]
    l64, gd64, ga64 = DR.loss_grad(d0.cpu(), gt[None], a0.cpu())
    _, gd32, ga32 = DR.loss_grad(d0, gt[None], a0, torch.float32, hip_device)
    want, eager = through(gd64[0], ga64[0]), through(gd32[0], ga32[0])
    assert abs(float(loss.detach()) - float(l64)) <= 1e-5 * max(1.0, float(l64))
    for name, g_k, g_e, g_w in zip(("means3D", "opacities"), got, eager, want):
        assert bool(g_k.isfinite().all()) and bool(g_k.any()), name
        e_k, e_e = _err(g_k, g_w.cpu()), _err(g_e, g_w.cpu())
        print(f"{name}: fused err {e_k:.3e}, eager fp32 err {e_e:.3e}, bound {_bound(e_e):.3e}")
        assert e_k <= _bound(e_e), name


# ---- guard bands (tests/guarded_alloc.py, the harness of tests/test_memory_guards.py) ----

GUARDED = {
    "fs_depth_loss_forward": "test_guard_bands_depth_loss",
    "fs_depth_loss_backward": "test_guard_bands_depth_loss",
}


@gpu
@pytest.mark.parametrize("H,W", STRADDLING)
@pytest.mark.parametrize("mode", DR.MODES)
def test_guard_bands_depth_loss(hip_device, mode, H, W):
    """Forward and backward unguarded and under the fills ("ff", "zero", "garbage"): no guard byte changes, nothing
    non-finite, the same bits."""
    from freesplat_amd import depth_loss as D
    from test_memory_guards import _four
    depth, gt, alpha = _raw_inputs(H, W, True, "holes", seed=H)
    gt = gt.nan_to_num(nan=0.0, posinf=-2.0)          # (the harness wants finite inputs; 0 and negative values are holes too)
    kw = _kw(mode, 4, "holes")

    def op(place):
        d, a = place(depth, True), place(alpha, True)
        loss = D.depth_loss(d, place(gt), a, **kw)
        return [loss], lambda: torch.autograd.grad([loss], [d, a])
    _four(op, hip_device, f"depth loss {mode} {H}x{W}")

    def without_alpha_one_term(place):               # alpha = g_alpha = NULL, g_point = NULL
        d = place(depth, True)
        terms = D.depth_loss_terms(d, place(gt), None, **kw)
        g = place(torch.randn(B, 4, generator=torch.Generator().manual_seed(1)).double())
        return list(terms), lambda: torch.autograd.grad([terms[2]], [d], [g])
    _four(without_alpha_one_term, hip_device, f"depth loss terms {mode} {H}x{W}")

    def point_alone(place):                          # g_grad = NULL: the saved pyramid is not read
        d = place(depth, True)
        terms = D.depth_loss_terms(d, place(gt), None, **kw)
        g = place(torch.tensor([0.5, -1.5], dtype=torch.float64))
        return [terms[0]], lambda: torch.autograd.grad([terms[0]], [d], [g])
    _four(point_alone, hip_device, f"depth loss point term {mode} {H}x{W}")


def test_every_depth_loss_entry_point_with_a_device_buffer_has_a_guarded_case():
    from freesplat_amd import _lib
    with_buffers = sorted(n for n, (_, args) in _lib.DEPTHLOSS_SIGNATURES.items() if any(a is _lib._VP for a in args))
    assert with_buffers == sorted(GUARDED) and len(with_buffers) == 2
    me = sys.modules[__name__]
    for n, t in GUARDED.items():
        fn = getattr(me, t, None)
        assert callable(fn), (n, t)
        assert "gpu" in [m.name for m in getattr(fn, "pytestmark", [])], f"{n}: {t} is not a GPU case"
