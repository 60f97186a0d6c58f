"""GPU checks of the fused normals loss and of depth_normals (freesplat_amd/normals_loss.py on fs_normals_loss_* and
fs_depth_normals_*) against the float64 restatement (tests/normals_loss_ref.py): values, NaN patterns, gradients for random
cotangents and through the scalar loss (bounded by the eager fp32 run's own error, the rule of tests/test_depth_loss_hip.py),
exact zeros, determinism, what is held for the backward, graph capture, guard bands, the path through the rasterizer and the
error cases that need a device.

No pixel is left out of a comparison: the inputs come from tests/normals_loss_cases.py, which asserts in float64 that no
threshold decision can flip in fp32 (tests/test_normals_loss_host.py runs that over every case on the CPU)."""
import sys

import pytest
import torch

import normals_loss_cases as NC
import normals_loss_ref as NR
from normals_loss_cases import B, FLOOR, STRADDLING

gpu = pytest.mark.gpu
# a float64 reference value below this is a structural zero (1 x 1: every Sobel tap is the one clamped element): the kernels
# give an exact 0 there, and no relative error is formed
ZERO = 1e-12


def _err(got, want):
    want = want.double()
    return float((got.detach().double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300))


def _bound(eager_err):
    return max(4.0 * eager_err, 1e-6)


def _dev(c, dev, requires_grad=False):
    d = c["depth"].to(dev).requires_grad_(requires_grad)
    a = None if c["alpha"] is None else c["alpha"].to(dev).requires_grad_(requires_grad)
    kw = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in c["kw"].items()}
    return d, a, c["intr"].to(dev), kw


def _invalid_E(c):
    """Pixels whose expected depth is invalid: they must receive exactly 0."""
    d = c["depth"].double()
    E = NR.expected_depth(d, None if c["alpha"] is None else c["alpha"].double(), FLOOR)
    return ~(torch.isfinite(E) & (E > 0))


def _compare(name, got, eager, want, failures):
    assert got.shape == want.shape and bool(got.isfinite().all()), name
    if float(want.abs().max()) <= ZERO:
        assert float(got.abs().max()) == 0.0, name
        return
    e_k, e_e = _err(got, want), _err(eager, want)
    print(f"{name}: kernel err {e_k:.3e}, eager fp32 err {e_e:.3e}, bound {_bound(e_e):.3e}, err/bound {e_k / _bound(e_e):.3f}, "
          f"kernel/eager {e_k / max(e_e, 1e-30):.2f}")
    if e_k > _bound(e_e):
        failures.append((name, e_k, e_e))


@gpu
@pytest.mark.parametrize("H,W,smoothing,with_alpha,target,mask", NC.CASES)
def test_values_and_gradients_vs_float64(hip_device, H, W, smoothing, with_alpha, target, mask):
    """cnt exact; sum and the gradients to depth and alpha: error relative to the tensor's max-abs at most max(4 x the eager fp32
    run's error on the same device, 1e-6), for random per-view cotangents and through the scalar loss; exact zeros at pixels
    whose E is invalid and in a view without a valid pixel."""
    from freesplat_amd import normals_loss as N
    c = NC.case(H, W, smoothing, with_alpha, target, mask)
    NC.assert_decidable(c, smoothing, mask)
    depth, alpha, intr, kw = _dev(c, hip_device)
    total, cnt = N.normals_loss_terms(depth, intr, alpha=alpha, **kw)
    eager = NR.values(c["depth"], c["intr"], c["alpha"], torch.float32, hip_device, **c["kw"])
    assert tuple(total.shape) == (B,) == tuple(cnt.shape) and total.dtype == cnt.dtype == torch.float64
    assert total.grad_fn is None and cnt.grad_fn is None and total.device == depth.device
    assert torch.equal(cnt.cpu(), c["vals"][1])
    failures = []
    _compare("sum", total, eager[0], c["vals"][0], failures)
    if mask == "view_invalid":
        assert float(total[-1]) == 0.0 and float(cnt[-1]) == 0.0
    dead = _invalid_E(c)
    g_sum = c["g_sum"].to(hip_device)
    for which in ("terms", "loss"):
        depth, alpha, intr, kw = _dev(c, hip_device, True)
        leaves = [depth] if alpha is None else [depth, alpha]
        if which == "loss":
            loss = N.normals_loss(depth, intr, alpha=alpha, **kw)
            assert loss.dtype == torch.float32 and loss.dim() == 0
            assert abs(float(loss.detach()) - float(c["loss"])) <= 1e-5 * max(1.0, abs(float(c["loss"])))
            if loss.grad_fn is None:
                continue
            grads = torch.autograd.grad(loss, leaves)
            eager_g = NR.loss_grad(c["depth"], c["intr"], c["alpha"], torch.float32, hip_device, **c["kw"])[1:]
        else:
            total, cnt = N.normals_loss_terms(depth, intr, alpha=alpha, **kw)
            assert total.requires_grad and not cnt.requires_grad
            grads = torch.autograd.grad((total * g_sum).sum(), leaves)
            eager_g = NR.grad(c["depth"], c["intr"], c["alpha"], g_sum, torch.float32, hip_device, **c["kw"])
        for name, g_k, g_e, want in zip(("g_depth", "g_alpha"), grads, eager_g, c["grads"][which]):
            assert g_k.dtype == torch.float32
            assert not bool(g_k.cpu()[dead].any()), f"{which} {name}: a pixel whose E is invalid must get exactly zero"
            if mask == "view_invalid":
                assert not bool(g_k[-1].any()), f"{which} {name}: a view without a valid pixel must get exactly zero"
            _compare(f"{which} {name}", g_k, g_e, want, failures)
    assert not failures, failures


@gpu
@pytest.mark.parametrize("H,W,smoothing,with_alpha,mask", NC.MAP_CASES)
def test_depth_normals_vs_float64(hip_device, H, W, smoothing, with_alpha, mask):
    """The NaN pattern is exactly float64's; the valid normals and the gradients for a random [B, 3, H, W] cotangent obey the
    bound of the loss; the cotangent of an invalid pixel is ignored (here: NaN)."""
    from freesplat_amd import normals_loss as N
    c = NC.map_case(H, W, smoothing, with_alpha, mask)
    NC.assert_decidable(c, smoothing, mask, for_map=True)
    depth, alpha, intr, kw = _dev(c, hip_device, True)
    n = N.depth_normals(depth, intr, alpha, **kw)
    want = c["normals"]
    ok = torch.isfinite(want)
    assert tuple(n.shape) == (B, 3, H, W) and n.dtype == torch.float32 and n.requires_grad
    assert torch.equal(torch.isfinite(n).cpu(), ok) and torch.equal(torch.isnan(n).cpu(), ~ok)
    eager = NR.normals_values(c["depth"], c["intr"], c["alpha"], torch.float32, hip_device, **c["kw"])
    failures = []
    if bool(ok.any()):
        z = lambda t: torch.where(ok, t.detach().cpu().double(), torch.zeros_like(want))
        _compare("normals", z(n), z(eager), z(want), failures)
    g = torch.where(ok, c["g"], torch.full_like(c["g"], float("nan"))).to(hip_device)   # ignored where the output is invalid
    grads = torch.autograd.grad(n, [depth] if alpha is None else [depth, alpha], g)
    eager_g = NR.normals_grad(c["depth"], c["intr"], c["alpha"], c["g"], torch.float32, hip_device, **c["kw"])
    dead = _invalid_E(c)
    for name, g_k, g_e, g_w in zip(("g_depth", "g_alpha"), grads, eager_g, c["grads"]):
        assert not bool(g_k.cpu()[dead].any()), name
        _compare(name, g_k, g_e, g_w, failures)
    with torch.no_grad():
        again = N.depth_normals(depth, intr, alpha, **kw)
    assert again.grad_fn is None and torch.equal(again.nan_to_num(7.0), n.detach().nan_to_num(7.0))
    assert not failures, failures


@gpu
@pytest.mark.parametrize("smoothing", NC.SMOOTHINGS)
def test_precomputed_normals_give_the_gt_depth_loss(hip_device, smoothing):
    """depth_normals of the sensor depth (thresholds applied) as gt_normals is the gt_depth form: the same counts, the same sum to
    fp32 rounding of the stored target."""
    from freesplat_amd import normals_loss as N
    H, W = STRADDLING[1]
    c = NC.case(H, W, smoothing, True, "gt_depth", "holes")
    depth, alpha, intr, kw = _dev(c, hip_device)
    gt = kw.pop("gt_depth")
    gt = torch.where(gt < 0, torch.zeros_like(gt), gt)                          # (a negative sensor value: below min_depth either way)
    with torch.no_grad():
        tn = N.depth_normals(gt, intr, smoothing=smoothing, min_depth=kw["min_depth"], max_depth=kw["max_depth"])
    a = N.normals_loss_terms(depth, intr, alpha=alpha, gt_depth=gt, **kw)
    b = N.normals_loss_terms(depth, intr, alpha=alpha, gt_normals=tn, **kw)
    assert torch.equal(a[1], b[1]) and float(a[1].sum()) > 0
    assert float((a[0] - b[0]).abs().max()) <= 1e-6 * float(a[1].max())


@gpu
@pytest.mark.parametrize("smoothing", NC.SMOOTHINGS)
@pytest.mark.parametrize("target", NC.TARGETS)
def test_determinism_runs_streams_and_batches(hip_device, smoothing, target):
    """Two runs, a side stream and the batch split into single views: bit-equal sums, normals and gradients."""
    from freesplat_amd import normals_loss as N
    V, (H, W) = 3, STRADDLING[1]
    raw = NC.raw_inputs(H, W, True, target, "holes", 9, views=V)
    depth, alpha, intr, gt = (raw[k].to(hip_device) for k in ("depth", "alpha", "intr", target))
    kw = dict(smoothing=smoothing, alpha_floor=FLOOR, **NC.thresholds("holes"))
    g_sum = torch.randn(V, generator=torch.Generator().manual_seed(2)).to(hip_device)
    g_map = torch.randn(V, 3, H, W, generator=torch.Generator().manual_seed(3)).to(hip_device)

    def run(d, a, k, t, cs, cm):
        d, a = d.clone().requires_grad_(True), a.clone().requires_grad_(True)
        total, cnt = N.normals_loss_terms(d, k, alpha=a, **{target: t}, **kw)
        n = N.depth_normals(d, k, a, **kw)
        return (total.detach(), cnt, n.detach().nan_to_num(7.0)) + torch.autograd.grad((total * cs).sum(), [d, a]) + \
            torch.autograd.grad(n, [d, a], cm)

    first = run(depth, alpha, intr, gt, g_sum, g_map)
    assert float(first[1].min()) > 0 and all(bool(t.isfinite().all()) and bool(t.any()) for t in first)
    for x, y in zip(first, run(depth, alpha, intr, gt, g_sum, g_map)):
        assert torch.equal(x, y)
    side = torch.cuda.Stream(device=hip_device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = run(depth, alpha, intr, gt, g_sum, g_map)
    torch.cuda.current_stream().wait_stream(side)
    for x, y in zip(first, third):
        assert torch.equal(x, y)
    for k in range(V):
        s = slice(k, k + 1)
        alone = run(depth[s], alpha[s], intr[s], gt[s], g_sum[s], g_map[s])
        for x, y in zip(first, alone):
            assert torch.equal(x[s], y)


@gpu
def test_nothing_is_held_without_a_pending_backward(hip_device, monkeypatch):
    """Under no_grad, or when no input asks for a gradient, no buffer outlives the call; with a backward pending only references
    to the inputs do (the backward recomputes everything): the allocations the module makes are counted through torch.empty."""
    from freesplat_amd import normals_loss as N
    H, W = 256, 384
    raw = NC.raw_inputs(H, W, True, "gt_depth", "holes", 3)
    depth, alpha, intr, gt = (raw[k].to(hip_device) for k in ("depth", "alpha", "intr", "gt_depth"))
    made, real = [], torch.empty

    def counting(*a, **k):
        t = real(*a, **k)
        made.append(t.numel() * t.element_size())
        return t
    monkeypatch.setattr(N.torch, "empty", counting)
    one_map = 4 * B * H * W
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(hip_device)
    out = N.normals_loss(depth, intr, gt_depth=gt, alpha=alpha)                   # no input requires a gradient
    with torch.no_grad():
        out2 = N.normals_loss(depth.clone().requires_grad_(True), intr, gt_depth=gt, alpha=alpha)      # grad mode off
    torch.cuda.synchronize()
    assert out.grad_fn is None and out2.grad_fn is None and not out2.requires_grad
    assert len(made) == 6 and max(made) < one_map // 8                            # per call: the partial rows, sum, cnt
    assert torch.cuda.memory_allocated(hip_device) - before < one_map // 8
    d = depth.clone().requires_grad_(True)
    torch.cuda.synchronize()
    before, made[:] = torch.cuda.memory_allocated(hip_device), []
    out3 = N.normals_loss(d, intr, gt_depth=gt, alpha=alpha)
    torch.cuda.synchronize()
    assert out3.grad_fn is not None and len(made) == 3 and max(made) < one_map // 8
    assert torch.cuda.memory_allocated(hip_device) - before < one_map // 8       # a pending backward holds references only
    out3.backward()
    assert d.grad is not None and bool(d.grad.isfinite().all()) and bool(d.grad.any())
    assert made[3:] == [one_map // B * B] * 2                                     # the backward: g_depth and g_alpha, nothing else
    a = alpha.clone().requires_grad_(True)                                        # alpha alone asks for a backward too
    out4 = N.normals_loss(depth, intr, gt_depth=gt, alpha=a)
    assert out4.grad_fn is not None
    out4.backward()
    assert a.grad is not None and bool(a.grad.any())
    made[:] = []
    with torch.no_grad():
        n = N.depth_normals(depth, intr, alpha)
    assert made == [3 * one_map] and n.grad_fn is None


@gpu
def test_graph_capture(hip_device):
    """Forward and backward of both ops record into one graph (device intrinsics: no host copy) and replay to the same bits."""
    from freesplat_amd import normals_loss as N
    H, W = STRADDLING[0]
    raw = NC.raw_inputs(H, W, True, "gt_depth", "valid", 21)
    depth, alpha, intr, gt = (raw[k].to(hip_device) for k in ("depth", "alpha", "intr", "gt_depth"))
    depth.requires_grad_(True)
    alpha.requires_grad_(True)
    g_map = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(3)).to(hip_device)

    def step():
        loss = N.normals_loss(depth, intr, gt_depth=gt, alpha=alpha)
        n = N.depth_normals(depth, intr, alpha)
        return (loss, n) + torch.autograd.grad(loss, [depth, alpha]) + torch.autograd.grad(n, [depth, alpha], g_map)

    side = torch.cuda.Stream(device=hip_device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                         # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        outs = step()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        got = [t.detach().clone() for t in outs]
        for a, b in zip(got, step()):
            assert torch.equal(a, b.detach())
    assert all(bool(t.any()) and bool(t.isfinite().all()) for t in got)


@gpu
def test_error_cases(hip_device):
    from freesplat_amd import normals_loss as N
    a = 1.5 + torch.rand(2, 16, 20, device=hip_device)
    k = torch.tensor([16.0, 16.0, 9.5, 7.5], device=hip_device)
    n3 = torch.zeros(2, 3, 16, 20, device=hip_device)
    for fn in (N.normals_loss, N.normals_loss_terms):
        with pytest.raises(ValueError):
            fn(a.cpu(), k, gt_depth=a)
        with pytest.raises(ValueError):
            fn(a, k, gt_depth=a.cpu())
        with pytest.raises(ValueError):
            fn(a, k, gt_depth=a, alpha=a.cpu())
        with pytest.raises(ValueError):
            fn(a, k, gt_depth=a[:, :15])
        with pytest.raises(ValueError):
            fn(a, k, gt_depth=a, alpha=a[:, :, :19])
        with pytest.raises(ValueError):
            fn(a, k, gt_normals=a)
        with pytest.raises(ValueError):
            fn(a, k, gt_normals=n3[:, :2])
        with pytest.raises(ValueError):
            fn(a[0], k, gt_depth=a[0])
        with pytest.raises(ValueError):
            fn(a[:0], k, gt_depth=a[:0])
        with pytest.raises(ValueError):
            fn(a, k, gt_depth=a, gt_normals=n3)
        with pytest.raises(ValueError):
            fn(a, k)
        with pytest.raises(ValueError):
            fn(a, k.expand(3, 4), gt_depth=a)
        with pytest.raises(ValueError):
            fn(a, (16.0, 0.0, 9.5, 7.5), gt_depth=a)
        with pytest.raises(RuntimeError):
            fn(a, k, gt_depth=a.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        N.depth_normals(a, k, a[:, :3])
    # what the inputs go through: host intrinsics, other dtypes and non-contiguous views
    want = N.normals_loss(a, k, gt_depth=a * 0.9 + 0.1)
    assert float(want) > 0
    assert torch.equal(N.normals_loss(a, (16.0, 16.0, 9.5, 7.5), gt_depth=a * 0.9 + 0.1), want)
    assert torch.equal(N.normals_loss(a, k.expand(2, 4), gt_depth=a * 0.9 + 0.1), want)
    assert torch.equal(N.normals_loss(a.double(), k.double(), gt_depth=(a * 0.9 + 0.1).double()), want)
    at = a.transpose(1, 2).contiguous().transpose(1, 2)
    assert not at.is_contiguous() and torch.equal(N.normals_loss(at, k, gt_depth=a * 0.9 + 0.1), want)
    d = at.clone().requires_grad_(True)
    N.normals_loss(d, k, gt_depth=a * 0.9 + 0.1).backward()
    assert d.grad.shape == d.shape and bool(d.grad.isfinite().all()) and bool(d.grad.any())
    assert float(N.normals_loss(a, k, gt_depth=torch.full_like(a, float("nan")))) == 0.0       # no valid pixel anywhere: exactly 0
    # a fronto-parallel plane looks away from the camera
    n = N.depth_normals(torch.full_like(a, 2.0), k)
    assert float((n - torch.tensor([0.0, 0.0, 1.0], device=hip_device).view(1, 3, 1, 1)).abs().max()) <= 1e-6


# ---- through the rasterizer --------------------------------------------------------------------------------------------------

@gpu
def test_through_the_rasterizer(hip_device, monkeypatch):
    """A 64-Gaussian scene at 32 x 32 in the (scales, rotations) form: the gradients the fused loss sends to means3D and
    opacities through the rasterizer's depth and alpha outputs, against those of the float64 restatement's cotangents sent
    through the same backward, bounded by the eager fp32 restatement's error."""
    from freesplat_amd import normals_loss as N, rasterizer as R
    from test_raster_scale_rot_alpha import _render, _scale_rot_for
    from util_raster import small_scene, view_inputs
    monkeypatch.setattr(R, "DETERMINISTIC", True)
    H = W = 32
    scene, cams = small_scene(N=64, H=H, W=W, seed=11)
    vi = view_inputs(scene, cams, 0, H, W)
    sc, rq = _scale_rot_for(vi, 4)
    (_, _, depth, alpha), leaves = _render(vi, hip_device, requires_grad=True, scales=sc, rotations=rq)
    assert tuple(depth.shape) == (H, W) and tuple(alpha.shape) == (H, W)
    intr = torch.tensor([N.intrinsics_from_fov(float(vi["tanfovx"]), float(vi["tanfovy"]), H, W)])
    E = (depth / alpha.clamp_min(FLOOR)).detach().cpu()
    g = torch.Generator().manual_seed(1)
    gt = (E * torch.exp(0.05 * torch.randn(H, W, generator=g))).clamp_min(0.05)
    gt = torch.where(NC.blocky(H, W, 1, g, 0.1)[0], torch.full_like(gt, float("nan")), gt)
    wrt = [leaves["means3D"], leaves["opacities"]]
    kw = dict(smoothing=None, alpha_floor=FLOOR)

    def through(g_depth, g_alpha):
        return torch.autograd.grad([depth, alpha], wrt, [g_depth.to(hip_device).float(), g_alpha.to(hip_device).float()],
                                   retain_graph=True)

    loss = N.normals_loss(depth[None], intr, gt_depth=gt[None].to(hip_device), alpha=alpha[None], **kw)
    got = torch.autograd.grad(loss, wrt, retain_graph=True)
    d0, a0 = depth.detach()[None], alpha.detach()[None]
    l64, gd64, ga64 = NR.loss_grad(d0.cpu(), intr, a0.cpu(), gt_depth=gt[None], **kw)
    _, gd32, ga32 = NR.loss_grad(d0, intr, a0, torch.float32, hip_device, gt_depth=gt[None], **kw)
    want, eager = through(gd64[0], ga64[0]), through(gd32[0], ga32[0])
    assert float(l64) > 0 and abs(float(loss.detach()) - float(l64)) <= 1e-5 * max(1.0, float(l64))
    for name, g_k, g_e, g_w in zip(("means3D", "opacities"), got, eager, want):
        assert bool(g_k.isfinite().all()) and bool(g_k.any()), name
        e_k, e_e = _err(g_k, g_w.cpu()), _err(g_e, g_w.cpu())
        print(f"{name}: fused err {e_k:.3e}, eager fp32 err {e_e:.3e}, bound {_bound(e_e):.3e}")
        assert e_k <= _bound(e_e), name


# ---- guard bands (tests/guarded_alloc.py, the harness of tests/test_memory_guards.py) ----

GUARDED = {
    "fs_normals_loss_forward": "test_guard_bands_normals_loss",
    "fs_normals_loss_backward": "test_guard_bands_normals_loss",
    "fs_depth_normals_forward": "test_guard_bands_depth_normals",
    "fs_depth_normals_backward": "test_guard_bands_depth_normals",
}


def _finite_inputs(H, W, target, seed):
    """(the harness wants finite inputs and results; 0 and negative values are holes too)"""
    raw = NC.raw_inputs(H, W, True, target, "holes", seed)
    return {k: (v.nan_to_num(nan=0.0, posinf=-2.0, neginf=-2.0) if isinstance(v, torch.Tensor) else v) for k, v in raw.items()}


@gpu
@pytest.mark.parametrize("H,W", STRADDLING)
@pytest.mark.parametrize("smoothing", NC.SMOOTHINGS)
def test_guard_bands_normals_loss(hip_device, smoothing, H, W):
    """Forward and backward unguarded and under the fills ("ff", "zero", "garbage"): no guard byte changes, nothing non-finite,
    the same bits; both targets, with and without alpha."""
    from freesplat_amd import normals_loss as N
    from test_memory_guards import _four
    kw = dict(smoothing=smoothing, alpha_floor=FLOOR, **NC.thresholds("holes"))
    raw = _finite_inputs(H, W, "gt_depth", seed=H)

    def op(place):
        d, a = place(raw["depth"], True), place(raw["alpha"], True)
        loss = N.normals_loss(d, place(raw["intr"]), gt_depth=place(raw["gt_depth"]), alpha=a, **kw)
        return [loss], lambda: torch.autograd.grad([loss], [d, a])
    base = _four(op, hip_device, f"normals loss {smoothing} {H}x{W}")
    assert float(base[0][0]) > 0
    rawn = NC.raw_inputs(H, W, False, "gt_normals", "valid", seed=H + 1)

    def given_normals_without_alpha(place):          # alpha = g_alpha = NULL
        d = place(rawn["depth"], True)
        total, cnt = N.normals_loss_terms(d, place(rawn["intr"]), gt_normals=place(rawn["gt_normals"]), **kw)
        g = place(torch.tensor([0.5, -1.5], dtype=torch.float64))
        return [total, cnt], lambda: torch.autograd.grad([total], [d], [g])
    _four(given_normals_without_alpha, hip_device, f"normals loss terms {smoothing} {H}x{W}")


@gpu
@pytest.mark.parametrize("H,W", STRADDLING)
@pytest.mark.parametrize("smoothing", NC.SMOOTHINGS)
def test_guard_bands_depth_normals(hip_device, smoothing, H, W):
    from freesplat_amd import normals_loss as N
    from test_memory_guards import _four
    raw = NC.raw_inputs(H, W, True, "gt_depth", "valid", seed=H + 2)
    g = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(1))

    def op(place):
        d, a = place(raw["depth"], True), place(raw["alpha"], True)
        n = N.depth_normals(d, place(raw["intr"]), a, smoothing=smoothing, alpha_floor=FLOOR)
        return [n], lambda: torch.autograd.grad([n], [d, a], [place(g)])
    _four(op, hip_device, f"depth normals {smoothing} {H}x{W}")

    def without_alpha(place):
        d = place(raw["gt_depth"], True)
        n = N.depth_normals(d, place(raw["intr"]), smoothing=smoothing)
        return [n], lambda: torch.autograd.grad([n], [d], [place(g)])
    _four(without_alpha, hip_device, f"depth normals without alpha {smoothing} {H}x{W}")


def test_every_normals_entry_point_with_a_device_buffer_has_a_guarded_case():
    from freesplat_amd import _lib
    with_buffers = sorted(n for n, (_, args) in _lib.NORMALS_SIGNATURES.items() if any(a is _lib._VP for a in args))
    assert with_buffers == sorted(GUARDED) and len(with_buffers) == 4
    me = sys.modules[__name__]
    for n, t in GUARDED.items():
        fn = getattr(me, t, None)
        assert callable(fn), (n, t)
        assert "gpu" in [m.name for m in getattr(fn, "pytestmark", [])], f"{n}: {t} is not a GPU case"
