"""GPU checks of the LPIPS distance head (csrc/lpips.hip) and of freesplat_amd.lpips against the float64 restatement
(tests/lpips_ref.py).  No fixture comes from the reference: it imports LPIPS from a package outside its tree.

Tolerances: error relative to the checked tensor's max-abs.  The yardstick is the eager fp32 torch head (for the module
tests: eager fp32 torch VGG + head) on the same device and inputs against float64; the kernel may be at most 4x that error
(a different but fixed summation order over up to 512 channels, not a looser algorithm) and never has to beat 1e-6.  The
bound is computed here from the eager run, and every figure is printed before it is asserted."""
import pytest
import torch

import lpips_ref as R

pytestmark = pytest.mark.gpu


def _err(got, want):
    want = want.double()
    return float((got.double() - want).abs().max() / want.abs().max().clamp_min(1e-300))


def _bound(eager_err):
    return max(4.0 * eager_err, 1e-6)


def _maps(B, C, H, W, seed, dev, near=None):
    g = torch.Generator().manual_seed(seed)
    f0 = torch.relu(torch.randn(B, C, H, W, generator=g))
    if near is None:
        f1 = torch.relu(torch.randn(B, C, H, W, generator=g))
    else:
        f1 = f0 * (1 + near * torch.randn(B, C, H, W, generator=g))
    w = torch.rand(C, generator=g)
    for f in (f0, f1):      # nothing is masked out below: the inputs have no zero-norm pixel
        assert float(f.pow(2).sum(1).min()) > 0
    return f0.to(dev), f1.to(dev), w.to(dev)


def _layer_raw(f0, f1, w, dist=None, want_g1=True, g_dist=None):
    """the C entry points directly: -> dist, g_f0, g_f1"""
    from freesplat_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    B, C, H, W = f0.shape
    dist = torch.zeros(B, device=f0.device) if dist is None else dist
    saved = torch.empty(L.fs_lpips_saved_bytes(B, C, H, W) // 4, device=f0.device)
    scratch = torch.empty(L.fs_lpips_scratch_bytes(B, C, H, W), dtype=torch.uint8, device=f0.device)
    st = _lib.current_stream()
    _lib.check(L.fs_lpips_layer_forward(p(f0), p(f1), p(w), B, C, H, W, p(dist), p(saved), p(scratch), st), "forward")
    g_dist = torch.ones(B, device=f0.device) if g_dist is None else g_dist
    g0 = torch.full_like(f0, float("nan"))
    g1 = torch.full_like(f1, float("nan")) if want_g1 else None
    _lib.check(L.fs_lpips_layer_backward(p(g_dist), p(f0), p(f1), p(w), p(saved), B, C, H, W, p(g0), p(g1), st), "backward")
    return dist, g0, g1


def _autograd(f0, f1, w, g_dist, dtype):
    a, b = f0.to(dtype).requires_grad_(True), f1.to(dtype).requires_grad_(True)
    d = R.layer(a, b, w, dtype)
    ga, gb = torch.autograd.grad((d * g_dist.to(dtype)).sum(), [a, b])
    return d.detach(), ga, gb


CASES = [(1, 64, 37, 53), (3, 64, 3, 5), (3, 128, 37, 53), (1, 256, 16, 64), (3, 512, 3, 5), (1, 512, 37, 53), (3, 256, 60, 81)]


@pytest.mark.parametrize("B,C,H,W", CASES)
@pytest.mark.parametrize("near", [None, 1e-3], ids=["unrelated", "near_identical"])
def test_head_forward_and_backward_vs_float64(hip_device, B, C, H, W, near):
    f0, f1, w = _maps(B, C, H, W, seed=B * 1000 + C + H, dev=hip_device, near=near)
    g_dist = torch.rand(B, generator=torch.Generator().manual_seed(5)).to(hip_device) + 0.5
    want = _autograd(f0, f1, w, g_dist, torch.float64)
    eager = _autograd(f0, f1, w, g_dist, torch.float32)
    got = _layer_raw(f0, f1, w, g_dist=g_dist)
    _, only0, none1 = _layer_raw(f0, f1, w, want_g1=False, g_dist=g_dist)
    assert none1 is None and torch.equal(only0, got[1]), "g_f1 = NULL must not change g_f0"
    for name, g, e, t in zip(("dist", "g_f0", "g_f1"), got, eager, want):
        eg, ee = _err(g, t), _err(e, t)
        print(f"lpips head {name} B{B} C{C} {H}x{W} near={near}: kernel {eg:.3e}, eager fp32 {ee:.3e}, bound {_bound(ee):.3e}")
        assert torch.isfinite(g).all()
        assert eg <= _bound(ee), (name, eg, ee)
    assert bool((got[0] >= 0).all())


def test_identical_pair_is_exactly_zero(hip_device):
    f0, _, w = _maps(2, 128, 37, 53, seed=7, dev=hip_device)
    dist, g0, g1 = _layer_raw(f0, f0.clone(), w)
    assert torch.equal(dist, torch.zeros_like(dist))
    assert torch.equal(g0, torch.zeros_like(g0)) and torch.equal(g1, torch.zeros_like(g1))


def test_zero_norm_pixel_gradient_is_finite_and_closed_form(hip_device):
    f0, f1, w = _maps(2, 64, 9, 11, seed=11, dev=hip_device)
    f0[0, :, 4, 5] = 0          # |f0| = 0 at one pixel, |f1| = 0 at another, both at a third
    f1[1, :, 2, 3] = 0
    f0[1, :, 8, 10] = 0
    f1[1, :, 8, 10] = 0
    g_dist = torch.tensor([0.7, 1.3], device=hip_device)
    dist, g0, g1 = _layer_raw(f0, f1, w, g_dist=g_dist)
    w0, w1 = R.layer_grad_closed_form(f0, f1, w, g_dist)
    assert torch.isfinite(g0).all() and torch.isfinite(g1).all() and torch.isfinite(dist).all()
    assert _err(dist, R.layer(f0, f1, w)) <= 1e-6
    # at the zero-norm pixel: 2 w_c d_c / (|f| + eps) * g_dist / (H W), |f| = 0 -> a = 1 / eps, d = -v
    v = f1[0, :, 4, 5].double() / f1[0, :, 4, 5].double().norm()
    closed = 0.7 / 99 * 2 * w.double() * (0 - v) / R.EPS
    assert _err(g0[0, :, 4, 5], closed) <= 1e-6
    assert _err(g0, w0) <= 1e-6 and _err(g1, w1) <= 1e-6
    assert torch.equal(g0[1, :, 8, 10], torch.zeros(64, device=hip_device))
    # torch's autograd is NaN there: the rule is the library's own, stated in the header
    a = f0.clone().requires_grad_(True)
    (R.layer(a, f1, w, torch.float32) * g_dist).sum().backward()
    assert torch.isnan(a.grad[0, :, 4, 5]).all()


def test_five_calls_accumulate_into_one_dist(hip_device):
    shapes = [(64, 32, 48), (128, 16, 24), (256, 8, 12), (512, 4, 6), (512, 2, 3)]
    layers = [_maps(2, C, H, W, seed=20 + i, dev=hip_device) for i, (C, H, W) in enumerate(shapes)]
    total = torch.zeros(2, device=hip_device)
    singles = []
    for f0, f1, w in layers:
        _layer_raw(f0, f1, w, dist=total)
        singles.append(_layer_raw(f0, f1, w)[0])
    acc = torch.zeros(2, device=hip_device)
    for s in singles:
        acc = acc + s
    assert torch.equal(total, acc)
    want = R.head([a for a, _, _ in layers], [b for _, b, _ in layers], [w for _, _, w in layers])
    assert _err(total, want) <= 2e-6


def test_head_is_bit_reproducible_and_batch_independent(hip_device):
    f0, f1, w = _maps(3, 256, 37, 53, seed=31, dev=hip_device)
    a = _layer_raw(f0, f1, w)
    b = _layer_raw(f0, f1, w)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    alone = _layer_raw(f0[1:2].contiguous(), f1[1:2].contiguous(), w)
    assert torch.equal(alone[0], a[0][1:2]) and torch.equal(alone[1], a[1][1:2])


def test_autograd_head_and_prepare(hip_device):
    from freesplat_amd import _lib
    from freesplat_amd.lpips import lpips_head
    f0, f1, w = _maps(2, 64, 12, 20, seed=41, dev=hip_device)
    a, b = f0.clone().requires_grad_(True), f1.clone().requires_grad_(True)
    d = lpips_head([a], [b], [w])
    (d * torch.tensor([1.0, 2.0], device=hip_device)).sum().backward()
    raw = _layer_raw(f0, f1, w, g_dist=torch.tensor([1.0, 2.0], device=hip_device))
    assert torch.equal(d.detach(), raw[0]) and torch.equal(a.grad, raw[1]) and torch.equal(b.grad, raw[2])
    # the input side against its formula
    L, p = _lib.lib(), _lib.ptr
    x0, x1 = torch.rand(2, 3, 7, 9, device=hip_device), torch.rand(2, 3, 7, 9, device=hip_device)
    shift, scale = torch.tensor(R.SHIFT, device=hip_device), torch.tensor(R.SCALE, device=hip_device)
    for normalize in (0, 1):
        out = torch.empty(4, 3, 7, 9, device=hip_device)
        _lib.check(L.fs_lpips_prepare_forward(p(x0), p(x1), p(shift), p(scale), 2, 3, 7, 9, normalize, p(out),
                                              _lib.current_stream()), "prepare")
        x = torch.cat([x0, x1])
        want = ((2 * x - 1 if normalize else x) - shift.view(1, 3, 1, 1)) / scale.view(1, 3, 1, 1)
        assert _err(out, want) <= 2e-7
        g = torch.randn(4, 3, 7, 9, device=hip_device)
        g0, g1 = torch.empty_like(x0), torch.empty_like(x1)
        _lib.check(L.fs_lpips_prepare_backward(p(g), p(scale), 2, 3, 7, 9, normalize, p(g0), p(g1), _lib.current_stream()),
                   "prepare backward")
        wg = g / scale.view(1, 3, 1, 1) * (2 if normalize else 1)
        assert _err(torch.cat([g0, g1]), wg) <= 2e-7


@pytest.mark.parametrize("normalize", [False, True])
def test_whole_module_vs_float64(hip_device, normalize):
    from freesplat_amd.lpips import LPIPS, random_state
    state = random_state(seed=2)
    m = LPIPS(net="vgg", weights="random", seed=2).to(hip_device)
    g = torch.Generator().manual_seed(9)
    in0, in1 = torch.rand(2, 3, 64, 96, generator=g), torch.rand(2, 3, 64, 96, generator=g)
    if not normalize:
        in0, in1 = 2 * in0 - 1, 2 * in1 - 1
    # float64 on the CPU, from the same weights
    a = in0.clone().requires_grad_(True)
    want = R.module(a, in1, state, normalize)
    want.sum().backward()
    # the yardstick: eager fp32 torch on the device
    e = in0.to(hip_device).requires_grad_(True)
    eager = R.module(e, in1.to(hip_device), state, normalize, dtype=torch.float32)
    eager.sum().backward()
    x = in0.to(hip_device).requires_grad_(True)
    got = m(x, in1.to(hip_device), normalize=normalize)
    assert got.shape == (2, 1, 1, 1)
    got.sum().backward()
    for name, gt, eg, wt in (("value", got.detach().flatten().cpu(), eager.detach().cpu(), want.detach()),
                             ("d/d in0", x.grad.cpu(), e.grad.cpu(), a.grad)):
        k, ee = _err(gt, wt), _err(eg, wt)
        print(f"lpips module {name} normalize={normalize}: ours {k:.3e}, eager fp32 {ee:.3e}, bound {_bound(ee):.3e}")
        assert k <= _bound(ee), (name, k, ee)
    # both inputs carrying a gradient (the packed path) and none: the value within the same bound, a gradient for in1 too
    x2, y2 = in0.to(hip_device).requires_grad_(True), in1.to(hip_device).requires_grad_(True)
    both = m(x2, y2, normalize=normalize)
    both.sum().backward()
    assert torch.isfinite(y2.grad).all() and bool(y2.grad.abs().max() > 0)
    assert _err(both.detach().flatten().cpu(), want.detach()) <= _bound(_err(eager.detach().cpu(), want.detach()))
    assert _err(x2.grad.cpu(), a.grad) <= _bound(_err(e.grad.cpu(), a.grad))
    with torch.no_grad():
        plain = m(in0.to(hip_device), in1.to(hip_device), normalize=normalize)
    assert _err(plain.flatten().cpu(), want.detach()) <= _bound(_err(eager.detach().cpu(), want.detach()))


def test_compute_lpips_and_lpips_loss(hip_device):
    from freesplat_amd import lpips as L
    L.set_default_weights("random")
    try:
        state = L.random_state(0)
        g = torch.Generator().manual_seed(3)
        gt, pred = torch.rand(2, 3, 64, 96, generator=g), torch.rand(2, 3, 64, 96, generator=g)
        val = L.compute_lpips(gt.to(hip_device), pred.to(hip_device).requires_grad_(True))
        assert val.shape == (2,) and not val.requires_grad
        want = R.module(gt, pred, state, normalize=True)
        eager = R.module(gt.to(hip_device), pred.to(hip_device), state, True, dtype=torch.float32)
        assert _err(val.cpu(), want) <= _bound(_err(eager.cpu(), want))
        p5 = pred.reshape(1, 2, 3, 64, 96).to(hip_device).requires_grad_(True)
        t5 = gt.reshape(1, 2, 3, 64, 96).to(hip_device)
        loss = L.lpips_loss(p5, t5, 0.05, apply_after_step=10, global_step=10)
        assert loss.shape == () and loss.requires_grad
        want_loss = 0.05 * R.module(pred, gt, state, normalize=False).mean()
        eager_loss = 0.05 * R.module(pred.to(hip_device), gt.to(hip_device), state, False, dtype=torch.float32).mean()
        assert _err(loss.detach().cpu(), want_loss) <= _bound(_err(eager_loss.cpu(), want_loss))
        loss.backward()
        assert p5.grad is not None and torch.isfinite(p5.grad).all() and bool(p5.grad.abs().max() > 0)
        zero = L.lpips_loss(p5, t5, 0.05, apply_after_step=10, global_step=9)
        assert float(zero) == 0.0 and zero.device == t5.device and zero.dtype == torch.float32
    finally:
        L.set_default_weights(None)


def test_head_hipgraph_capture_and_replay(hip_device):
    """Forward + backward of the head record into one hipGraph on a side stream (no allocation by the library, no host
    synchronisation), and replays give the eager bits."""
    from freesplat_amd.lpips import lpips_head
    dev = hip_device
    layers = [_maps(2, C, H, W, seed=50 + i, dev=dev) for i, (C, H, W) in enumerate([(64, 24, 40), (256, 6, 10), (512, 3, 5)])]
    f0s = [a.clone().requires_grad_(True) for a, _, _ in layers]
    f1s = [b for _, b, _ in layers]
    ws = [w for _, _, w in layers]
    gd = torch.tensor([0.5, 1.5], device=dev)

    def step():
        d = lpips_head(f0s, f1s, ws)
        return (d,) + torch.autograd.grad((d * gd).sum(), f0s)

    side = torch.cuda.Stream(device=dev)
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
        got = [t.clone() for t in outs]
        want = step()
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    assert all(bool(t.any()) for t in got)
