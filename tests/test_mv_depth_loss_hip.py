"""GPU checks of the fused multi-view and scale-invariant depth losses (freesplat_amd/mv_depth_loss.py on fs_mv_depth_* and
fs_si_depth_*) against the float64 restatement (tests/mv_depth_ref.py): exact counts and selection patterns, values and
gradients for random cotangents and through the scalar losses (bounded by the eager fp32 run's own error, the rule of
tests/test_normals_loss_hip.py), exact zeros, the reduction apart from the geometry, determinism across runs, streams, batch
composition and alignment, what is held for the backward, graph capture, guard bands, the path through the rasterizer and the
error cases that need a device.

No pixel is left out of a comparison: the inputs come from tests/mv_depth_cases.py, which makes a hole of every pixel one of
whose decisions could flip in fp32 (tests/test_mv_depth_loss_host.py runs assert_decidable over every case on the CPU)."""
import sys

import pytest
import torch

import mv_depth_cases as MC
import mv_depth_ref as MR
from mv_depth_cases import B, FLOOR

gpu = pytest.mark.gpu
ZERO = 1e-12      # a float64 reference value below this is a structural zero: the kernels give an exact 0 there


def _err(got, want):
    want = want.double()
    return float((got.detach().double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300))


def _bound(eager_err):
    return max(4.0 * eager_err, 1e-6)


def _compare(name, got, eager, want, failures):
    assert got.shape == want.shape and bool(got.isfinite().all()), name
    if float(want.abs().max()) <= ZERO:
        assert float(got.abs().max()) == 0.0, name
        return
    e_k, e_e = _err(got, want), _err(eager, want)
    print(f"{name}: kernel err {e_k:.3e}, eager fp32 err {e_e:.3e}, bound {_bound(e_e):.3e}, err/bound {e_k / _bound(e_e):.3f}")
    if e_k > _bound(e_e):
        failures.append((name, e_k, e_e))


def _dev(c, dev, requires_grad=False):
    """(depth, gt, src, pairs, alpha) on the device and the keyword arguments."""
    d = c["depth"].to(dev).requires_grad_(requires_grad)
    a = None if c["alpha"] is None else c["alpha"].to(dev).requires_grad_(requires_grad)
    kw = dict(c["kw"], src_index=None if c["src_index"] is None else c["src_index"].to(dev))
    return (d, c["gt"].to(dev), c["src"].to(dev), c["pairs"].to(dev), a), kw


def _si_kw(c):
    return MR._si_kw(c)


def _dead(c):
    """Pixels whose expected depth is not finite: they must receive exactly 0."""
    return ~MR.expected_depth(c["depth"].double(), None if c["alpha"] is None else c["alpha"].double(), MR.f32(FLOOR))[1]


@gpu
@pytest.mark.parametrize("cs", MC.CASES)
def test_multi_view_values_and_gradients_vs_float64(hip_device, cs):
    """cnt and the selection pattern of the residual map exact; sum, the residual values and the gradients to depth and alpha:
    error relative to the tensor's max-abs at most max(4 x the eager fp32 run's error on the same device, 1e-6), for a random
    [B, K] cotangent and through the scalar loss; exact zeros at pixels whose E is not finite and in a view without a valid
    pixel; the kernel's sum against the float64 sum of its own residual map (the reduction apart from the geometry)."""
    from freesplat_amd import mv_depth_loss as M
    c = MC.case(*cs)
    K = cs[4]
    args, kw = _dev(c, hip_device)
    total, cnt = M.mv_depth_terms(*args, **kw)
    res = M.mv_depth_residuals(*args, **kw)
    w_total, w_cnt, w_res = c["vals"]
    e_total, _, e_res = MR.mv_values(c, torch.float32, hip_device)
    assert tuple(total.shape) == (B, K) == tuple(cnt.shape) and total.dtype == cnt.dtype == torch.float64
    assert total.grad_fn is None and cnt.grad_fn is None and res.grad_fn is None and res.dtype == torch.float32
    assert torch.equal(cnt.cpu(), w_cnt)
    assert tuple(res.shape) == (B, K) + tuple(c["depth"].shape[1:])
    assert torch.equal(torch.isnan(res).cpu(), torch.isnan(w_res)) and torch.equal(torch.isfinite(res).cpu(), ~torch.isnan(w_res))
    failures = []
    _compare("sum", total, e_total, w_total, failures)
    _compare("residuals", res.nan_to_num(0.0), e_res.nan_to_num(0.0), w_res.nan_to_num(0.0), failures)
    if c["invalid_view"]:
        assert not bool(total[-1].any()) and not bool(cnt[-1].any())
    dead = _dead(c)
    for which in ("terms", "loss"):
        args, kw = _dev(c, hip_device, True)
        leaves = [args[0]] if args[4] is None else [args[0], args[4]]
        if which == "loss":
            loss = M.mv_depth_loss(*args, **kw)
            assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.grad_fn is not None
            assert abs(float(loss.detach()) - float(c["loss"])) <= 1e-5 * max(1.0, abs(float(c["loss"])))
            grads = torch.autograd.grad(loss, leaves)
            eager_g = MR.mv_loss_grad(c, torch.float32, hip_device)[1:]
        else:
            total, cnt = M.mv_depth_terms(*args, **kw)
            assert total.requires_grad and not cnt.requires_grad
            grads = torch.autograd.grad((total * c["g_sum"].to(hip_device)).sum(), leaves)
            eager_g = MR.mv_grad(c, c["g_sum"], torch.float32, hip_device)
        for name, g_k, g_e, want in zip(("g_depth", "g_alpha"), grads, eager_g, c["grads"][which]):
            assert g_k.dtype == torch.float32
            assert not bool(g_k.cpu()[dead].any()), f"{which} {name}: a pixel whose E is not finite must get exactly zero"
            assert not bool(g_k.cpu()[torch.isnan(w_res).all(1)].any()), f"{which} {name}: a pixel no source selects must get exactly zero"
            if c["invalid_view"]:
                assert not bool(g_k[-1].any()), f"{which} {name}: a view without a valid pixel must get exactly zero"
            _compare(f"{which} {name}", g_k, g_e, want, failures)
    assert not failures, failures


@gpu
@pytest.mark.parametrize("cs", MC.CASES)
def test_the_sum_is_the_float64_sum_of_the_kernels_own_residuals(hip_device, cs):
    """The reduction apart from the geometry: the kernel's sum against the float64 sum of its own residual map's |r|, 1e-12
    relative (the kernel adds the fp32 values the map holds, in its own fixed order); its count against the map's pattern."""
    from freesplat_amd import mv_depth_loss as M
    c = MC.case(*cs)
    args, kw = _dev(c, hip_device)
    total, cnt = M.mv_depth_terms(*args, **kw)
    res = M.mv_depth_residuals(*args, **kw).double()
    assert torch.equal((~torch.isnan(res)).flatten(2).sum(2).double(), cnt)
    own = res.nan_to_num(0.0).abs().flatten(2).sum(2)
    assert float(own.max()) > 0 and float((total - own).abs().max()) <= 1e-12 * float(own.max())


@gpu
@pytest.mark.parametrize("cs", MC.CASES)
def test_scale_invariant_values_and_gradients_vs_float64(hip_device, cs):
    """n exact; s1, s2 and the gradients for random [B] cotangents and through the scalar loss under the same rule."""
    from freesplat_amd import mv_depth_loss as M
    c = MC.case(*cs)
    (d, gt, _, _, a), _ = _dev(c, hip_device)
    kw = _si_kw(c)
    s1, s2, n = M.si_depth_terms(d, gt, a, **kw)
    e1, e2, _ = MR.si_values(c, torch.float32, hip_device)
    assert tuple(s1.shape) == (B,) and s1.dtype == s2.dtype == n.dtype == torch.float64 and s1.grad_fn is None
    assert torch.equal(n.cpu(), c["si_vals"][2])
    failures = []
    _compare("s1", s1, e1, c["si_vals"][0], failures)
    _compare("s2", s2, e2, c["si_vals"][1], failures)
    if c["invalid_view"]:
        assert float(s1[-1]) == 0.0 and float(s2[-1]) == 0.0 and float(n[-1]) == 0.0
    dead = _dead(c)
    for which in ("terms", "loss"):
        (d, gt, _, _, a), _ = _dev(c, hip_device, True)
        leaves = [d] if a is None else [d, a]
        if which == "loss":
            loss = M.scale_invariant_loss(d, gt, a, **kw)
            assert loss.dtype == torch.float32 and loss.dim() == 0
            assert abs(float(loss.detach()) - float(c["si_loss"])) <= 1e-5 * max(1.0, float(c["si_loss"]))
            grads = torch.autograd.grad(loss, leaves)
            eager_g = MR.si_loss_grad(c, torch.float32, hip_device)[1:]
        else:
            s1, s2, n = M.si_depth_terms(d, gt, a, **kw)
            assert s1.requires_grad and s2.requires_grad and not n.requires_grad
            g1, g2 = (g.to(hip_device) for g in c["g_si"])
            grads = torch.autograd.grad((s1 * g1).sum() + (s2 * g2).sum(), leaves)
            eager_g = MR.si_grad(c, *c["g_si"], torch.float32, hip_device)
        for name, g_k, g_e, want in zip(("g_depth", "g_alpha"), grads, eager_g, c["si_grads"][which]):
            assert g_k.dtype == torch.float32 and not bool(g_k.cpu()[dead].any()), f"{which} {name}"
            if c["invalid_view"]:
                assert not bool(g_k[-1].any()), f"{which} {name}: a view without a valid pixel must get exactly zero"
            _compare(f"si {which} {name}", g_k, g_e, want, failures)
    assert not failures, failures


def _run_all(M, depth, gt, src, pairs, alpha, idx, g_sum, g1, g2, kw):
    """Everything the module computes, with gradients, as a tuple of tensors."""
    d, a = depth.clone().requires_grad_(True), alpha.clone().requires_grad_(True)
    total, cnt = M.mv_depth_terms(d, gt, src, pairs, a, src_index=idx, **kw)
    res = M.mv_depth_residuals(d, gt, src, pairs, a, src_index=idx, **kw)
    si_kw = {k: v for k, v in kw.items() if k != "occlusion"}
    s1, s2, n = M.si_depth_terms(d, gt, a, **si_kw)
    return (total.detach(), cnt, res.nan_to_num(7.0), s1.detach(), s2.detach(), n) + torch.autograd.grad((total * g_sum).sum(), [d, a]) + \
        torch.autograd.grad((s1 * g1).sum() + (s2 * g2).sum(), [d, a])


def _three_views(dev, pool):
    """A batch of three views of 33 x 130 (several workgroups per view), K = 3."""
    H, W, K, V = 33, 130, 3, 3
    if pool:
        raw = MC.build_case(H, W, H, W, 4, True, True, False, 1)
        pick = [0, 1, 0]                                 # view 2 repeats view 0's maps with other sources
        c = {k: (raw[k][pick] if k in ("depth", "gt", "alpha", "pairs") else raw[k]) for k in ("depth", "gt", "alpha", "pairs", "src")}
        c["src_index"] = torch.tensor(MC.POOL_INDEX + [[0, 3, 2, 1]], dtype=torch.int32)
        K = 4
    else:
        c = MC.build_case(H, W, H, W, K, True, False, False, 2, views=V)
    t = {k: (None if c[k] is None else c[k].to(dev)) for k in ("depth", "gt", "src", "pairs", "alpha", "src_index")}
    gen = torch.Generator().manual_seed(5)
    cot = [torch.randn(V, K, generator=gen).to(dev), torch.randn(V, generator=gen).to(dev), torch.randn(V, generator=gen).to(dev)]
    return t, cot, dict(MC.KW)


@gpu
@pytest.mark.parametrize("pool", [False, True])
def test_determinism_runs_streams_batches_and_alignment(hip_device, pool):
    """Two runs, a side stream, every view alone against the batch of three, and inputs at a storage offset of one float (the
    dword path) against aligned ones (the 16-byte path): bit-equal sums, counts, residuals and gradients."""
    from freesplat_amd import mv_depth_loss as M
    t, cot, kw = _three_views(hip_device, pool)
    run = lambda tt, cc: _run_all(M, tt["depth"], tt["gt"], tt["src"], tt["pairs"], tt["alpha"], tt["src_index"], *cc, kw)
    first = run(t, cot)
    assert float(first[1].sum(1).min()) > 0 and all(bool(x.isfinite().all()) and bool(x.any()) for x in first)
    for x, y in zip(first, run(t, cot)):
        assert torch.equal(x, y)
    side = torch.cuda.Stream(device=hip_device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = run(t, cot)
    torch.cuda.current_stream().wait_stream(side)
    for x, y in zip(first, third):
        assert torch.equal(x, y)
    for v in range(3):
        s = slice(v, v + 1)
        one = {k: (t[k][s] if k in ("depth", "gt", "pairs", "alpha") or (k == "src_index" and pool) or (k == "src" and not pool) else t[k])
               for k in t}
        alone = run(one, [g[s] for g in cot])
        for x, y in zip(first, alone):
            assert torch.equal(x[s], y)

    def shifted(x):                                      # the same values, one float past a 16-byte boundary
        if x is None or not x.is_floating_point():
            return x
        buf = torch.empty(x.numel() + 1, device=x.device)
        out = buf[1:].view(x.shape)
        out.copy_(x)
        assert out.is_contiguous() and out.data_ptr() % 16 == 4
        return out
    for x, y in zip(first, run({k: shifted(v) for k, v in t.items()}, cot)):
        assert torch.equal(x, y)


@gpu
def test_nothing_is_held_without_a_pending_backward(hip_device, monkeypatch):
    """Under no_grad, or when no input asks for a gradient, no buffer outlives the call; with a backward pending only references
    to the inputs do (the backward recomputes the gathers): the allocations the module makes are counted through torch.empty."""
    from freesplat_amd import mv_depth_loss as M
    H, W, K = 256, 384, 3
    c = MC.raw_case(H, W, H, W, K, True, False, False, 3)
    (depth, gt, src, pairs, alpha), kw = _dev(c, hip_device)
    made, real = [], torch.empty

    def counting(*a, **k):
        t = real(*a, **k)
        made.append(t.numel() * t.element_size())
        return t
    monkeypatch.setattr(M.torch, "empty", counting)
    one_map = 4 * B * H * W
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(hip_device)
    out = M.mv_depth_loss(depth, gt, src, pairs, alpha, **kw) + M.scale_invariant_loss(depth, gt, alpha)
    with torch.no_grad():
        out2 = M.mv_depth_loss(depth.clone().requires_grad_(True), gt, src, pairs, alpha, **kw)
    torch.cuda.synchronize()
    assert out.grad_fn is None and out2.grad_fn is None and not out2.requires_grad
    assert len(made) == 3 + 4 + 3 and max(made) < one_map // 8          # per call: the partial rows and the [B, K] / [B] results
    assert torch.cuda.memory_allocated(hip_device) - before < one_map // 8
    d = depth.clone().requires_grad_(True)
    torch.cuda.synchronize()
    before, made[:] = torch.cuda.memory_allocated(hip_device), []
    out3 = M.mv_depth_loss(d, gt, src, pairs, alpha, **kw) + M.scale_invariant_loss(d, gt, alpha)
    torch.cuda.synchronize()
    assert out3.grad_fn is not None and len(made) == 3 + 4 and max(made) < one_map // 8
    assert torch.cuda.memory_allocated(hip_device) - before < one_map // 8       # a pending backward holds references only
    out3.backward()
    assert d.grad is not None and bool(d.grad.isfinite().all()) and bool(d.grad.any())
    assert sorted(made[7:]) == [one_map] * 4                                      # the backwards: g_depth and g_alpha each, nothing else
    a = alpha.clone().requires_grad_(True)                                        # alpha alone asks for a backward too
    out4 = M.mv_depth_loss(depth, gt, src, pairs, a, **kw)
    assert out4.grad_fn is not None
    out4.backward()
    assert a.grad is not None and bool(a.grad.any())


@gpu
def test_graph_capture(hip_device):
    """Forward and backward of both losses record into one graph and replay to the same bits (the pool form: the indices stay
    on the device)."""
    from freesplat_amd import mv_depth_loss as M
    c = MC.case(*MC.CASES[12])
    (depth, gt, src, pairs, alpha), kw = _dev(c, hip_device, True)

    def step():
        loss = M.mv_depth_loss(depth, gt, src, pairs, alpha, **kw)
        si = M.scale_invariant_loss(depth, gt, alpha, **_si_kw(c))
        return (loss, si) + torch.autograd.grad(loss, [depth, alpha]) + torch.autograd.grad(si, [depth, alpha])

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
        for x, y in zip(got, step()):
            assert torch.equal(x, y.detach())
    assert all(bool(t.any()) and bool(t.isfinite().all()) for t in got)


@gpu
def test_error_cases(hip_device):
    from freesplat_amd import mv_depth_loss as M
    from freesplat_amd._lib import FreeSplatHipError
    d = 1.5 + torch.rand(2, 16, 20, device=hip_device)
    src = 1.5 + torch.rand(2, 3, 16, 20, device=hip_device)
    pairs = torch.eye(3, 4, device=hip_device).expand(2, 3, 3, 4).contiguous()
    for fn in (M.mv_depth_loss, M.mv_depth_terms, M.mv_depth_residuals):
        with pytest.raises((FreeSplatHipError, ValueError)):
            fn(d, d, src[:, :1].expand(2, 17, 16, 20), pairs[:, :1].expand(2, 17, 3, 4))            # K = 17
        with pytest.raises(RuntimeError):
            fn(d, d.clone().requires_grad_(True), src, pairs)
        with pytest.raises(RuntimeError):
            fn(d, d, src.clone().requires_grad_(True), pairs)
        for bad in (lambda: fn(d.cpu(), d, src, pairs), lambda: fn(d, d.cpu(), src, pairs), lambda: fn(d, d, src.cpu(), pairs),
                    lambda: fn(d, d, src, pairs.cpu()), lambda: fn(d, d, src, pairs, d.cpu()), lambda: fn(d, d[:, :15], src, pairs),
                    lambda: fn(d, d, src, pairs, d[:, :, :19]), lambda: fn(d[0], d[0], src, pairs), lambda: fn(d[:0], d[:0], src[:0], pairs[:0]),
                    lambda: fn(d, d, src[:, :2], pairs), lambda: fn(d, d, src, pairs[:, :, :2]), lambda: fn(d, d, src[0], pairs),
                    lambda: fn(d, d, src, pairs, src_index=torch.zeros(2, 3, dtype=torch.int32, device=hip_device)),
                    lambda: fn(d, d, src[0], pairs, src_index=torch.zeros(2, 2, dtype=torch.int32, device=hip_device)),
                    lambda: fn(d, d, src[0], pairs, src_index=torch.zeros(2, 3, dtype=torch.int32)),
                    lambda: fn(d, d, src[0], pairs, src_index=torch.zeros(2, 3, device=hip_device))):
            with pytest.raises(ValueError):
                bad()
    # what the inputs go through: other dtypes, non-contiguous views, int64 indices; the identity pair
    want = M.mv_depth_loss(d * 1.1, d, src, pairs)
    assert float(want) > 0
    assert torch.equal(M.mv_depth_loss((d * 1.1).double(), d.double(), src.double(), pairs.double()), want)
    dt = (d * 1.1).transpose(1, 2).contiguous().transpose(1, 2)
    assert not dt.is_contiguous() and torch.equal(M.mv_depth_loss(dt, d, src, pairs), want)
    idx = torch.tensor([[0, 1, 2], [3, 4, 5]], device=hip_device)
    assert torch.equal(M.mv_depth_loss(d * 1.1, d, src.view(6, 16, 20), pairs, src_index=idx), want)
    r = M.mv_depth_residuals(d * 1.1, d, src, pairs)
    sel = d[:, None] + 1e-8 < 1.05 * src
    assert torch.equal(~torch.isnan(r), sel) and bool(sel.any()) and not bool(sel.all())
    assert float((r - (torch.log(d * 1.1)[:, None] - torch.log(src)))[sel].abs().max()) <= 1e-6
    nothing = torch.full_like(d, float("nan"))
    assert float(M.mv_depth_loss(d, nothing, src, pairs)) == 0.0 and float(M.scale_invariant_loss(d, nothing)) == 0.0
    assert float(M.scale_invariant_loss(3.0 * d, d, si_lambda=1.0)) <= 1e-6       # a pure scale error costs nothing at lambda = 1
    assert abs(float(M.scale_invariant_loss(3.0 * d, d, si_lambda=0.0)) - 1.0986123) <= 1e-5


# ---- through the rasterizer --------------------------------------------------------------------------------------------------

@gpu
def test_through_the_rasterizer(hip_device):
    """Two views of a small synthetic scene (freesplat_amd.synthetic through util_raster.small_scene): the second view's render
    is the neighbour's sensor map, the first view's depth / alpha carry the loss back to the means; the gradient is finite and
    non-zero."""
    from freesplat_amd import mv_depth_loss as M
    from freesplat_amd.normals_loss import intrinsics_from_fov
    from test_raster_scale_rot_alpha import _render, _scale_rot_for
    from util_raster import small_scene, view_inputs
    H = W = 32
    scene, cams = small_scene(N=64, H=H, W=W, seed=11)
    views = [view_inputs(scene, cams, i, H, W) for i in range(2)]
    sc, rq = _scale_rot_for(views[0], 4)
    (_, _, depth, alpha), leaves = _render(views[0], hip_device, requires_grad=True, scales=sc, rotations=rq)
    with torch.no_grad():
        (_, _, depth1, alpha1), _ = _render(views[1], hip_device, scales=sc, rotations=rq)
    hole = torch.full_like(depth1, float("nan"))
    sensor_pool = torch.where(alpha1 > 0.5, depth1 / alpha1.clamp_min(FLOOR), hole)[None]
    gen = torch.Generator().manual_seed(1)
    noise = torch.exp(0.02 * torch.randn(H, W, generator=gen)).to(hip_device)
    gt = torch.where(alpha.detach() > 0.5, depth.detach() / alpha.detach().clamp_min(FLOOR) * noise, hole)
    intr = intrinsics_from_fov(views[0]["tanfovx"], views[0]["tanfovy"], H, W)
    world_to_cam = torch.stack([v["viewmatrix"].double().T for v in views])          # (the rasterizer stores the transpose)
    nbrs = torch.tensor([[0]], dtype=torch.int32, device=hip_device)
    pairs = M.pair_transforms(intr, torch.linalg.inv(world_to_cam[:1]).to(hip_device), intr, world_to_cam[1:].to(hip_device), nbrs)
    total, cnt = M.mv_depth_terms(depth[None], gt[None], sensor_pool, pairs, alpha[None], src_index=nbrs)
    print(f"{int(cnt)} of {int(torch.isfinite(gt).sum())} pixels with a sensor depth find their neighbour")
    assert float(cnt) > 0
    loss = M.mv_depth_loss(depth[None], gt[None], sensor_pool, pairs, alpha[None], src_index=nbrs)
    g_means, = torch.autograd.grad(loss, [leaves["means3D"]])
    assert float(loss.detach()) > 0 and bool(g_means.isfinite().all()) and bool(g_means.any())


# ---- guard bands (tests/guarded_alloc.py, the harness of tests/test_memory_guards.py) ----

GUARDED = {
    "fs_mv_depth_forward": "test_guard_bands_multi_view",
    "fs_mv_depth_backward": "test_guard_bands_multi_view",
    "fs_si_depth_forward": "test_guard_bands_scale_invariant",
    "fs_si_depth_backward": "test_guard_bands_scale_invariant",
}
GUARD_CASES = [MC.CASES[4], MC.CASES[7], MC.CASES[11], MC.CASES[12]]     # 37 x 53, 33 x 130, 5 x 130 onto 7 x 96, the pool form


def _finite(t):
    """(the harness wants finite inputs and results; 0 and negative values are holes too)"""
    return None if t is None else (t.nan_to_num(nan=0.0, posinf=-2.0, neginf=-2.0) if t.is_floating_point() else t)


@gpu
@pytest.mark.parametrize("cs", GUARD_CASES)
def test_guard_bands_multi_view(hip_device, cs):
    """Forward (sums, counts and the residual map) and backward unguarded and under the fills ("ff", "zero", "garbage"): no guard
    byte changes, every byte of every output is written (the same bits under every fill), scratch contents are not relied on."""
    from freesplat_amd import mv_depth_loss as M
    from test_memory_guards import _four
    c = MC.case(*cs)
    kw = dict(c["kw"])
    g = c["g_sum"]

    def op(place):
        d = place(_finite(c["depth"]), True)
        a = None if c["alpha"] is None else place(c["alpha"], True)
        gt, src, pairs = place(_finite(c["gt"])), place(_finite(c["src"])), place(c["pairs"])
        idx = None if c["src_index"] is None else place(c["src_index"])
        total, cnt = M.mv_depth_terms(d, gt, src, pairs, a, src_index=idx, **kw)
        res = M.mv_depth_residuals(d, gt, src, pairs, a, src_index=idx, **kw)
        return [total, cnt, res], lambda: torch.autograd.grad([total], [d] if a is None else [d, a], [place(g)])
    base = _four(op, hip_device, f"multi-view {cs}", finite=False)
    assert float(base[0][1].sum()) > 0 and all(bool(t.isfinite().all()) for t in base[0][:2] + base[1])
    assert bool(torch.isnan(base[0][2]).any()) and bool(torch.isfinite(base[0][2]).any())


@gpu
@pytest.mark.parametrize("cs", GUARD_CASES[:3])
def test_guard_bands_scale_invariant(hip_device, cs):
    from freesplat_amd import mv_depth_loss as M
    from test_memory_guards import _four
    c = MC.case(*cs)
    kw = _si_kw(c)

    def op(place):
        d = place(_finite(c["depth"]), True)
        a = None if c["alpha"] is None else place(c["alpha"], True)
        s1, s2, n = M.si_depth_terms(d, place(_finite(c["gt"])), a, **kw)
        loss = M.combine_si(s1, s2, n)
        return [s1, s2, n, loss], lambda: torch.autograd.grad([loss], [d] if a is None else [d, a])
    base = _four(op, hip_device, f"scale-invariant {cs}")
    assert float(base[0][3]) > 0 and bool(base[1][0].any())


def test_every_mvdepth_entry_point_with_a_device_buffer_has_a_guarded_case():
    from freesplat_amd import _lib
    with_buffers = sorted(n for n, (_, args) in _lib.MVDEPTH_SIGNATURES.items() if any(a is _lib._VP for a in args))
    assert with_buffers == sorted(GUARDED) and len(with_buffers) == 4
    me = sys.modules[__name__]
    for n, t in GUARDED.items():
        fn = getattr(me, t, None)
        assert callable(fn), (n, t)
        assert "gpu" in [m.name for m in getattr(fn, "pytestmark", [])], f"{n}: {t} is not a GPU case"
