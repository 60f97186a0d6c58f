"""GPU tests of the fused Gaussian Adam step (freesplat_amd.refine.GaussianAdam, fs_gaussian_adam_step, csrc/gaussian_adam.hip)
against the float64 restatement tests/gaussian_adam_ref.py.

Bound of every value comparison (the rule of the SSIM loss tests): max(4 E, K 2^-23 max|ref|), E = the error of the same
formulas run eagerly in fp32 torch on the same device against the same float64 result, K = the number of steps.  The floor
allows K roundings of the stored value (half an ulp each), doubled for the update's own arithmetic.  Inputs: |g| = |normal|
10^U(-4, 2) fresh for each step, logits clamped to [-6, 6], log-scales ~ N(0, 3), means ~ N(0, 10); saturated logits and
gradients that underflow in fp32 are outside these tests (Adam's normalisation turns an underflowed gradient into a full step
in any fp32 implementation).  Every comparison prints its error / bound ratio before it asserts (run with -s to see them).
"""
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gaussian_adam_ref as R  # noqa: E402
from guarded_alloc import FILLS, guarded  # noqa: E402

pytestmark = pytest.mark.gpu
K = R.K_STEPS
SHAPES = [(N, M) for N in R.N_SHAPES for M in R.M_SHAPES]


@functools.lru_cache(maxsize=None)
def _reference(N, M):
    """(raw, grads, float64 state after K dense steps): computed once per shape and shared; read-only."""
    raw, grads = R.make_inputs(N, M, K)
    ref = R.RefAdam(raw)
    for g in grads:
        ref.step(g)
    return raw, grads, ref


def _opt(raw, dev, **kw):
    """A GaussianAdam whose raw parameters are exactly `raw` (the constructor inverts the activations in fp32, which does not
    round-trip; the exact raw values go in through load_state_dict)."""
    from freesplat_amd.refine import GaussianAdam
    d = lambda t: t.to(dev)
    opt = GaussianAdam(d(raw[0]), d(torch.exp(raw[1])), d(raw[2]), d(torch.sigmoid(raw[3])), d(raw[4]), **kw)
    sd = opt.state_dict()
    for name, t in zip(R.ARRAYS, raw):
        sd[name] = d(t)
    opt.load_state_dict(sd)
    return opt


def _set_grads(opt, grads, skip=()):
    for k, (leaf, g) in enumerate(zip(opt.leaves(), grads)):
        leaf.grad = None if k in skip else g.to(leaf.device).reshape(leaf.shape).clone()


def _snapshot(opt):
    """Everything a step may write, as clones: raw parameters, moments, step, and the two activated leaves."""
    sd = opt.state_dict()
    out = {k: v for k, v in sd.items() if isinstance(v, torch.Tensor)}
    out["scales"], out["opacities"] = opt.scales.detach().clone(), opt.opacities.detach().clone()
    return out


def _same(a: dict, b: dict, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


def _poison(grads, radii):
    """Gradient rows of Gaussians that are not visible filled with NaN."""
    on = radii > 0
    return [torch.where(on.reshape((-1,) + (1,) * (g.dim() - 1)), g, torch.full_like(g, float("nan"))) for g in grads]


def _check_values(opt, ref, eager, k_steps, what):
    """p, exp_avg, exp_avg_sq of every array against the float64 state `ref`, with E from the fp32 restatement `eager`."""
    sd = opt.state_dict()
    worst = 0.0
    for k, name in enumerate(R.ARRAYS):
        for got, want, e32, q in ((sd[name], ref.p[k], eager.p[k], "p"), (sd["exp_avg." + name], ref.m[k], eager.m[k], "m"),
                                  (sd["exp_avg_sq." + name], ref.v[k], eager.v[k], "v")):
            E, e = R.err(e32, want), R.err(got, want)
            b = R.bound(E, want, k_steps)
            print(f"{what} {name}.{q}: err {e:.3e} eager {E:.3e} bound {b:.3e} ratio {e / b:.3f}")
            worst = max(worst, e / b)
            assert e <= b, f"{what} {name}.{q}: {e} > {b} (eager fp32: {E})"
    # the activated outputs against float64 exp / sigmoid of the kernel's own new raw values
    for got, raw_t, fn, name in ((opt.scales, sd["log_scales"], torch.exp, "out_scales"),
                                 (opt.opacities, sd["logits"], torch.sigmoid, "out_opacities")):
        want = fn(raw_t.double().cpu())
        E, e = R.err(fn(raw_t), want), R.err(got, want)
        b = R.bound(E, want, k_steps)
        print(f"{what} {name}: err {e:.3e} eager {E:.3e} bound {b:.3e} ratio {e / b:.3f}")
        worst = max(worst, e / b)
        assert e <= b, f"{what} {name}: {e} > {b} (torch fp32: {E})"
    print(f"{what} worst ratio {worst:.3f}")


def _activate(log_scales, logits):
    """fs_gaussian_activate of the given raw values into fresh buffers."""
    from freesplat_amd import _lib
    N = logits.numel()
    s, o = torch.empty(N, 3, device=logits.device), torch.empty(N, 1, device=logits.device)
    _lib.check(_lib.lib().fs_gaussian_activate(N, _lib.ptr(log_scales), _lib.ptr(logits), _lib.ptr(s), _lib.ptr(o),
                                               _lib.current_stream()), "fs_gaussian_activate")
    return s, o


@pytest.mark.parametrize("N,M", SHAPES)
def test_values_after_k_steps(hip_device, N, M):
    raw, grads, ref = _reference(N, M)
    opt = _opt(raw, hip_device)
    eager = R.RefAdam(raw, dtype=torch.float32, device=hip_device)
    for g in grads:
        _set_grads(opt, g)
        opt.step()
        eager.step(g)
        assert all(t.grad is None for t in opt.leaves())
    assert int(opt.step_count) == K
    _check_values(opt, ref, eager, K, f"dense N={N} M={M}")
    # consistency: the leaves the next forward reads are fs_gaussian_activate of the new raw values, bit for bit
    sd = opt.state_dict()
    s, o = _activate(sd["log_scales"], sd["logits"])
    assert torch.equal(s, opt.scales.detach()) and torch.equal(o, opt.opacities.detach())


@pytest.mark.parametrize("N,M", SHAPES)
def test_sparse_step_skips_invisible_rows(hip_device, N, M):
    raw, grads, _ = _reference(N, M)
    radii = [R.radii_pattern(N, 0), R.radii_pattern(N, 4)]
    dense, sparse = _opt(raw, hip_device), _opt(raw, hip_device, sparse=True)
    before = _snapshot(sparse)
    _set_grads(dense, grads[0])
    dense.step()
    _set_grads(sparse, _poison(grads[0], radii[0]))
    sparse.step(radii[0].to(hip_device))
    after, full = _snapshot(sparse), _snapshot(dense)
    on = (radii[0] > 0).to(hip_device)
    for k in after:
        if k in ("step", "lr"):
            continue
        a, b, d = (t[k].reshape(N, -1) for t in (after, before, full))
        assert bool(torch.isfinite(a).all()), k
        assert torch.equal(a[~on], b[~on]), f"{k}: a row that is not visible was written"
        assert torch.equal(a[on], d[on]), f"{k}: a visible row differs from the dense step"
    assert int(after["step"]) == 1
    # a second step with another visibility: t is global (a row first seen now is corrected with t = 2)
    ref, eager = R.RefAdam(raw), R.RefAdam(raw, dtype=torch.float32, device=hip_device)
    for r, g in zip(radii, grads[:2]):
        ref.step(g, r)
        eager.step(g, r)
    _set_grads(sparse, _poison(grads[1], radii[1]))
    sparse.step(radii[1].to(hip_device))
    assert int(sparse.step_count) == 2
    _check_values(sparse, ref, eager, 2, f"sparse N={N} M={M}")
    with pytest.raises(ValueError, match="radii"):
        _set_grads(sparse, grads[2])
        sparse.step()


@pytest.mark.parametrize("skip", [(0,), (1,), (2,), (3,), (4,), (0, 2, 4), (1, 3)])
def test_null_gradient_arrays_are_left_untouched(hip_device, skip):
    N, M = 65, 4
    raw, grads, _ = _reference(N, M)
    full, part = _opt(raw, hip_device), _opt(raw, hip_device)
    for o in (full, part):
        _set_grads(o, grads[0])
        o.step()
    before = _snapshot(part)
    _set_grads(full, grads[1])
    full.step()
    _set_grads(part, grads[1], skip=skip)
    part.step()
    got, want = _snapshot(part), _snapshot(full)
    act = {1: "scales", 3: "opacities"}
    for k, name in enumerate(R.ARRAYS):
        keys = [name, "exp_avg." + name, "exp_avg_sq." + name] + ([act[k]] if k in act else [])
        for key in keys:
            assert torch.equal(got[key], before[key] if k in skip else want[key]), (key, skip)
            assert not torch.equal(before[key], want[key])                 # the step does move every array it is given
    assert int(got["step"]) == 2
    with pytest.raises(ValueError, match="without any gradient"):
        part.step()


def _run(raw, grads, dev, sparse, steps=3):
    opt = _opt(raw, dev, sparse=sparse)
    for i in range(steps):
        _set_grads(opt, grads[i])
        opt.step(R.radii_pattern(raw[0].shape[0], i).to(dev) if sparse else None)
    return _snapshot(opt)


@pytest.mark.parametrize("sparse", [False, True])
def test_same_bits_on_every_run_and_stream(hip_device, sparse):
    raw, grads, _ = _reference(1031, 9)
    first = _run(raw, grads, hip_device, sparse)
    _same(first, _run(raw, grads, hip_device, sparse), "second run")
    side = torch.cuda.Stream(device=hip_device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _run(raw, grads, hip_device, sparse)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _same(first, other, "side stream")


def test_unaligned_arrays_take_four_byte_accesses(hip_device):
    """The library call itself with every array 4 bytes off a 16-byte boundary: the same bits as the aligned call."""
    import ctypes as C
    from freesplat_amd import _lib
    N, M = 65, 4
    raw, grads, _ = _reference(N, M)
    dev = hip_device

    def call(off):
        place = lambda t: torch.empty(t.numel() + 4, device=dev)[off:off + t.numel()].copy_(t.to(dev).flatten())
        p, g = [place(t) for t in raw], [place(t) for t in grads[0]]
        m, v = [place(torch.zeros_like(t)) for t in raw], [place(torch.zeros_like(t)) for t in raw]
        outs = [place(torch.zeros(3 * N)), place(torch.zeros(N))]
        assert all(t.data_ptr() % 16 == 4 * off for t in p + g + m + v + outs)
        lr = torch.tensor([R.DEFAULT_LR[k] for k in R.GROUPS], device=dev)
        step = torch.zeros(1, dtype=torch.int32, device=dev)
        radii = R.radii_pattern(N, 0).to(dev)
        tab = lambda ts: (C.c_void_p * 5)(*[t.data_ptr() for t in ts])
        for vis in (None, radii):
            _lib.check(_lib.lib().fs_gaussian_adam_step(N, M, tab(p), tab(g), tab(m), tab(v), _lib.ptr(vis), _lib.ptr(lr),
                                                        _lib.ptr(step), 0.9, 0.999, 1e-15, _lib.ptr(outs[0]), _lib.ptr(outs[1]),
                                                        _lib.current_stream()), "fs_gaussian_adam_step")
        assert int(step) == 2
        return [t.clone() for t in p + m + v + outs]

    for a, b in zip(call(0), call(1)):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())


def test_graph_capture_and_replay(hip_device):
    """step() recorded into one graph on a side stream; three replays with fresh gradients copied into the captured buffers
    give the bits of three eager steps, and a set_lr between replays takes effect."""
    N, M = 257, 9
    raw, grads, _ = _reference(N, M)
    dev = hip_device
    eager, cap = _opt(raw, dev), _opt(raw, dev)
    warm = _opt(raw, dev)                                # loads the kernels outside the capture
    _set_grads(warm, grads[0])
    warm.step()
    bufs = [torch.zeros_like(t) for t in cap.leaves()]
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    for leaf, b in zip(cap.leaves(), bufs):
        leaf.grad = b
    with torch.cuda.graph(graph, stream=side):
        cap.step()
    torch.cuda.synchronize()
    assert int(cap.step_count) == 0                      # capture records, it does not run
    for i in range(3):
        if i == 2:
            for o in (eager, cap):
                o.set_lr("means", 0.05)
                o.set_lr("sh_rest", 0.01)
        _set_grads(eager, grads[i])
        eager.step()
        for b, g in zip(bufs, grads[i]):
            b.copy_(g.to(dev).reshape(b.shape))
        graph.replay()
        torch.cuda.synchronize()
        _same(_snapshot(eager), _snapshot(cap), f"replay {i}")
    assert int(cap.step_count) == 3
    # the new rate was used: the third step moved the means by about 0.05, not 1.6e-4
    sd = cap.state_dict()
    assert float((sd["means"].cpu() - raw[0]).abs().max()) > 0.01


def test_state_dict_round_trip(hip_device):
    from freesplat_amd.refine import GaussianAdam
    N, M = 65, 4
    raw, grads, _ = _reference(N, M)
    dev = hip_device
    whole = _opt(raw, dev, sparse=True, lr=dict(means=1e-3), betas=(0.8, 0.99))
    radii = [R.radii_pattern(N, i).to(dev) for i in range(4)]
    for i in range(2):
        _set_grads(whole, grads[i])
        whole.step(radii[i])
    sd = whole.state_dict()
    other = GaussianAdam(*[torch.rand(s, device=dev) * 0.5 + 0.25 for s in ((N, 3), (N, 3), (N, 4), (N,), (N, M, 3))])
    other.load_state_dict(sd)
    assert other.sparse and other.betas == (0.8, 0.99)
    _same(_snapshot(whole), _snapshot(other), "after load")
    for i in range(2, 4):
        for o in (whole, other):
            _set_grads(o, grads[i])
            o.step(radii[i])
    _same(_snapshot(whole), _snapshot(other), "load -> step")
    assert int(other.step_count) == 4
    with pytest.raises(ValueError, match="state of shape"):
        GaussianAdam(*[torch.rand(s, device=dev) * 0.5 + 0.25 for s in ((3, 3), (3, 3), (3, 4), (3,), (3, M, 3))]).load_state_dict(sd)


def test_constructor_and_from_gaussians(hip_device):
    """The leaves have the rasterizer's form and hold the inputs (to the rounding of log / exp); from_gaussians takes the
    adapter's Gaussians: (scales, rotations) rebuild the world covariances, harmonics arrive as [N, M, 3]."""
    from freesplat_amd import synthetic
    from freesplat_amd.gaussian_adapter import Gaussians
    from freesplat_amd.rasterizer import build_cov3d
    from freesplat_amd.refine import GaussianAdam
    dev = hip_device
    sc = synthetic.make_scene(300, n_context=2, seed=3, sh_degree=1, ctx_hw=(32, 48))
    g = Gaussians(means=sc["means"][None].to(dev), covariances=sc["covariances"][None].to(dev), scales=None, rotations=None,
                  harmonics=sc["harmonics"][None].to(dev), opacities=sc["opacities"][None].to(dev))
    opt = GaussianAdam.from_gaussians(g, sparse=True)
    assert [tuple(t.shape) for t in opt.leaves()] == [(300, 3), (300, 3), (300, 4), (300, 1), (300, 4, 3)]
    assert all(t.requires_grad and t.is_leaf and t.dtype == torch.float32 for t in opt.leaves())
    assert torch.equal(opt.means.detach().cpu(), sc["means"]) and torch.equal(opt.shs.detach().cpu(), sc["harmonics"].transpose(1, 2))
    assert float((opt.opacities.detach().cpu().flatten() - sc["opacities"]).abs().max()) <= 1e-6
    cov = build_cov3d(opt.scales.detach().double().cpu(), opt.rotations.detach().double().cpu(), 1.0)
    i, j = torch.triu_indices(3, 3)
    want = sc["covariances"][:, i, j].double()
    assert float((cov - want).abs().max()) <= 1e-5 * float(want.abs().max())
    with pytest.raises(ValueError, match="float32"):
        GaussianAdam(opt.means.double(), opt.scales, opt.rotations, opt.opacities, opt.shs)
    with pytest.raises(ValueError, match="positive"):
        GaussianAdam(opt.means, -opt.scales, opt.rotations, opt.opacities, opt.shs)
    with pytest.raises(ValueError, match="learning-rate group"):
        opt.set_lr("colour", 1.0)


def test_guard_bands_dense_and_sparse(hip_device):
    """Construction plus two steps, dense and sparse, with every allocation of the package inside guard bands: unguarded, then
    pre-filled with 0xFF bytes, zeros and finite garbage.  Nothing is written outside a block; the four runs agree bit for bit."""
    from freesplat_amd.refine import GaussianAdam
    N, M = 65, 4
    raw, grads, _ = _reference(N, M)
    dev = hip_device
    acts = [raw[0], torch.exp(raw[1]), raw[2], torch.sigmoid(raw[3]), raw[4]]

    def run(sparse, place):
        opt = GaussianAdam(*[place(t.to(dev)) for t in acts], sparse=sparse)
        for i in range(2):
            radii = R.radii_pattern(N, i).to(dev)
            g = _poison(grads[i], R.radii_pattern(N, i)) if sparse else grads[i]
            for leaf, t in zip(opt.leaves(), g):
                leaf.grad = place(t.to(dev).reshape(leaf.shape))
            opt.step(place(radii) if sparse else None)
        return _snapshot(opt)

    for sparse in (False, True):
        base = run(sparse, lambda t: t.clone())
        assert all(bool(torch.isfinite(t).all()) for t in base.values())
        for fill in FILLS:
            with guarded(fill) as arena:
                got = run(sparse, arena.place)
                torch.cuda.synchronize()
                arena.check(f"GaussianAdam sparse={sparse}")
            assert len(arena.records) > 20
            _same(base, got, f"fill {fill} sparse={sparse}")


# ------------------------------------------------------------------------------------------------------------ end to end

def _scene(dev):
    """A synthetic scene of 500 Gaussians seen at 32 x 48 in (scales, rotations) form, and the rasterizer for its first view."""
    from freesplat_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    from freesplat_amd.refine import scale_rot_from_covariances
    from util_raster import small_scene, view_inputs
    H, W = 32, 48
    scene, cams = small_scene(N=500, H=H, W=W, seed=7, n_views=2, sh_degree=2)
    scene["means"][3::7, 2] = -2.0                       # every seventh Gaussian behind the camera: radii 0 in this view
    vi = view_inputs(scene, cams, 0, H, W, bg=(0.1, 0.1, 0.1))
    N = vi["means3D"].shape[0]
    cov = torch.zeros(N, 3, 3)
    r, c = torch.triu_indices(3, 3)
    cov[:, r, c] = vi["cov3D"]
    cov[:, c, r] = vi["cov3D"]
    scales, rotations = scale_rot_from_covariances(cov.to(dev))
    d = lambda t: t.to(dev)
    s = GaussianRasterizationSettings(H, W, vi["tanfovx"], vi["tanfovy"], d(vi["bg"]), 1.0, d(vi["viewmatrix"]),
                                      d(vi["projmatrix"]), vi["sh_degree"], d(vi["campos"]), False, False)
    return GaussianRasterizer(s), [d(vi["means3D"]), scales, rotations, d(vi["opacities"]), d(vi["shs"])]


def _render(rast, opt_or_list):
    m, s, q, o, sh = opt_or_list.leaves() if hasattr(opt_or_list, "leaves") else opt_or_list
    color, radii, _, _ = rast(m, None, o, shs=sh, scales=s, rotations=q)
    return color, radii


def test_refinement_loop_end_to_end(hip_device):
    from freesplat_amd import rasterizer
    from freesplat_amd.refine import GaussianAdam
    from freesplat_amd.ssim_loss import photometric_loss
    dev = hip_device
    saved = rasterizer.DETERMINISTIC
    rasterizer.DETERMINISTIC = True
    try:
        rast, truth = _scene(dev)
        with torch.no_grad():
            target = _render(rast, truth)[0][None]
        gen = torch.Generator().manual_seed(11)
        rnd = lambda t, s: (s * torch.randn(t.shape, generator=gen)).to(dev)
        m, s, q, o, sh = truth
        logit = torch.log(o) - torch.log1p(-o)
        start = [m + rnd(m, 0.02), s * torch.exp(rnd(s, 0.3)), q, torch.sigmoid(logit + rnd(o, 1.0)), sh]

        # step 1 against torch.optim.Adam in fp32 with eager activations, on the same raw values and the same gradients
        opt = GaussianAdam(*start)
        raw0 = [opt.state_dict()[k] for k in R.ARRAYS]
        color, radii = _render(rast, opt)
        loss0 = photometric_loss(color[None], target)
        loss0.backward()
        grads = [t.grad.detach().clone().reshape(r.shape) for t, r in zip(opt.leaves(), raw0)]
        assert all(bool(torch.isfinite(g).all()) for g in grads) and all(bool(g.any()) for g in grads)
        opt.step()
        leaves = [t.clone().requires_grad_(True) for t in (raw0[0], raw0[1], raw0[2], raw0[3], raw0[4][:, :1], raw0[4][:, 1:])]
        adam = torch.optim.Adam([dict(params=[p], lr=R.DEFAULT_LR[n]) for p, n in zip(leaves, R.GROUPS)], betas=(0.9, 0.999),
                                eps=1e-15)
        acts = (leaves[0], torch.exp(leaves[1]), leaves[2], torch.sigmoid(leaves[3]), torch.cat([leaves[4], leaves[5]], 1))
        sum((a * g).sum() for a, g in zip(acts, grads)).backward()
        adam.step()
        eager = R.RefAdam(raw0, dtype=torch.float32, device=dev)
        eager.step(grads)
        join = lambda ts: ts[:4] + [torch.cat(ts[4:], 1)]
        want = dict(p=join([t.detach() for t in leaves]), m=join([adam.state[t]["exp_avg"] for t in leaves]),
                    v=join([adam.state[t]["exp_avg_sq"] for t in leaves]))
        sd = opt.state_dict()
        for k, name in enumerate(R.ARRAYS):
            for q_, got, e32 in (("p", sd[name], eager.p[k]), ("m", sd["exp_avg." + name], eager.m[k]),
                                 ("v", sd["exp_avg_sq." + name], eager.v[k])):
                ref = want[q_][k]
                E, e = R.err(e32, ref), R.err(got, ref)
                b = R.bound(E, ref, 1)
                print(f"step 1 vs torch.optim.Adam {name}.{q_}: err {e:.3e} eager {E:.3e} bound {b:.3e}")
                assert e <= b, f"{name}.{q_}: {e} > {b}"

        # 19 more steps: the loss goes down
        for _ in range(19):
            color, radii = _render(rast, opt)
            photometric_loss(color[None], target).backward()
            opt.step(radii)                              # a dense optimizer ignores radii
        with torch.no_grad():
            loss20 = photometric_loss(_render(rast, opt)[0][None], target)
        loss0 = float(loss0.detach())
        print(f"photometric loss {loss0:.5f} -> {float(loss20):.5f} after 20 steps")
        assert float(loss20) < loss0

        # the sparse step through the same loop
        sparse = GaussianAdam(*start, sparse=True)
        first, seen = None, torch.zeros(sparse.N, dtype=torch.bool, device=dev)
        for _ in range(5):
            color, radii = _render(rast, sparse)
            loss = photometric_loss(color[None], target)
            first = float(loss.detach()) if first is None else first
            loss.backward()
            sparse.step(radii)
            seen |= radii > 0
        assert int(sparse.step_count) == 5 and int((~seen).sum()) >= 50 and int(seen.sum()) >= 400
        after = _snapshot(sparse)
        assert all(bool(torch.isfinite(t).all()) for t in after.values())
        with torch.no_grad():
            assert float(photometric_loss(_render(rast, sparse)[0][None], target)) < first
        fresh = _snapshot(GaussianAdam(*start, sparse=True))
        for k in after:                                      # rows never seen: parameters as constructed, no moments
            if k not in ("step", "lr"):
                assert torch.equal(after[k].reshape(sparse.N, -1)[~seen], fresh[k].reshape(sparse.N, -1)[~seen]), k
    finally:
        rasterizer.DETERMINISTIC = saved
