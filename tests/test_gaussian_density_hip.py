"""GPU tests of adaptive density control (freesplat_amd.refine.GaussianAdam.accumulate / densify / reset_opacity,
include/freesplat_amd_density.h, csrc/gaussian_density.hip) against the restatement tests/gaussian_density_ref.py.

What is exact is compared for equality: the plan (kind, offset, totals, the source map) given the device's own fp32 inputs,
every copied parameter and moment, the zeroed moments, the activated outputs against fs_gaussian_activate.  The children's
means and log-scales and the accumulated gradient norms are fp32 arithmetic: bound max(4 E, K 2^-23 max|ref|) with E the error
of the same formulas run eagerly in fp32 torch on the same device against the same float64 result (the rule of the Gaussian
Adam tests), K = 1 for the children and K = the number of calls for the accumulation.  Every such comparison prints its
error / bound before it asserts (run with -s).
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gaussian_adam_ref as R  # noqa: E402
import gaussian_density_ref as D  # noqa: E402
from guarded_alloc import FILLS, guarded  # noqa: E402

pytestmark = pytest.mark.gpu
N_SHAPES = (1, 5, 1023, 1024, 1025, 4099)
M_SHAPES = (1, 9, 16)
N_BIG = 1024 * 1024 + 1                       # (rows per scan workgroup) x (threads of the block-sum scan) + 1
KW = dict(extent=1.0, grad_threshold=D.GRAD_T, min_opacity=D.MIN_OP, percent_dense=D.DENSE)       # thresholds of stats_for
TH = D.thresholds(**KW)
MODES = {"kept": D.KEPT, "cloned": D.CLONE, "split": D.SPLIT}


def _kinds(N, mode, k=0):
    if mode == "pattern":
        return D.kind_pattern(N, k)
    if mode == "one_left":
        kind = np.full(N, D.DROPPED, np.uint8)
        kind[(2 * N) // 3] = D.CLONE
        return kind
    if mode == "none_left":
        return np.full(N, D.DROPPED, np.uint8)
    return np.full(N, MODES[mode], np.uint8)


@functools.lru_cache(maxsize=None)
def _case(N, M, mode="pattern", k=0):
    """(kind, raw, exp_avg, exp_avg_sq, stats): a state whose plan under KW is `kind`; float32 CPU tensors, read-only."""
    kind = _kinds(N, mode, k)
    raw, m, v = D.make_state(N, M)
    ga, dn, mr, sc, op = D.stats_for(kind, ties=False)
    raw[D.SCALES] = torch.log(torch.from_numpy(sc))
    op = torch.from_numpy(op)
    raw[D.OPACITIES] = torch.log(op) - torch.log1p(-op)
    return kind, raw, m, v, tuple(torch.from_numpy(a) for a in (ga, dn, mr))


def _opt(case, dev, place=lambda t: t, **kw):
    """A GaussianAdam holding exactly the case's raw values, moments and statistics, with 3 steps on its counter."""
    from freesplat_amd.refine import GaussianAdam
    _, raw, m, v, stats = case
    d = lambda t: place(t.to(dev))
    opt = GaussianAdam(d(raw[0]), d(torch.exp(raw[1])), d(raw[2]), d(torch.sigmoid(raw[3])), d(raw[4]), **kw)
    sd = opt.state_dict()
    for name, p_, m_, v_ in zip(R.ARRAYS, raw, m, v):
        sd[name], sd["exp_avg." + name], sd["exp_avg_sq." + name] = d(p_), d(m_), d(v_)
    for name, t in zip(("grad_accum", "denom", "max_radii"), stats):
        sd["density." + name] = d(t)
    sd["step"] = torch.full((1,), 3, dtype=torch.int32, device=dev)
    opt.load_state_dict(sd)
    return opt


def _snapshot(opt):
    sd = opt.state_dict()
    out = {k: v for k, v in sd.items() if isinstance(v, torch.Tensor)}
    out["scales"], out["opacities"] = opt.scales.detach().clone(), opt.opacities.detach().clone()
    return out


def _same(a: dict, b: dict, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), f"{what}: {k} differs"


def _activate(log_scales, logits):
    from freesplat_amd import _lib
    N = logits.numel()
    s, o = torch.empty(N, 3, device=logits.device), torch.empty(N, 1, device=logits.device)
    _lib.check(_lib.lib().fs_gaussian_activate(N, _lib.ptr(log_scales), _lib.ptr(logits), _lib.ptr(s), _lib.ptr(o),
                                               _lib.current_stream()), "fs_gaussian_activate")
    return s, o


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _check_plan(opt, kind_want, th=TH):
    """The device's plan against the restatement fed with the device's own statistics, scales and opacities."""
    kind, offset, src, totals = opt._plan([float(t) for t in th])
    ref_kind, ref_offset, ref_totals = D.plan(opt.grad_accum.cpu().numpy(), opt.denom.cpu().numpy(), opt.max_radii.cpu().numpy(),
                                              opt.scales.detach().cpu().numpy(), opt.opacities.detach().cpu().numpy(), th)
    assert np.array_equal(kind.cpu().numpy(), ref_kind) and np.array_equal(_u32(offset), ref_offset) and totals == ref_totals
    rows, j = D.source_map(ref_kind)
    tag = (ref_kind[rows] == D.SPLIT).astype(np.uint32) << np.uint32(31)             # src[o] = (2 i + j) | (split ? 2^31 : 0)
    assert np.array_equal(_u32(src)[:totals[0]], (2 * rows + j).astype(np.uint32) | tag)
    if kind_want is not None:
        assert np.array_equal(ref_kind, kind_want)
    return ref_kind, totals


def _check_apply(case, opt, info, seed, dev, what):
    """The optimizer after densify(seed=seed) against the float64 gather of the case's state."""
    kind, raw, m, v, _ = case
    N = len(kind)
    ref = D.apply(raw, m, v, kind, seed)
    eager = D.apply(raw, m, v, kind, seed, dtype=torch.float32, device=dev)
    rows, is_split = torch.from_numpy(ref["rows"]), torch.from_numpy(ref["kind"] == D.SPLIT)
    n_out = len(rows)
    assert info == dict(n_out=n_out, n_cloned=int((kind == D.CLONE).sum()), n_split=int((kind == D.SPLIT).sum()),
                        n_dropped=int((kind == D.DROPPED).sum()))
    assert opt.N == n_out and [t.shape[0] for t in opt.leaves()] == [n_out] * 5 and tuple(opt.viewspace.shape) == (n_out, 3)
    assert all(t.requires_grad and t.is_leaf and t.grad is None for t in opt.leaves() + [opt.viewspace])
    sd = opt.state_dict()
    for k, name in enumerate(R.ARRAYS):
        got = sd[name].cpu()
        src_rows = raw[k][rows]
        exact = torch.ones(n_out, dtype=torch.bool) if k not in (D.MEANS, D.SCALES) else ~is_split
        assert torch.equal(got[exact], src_rows[exact]), f"{what} {name}: a copied row is not a bit copy"
        if k in (D.MEANS, D.SCALES) and bool(is_split.any()):
            want, e32 = ref["p"][k][is_split], eager["p"][k][is_split.to(dev)]
            E, e = D.err(e32, want), D.err(got[is_split], want)
            b = D.bound(E, want, 1)
            print(f"{what} children {name}: err {e:.3e} eager {E:.3e} bound {b:.3e} ratio {e / b:.3f}")
            assert e <= b, f"{what} children {name}: {e} > {b} (eager fp32: {E})"
            assert not torch.equal(got[is_split], src_rows[is_split])
        for key, want in (("exp_avg." + name, ref["m"][k]), ("exp_avg_sq." + name, ref["v"][k])):
            assert torch.equal(sd[key].cpu().double(), want), f"{what} {key}"
    s, o = _activate(sd["log_scales"], sd["logits"])
    assert torch.equal(s, opt.scales.detach()) and torch.equal(o, opt.opacities.detach()), f"{what}: activated outputs"
    assert int(sd["step"]) == 3 and torch.equal(sd["lr"].cpu(), torch.tensor([R.DEFAULT_LR[g] for g in R.GROUPS]))
    for name in ("grad_accum", "denom", "max_radii"):
        assert tuple(sd["density." + name].shape) == (n_out,) and not bool(sd["density." + name].any())
    assert not bool(opt.viewspace.detach().any()) and N == len(kind)


# ------------------------------------------------------------------------------------------------------------ accumulate

@pytest.mark.parametrize("N", [1, 5, 1023, 1025, 4099])
def test_accumulate_three_calls(hip_device, N):
    dev = hip_device
    case = _case(N, 1)
    opt = _opt(case, dev)
    gen = torch.Generator().manual_seed(N)
    start = tuple(t.clone() for t in case[4])
    ref = tuple(t.double() for t in start)
    eager = tuple(t.to(dev) for t in start)
    seen = torch.zeros(N, dtype=torch.bool)
    for call in range(3):
        radii = R.radii_pattern(N, call) * (1 + (torch.arange(N, dtype=torch.int32) * 7 + call) % 50)
        g = torch.randn(N, 3, generator=gen) * 10.0 ** (4.0 * torch.rand(N, 1, generator=gen) - 6.0)
        g[:, 2] = float("nan")                                             # the third component is never read
        g = torch.where((radii > 0)[:, None], g, torch.full_like(g, float("nan")))
        opt.viewspace.grad = g.to(dev)
        opt.accumulate(radii.to(dev))
        assert opt.viewspace.grad is None
        ref = D.accumulate(ref, g, radii)
        eager = D.accumulate(eager, g.to(dev), radii.to(dev), dtype=torch.float32)
        seen |= radii > 0
    got = (opt.grad_accum, opt.denom, opt.max_radii)
    E, e = D.err(eager[0], ref[0]), D.err(got[0], ref[0])
    b = D.bound(E, ref[0], 3)
    print(f"accumulate N={N}: err {e:.3e} eager {E:.3e} bound {b:.3e}")
    assert e <= b and bool(torch.isfinite(got[0]).all())
    assert torch.equal(got[1].cpu().double(), ref[1]) and torch.equal(got[2].cpu().double(), ref[2])   # denom, max_radii: exact
    for t, s in zip(got, start):
        assert torch.equal(t.cpu()[~seen], s[~seen])                       # rows never visible: bit-identical
    with pytest.raises(ValueError, match="view-space gradient"):
        opt.accumulate(radii.to(dev))
    opt.viewspace.grad = torch.zeros(N, 3, device=dev)
    for bad in (radii.to(dev).long(), radii, torch.zeros(N + 1, dtype=torch.int32, device=dev)):
        with pytest.raises(ValueError, match="radii"):
            opt.accumulate(bad)


def test_accumulated_ties_are_hot(hip_device):
    """Gradients (3, 4) 2^-k over three views sum to exactly 3 x 5 2^-k: hot at grad_threshold = 5 2^-k (>=), not hot one ulp
    above; accumulate and step() commute."""
    from freesplat_amd.refine import GaussianAdam
    dev, N = hip_device, 67
    raw, _ = R.make_inputs(N, 4)
    opt = GaussianAdam(raw[0].to(dev), torch.full((N, 3), 0.5, device=dev), raw[2].to(dev), torch.full((N,), 0.5, device=dev), raw[4].to(dev))
    g = torch.tensor([3.0, 4.0, float("nan")]).repeat(N, 1) * 2.0 ** -D.TIE_K
    radii = torch.full((N,), 9, dtype=torch.int32, device=dev)
    for _ in range(3):
        opt.viewspace.grad = g.to(dev)
        opt.accumulate(radii)
    assert bool((opt.grad_accum == 15.0 * 2.0 ** -D.TIE_K).all()) and bool((opt.denom == 3.0).all()) and bool((opt.max_radii == 9.0).all())
    above = float(np.nextafter(np.float32(D.GRAD_T), np.float32(1.0)))
    assert opt._plan([above, 1.0, 0.0, 0.0, 0.0, 0.0])[3] == [N, 0, 0, 0]
    assert opt._plan([D.GRAD_T, 1.0, 0.0, 0.0, 0.0, 0.0])[3] == [2 * N, N, 0, 0]
    assert opt._plan([D.GRAD_T, 0.25, 0.0, 0.0, 0.0, 0.0])[3] == [2 * N, 0, N, 0]


# ------------------------------------------------------------------------------------------------------------------ plan

def test_plan_ties_through_the_library(hip_device):
    """fs_density_plan on arrays that sit exactly on the thresholds: grad_accum == grad_threshold x denom (hot), s_max ==
    dense_scale (not split), opacity == min_opacity (not dropped); then the screen-size and world-size rules."""
    from freesplat_amd import _lib
    dev, N = hip_device, 1025
    L, p = _lib.lib(), _lib.ptr
    kind_want = D.kind_pattern(N, 1)
    arrays = D.stats_for(kind_want, ties=True)
    dv = [torch.from_numpy(a).to(dev) for a in arrays]

    def run(th):
        kind = torch.empty(N, dtype=torch.uint8, device=dev)
        offset, src = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(2 * N, dtype=torch.int32, device=dev)
        totals = torch.empty(4, dtype=torch.int32, device=dev)
        scratch = torch.empty(L.fs_density_plan_scratch_bytes(N), dtype=torch.uint8, device=dev).fill_(0xFF)
        _lib.check(L.fs_density_plan(N, *[p(t) for t in dv], *[float(t) for t in th], p(kind), p(offset), p(src), p(totals), p(scratch),
                                     _lib.current_stream()), "fs_density_plan")
        want = D.plan(*arrays, th)
        assert np.array_equal(kind.cpu().numpy(), want[0]) and np.array_equal(_u32(offset), want[1]) and totals.tolist() == want[2]
        return want[0]

    th = tuple(np.float32(t) for t in (D.GRAD_T, D.DENSE, D.MIN_OP, 0.0, 0.0, 0.0))
    assert np.array_equal(run(th), kind_want)
    screen = run(th[:3] + (np.float32(20.0), np.float32(0.0), np.float32(0.0)))
    big = arrays[2] > 20.0
    assert (screen[big & (kind_want != D.SPLIT)] == D.DROPPED).all() and np.array_equal(screen[~big | (kind_want == D.SPLIT)],
                                                                                     kind_want[~big | (kind_want == D.SPLIT)])
    # world size: unsplit rows with s_max = 0.25 (the ties) go at prune_scale 0.2, split parents (0.5) stay until 1.6 p < 0.5
    world = run(th[:4] + (np.float32(0.2), np.float32(1.6 * 0.2)))
    assert (world[kind_want == D.SPLIT] == D.DROPPED).all()
    world = run(th[:4] + (np.float32(0.4), np.float32(1.6 * 0.4)))
    assert np.array_equal(world, kind_want)
    assert set(run((np.float32("inf"),) + th[1:]).tolist()) == {D.DROPPED, D.KEPT}          # prune only


# ----------------------------------------------------------------------------------------------------------------- apply

@pytest.mark.parametrize("k", [0, 3])
@pytest.mark.parametrize("N,M", [(N, M) for N in N_SHAPES for M in M_SHAPES])
def test_densify_pattern(hip_device, N, M, k):
    case = _case(N, M, "pattern", k)
    opt = _opt(case, hip_device)
    _check_plan(opt, case[0])
    assert D.OUTPUTS[case[0]].sum() > 0
    info = opt.densify(seed=5 + k, **KW)
    _check_apply(case, opt, info, 5 + k, hip_device, f"N={N} M={M} k={k}")
    assert opt.densify_calls == 1


def test_densify_past_the_first_scan_level(hip_device):
    """More block sums than the block-sum scan has threads: 1 048 577 rows at M = 1."""
    case = _case(N_BIG, 1, "pattern", 2)
    opt = _opt(case, hip_device)
    _, totals = _check_plan(opt, case[0])
    assert totals[0] > N_BIG
    info = opt.densify(seed=9, **KW)
    _check_apply(case, opt, info, 9, hip_device, f"N={N_BIG}")


@pytest.mark.parametrize("mode", ["kept", "cloned", "split", "one_left"])
@pytest.mark.parametrize("N,M", [(5, 9), (1025, 1), (1025, 16)])
def test_densify_uniform_kinds(hip_device, N, M, mode):
    case = _case(N, M, mode)
    opt = _opt(case, hip_device)
    before = _snapshot(opt)
    _check_plan(opt, case[0])
    info = opt.densify(seed=1, **KW)
    _check_apply(case, opt, info, 1, hip_device, f"{mode} N={N} M={M}")
    assert info["n_out"] == {"kept": N, "cloned": 2 * N, "split": 2 * N, "one_left": 2}[mode]
    if mode == "kept":
        after = _snapshot(opt)
        _same({k: v for k, v in after.items() if not k.startswith("density.")}, {k: v for k, v in before.items() if not k.startswith("density.")},
              "all kept")


@pytest.mark.parametrize("N,M", [(5, 9), (1025, 4)])
def test_everything_dropped_raises_and_leaves_the_state(hip_device, N, M):
    opt = _opt(_case(N, M, "none_left"), hip_device)
    leaves, tables = opt.leaves() + [opt.viewspace], opt._tables
    before = _snapshot(opt)
    with pytest.raises(ValueError, match="every Gaussian"):
        opt.densify(**KW)
    _same(before, _snapshot(opt), "after the refused densify")
    assert all(a is b for a, b in zip(leaves, opt.leaves() + [opt.viewspace])) and tables is opt._tables and opt.N == N
    assert opt.densify_calls == 0
    with pytest.raises(ValueError, match="negative or NaN"):
        opt.densify(extent=-1.0)


def test_max_gaussians_plans_prune_only(hip_device):
    case = _case(1025, 4, "pattern", 1)
    capped, pruned, free = _opt(case, hip_device), _opt(case, hip_device), _opt(case, hip_device)
    n_kept_or_hot = int((case[0] != D.DROPPED).sum())
    info = capped.densify(seed=2, max_gaussians=n_kept_or_hot + 3, **KW)
    want = pruned.densify(seed=2, **dict(KW, grad_threshold=float("inf")))
    assert info == want == dict(n_out=n_kept_or_hot, n_cloned=0, n_split=0, n_dropped=1025 - n_kept_or_hot)
    _same(_snapshot(capped), _snapshot(pruned), "prune only")
    rows = torch.from_numpy(np.nonzero(case[0] != D.DROPPED)[0])
    assert torch.equal(capped.state_dict()["means"].cpu(), case[1][0][rows])
    n_free = int(D.OUTPUTS[case[0]].sum())
    assert free.densify(seed=2, max_gaussians=n_free, **KW)["n_out"] == n_free > n_kept_or_hot     # at the cap: not over it


# ------------------------------------------------------------------------------------------------------------- generator

def test_generator_bits_and_statistics(hip_device):
    """All 4099 rows split: the recovered z = R^T (mean_child - mean) / s (24 594 values) have |mean| < 0.05 and a standard
    deviation inside [0.95, 1.05]; the same seed gives the same bits, another seed moves every child, the two children of a
    parent differ; the default seed is the number of densify calls so far."""
    dev, N = hip_device, 4099
    case = _case(N, 1, "split")
    _, raw, _, _, _ = case

    def run(**kw):
        opt = _opt(case, dev)
        opt.densify(**kw, **KW)
        return opt.state_dict()["means"].cpu()

    a, again, other, default = run(seed=0), run(seed=0), run(seed=1), run()
    assert torch.equal(a, again) and torch.equal(a, default)
    assert bool((a != other).any(1).all()), "another seed must move every child"
    assert bool((a[0::2] != a[1::2]).any(1).all()), "the two children of a parent must differ"
    parent = raw[D.MEANS].double().repeat_interleave(2, 0)
    Rm = D.rotation(raw[D.ROTATIONS].double()).repeat_interleave(2, 0)
    s = torch.exp(raw[D.SCALES].double()).repeat_interleave(2, 0)
    z = (torch.einsum("nji,nj->ni", Rm, a.double() - parent) / s).numpy()
    assert z.size == 24594
    print(f"recovered z: mean {z.mean():+.4f} std {z.std():.4f}")
    assert abs(z.mean()) < 0.05 and 0.95 <= z.std() <= 1.05
    want = D.normals(0, np.repeat(np.arange(N), 2), np.tile(np.arange(2), N)).numpy()
    # the restated generator, value by value: the child's mean is an fp32 number (half an ulp of |mean| + |offset|, doubled
    # for the offset's own arithmetic), R^T sums three such errors, the division by s scales them
    tol = 3 * 2.0 ** -22 * ((parent.abs().max(1).values + (s * torch.from_numpy(want).abs()).max(1).values)[:, None] / s).numpy()
    assert (np.abs(z - want) <= tol).all(), float((np.abs(z - want) / tol).max())
    opt = _opt(case, dev)
    opt.densify(**dict(KW, grad_threshold=float("inf")))                   # call 0 (prune only, nothing dropped: 4099 rows stay)
    sd = opt.state_dict()
    sd.update({"density." + k: t.to(dev) for k, t in zip(("grad_accum", "denom", "max_radii"), case[4])})
    opt.load_state_dict(sd)
    opt.densify(**KW)                                                      # call 1: seed 1
    assert torch.equal(opt.state_dict()["means"].cpu(), other) and opt.densify_calls == 2


# ----------------------------------------------------------------------------------------------------------- continuation

def test_step_after_densify_equals_a_fresh_optimizer(hip_device):
    from freesplat_amd.refine import GaussianAdam
    dev, N, M = hip_device, 1031, 9
    case = _case(N, M, "pattern", 1)
    for sparse in (False, True):
        opt = _opt(case, dev, sparse=sparse, lr=dict(means=1e-3), betas=(0.8, 0.99))
        n = opt.densify(seed=4, **KW)["n_out"]
        sd = opt.state_dict()
        fresh = GaussianAdam(*[torch.rand(s, device=dev) * 0.5 + 0.25 for s in ((n, 3), (n, 3), (n, 4), (n,), (n, M, 3))])
        fresh.load_state_dict(sd)
        _same(_snapshot(opt), _snapshot(fresh), "after load")
        _, grads = R.make_inputs(n, M, K=1, seed=3)
        radii = R.radii_pattern(n, 1).to(dev)
        for o in (opt, fresh):
            for leaf, g in zip(o.leaves(), grads[0]):
                leaf.grad = g.to(dev).reshape(leaf.shape).clone()
            o.step(radii)
        _same(_snapshot(opt), _snapshot(fresh), f"densify -> step, sparse={sparse}")
        assert int(opt.step_count) == 4
        # the old state dict no longer fits, the new statistics round-trip, a state without them zeroes them
        with pytest.raises(ValueError, match="state of shape"):
            _opt(case, dev).load_state_dict(sd)
        sd["density.denom"] = torch.ones(n, device=dev)
        fresh.load_state_dict(sd)
        assert bool((fresh.denom == 1).all())
        fresh.load_state_dict({k: v for k, v in sd.items() if not k.startswith("density.")})
        assert not bool(fresh.denom.any())


# ---------------------------------------------------------------------------------------------------------- reset_opacity

@pytest.mark.parametrize("N", [1, 1025])
def test_reset_opacity(hip_device, N):
    import math
    opt = _opt(_case(N, 4, "pattern", 0), hip_device)
    before = _snapshot(opt)
    opt.reset_opacity()
    after = _snapshot(opt)
    limit = np.float32(math.log(0.01 / 0.99))
    assert torch.equal(after["logits"].cpu(), torch.from_numpy(np.minimum(before["logits"].cpu().numpy(), limit)))
    assert bool((after["logits"] <= float(limit)).all()) and (N == 1 or bool((after["logits"] < float(limit)).any()))
    assert not bool(after["exp_avg.logits"].any()) and not bool(after["exp_avg_sq.logits"].any()) and bool(before["exp_avg.logits"].any())
    _, o = _activate(after["log_scales"], after["logits"])
    assert torch.equal(o, after["opacities"]) and float(after["opacities"].max()) <= 0.01 * (1 + 1e-5)
    for k in before:
        if k not in ("logits", "exp_avg.logits", "exp_avg_sq.logits", "opacities"):
            assert torch.equal(before[k], after[k]), k
    opt.reset_opacity(0.5)
    assert torch.equal(_snapshot(opt)["logits"], after["logits"])
    for bad in (0.0, 1.0, float("nan")):
        with pytest.raises(ValueError, match="max_opacity"):
            opt.reset_opacity(bad)


# ------------------------------------------------------------------------------------- determinism, alignment, guard bands

def _sequence(case, dev, place=lambda t: t):
    """accumulate -> densify -> step -> reset_opacity; the snapshot after it."""
    N, M = len(case[0]), case[1][4].shape[1]
    opt = _opt(case, dev, place=place, sparse=True)
    gen = torch.Generator().manual_seed(5)
    radii = R.radii_pattern(N, 2)
    g = torch.where((radii > 0)[:, None], 1e-3 * torch.randn(N, 3, generator=gen), torch.full((N, 3), float("nan")))
    opt.viewspace.grad = place(g.to(dev))
    opt.accumulate(place(radii.to(dev)))
    n = opt.densify(seed=3, **KW)["n_out"]
    _, grads = R.make_inputs(n, M, K=1, seed=8)
    for leaf, t in zip(opt.leaves(), grads[0]):
        leaf.grad = place(t.to(dev).reshape(leaf.shape))
    opt.step(place(R.radii_pattern(n, 0).to(dev)))
    opt.reset_opacity(0.3)
    return _snapshot(opt)


def test_same_bits_on_every_run_and_stream(hip_device):
    case = _case(4099, 9, "pattern", 0)
    first = _sequence(case, hip_device)
    assert all(bool(torch.isfinite(t).all()) for t in first.values())
    _same(first, _sequence(case, hip_device), "second run")
    side = torch.cuda.Stream(device=hip_device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _sequence(case, hip_device)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _same(first, other, "side stream")


@pytest.mark.parametrize("M", [1, 4, 9])
def test_unaligned_arrays_take_four_byte_accesses(hip_device, M):
    """The library calls themselves with every array 4 bytes off a 16-byte boundary: the same bits as the aligned calls."""
    from freesplat_amd import _lib
    dev, N = hip_device, 1031
    kind_want, raw, m, v, stats = _case(N, M, "pattern", 0)
    L, p = _lib.lib(), _lib.ptr
    n_out = int(D.OUTPUTS[kind_want].sum())

    def call(off):
        place = lambda t: torch.empty(t.numel() + 4, device=dev)[off:off + t.numel()].copy_(t.to(dev).flatten())
        fresh = lambda n, dt=torch.float32: torch.full((n + 4,), -1, dtype=dt, device=dev)[off:off + n]
        ps, ms, vs, st = [place(t) for t in raw], [place(t) for t in m], [place(t) for t in v], [place(t) for t in stats]
        act = [place(torch.exp(raw[1])), place(torch.sigmoid(raw[3]))]
        kind = torch.full((N + 7,), 9, dtype=torch.uint8, device=dev)[3 * off:3 * off + N]
        offset, src, totals = fresh(N, torch.int32), fresh(2 * N, torch.int32), fresh(4, torch.int32)
        scratch = torch.empty(L.fs_density_plan_scratch_bytes(N) + 16, dtype=torch.uint8, device=dev)[4 * off:]
        pd, md, vd = ([fresh(n_out * (t.numel() // N)) for t in raw] for _ in range(3))
        outs = [fresh(3 * n_out), fresh(n_out)]
        assert all(t.data_ptr() % 16 == 4 * off for t in ps + ms + vs + st + pd + md + vd + outs + [offset, src])
        tab = lambda ts: (C.c_void_p * 5)(*[t.data_ptr() for t in ts])
        _lib.check(L.fs_density_plan(N, *[p(t) for t in st], p(act[0]), p(act[1]), *[float(t) for t in TH], p(kind), p(offset), p(src),
                                     p(totals), p(scratch), _lib.current_stream()), "fs_density_plan")
        assert totals.tolist()[0] == n_out and np.array_equal(kind.cpu().numpy(), kind_want)
        _lib.check(L.fs_density_apply(N, M, n_out, p(src), tab(ps), tab(ms), tab(vs), tab(pd), tab(md), tab(vd), p(outs[0]),
                                      p(outs[1]), 6, _lib.current_stream()), "fs_density_apply")
        return [t.clone() for t in pd + md + vd + outs + [offset, src[:n_out]]]

    for a, b in zip(call(0), call(1)):
        assert torch.equal(a, b) and (a.dtype != torch.float32 or bool(torch.isfinite(a).all()))


def test_guard_bands(hip_device):
    """accumulate -> densify -> step -> reset_opacity with every allocation of the package inside guard bands and every input
    placed: nothing is written outside a block, and the result has the bits of the unguarded run, for all three fills."""
    case = _case(1031, 4, "pattern", 0)
    base = _sequence(case, hip_device)
    for fill in FILLS:
        with guarded(fill) as arena:
            got = _sequence(case, hip_device, place=arena.place)
            torch.cuda.synchronize()
            arena.check(f"density control, fill {fill}")
        assert len(arena.records) > 40
        _same(base, got, f"fill {fill}")


# ------------------------------------------------------------------------------------------------------------ end to end

def _scene(dev):
    """The 500-Gaussian 32 x 48 scene of tests/test_gaussian_adam_hip.py in (scales, rotations) form, and its rasterizer."""
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


def _render(rast, leaves, viewspace=None):
    m, s, q, o, sh = leaves
    color, radii, _, _ = rast(m, viewspace, o, shs=sh, scales=s, rotations=q)
    return color, radii


def test_refinement_loop_with_densification(hip_device):
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
        opt = GaussianAdam(m + rnd(m, 0.02), s * torch.exp(rnd(s, 0.3)), q, torch.sigmoid(logit + rnd(o, 1.0)), sh, sparse=True)

        def iterate():
            color, radii = _render(rast, opt.leaves(), opt.viewspace)
            loss = photometric_loss(color[None], target)
            loss.backward()
            opt.accumulate(radii)
            opt.step(radii)
            return float(loss.detach()), radii

        for _ in range(5):
            _, radii = iterate()
        seen = opt.denom > 0
        assert int(seen.sum()) >= 400 and int((~seen).sum()) >= 50 and float(opt.denom.max()) == 5.0
        assert bool(torch.isfinite(opt.grad_accum).all()) and bool((opt.grad_accum[seen] > 0).any()) and not bool(opt.grad_accum[~seen].any())
        assert bool((opt.max_radii[seen] > 0).all())
        avg = (opt.grad_accum / opt.denom)[seen]
        threshold = float(avg.median())
        dense = float(opt.scales.detach().max(1).values[seen].median())
        info = opt.densify(extent=1.0, grad_threshold=threshold, percent_dense=dense, min_opacity=0.005)
        print(f"densify at grad_threshold {threshold:.3e}, dense_scale {dense:.3e}: {info}")
        hot = int((avg >= threshold).sum())
        assert info["n_cloned"] > 0 and info["n_split"] > 0 and info["n_cloned"] + info["n_split"] <= hot + 2     # (+2: ties at the median)
        assert info["n_out"] == 500 + info["n_cloned"] + info["n_split"] - info["n_dropped"] != 500 and info["n_dropped"] < 250
        with torch.no_grad():
            color, radii = _render(rast, opt.leaves())
            after = float(photometric_loss(color[None], target))
        assert radii.shape[0] == info["n_out"] == opt.N and np.isfinite(after)
        for _ in range(10):
            loss, radii = iterate()
            assert np.isfinite(loss) and radii.shape[0] == info["n_out"]
        with torch.no_grad():
            final = float(photometric_loss(_render(rast, opt.leaves())[0][None], target))
        print(f"photometric loss right after the densify {after:.5f} -> {final:.5f} after ten more steps")
        assert final < after
        assert int(opt.step_count) == 15 and float(opt.denom.max()) == 10.0
    finally:
        rasterizer.DETERMINISTIC = saved
