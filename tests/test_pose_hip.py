"""GPU checks of the pose and transform gradients (include/freesplat_amd_pose.h, csrc/gaussian_pose.hip, freesplat_amd/pose.py,
the transform gradient of freesplat_amd/transform.py) against the float64 restatement tests/pose_ref.py: the reduction at a
derived fp64 bound, its bit-level properties, guard bands, transform_gaussians with a transform that requires grad, observe
(values, bits, graph capture) and the recovery of a perturbed camera.  Every case prints its worst error / bound ratio.

The bound of the reduction, for each of the 7 V outputs: |got - want| <= 4 n 2^-53 S, n the number of scalar summands behind the
output and S the sum of their absolute values, both from the restatement (pose_ref.tangent).  The kernel forms every product
exactly (fp32 x fp32 in fp64) or with one rounding (a third factor: 1/2, 2 or a generator), and adds the n terms in some fixed
order: at most n + 1 roundings of partial sums bounded by S, against the 4 n allowed."""
import math

import numpy as np
import pytest
import torch

import pose_ref as PR
import transform_cases as TC
import transform_ref as TR
from guarded_alloc import guarded
from test_transform_hip import _bounds as transform_bounds

pytestmark = pytest.mark.gpu
F64 = torch.float64
EPS = TC.EPS
KW = dict(means="means", scales="scales", rotations="rotations", cov="covariances", shs="harmonics")     # pose_ref name -> keyword


def _case(N, M, seed, cov_full, layout):
    """(values, gradients): float32 CPU dicts over pose_ref.ARRAYS."""
    a = TC.arrays(N, M, seed, cov_full, layout)
    g = TC.arrays(N, M, seed + 1000, cov_full, layout)
    g["scales"] = g["scales"] - 1.5                                         # (TC.arrays makes scales positive: both signs here)
    return a, g


def _call(dev, a, g, ids, V, quat_order, layout, which=PR.ARRAYS, place=lambda t: t):
    from freesplat_amd.pose import sim3_tangent
    kw = {KW[k]: place(a[k].to(dev)) for k in which if a.get(k) is not None}
    grads = {KW[k]: place(g[k].to(dev)) for k in which}
    return sim3_tangent(**kw, grads=grads, view_ids=None if ids is None else place(ids.to(dev)), rows=V, quat_order=quat_order,
                        sh_layout=layout)


def _ratio(got, want, bound):
    err = (got.detach().cpu().double() - want).abs()
    assert bool((err[bound == 0] == 0).all()), "an output without a summand must be exactly 0"
    return float((err / bound.clamp_min(1e-300)).max())


# ---- 1. the reduction against the restatement ---------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 65, 257, 1000])
@pytest.mark.parametrize("M", [1, 4, 9, 16])
def test_the_reduction_matches_the_restatement(hip_device, N, M):
    """All five arrays together, for both SH layouts x V in {1, 3} (ids with -1 and V; V = 1 once without ids), the quaternion
    order and the covariance form alternating."""
    worst = 0.0
    for i, layout in enumerate(("coeff_major", "channel_major")):
        for j, V in enumerate(TC.VS):
            seed = 10 * N + M + 2 * i + j
            quat_order, cov_full = ("wxyz", "xyzw")[(i + j) % 2], bool(i)
            ids = TC.ids_for(N, V, seed + i)
            a, g = _case(N, M, seed, cov_full, layout)
            got = _call(hip_device, a, g, ids, V, quat_order, layout)
            assert got.dtype == F64 and tuple(got.shape) == (V, 7)
            want, bound = PR.tangent(V, ids, a, g, quat_order, layout)
            worst = max(worst, _ratio(got, want, bound))
    print(f"N = {N}, M = {M}: worst error / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("which", PR.ARRAYS + ("g_means only",))
def test_each_array_alone(hip_device, which):
    """One (values, gradient) pair given, N = 257, M = 16, V = 3, both covariance forms: against the restatement of that pair
    alone; the gradient of the means without the means gives tau_u and exact zeros elsewhere."""
    N, M, V = 257, 16, 3
    ids = TC.ids_for(N, V, 3)
    worst = 0.0
    for cov_full in (False, True):
        a, g = _case(N, M, 3, cov_full, "channel_major")
        if which == "g_means only":
            a, keys = dict(a, means=None), ("means",)
        else:
            keys = (which,)
        got = _call(hip_device, a, g, ids, V, "xyzw", "channel_major", keys)
        want, bound = PR.tangent(V, ids, {k: a[k] for k in keys}, {k: g[k] for k in keys}, "xyzw", "channel_major")
        assert float(want.abs().max()) > 0
        worst = max(worst, _ratio(got, want, bound))
    print(f"{which}: worst error / bound {worst:.3f}")
    assert worst <= 1.0


# ---- 2. bit-level properties --------------------------------------------------------------------------------------------------

def _shifted(t, device):
    """A copy of t that starts one float past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 5, dtype=torch.float32, device=device)
    off = 1 + (-(buf.data_ptr() // 4) % 4)
    assert (buf.data_ptr() + 4 * off) % 16 == 4
    v = buf[off: off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("N", [1, 65, 257, 1000])
@pytest.mark.parametrize("M,layout", [(1, "coeff_major"), (4, "channel_major"), (9, "coeff_major"), (16, "coeff_major"), (16, "channel_major")])
def test_runs_alignments_streams_and_id_patterns_give_the_same_bits(hip_device, N, M, layout):
    """A second run, every float array one float past a 16-byte boundary (the dword path) and another stream give torch.equal
    outputs; relabelling the ids moves each row's bits with its Gaussians; a run on the Gaussians of one row alone (every other
    id out of range, V = 1) gives that row's bits."""
    V, cov_full, quat_order = 3, M != 9, "xyzw" if M == 4 else "wxyz"
    seed = N + M
    ids = TC.ids_for(N, V, seed)
    a, g = _case(N, M, seed, cov_full, layout)
    ref = _call(hip_device, a, g, ids, V, quat_order, layout)
    assert bool(torch.isfinite(ref).all())
    assert torch.equal(_call(hip_device, a, g, ids, V, quat_order, layout), ref), "a second run"
    shift = lambda t: _shifted(t, hip_device) if t.dtype == torch.float32 else t
    assert torch.equal(_call(hip_device, a, g, ids, V, quat_order, layout, place=shift), ref), "misaligned"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _call(hip_device, a, g, ids, V, quat_order, layout)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(other, ref), "another stream"
    inside = (ids >= 0) & (ids < V)
    moved = torch.where(inside, (ids + 1) % V, ids)
    got = _call(hip_device, a, g, moved, V, quat_order, layout)
    for v in range(V):
        assert torch.equal(got[(v + 1) % V], ref[v]), f"row {v} after relabelling"
        alone = _call(hip_device, a, g, torch.where(ids == v, 0, -1), 1, quat_order, layout)
        assert torch.equal(alone[0], ref[v]), f"row {v} alone"


# ---- 3. guard bands -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fill", ["ff", "garbage"])
@pytest.mark.parametrize("N,M", [(1, 16), (65, 9), (257, 16), (1000, 4)])
def test_nothing_is_written_outside_a_buffer(hip_device, fill, N, M):
    """sim3_tangent, transform_gaussians with a transform that requires grad (forward and backward) and observe's backward with
    every buffer the Python layer allocates (outputs, scratch) between guard bands and poisoned, inputs between NaN guards: no
    guard byte changes, no poison and no NaN reaches a result."""
    from freesplat_amd.pose import observe
    from freesplat_amd.transform import transform_gaussians
    V = 3
    ids = TC.ids_for(N, V, N)
    a, g = _case(N, M, N, True, "channel_major")
    with guarded(fill) as arena:
        got = _call(hip_device, a, g, ids, V, "wxyz", "channel_major", place=arena.place)
        torch.cuda.synchronize()
        arena.check("sim3_tangent")
        want, bound = PR.tangent(V, ids, a, g, "wxyz", "channel_major")
        assert _ratio(got, want, bound) <= 1.0
        d = {k: arena.place(v.to(hip_device)).requires_grad_(True) for k, v in a.items()}
        xf = arena.place(TC.transforms(V, N).to(hip_device)).requires_grad_(True)
        out = transform_gaussians(None, xf, means=d["means"], scales=d["scales"], rotations=d["rotations"], covariances=d["cov"],
                                  harmonics=d["shs"], view_ids=arena.place(ids.to(hip_device)))
        torch.autograd.backward(list(out), [arena.place(g[k].to(hip_device)) for k in PR.ARRAYS])
        E = arena.place(torch.eye(4, device=hip_device)).requires_grad_(True)
        seen = observe(E, means=d["means"], scales=d["scales"], rotations=d["rotations"], covariances=d["cov"], harmonics=d["shs"],
                       sh_layout="channel_major")
        torch.autograd.backward(list(seen), [arena.place(g[k].to(hip_device)) for k in PR.ARRAYS])
        torch.cuda.synchronize()
        arena.check("transform_gaussians with a transform gradient, observe")
        assert bool(torch.isfinite(xf.grad).all()) and bool(torch.isfinite(E.grad).all()) and float(xf.grad.abs().max()) > 0
        tau, _ = PR.tangent(1, None, a, g, "wxyz", "channel_major")
        assert float((E.grad.cpu().double()[:3, 3] + tau[0, :3]).abs().max()) <= 1e-5 * float(tau[0, :3].abs().max())


# ---- 4. the gradient of a transform -------------------------------------------------------------------------------------------

def _ambient_bound(s, R, b_tau, tau):
    """A bound b_tau on tau pushed through transform_ambient (linear, with |R| and |[.]x|), plus 4 x 2^-24 of the same map on
    |tau|: the table's s and R are fp32 roundings of the float64 ones the reference uses (one rounding each) and the result is
    rounded to fp32 once; margin 4 / 3."""
    from freesplat_amd.pose import transform_ambient

    def push(t):
        B = t[:, 6, None, None] / 3.0 * torch.eye(3, dtype=F64) + 0.5 * PR.skew(t[:, 3:6]).abs()
        return torch.cat([R.abs() @ B, (R.abs() @ t[:, :3, None])], 2) / s[:, None, None]

    return push(b_tau) + 4 * EPS * push(tau.abs()), transform_ambient((s, R), tau)


@pytest.mark.parametrize("form,V", [("matrix", 1), ("tuple", 3)])
def test_a_transform_that_requires_grad_receives_its_gradient(hip_device, form, V):
    """N = 257, M = 16, all five arrays (V = 3: ids with -1 and V).
    (a) every array gradient is torch.equal to the one the same call returns when the transform does not require grad;
    (b) the transform's gradient equals transform_ambient of the restatement's reduction over the inputs and the DEVICE's own
        input gradients, at the bound of the reduction pushed through transform_ambient (_ambient_bound);
    (c) it agrees with central differences of transform_ref.transform in float64 (h = 1e-5, as tests/test_pose_host.py): the
        device's input gradients are within test_transform_hip._bounds / TC.band_bound of the float64 ones, and those bounds
        pushed through the reduction (pose_ref.pushed), plus the reduction's own bound, plus 1e-8 |tau| for the differences' own
        truncation (the bound the host test holds them to), bound tau; then _ambient_bound.
    Tuple form (the reference takes the rows (s R | t) as fp32 forms them of the fp32 leaves): ds, dR, dt by autograd through xf = (s R | t) in fp32 -- dR = s G_A (one more rounding: + 2^-23 |dR|), dt = G_t,
    ds = sum G_A . R (nine fp32 terms: + gamma_10 sum |G_A| |R|)."""
    from freesplat_amd.pose import sim3_exp
    from freesplat_amd.transform import transform_gaussians
    N, M, layout, quat_order = 257, 16, "coeff_major", "wxyz"
    xf = TC.transforms(V, 40 + V)
    ids = TC.ids_for(N, V, 41)
    a, cot = _case(N, M, 42, False, layout)
    sf, Rf, tf = (x.float() for x in TR.split_xf(xf))                       # the leaves of the tuple form
    if form == "tuple":
        xf = torch.cat([sf[:, None, None] * Rf, tf[:, :, None]], 2)          # the rows the package forms of them, bit for bit
    s, R, t = TR.split_xf(xf)
    dev_ids = None if ids is None else ids.to(hip_device)

    def run(with_grad):
        d = {k: v.to(hip_device).requires_grad_(True) for k, v in a.items()}
        if form == "matrix":
            T = torch.eye(4, device=hip_device)
            T[:3] = xf[0].to(hip_device)
            leaves = [T.requires_grad_(with_grad)]
            transform = T
        else:
            leaves = [x.to(hip_device).requires_grad_(with_grad) for x in (sf, Rf, tf)]
            transform = tuple(leaves)
        out = transform_gaussians(None, transform, means=d["means"], scales=d["scales"], rotations=d["rotations"],
                                  covariances=d["cov"], harmonics=d["shs"], view_ids=dev_ids, quat_order=quat_order, sh_layout=layout)
        torch.autograd.backward(list(out), [cot[k].to(hip_device) for k in PR.ARRAYS])
        return out, {k: d[k].grad for k in PR.ARRAYS}, leaves

    out0, g0, leaves0 = run(False)
    out1, g1, leaves1 = run(True)
    for k, (x, y) in enumerate(zip(out0, out1)):
        assert torch.equal(x, y), PR.ARRAYS[k]
    for k in PR.ARRAYS:
        assert torch.equal(g0[k], g1[k]), k                                                     # (a)
    assert all(x.grad is None for x in leaves0)
    # (b)
    a64 = {k: v.double() for k, v in a.items()}
    g_dev = {k: v.cpu() for k, v in g1.items()}
    tau_b, b_b = PR.tangent(V, ids, a64, g_dev, quat_order, layout)
    bound_b, G_b = _ambient_bound(s, R, b_b, tau_b)
    # (c)
    c64 = {k: v.double() for k, v in cot.items()}

    def loss(T):
        o = TR.transform(T[:, :3], ids, a64["means"], a64["scales"], a64["rotations"], a64["cov"], a64["shs"], quat_order, layout)
        return sum((x * c64[k]).sum() for x, k in zip(o, PR.ARRAYS))

    T0 = torch.eye(4, dtype=F64).repeat(V, 1, 1)
    T0[:, :3] = torch.cat([s[:, None, None] * R, t[:, :, None]], 2)
    h, tau_c = 1e-5, torch.zeros(V, 7, dtype=F64)
    for v in range(V):
        for e in range(7):
            xi = torch.zeros(V, 7, dtype=F64)
            xi[v, e] = h
            tau_c[v, e] = (loss(T0 @ sim3_exp(xi)) - loss(T0 @ sim3_exp(-xi))) / (2 * h)
    per, on = transform_bounds(xf, ids, c64, quat_order, True)
    cm = c64["shs"]
    per["shs"] = torch.cat([torch.zeros(N, 1, 3, dtype=F64)] + [TC.band_bound(cm[:, l * l:(l + 1) ** 2], l).expand(N, 2 * l + 1, 3)
                                                                  for l in (1, 2, 3)], 1)
    b_c = PR.pushed(V, ids, a64, per, quat_order, layout) + b_b + 1e-8 * tau_c.abs()
    bound_c, G_c = _ambient_bound(s, R, b_c, tau_c)
    if form == "matrix":
        got = leaves1[0].grad.cpu().double()
        assert not bool(got[3].any())                                                           # the last row gets nothing
        checks = [("xf", got[None, :3], G_b, bound_b, G_c, bound_c)]
    else:
        gs, gR, gt = (x.grad.cpu().double() for x in leaves1)
        Rf, sf = Rf.double(), sf.double()
        to_s = lambda G, b: ((G[:, :, :3] * Rf).sum((1, 2)), (b[:, :, :3] * Rf.abs()).sum((1, 2)) + TC.gamma(10) * (G[:, :, :3] * Rf).abs().sum((1, 2)))
        to_R = lambda G, b: (sf[:, None, None] * G[:, :, :3], sf[:, None, None] * b[:, :, :3] + 2 * EPS * (sf[:, None, None] * G[:, :, :3]).abs())
        checks = [("s", gs, *to_s(G_b, bound_b), *to_s(G_c, bound_c)), ("R", gR, *to_R(G_b, bound_b), *to_R(G_c, bound_c)),
                  ("t", gt, G_b[:, :, 3], bound_b[:, :, 3], G_c[:, :, 3], bound_c[:, :, 3])]
    for name, got, want_b, bb, want_c, bc in checks:
        rb = float(((got - want_b).abs() / bb.clamp_min(1e-300)).max())
        rc = float(((got - want_c).abs() / bc.clamp_min(1e-300)).max())
        print(f"{form} d{name}: error / bound against the restatement on the device's gradients {rb:.3f}, against central differences {rc:.3f}")
        assert float(want_c.abs().max()) > 0 and rb <= 1.0 and rc <= 1.0, name


# ---- 5. observe ---------------------------------------------------------------------------------------------------------------

def _optimizer(sc, device):
    from freesplat_amd.refine import GaussianAdam
    return GaussianAdam(sc["means"].to(device), sc["scales"].to(device), sc["rotations"].to(device), sc["opacities"].to(device),
                        sc["shs"].to(device))


def _render(arrays, sc, c2w, device, H=64, W=80):
    """Colour [3, H, W] and depth [H, W] of (means, scales, rotations, opacities, shs) from the camera c2w (a CPU matrix)."""
    from freesplat_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    view, proj, campos, tx, ty = TC.camera_matrices(c2w.detach().cpu().double(), sc["near"], sc["far"])
    d = lambda x: x.float().to(device)
    st = GaussianRasterizationSettings(H, W, tx, ty, torch.tensor([0.2, 0.3, 0.1], device=device), 1.0, d(view), d(proj),
                                       sc["sh_degree"], d(campos), False, False)
    means, scales, rotations, opacities, shs = arrays
    out = GaussianRasterizer(st)(means3D=means, means2D=torch.zeros_like(means), opacities=opacities, shs=shs, scales=scales,
                                 rotations=rotations)
    return out[0], out[2].reshape(H, W)


def _camera_bound(E, b_tau, tau):
    """A bound on tau pushed through camera_ambient, plus 2^-23 of the same map on |tau| for the rounding of the result to fp32."""
    def push(x):
        G = torch.zeros(4, 4, dtype=F64)
        tE = E[:3, 3].abs()
        cross = torch.stack([tE[1] * x[2] + tE[2] * x[1], tE[2] * x[0] + tE[0] * x[2], tE[0] * x[1] + tE[1] * x[0]])
        G[:3, :3] = 0.5 * PR.skew(x[3:6] + cross).abs() @ E[:3, :3].abs()
        G[:3, 3] = x[:3]
        return G
    return push(b_tau) + 2 * EPS * push(tau.abs())


def test_observe_passes_gradients_through_and_gives_the_camera_its_own(hip_device, monkeypatch):
    """64 x 80, 600 Gaussians, degree 3, a loss with random weights on colour and depth, the rasterizer's backward in its
    deterministic mode (two backward passes of the default mode differ in their bits with or without observe): the leaves'
    gradients are torch.equal to those of a render without observe; extrinsics.grad equals camera_ambient of the restatement's
    reduction of those gradients at the reduction's bound pushed through camera_ambient; its last row is zero."""
    from freesplat_amd import rasterizer
    from freesplat_amd.pose import camera_ambient
    monkeypatch.setattr(rasterizer, "DETERMINISTIC", True)
    sc = TC.render_scene()
    H, W = 64, 80
    g = torch.Generator().manual_seed(50)
    wc, wd = torch.randn(3, H, W, generator=g).to(hip_device), (torch.randn(H, W, generator=g) / 4.0).to(hip_device)
    grads = []
    for observed in (False, True):
        opt = _optimizer(sc, hip_device)
        E = sc["c2w"].float().to(hip_device).requires_grad_(True)
        arrays = opt.observed(E) if observed else opt.leaves()
        assert arrays[3] is opt.opacities
        color, depth = _render(arrays, sc, E, hip_device)
        ((color * wc).sum() + (depth * wd).sum()).backward()
        grads.append([leaf.grad.clone() for leaf in opt.leaves()])
        if not observed:
            assert E.grad is None
    for x, y, name in zip(grads[0], grads[1], ("means", "scales", "rotations", "opacities", "shs")):
        assert torch.equal(x, y), name
    gm, gs, gq, _, gsh = (x.cpu() for x in grads[1])
    vals = dict(means=sc["means"], scales=opt.scales.detach().cpu(), rotations=sc["rotations"], shs=sc["shs"])
    tau, b = PR.tangent(1, None, vals, dict(means=gm, scales=gs, rotations=gq, shs=gsh))
    Ec = sc["c2w"].float().double()
    want = camera_ambient(Ec, tau[0])
    bound = _camera_bound(Ec, b[0], tau[0])
    got = E.grad.cpu().double()
    assert not bool(got[3].any()) and float(want.abs().max()) > 0
    ratio = float(((got - want).abs()[:3] / bound[:3].clamp_min(1e-300)).max())
    print(f"observe: extrinsics.grad worst error / bound {ratio:.3f}")
    assert ratio <= 1.0


def test_observe_is_capturable(hip_device):
    """observe and its backward (the reduction's two launches and the closed form) captured in a graph and replayed on new
    inputs: the bits of the eager call."""
    from freesplat_amd.pose import observe
    N, M = 257, 16
    a1, g1 = _case(N, M, 1, False, "coeff_major")
    a2, g2 = _case(N, M, 2, False, "coeff_major")
    dev = lambda d: {k: v.to(hip_device) for k, v in d.items()}

    def run(a, g, E):
        a = {k: v.detach().requires_grad_(True) for k, v in a.items()}
        E = E.detach().requires_grad_(True)
        out = observe(E, means=a["means"], scales=a["scales"], rotations=a["rotations"], covariances=a["cov"], harmonics=a["shs"])
        return torch.autograd.grad(list(out), [E] + [a[k] for k in PR.ARRAYS], [g[k] for k in PR.ARRAYS])

    E1, E2 = torch.eye(4, device=hip_device), torch.eye(4, device=hip_device)
    E1[:3], E2[:3] = TC.transforms(1, 4)[0].to(hip_device), TC.transforms(1, 5)[0].to(hip_device)
    want = run(dev(a2), dev(g2), E2)
    sa, sg, sE = dev(a1), dev(g1), E1.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(sa, sg, sE)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(sa, sg, sE)
    for k in sa:
        sa[k].copy_(a2[k])
        sg[k].copy_(g2[k])
    sE.copy_(E2)
    graph.replay()
    torch.cuda.synchronize()
    assert float(want[0].abs().max()) > 0
    for o, w in zip(out, want):
        assert torch.equal(o, w)
    graph.replay()
    torch.cuda.synchronize()
    for o, w in zip(out, want):
        assert torch.equal(o, w)


# ---- 6. pose recovery ---------------------------------------------------------------------------------------------------------

def pose_error(E, E_true, points):
    """Mean distance between the scene's points as the two cameras see them (camera frames), in scene units."""
    a = (points - E[:3, 3]) @ E[:3, :3]
    b = (points - E_true[:3, 3]) @ E_true[:3, :3]
    return float((a - b).norm(dim=1).mean())


def perturbed_camera(c2w, depth, seed=3):
    """c2w turned by 0.5 degrees about a random axis and moved by 0.5 % of the scene depth in a random direction."""
    g = torch.Generator().manual_seed(seed)
    ax, dr = torch.randn(3, dtype=F64, generator=g), torch.randn(3, dtype=F64, generator=g)
    xi = torch.cat([0.005 * depth * dr / dr.norm(), math.radians(0.5) * ax / ax.norm(), torch.zeros(1, dtype=F64)])
    return c2w.double() @ torch.linalg.matrix_exp(PR.hat(xi))


POSE_LR, POSE_STEPS = 1e-3, 100


def test_a_perturbed_camera_is_recovered(hip_device):
    """TC.render_scene (64 x 80, 600 Gaussians, depth 4): one camera turned by 0.5 degrees and moved by 0.5 % of the depth, 100
    Adam steps (lr 1e-3) on Poses.delta against the image rendered from the true pose, the Gaussians fixed.  The final loss is
    below half the initial loss and the final pose error (pose_error) below half the initial one.

    The same loop in float64 on the host (oracle.raster_dense_torch.render_dense at 24 x 32 with the C oracle's discrete inputs
    per step, autograd through the camera matrices, the same perturbation, lr and steps) took the loss from 9.35e-4 to 9.80e-7
    (ratio 0.001) and the pose error from 3.92e-2 to 2.48e-3 (ratio 0.063): the reference meets both factors with room."""
    from freesplat_amd.pose import Poses
    sc = TC.render_scene()
    opt = _optimizer(sc, hip_device)
    E_true = sc["c2w"].double()
    with torch.no_grad():
        target, _ = _render(opt.leaves(), sc, E_true, hip_device)
    poses = Poses(perturbed_camera(E_true, 4.0)[None].float().to(hip_device))
    adam = torch.optim.Adam([poses.delta], lr=POSE_LR)
    points = sc["means"].double()
    first = last = None
    err0 = pose_error(poses.matrices()[0].detach().cpu().double(), E_true, points)
    for step in range(POSE_STEPS):
        adam.zero_grad()
        E = poses.matrices()[0]
        color, _ = _render(opt.observed(E), sc, E, hip_device)
        loss = ((color - target) ** 2).mean()
        loss.backward()
        adam.step()
        opt.zero_grad()
        first = loss.detach() if first is None else first
    with torch.no_grad():
        E = poses.matrices()[0]
        last = ((_render(opt.leaves(), sc, E, hip_device)[0] - target) ** 2).mean()
    err1 = pose_error(E.cpu().double(), E_true, points)
    first, last = float(first), float(last)
    print(f"pose recovery: loss {first:.3e} -> {last:.3e} (ratio / bound {last / (0.5 * first):.3f}), pose error {err0:.3e} -> {err1:.3e} "
          f"(ratio / bound {err1 / (0.5 * err0):.3f})")
    assert first > 0 and last < 0.5 * first and err1 < 0.5 * err0
