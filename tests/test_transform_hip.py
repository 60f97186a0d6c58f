"""GPU checks of the similarity transform of Gaussians (include/freesplat_amd_transform.h, csrc/gaussian_transform.hip,
freesplat_amd/transform.py) against the float64 restatement tests/transform_ref.py: the table, forward and backward at
first-order fp32 bounds, the bit-level properties (pass-through, in place, alignment, repeatability), guard bands, graph
capture, GaussianAdam.transform_ and the adapter's coords=None path.  Every case prints its worst error / bound ratio."""
import numpy as np
import pytest
import torch

import transform_cases as TC
import transform_ref as TR
from guarded_alloc import guarded

pytestmark = pytest.mark.gpu
F64 = torch.float64
EPS = TC.EPS
g_ = TC.gamma


def _lib():
    from freesplat_amd import _lib as L
    return L


def _raw(which, N, M, V, flags, table, ids, ins, outs):
    L = _lib()
    p = L.ptr
    L.check(getattr(L.lib(), "fs_gaussians_transform_" + which)(N, M, V, flags, p(table), p(ids), *[p(a) for a in ins],
                                                               *[p(a) for a in outs], L.current_stream()), which)


def _rot_raw(N, M, V, flags, sh, table, ids, out):
    L = _lib()
    p = L.ptr
    L.check(L.lib().fs_sh_rotate(N, M, V, flags, p(sh), p(table), p(ids), p(out), L.current_stream()), "fs_sh_rotate")


def _flags(cov_full, sh_layout, quat_order):
    L = _lib()
    return ((L.TRANSFORM_COV_FULL if cov_full else 0) | (L.TRANSFORM_SH_CHANNEL_MAJOR if sh_layout == "channel_major" else 0)
            | (L.TRANSFORM_QUAT_XYZW if quat_order == "xyzw" else 0))


ORDER = ("means", "scales", "rotations", "cov", "shs")


# ---- 1. the table -------------------------------------------------------------------------------------------------------------

def test_the_table_is_the_float64_table_rounded_once(hip_device):
    """Entrywise |got - want| <= 2^-23 |want| + 1e-12 max(1, s, |t|): one rounding of an fp64 result (2^-24 relative) with margin 2.
    The absolute term is the fp64 derivations' own error (the kernel sums a 26-node quadrature, the restatement solves a
    least-squares system; both are accurate to about 1e-15 of an entry of an orthogonal matrix), five orders below fp32's
    roundoff.  Rotations: random ones (one of them by more than pi about its axis, so the sign choice of q is taken), the
    identity, a quarter turn about z (exact zeros and ones), and a rotation by 179 degrees (the branch of q where w is small)."""
    from freesplat_amd.transform import prepare_table
    xf = TC.transforms(5, seed=1)
    xf[3] = torch.tensor([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]])
    xf[4] = torch.tensor([[0.0, -2, 0, 1], [2, 0, 0, -1], [0, 0, 2, 0.5]])
    a = np.deg2rad(179.0)
    ax = torch.tensor([1.0, 2.0, -2.0], dtype=F64) / 3.0
    K = torch.tensor([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]], dtype=F64)
    xf = torch.cat([xf, torch.cat([0.7 * (torch.eye(3, dtype=F64) + np.sin(a) * K + (1 - np.cos(a)) * K @ K), torch.ones(3, 1, dtype=F64)], 1)[None].float()])
    want = TR.table(xf)
    got = prepare_table(xf.to(hip_device)).cpu()
    assert got.dtype == torch.float32 and tuple(got.shape) == (6, TR.TABLE_FLOATS)
    scale = torch.maximum(want[:, :1].abs(), want[:, 10:13].abs().amax(1, keepdim=True)).clamp_min(1.0)
    bound = 2.0 ** -23 * want.abs() + 1e-12 * scale
    ratio = float(((got.double() - want).abs() / bound).max())
    print(f"table: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0
    assert bool((got[:, 13] >= 0).all()) and float((got[:, 13:17].double().norm(dim=1) - 1).abs().max()) <= 2 * EPS
    assert torch.equal(got[:, 10:13], xf[:, :, 3])                          # t is copied


# ---- 2. forward and backward against the restatement --------------------------------------------------------------------------

def _abs_quat_terms(p, g):
    """sum of |terms| of each component of the Hamilton product (w, x, y, z)."""
    pw, px, py, pz = p.abs().unbind(-1)
    gw, gx, gy, gz = g.abs().unbind(-1)
    return torch.stack([pw * gw + px * gx + py * gy + pz * gz, pw * gx + px * gw + py * gz + pz * gy,
                        pw * gy + px * gz + py * gw + pz * gx, pw * gz + px * gy + py * gx + pz * gw], -1)


def _bounds(xf, ids, a, quat_order, backward):
    """First-order fp32 bounds of the five results for inputs `a` (float64 views of the fp32 inputs or cotangents), margin 2:
      means      2 gamma_6 (s (|R| |m|)_i + |t_i|): R rounded, a 3-term fma dot product, s rounded, the last fma (backward: no t)
      scales     2 gamma_2 |s x|: s rounded, one product
      rotations  2 gamma_5 sum |p_k g_k|: q_R rounded, a 4-term fma dot product
      cov        2 gamma_12 s^2 (|R| |S| |R|^T)_ij: two 3-term products with R rounded in each, s rounded twice, s * s, the product
                 (six-entry backward: on |K|, the off-diagonal results doubled)
      shs        2 (2l + 3) 2^-24 |c_l|_2 per band: 2l + 1 fmas and the rounding of D, against rows of an orthogonal matrix"""
    s, R, t = TR.split_xf(xf)
    V = xf.shape[0]
    N = next(v.shape[0] for v in a.values() if v is not None)
    ids_, on = TR._resolve(ids, N, V)
    k = ids_.clamp(0, V - 1)
    s, R, t = s[k], (R[k].transpose(1, 2) if backward else R[k]).abs(), t[k]
    out = {}
    if a.get("means") is not None:
        out["means"] = 2 * g_(6) * (s[:, None] * torch.einsum("nij,nj->ni", R, a["means"].abs()) + (0 if backward else t.abs()))
    if a.get("scales") is not None:
        out["scales"] = 2 * g_(2) * (s[:, None] * a["scales"]).abs()
    if a.get("rotations") is not None:
        q = a["rotations"] if quat_order == "wxyz" else a["rotations"][:, [3, 0, 1, 2]]
        qr = torch.stack([TR.matrix_to_quat(r) for r in TR.split_xf(xf)[1]])[k]
        b = 2 * g_(5) * _abs_quat_terms(qr, q)
        out["rotations"] = b if quat_order == "wxyz" else b[:, [1, 2, 3, 0]]
    if a.get("cov") is not None:
        c = a["cov"].abs()
        if c.dim() == 3:
            out["cov"] = 2 * g_(12) * (s ** 2)[:, None, None] * (R @ c @ R.transpose(1, 2))
        else:
            half = torch.tensor([1, 0.5, 0.5, 1, 0.5, 1], dtype=F64) if backward else torch.ones(6, dtype=F64)
            W = (s ** 2)[:, None, None] * (R @ TR.cov6_to_mat(c * half) @ R.transpose(1, 2))
            out["cov"] = 2 * g_(12) * TR.mat_to_cov6(W) / half
    return out, on


def _check(name, got, want, bound, on, src, ratios):
    got, want = got.detach().cpu(), want.detach()
    assert torch.equal(got[~on], src[~on]), f"{name}: a passed-through row is not bit-identical"
    r = ((got.double() - want).abs() / bound.clamp_min(1e-300))[on]
    r = float(r.max()) if r.numel() else 0.0
    ratios[name] = max(ratios.get(name, 0.0), r)
    assert r <= 1.0, f"{name}: error / bound {r}"


def _sh_check(name, got, want, src64, layout, on, src, ratios):
    got, want = got.detach().cpu(), want.detach()
    assert torch.equal(got[~on], src[~on]), f"{name}: a passed-through row is not bit-identical"
    cm = (lambda x: x) if layout == "coeff_major" else (lambda x: x.transpose(1, 2))
    g, w, c = cm(got.double()), cm(want), cm(src64)
    assert torch.equal(cm(got)[:, 0], cm(src)[:, 0])                        # band 0 is copied
    for l in range(1, int(round(c.shape[1] ** 0.5))):
        b = slice(l * l, (l + 1) * (l + 1))
        r = ((g[:, b] - w[:, b]).abs() / TC.band_bound(c[:, b], l).clamp_min(1e-300))[on]
        r = float(r.max()) if r.numel() else 0.0
        ratios[f"{name} l={l}"] = max(ratios.get(f"{name} l={l}", 0.0), r)
        assert r <= 1.0, f"{name} band {l}: error / bound {r}"


@pytest.mark.parametrize("N", TC.NS)
@pytest.mark.parametrize("M", TC.MS)
def test_forward_and_backward_match_the_restatement(hip_device, N, M):
    """All five arrays together through transform_gaussians and its autograd, for both SH layouts x V in {1, 3} (ids with -1 and
    V; V = 1 once without ids), the quaternion order and the covariance form alternating: against tests/transform_ref.py in
    float64 and torch.autograd of it, at the bounds of _bounds."""
    from freesplat_amd.transform import transform_gaussians
    ratios = {}
    for i, layout in enumerate(("coeff_major", "channel_major")):
        for j, V in enumerate(TC.VS):
            seed = 10 * N + M + 2 * i + j
            quat_order, cov_full = ("wxyz", "xyzw")[(i + j) % 2], bool(i)
            xf, ids = TC.transforms(V, seed), TC.ids_for(N, V, seed + i)
            a = TC.arrays(N, M, seed, cov_full, layout)
            dev = {k: v.to(hip_device).requires_grad_(True) for k, v in a.items()}
            got = transform_gaussians(None, xf.to(hip_device), means=dev["means"], scales=dev["scales"], rotations=dev["rotations"],
                                      covariances=dev["cov"], harmonics=dev["shs"], view_ids=None if ids is None else ids.to(hip_device),
                                      quat_order=quat_order, sh_layout=layout)
            a64 = {k: v.double().requires_grad_(True) for k, v in a.items()}
            want = TR.transform(xf, ids, a64["means"], a64["scales"], a64["rotations"], a64["cov"], a64["shs"], quat_order, layout)
            bounds, on = _bounds(xf, ids, {k: v.detach() for k, v in a64.items()}, quat_order, False)
            for k, name in enumerate(ORDER[:4]):
                _check("fwd " + name, got[k], want[k], bounds[name], on, a[name], ratios)
            _sh_check("fwd shs", got[4], want[4], a64["shs"].detach(), layout, on, a["shs"], ratios)
            cot = {k: torch.randn(v.shape, generator=torch.Generator().manual_seed(seed + 7)) for k, v in a.items()}
            torch.autograd.backward(list(got), [cot[k].to(hip_device) for k in ORDER])
            torch.autograd.backward(want, [cot[k].double() for k in ORDER])
            c64 = {k: v.double() for k, v in cot.items()}
            bounds, on = _bounds(xf, ids, c64, quat_order, True)
            for name in ORDER[:4]:
                _check("bwd " + name, dev[name].grad, a64[name].grad, bounds[name], on, cot[name], ratios)
            _sh_check("bwd shs", dev["shs"].grad, a64["shs"].grad, c64["shs"], layout, on, cot["shs"], ratios)
    print(f"N = {N}, M = {M}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(ratios.items())))


@pytest.mark.parametrize("which", ORDER)
def test_each_array_alone(hip_device, which):
    """One array given, the other four None, forward and backward: the same bits as with all five together."""
    from freesplat_amd.transform import transform_gaussians
    N, M, V = 257, 16, 3
    xf, ids = TC.transforms(V, 3).to(hip_device), TC.ids_for(N, V, 3).to(hip_device)
    a = {k: v.to(hip_device) for k, v in TC.arrays(N, M, 3, True, "channel_major").items()}
    kw = lambda d: dict(means=d.get("means"), scales=d.get("scales"), rotations=d.get("rotations"), covariances=d.get("cov"),
                        harmonics=d.get("shs"), view_ids=ids)
    full = {k: v.clone().requires_grad_(True) for k, v in a.items()}
    out_full = transform_gaussians(None, xf, **kw(full))
    cot = torch.randn(a[which].shape, device=hip_device, generator=torch.Generator(hip_device).manual_seed(5))
    k = ORDER.index(which)
    out_full[k].backward(cot)
    one = a[which].clone().requires_grad_(True)
    out = transform_gaussians(None, xf, **kw({which: one}))
    assert [o is None for o in out] == [n != which for n in ORDER]
    out[k].backward(cot)
    assert torch.equal(out[k], out_full[k]) and torch.equal(one.grad, full[which].grad)
    assert not torch.equal(out[k], a[which])


# ---- 3. bit-level properties --------------------------------------------------------------------------------------------------

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
def test_in_place_alignment_and_repeats_give_the_same_bits(hip_device, N, M, layout):
    """Through the C entry points, forward and backward: out == in (in place), every array one float past a 16-byte boundary
    (the dword path), and a second run all give the bits of the aligned out-of-place run; fs_sh_rotate alone agrees with the
    harmonics of the fused call; D^T after D returns the harmonics within twice the band bound."""
    from freesplat_amd.transform import prepare_table
    V, cov_full, quat_order = 3, M != 9, "xyzw" if M == 4 else "wxyz"
    seed = N + M
    table = prepare_table(TC.transforms(V, seed).to(hip_device))
    ids = TC.ids_for(N, V, seed).to(hip_device)
    a = TC.arrays(N, M, seed, cov_full, layout)
    ins = [a[k].to(hip_device) for k in ORDER]
    flags = _flags(cov_full, layout, quat_order)
    L = _lib()
    for which in ("forward", "backward"):
        ref = [torch.full_like(t, float("nan")) for t in ins]
        _raw(which, N, M, V, flags, table, ids, ins, ref)
        assert all(bool(torch.isfinite(t).all()) for t in ref)
        again = [torch.empty_like(t) for t in ins]
        _raw(which, N, M, V, flags, table, ids, ins, again)
        inplace = [t.clone() for t in ins]
        _raw(which, N, M, V, flags, table, ids, inplace, inplace)
        sh_in = [_shifted(t, hip_device) for t in ins]
        sh_out = [_shifted(torch.zeros_like(t), hip_device) for t in ins]
        _raw(which, N, M, V, flags, table, ids, sh_in, sh_out)
        sh_inplace = [_shifted(t, hip_device) for t in ins]
        _raw(which, N, M, V, flags, table, ids, sh_inplace, sh_inplace)
        for k, name in enumerate(ORDER):
            for label, other in (("a second run", again), ("in place", inplace), ("misaligned", sh_out), ("misaligned in place", sh_inplace)):
                assert torch.equal(other[k], ref[k]), f"{which} {name}: {label} differs from the aligned out-of-place run"
        sh_flags = (flags & L.TRANSFORM_SH_CHANNEL_MAJOR) | (L.TRANSFORM_SH_TRANSPOSE if which == "backward" else 0)
        alone = torch.empty_like(ins[4])
        _rot_raw(N, M, V, sh_flags, ins[4], table, ids, alone)
        assert torch.equal(alone, ref[4])
        if which == "forward" and M > 1:
            back = torch.empty_like(alone)
            _rot_raw(N, M, V, sh_flags | L.TRANSFORM_SH_TRANSPOSE, alone, table, ids, back)
            cm = (lambda x: x) if layout == "coeff_major" else (lambda x: x.transpose(1, 2))
            c, b = cm(a["shs"].double()), cm(back.cpu().double())
            for l in range(1, int(round(M ** 0.5))):
                sl = slice(l * l, (l + 1) * (l + 1))
                r = float(((b[:, sl] - c[:, sl]).abs() / (2 * TC.band_bound(c[:, sl], l)).clamp_min(1e-300)).max())
                assert r <= 1.0, f"D^T D c, band {l}: error / (2 x bound) {r}"
            assert not torch.equal(alone, ins[4])


# ---- 4. guard bands -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fill", ["ff", "garbage"])
@pytest.mark.parametrize("N,M", [(1, 16), (65, 9), (257, 16), (1000, 4)])
def test_no_entry_point_writes_outside_its_buffers(hip_device, fill, N, M):
    """fs_transform_prepare, fs_gaussians_transform_forward / _backward and fs_sh_rotate with every buffer the Python layer
    allocates between guard bands and poisoned, inputs placed between NaN guards: no guard byte changes, no poison and no NaN
    reaches a result.  Then the C calls with arrays skipped (NULL in): their poisoned outputs keep every bit."""
    from freesplat_amd.transform import prepare_table, rotate_sh, transform_gaussians
    V = 3
    a = TC.arrays(N, M, N, True, "channel_major")
    xf, ids = TC.transforms(V, N), TC.ids_for(N, V, N)
    with guarded(fill) as arena:
        d = {k: arena.place(v.to(hip_device)).requires_grad_(True) for k, v in a.items()}
        out = transform_gaussians(None, arena.place(xf.to(hip_device)), means=d["means"], scales=d["scales"], rotations=d["rotations"],
                                  covariances=d["cov"], harmonics=d["shs"], view_ids=arena.place(ids.to(hip_device)))
        torch.autograd.backward(list(out), [arena.place(torch.ones_like(o)) for o in out])
        rot = rotate_sh(d["shs"], arena.place(TR.split_xf(xf)[1].float().to(hip_device)), arena.place(ids.to(hip_device)))
        torch.cuda.synchronize()
        arena.check("transform_gaussians + backward + rotate_sh")
        want = TR.transform(xf, ids, *[a[k].double() for k in ORDER], "wxyz", "channel_major")
        for k, name in enumerate(ORDER):
            assert bool(torch.isfinite(out[k]).all()) and bool(torch.isfinite(d[name].grad).all()), name
            assert float((out[k].detach().cpu().double() - want[k]).abs().max()) <= 1e-4 * float(want[k].abs().max()), name
        assert bool(torch.isfinite(rot).all())
        # arrays skipped: NULL in, a poisoned buffer as out
        table = prepare_table(xf.to(hip_device))
        ins = [d[k].detach() for k in ORDER]
        for keep in range(5):
            outs = [torch.empty_like(t) for t in ins]                       # (guarded, filled with the poison)
            before = [o.clone() for o in outs]
            for which in ("forward", "backward"):
                _raw(which, N, M, V, _flags(True, "channel_major", "wxyz"), table, ids.to(hip_device),
                     [t if k == keep else None for k, t in enumerate(ins)], outs)
                torch.cuda.synchronize()
                for k in range(5):
                    same = torch.equal(outs[k].view(torch.int32), before[k].view(torch.int32))
                    assert same == (k != keep), (which, ORDER[keep], ORDER[k])
        arena.check("calls with skipped arrays")


# ---- 5. graph capture ---------------------------------------------------------------------------------------------------------

def test_transform_gaussians_is_capturable(hip_device):
    """One linear capture of the table launch and both kernels (a device transform: nothing is read on the host), replayed on
    new inputs: the bits of the eager call."""
    from freesplat_amd.transform import transform_gaussians
    N, M = 257, 16
    a = {k: v.to(hip_device) for k, v in TC.arrays(N, M, 1, False, "coeff_major").items()}
    b = {k: v.to(hip_device) for k, v in TC.arrays(N, M, 2, False, "coeff_major").items()}
    xf = torch.eye(4, device=hip_device)
    xf[:3] = TC.transforms(1, 4)[0].to(hip_device)
    xf2 = torch.eye(4, device=hip_device)
    xf2[:3] = TC.transforms(1, 5)[0].to(hip_device)
    call = lambda d, T: transform_gaussians(None, T, means=d["means"], scales=d["scales"], rotations=d["rotations"],
                                            covariances=d["cov"], harmonics=d["shs"], sh_layout="coeff_major")
    want = call(b, xf2)
    static = {k: v.clone() for k, v in a.items()}
    static_T = xf.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(static, static_T)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(static, static_T)
    for k in static:
        static[k].copy_(b[k])
    static_T.copy_(xf2)
    graph.replay()
    torch.cuda.synchronize()
    for o, w in zip(out, want):
        assert torch.equal(o, w)


# ---- 6. GaussianAdam.transform_ -----------------------------------------------------------------------------------------------

def _optimizer(sc, device, **kw):
    from freesplat_amd.refine import GaussianAdam
    return GaussianAdam(sc["means"].to(device), sc["scales"].to(device), sc["rotations"].to(device), sc["opacities"].to(device),
                        sc["shs"].to(device), **kw)


def test_adam_transform_leaves_a_fresh_optimizer(hip_device):
    """After transform_(): raw parameters are the transformed ones (within the forward bounds; log-scales + log s), moments, step
    counter and density statistics are zero, the leaves are the same tensors.  Then against a fresh optimizer loaded with the
    same raw values: one identical step() leaves every state entry bit-identical."""
    from freesplat_amd.refine import GaussianAdam
    sc = TC.render_scene(N=257, seed=21, sh_degree=2)
    opt = _optimizer(sc, hip_device)
    g = torch.Generator().manual_seed(3)
    grads = [torch.randn(t.shape, generator=g) * 1e-2 for t in opt.leaves()]
    for leaf, gr in zip(opt.leaves(), grads):
        leaf.grad = gr.to(hip_device)
    opt.step()
    opt.grad_accum.add_(1.0)
    opt.denom.add_(2.0)
    opt.max_radii.add_(3.0)
    before = opt.state_dict()
    leaves = opt.leaves()
    xf = TC.transforms(1, 8)
    T = torch.eye(4)
    T[:3] = xf[0]
    opt.transform_(T)
    assert all(x is y for x, y in zip(leaves, opt.leaves()))
    sd = opt.state_dict()
    s, R, t = TR.split_xf(xf)
    want = TR.transform(xf, None, before["means"].cpu(), None, before["rotations"].cpu(), None, before["shs"].cpu())
    a64 = dict(means=before["means"].cpu().double(), rotations=before["rotations"].cpu().double())
    bounds, on = _bounds(xf, None, a64, "wxyz", False)
    ratios = {}
    _check("means", sd["means"], want[0], bounds["means"], on, before["means"].cpu(), ratios)
    _check("rotations", sd["rotations"], want[2], bounds["rotations"], on, before["rotations"].cpu(), ratios)
    _sh_check("shs", sd["shs"], want[4], before["shs"].cpu().double(), "coeff_major", on, before["shs"].cpu(), ratios)
    want_ls = before["log_scales"].cpu().double() + torch.log(s)
    err = (sd["log_scales"].cpu().double() - want_ls).abs()
    assert bool((err <= 2 * EPS * (want_ls.abs() + abs(float(torch.log(s))))).all())      # log(fp32 s) and one fp32 add, margin 2
    assert torch.equal(sd["logits"], before["logits"])
    assert float((opt.scales.detach() / torch.exp(sd["log_scales"]) - 1).abs().max()) <= 4 * EPS          # the leaves are rewritten
    for k, v in sd.items():
        if k.startswith(("exp_avg", "density.")) or k == "step":
            assert not bool(v.any()), k
    assert all(leaf.grad is None for leaf in opt.leaves()) and opt.viewspace.grad is None
    fresh = GaussianAdam(sd["means"], opt.scales.detach(), sd["rotations"], opt.opacities.detach(), sd["shs"])
    fsd = fresh.state_dict()
    fsd.update({k: sd[k] for k in ("means", "log_scales", "rotations", "logits", "shs")})
    fresh.load_state_dict(fsd)
    for o in (opt, fresh):
        for leaf, gr in zip(o.leaves(), grads):
            leaf.grad = gr.to(hip_device)
        o.step()
    a, b = opt.state_dict(), fresh.state_dict()
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k], b[k]), k
    for x, y in zip(opt.leaves(), fresh.leaves()):
        assert torch.equal(x.detach(), y.detach())
    assert int(a["step"]) == 1


def _hip_render(opt, sc, c2w, device, H=64, W=80):
    from freesplat_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    view, proj, campos, tx, ty = TC.camera_matrices(c2w, sc["near"], sc["far"])
    d = lambda x: x.float().to(device)
    st = GaussianRasterizationSettings(H, W, tx, ty, torch.tensor([0.2, 0.3, 0.1], device=device), 1.0, d(view), d(proj),
                                       sc["sh_degree"], d(campos), False, False)
    with torch.no_grad():
        out = GaussianRasterizer(st)(means3D=opt.means, means2D=torch.zeros_like(opt.means), opacities=opt.opacities, shs=opt.shs,
                                     scales=opt.scales, rotations=opt.rotations)
    return out[0].cpu().numpy(), out[2].cpu().numpy().reshape(H, W)


def test_adam_transform_renders_the_same_image_from_the_transformed_camera(hip_device):
    """64 x 80, 600 Gaussians, degree 3, s = 1.6: the HIP render of the transformed optimizer from transform_cameras(...) against
    the HIP render before.  Pixels within reach of a discrete flip are excluded, and the CPU oracle alone says which: it renders
    the scene and its float64-transformed, fp32-rounded twin, and a pixel whose two colours differ by more than 1e-4 (or depths
    by more than 1e-4 of the largest) has flipped a decision -- the smallest contribution a flip adds or removes is alpha =
    1/255 of a colour.  On this scene the oracle's two renders differ by at most 3.1e-6 (fp32 noise) and no pixel flips; at least
    99 % of the pixels must stay in the comparison.  The kept pixels must agree within that same 1e-4: HIP must not show what
    counts as a flip in the oracle."""
    from freesplat_amd.transform import transform_cameras
    sc = TC.render_scene()
    xf = torch.cat([1.6 * TR.random_rotation(torch.Generator().manual_seed(70)), torch.tensor([[1.5], [-2.0], [0.7]], dtype=F64)], 1)[None].float()
    s, R, t = TR.split_xf(xf)
    c0, d0 = TC.oracle_render(sc, sc["means"], sc["scales"], sc["rotations"], sc["shs"], sc["c2w"])
    m, scl, q, _, sh = TR.transform(xf, None, sc["means"], sc["scales"], sc["rotations"], None, sc["shs"])
    c1, d1 = TC.oracle_render(sc, m, scl, q, sh, TR.transform_cameras(sc["c2w"], s[0], R[0], t[0]))
    dmax = float(d0.max())
    keep = (np.abs(c1 - c0).max(0) <= 1e-4) & (np.abs(d1 / float(s[0]) - d0) <= 1e-4 * dmax)
    share = float(keep.mean())
    assert share >= 0.99, f"the CPU oracle keeps {share:.4f} of the pixels"
    assert float(c0.std()) > 0.05 and float((d0 > 0).mean()) > 0.9
    opt = _optimizer(sc, hip_device)
    h0, hd0 = _hip_render(opt, sc, sc["c2w"], hip_device)
    T = torch.eye(4)
    T[:3] = xf[0]
    opt.transform_(T)
    c2w = transform_cameras(sc["c2w"][None], T)[0]
    h1, hd1 = _hip_render(opt, sc, c2w, hip_device)
    ec = float(np.abs(h1 - h0).max(0)[keep].max())
    ed = float(np.abs(hd1 / float(s[0]) - hd0)[keep].max()) / dmax
    print(f"kept {share:.4f} of the pixels; colour {ec:.3e}, depth / largest {ed:.3e}")
    assert ec <= 1e-4 and ed <= 1e-4, f"kept {share:.4f} of the pixels: colour {ec}, depth {ed}"
    opt2 = _optimizer(sc, hip_device)                                         # control: the camera alone moved
    assert float(np.abs(_hip_render(opt2, sc, c2w, hip_device)[0] - h0).max()) > 1e-2


# ---- 7. the adapter without coords --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh_degree", [0, 3])
def test_adapter_without_coords(hip_device, sh_degree):
    """fusion=False, coords=None: means equal the fusion=True means; covariances, scales, rotations, opacities equal the
    coords-given path bit for bit; the harmonics are the coords-given (camera-frame) ones rotated by each view's c2w rotation:
    within the band bounds of the float64 restatement, and _sh_color(R d, sh') = _sh_color(d, sh) per view; the gradient to
    raw_gaussians matches float64 autograd of the restatement applied to the head's camera-frame harmonics."""
    from freesplat_amd.gaussian_adapter import GaussianAdapter, GaussianAdapterCfg
    from oracle.raster_dense_torch import _sh_color
    b, v, h, w = 1, 3, 6, 11
    ad = GaussianAdapter(GaussianAdapterCfg(0.5, 15.0, sh_degree)).to(hip_device)
    g = torch.Generator().manual_seed(80)
    E = torch.eye(4).repeat(b, v, 1, 1)
    for j in range(v):
        E[0, j, :3, :3] = TR.random_rotation(g).float()
        E[0, j, :3, 3] = torch.randn(3, generator=g)
    E = E[:, :, None, None, None].to(hip_device)
    K = torch.tensor([[0.9, 0, 0.5], [0, 1.2, 0.5], [0, 0, 1]]).expand(b, v, 1, 1, 1, 3, 3).to(hip_device)
    lead = (b, v, h * w, 1, 1)
    depths = (1 + torch.rand(lead, generator=g)).to(hip_device)
    opac = torch.rand(lead, generator=g).to(hip_device)
    raw = torch.randn(*lead, ad.d_in, generator=g).to(hip_device).requires_grad_(True)
    raw2 = raw.detach().clone().requires_grad_(True)
    fused = ad(E, K, None, depths, opac, raw, (h, w), fusion=True)
    out = ad(E, K, None, depths, opac, raw, (h, w), fusion=False, coords=None)
    ref = ad(E, K, None, depths, opac, raw2, (h, w), fusion=False, coords=fused)
    assert torch.equal(out.means, fused)
    for name in ("covariances", "scales", "rotations", "opacities"):
        assert torch.equal(getattr(out, name), getattr(ref, name)), name
    M = b * v * h * w
    Rv = E.reshape(-1, 4, 4)[:, :3, :3].cpu().double()
    ids = torch.arange(v).repeat_interleave(h * w)
    cam = ref.harmonics.detach().cpu().reshape(M, 3, ad.d_sh)
    cam64 = cam.double().requires_grad_(True)
    want = TR.rotate_sh(cam64, Rv, ids, layout="channel_major")
    got = out.harmonics.detach().cpu().reshape(M, 3, ad.d_sh)
    ratios = {}
    _sh_check("harmonics", got, want, cam64.detach(), "channel_major", torch.ones(M, dtype=torch.bool), cam, ratios)
    d = torch.randn(M, 3, dtype=F64, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    rd = torch.einsum("nij,nj->ni", Rv[ids], d)
    col = _sh_color(sh_degree, d, cam.double().transpose(1, 2))
    assert float((_sh_color(sh_degree, rd, got.double().transpose(1, 2)) - col).abs().max()) <= 1e-5 * max(1.0, float(col.abs().max()))
    # gradients: the rotation's backward is D^T; chain it onto the head's own backward (the coords-given path)
    cot = torch.randn(out.harmonics.shape, generator=g)
    out.harmonics.backward(cot.to(hip_device))
    want.backward(cot.reshape(M, 3, ad.d_sh).double())
    ref.harmonics.backward(cam64.grad.float().reshape(ref.harmonics.shape).to(hip_device))
    scale = float(raw2.grad.abs().max())
    err = float((raw.grad - raw2.grad).abs().max())
    print(f"sh_degree {sh_degree}: " + ", ".join(f"{k} {x:.3f}" for k, x in ratios.items()) + f"; d raw {err:.3e} of {scale:.3e}")
    # a raw SH channel receives one coefficient's gradient times its mask (<= 1): the band bound at |g_l|_2 <= sqrt(7) max |g|,
    # plus the fp32 rounding of the float64 cotangent handed to the coords-given path
    assert scale > 0 and err <= (2 * 9 * 7 ** 0.5 + 1) * EPS * float(cot.abs().max())
