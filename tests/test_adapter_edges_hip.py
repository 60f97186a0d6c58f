"""The adapter kernels (csrc/adapter.hip: fs_unproject_*, fs_gaussian_head_*_sh) against the float64 restatement on the
branch-edge classes of adapter_cases.py, judged per row (util_raster.per_gaussian_err) within ADAPTER_TOL_GPU = 4 x what fp32
torch autograd of the restatement reads; the harmonics, their gradient and g_E's fourth row and column bit-exact.

On the MI355X every group reads 0.09 - 0.49 of its bound.  The quat_1e15 class is what found head_bwd_kernel's
`dot / (D * D * nq)`: the product overflows from |raw_q| = 7e12 on, the projection term of the normalisation's gradient became
0 and g_raw[:, 3:7] read 6 - 16 (2e5 - 6e5 bounds) on every row of the class; the kernel now divides in two steps."""
import ctypes as C

import pytest
import torch

import adapter_cases as ac
from adapter_ref import head64, unproject64
from util_raster import per_gaussian_err

pytestmark = pytest.mark.gpu
OUTS = ("cov", "sh", "scales", "rot")


def _head_on_device(case, cots, dev, mult=None):
    """_Head.apply on the case and its backward for the cotangents named in `cots`; the others reach the kernel as NULL.
    Returns run_head's dict on the CPU, and the extrinsics as placed."""
    from freesplat_amd.gaussian_adapter import _Head
    raw = case["raw"].to(dev).requires_grad_(True)
    dep = case["dep"].to(dev).requires_grad_(True)
    E = ac.place(case["E"], dev, case["e_offset"]).requires_grad_(True)
    mult = case["mult"] if mult is None else mult
    o = _Head.apply(raw, dep, E, mult.to(dev), case["mask"].to(dev), ac.SMIN, ac.SMAX)
    outs = dict(zip(OUTS, o))
    g = torch.autograd.grad([outs[k] for k in cots], (raw, dep, E), [case["g_" + k].to(dev) for k in cots])
    res = dict(cov=o[0], harmonics=o[1], scales=o[2], rotations=o[3], g_raw=g[0], g_depths=g[1], g_E=g[2])
    return {k: t.detach().cpu() for k, t in res.items()}, E


def _exact_checks(case, cots, got, what):
    M, d_sh = case["M"], case["d_sh"]
    for k, t in got.items():
        assert bool(torch.isfinite(t).all()), (what, k, "not finite")
    assert torch.equal(got["harmonics"], case["raw"][:, 7:].reshape(M, 3, d_sh) * case["mask"]), (what, "harmonics")
    want = (case["g_sh"] * case["mask"]).reshape(M, -1) if "sh" in cots else torch.zeros(M, 3 * d_sh)
    assert torch.equal(got["g_raw"][:, 7:], want), (what, "g_raw[:, 7:]")
    assert bool((got["g_E"][:, 3, :] == 0).all()) and bool((got["g_E"][:, :, 3] == 0).all()), (what, "g_E fourth row / column")


@pytest.mark.parametrize("cls", ac.CLASSES)
@pytest.mark.parametrize("d_sh", ac.D_SHS)
def test_head_edge_class_vs_float64_per_row(hip_device, d_sh, cls):
    """_Head.apply on one class at M = 1 and 300, all four cotangents together and each alone: every judged group within
    ADAPTER_TOL_GPU of float64 (a group no cotangent reaches must be exactly zero), the exact assertions, and the class's
    properties on the tensors as placed on the device.  Prints the worst figure / bound ratio of each group."""
    ratios = {}
    for M in ac.MS:
        case = ac.build_case(cls, d_sh, M)
        for cots in ac.COT_SETS:
            got, E = _head_on_device(case, cots, hip_device)
            ac.assert_cases_present(case, E)
            ref = ac.run_head(case, cots)
            what = (cls, d_sh, M, "+".join(cots))
            _exact_checks(case, cots, got, what)
            for name, (e, row) in ac.figures(got, ref).items():
                r = e / ac.ADAPTER_TOL_GPU[cls][name]
                if r > ratios.get(name, (0.0,))[0]:
                    ratios[name] = (r, e, M, "+".join(cots), row)
    print(f"{cls}, d_sh {d_sh}: worst figure / bound " + ", ".join(f"{k} {v[0]:.3f} ({v[1]:.2e})" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if v[0] > 1.0}
    assert not bad, f"{cls}, d_sh {d_sh}: (ratio, figure, M, cotangents, row) {bad}"


@pytest.mark.parametrize("d_sh", ac.D_SHS)
def test_head_placement_and_multiplier_layout_change_no_bit(hip_device, d_sh):
    """The same rows with the extrinsics on and off the 16-byte grid (load_row4's two paths), and a one-element multiplier
    against the same value repeated per row (mult_stride 0 / 1): every output and gradient bit for bit."""
    for M in ac.MS:
        a, _ = _head_on_device(ac.build_case("extrinsics", d_sh, M), ac.COTANGENTS, hip_device)
        b, E = _head_on_device(ac.build_case("extrinsics_off16", d_sh, M), ac.COTANGENTS, hip_device)
        assert E.data_ptr() % 16 == 4
        for k in a:
            assert torch.equal(a[k], b[k]), ("placement", M, k)
        case = ac.build_case("depth_large", d_sh, M)
        a, _ = _head_on_device(case, ac.COTANGENTS, hip_device)
        b, _ = _head_on_device(case, ac.COTANGENTS, hip_device, mult=case["mult"].expand(M).contiguous())
        for k in a:
            assert torch.equal(a[k], b[k]), ("multiplier layout", M, k)


@pytest.mark.parametrize("cls", ["plain", "extrinsics", "extrinsics_off16"])
def test_d_sh_9_abi_entry_points_equal_the_sh_ones(hip_device, cls):
    """fs_gaussian_head_forward / _backward (ABI 4) are the d_sh = 9 case of the _sh entry points, bit for bit; with every
    cotangent and with the covariance's alone (the others NULL)."""
    from freesplat_amd import _lib
    dev, p = hip_device, _lib.ptr
    case = ac.build_case(cls, 9, 300)
    M = case["M"]
    raw, dep, mult, mask = (case[k].to(dev) for k in ("raw", "dep", "mult", "mask"))
    E = ac.place(case["E"], dev, case["e_offset"])
    stride = int(mult.numel() == M)
    f32 = C.c_float
    outs = {}
    for name, extra in (("fs_gaussian_head_forward", ()), ("fs_gaussian_head_forward_sh", (9,))):
        o = [torch.full(s, float("nan"), device=dev) for s in ((M, 3, 3), (M, 3, 9), (M, 3), (M, 4))]
        _lib.launch(name, M, *extra, p(raw), p(dep), p(E), p(mult), stride, p(mask), f32(ac.SMIN), f32(ac.SMAX), *map(p, o))
        outs[name] = o
    for a, b in zip(*outs.values()):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    g = [case["g_" + k].to(dev) for k in OUTS]
    for present in ((True,) * 4, (True, False, False, False)):
        outs = {}
        for name, extra in (("fs_gaussian_head_backward", ()), ("fs_gaussian_head_backward_sh", (9,))):
            o = [torch.full(s, float("nan"), device=dev) for s in ((M, 34), (M,), (M, 4, 4))]
            _lib.launch(name, M, *extra, p(raw), p(dep), p(E), p(mult), stride, p(mask), f32(ac.SMIN), f32(ac.SMAX),
                        *(p(t) if on else None for t, on in zip(g, present)), *map(p, o))
            outs[name] = o
        for a, b in zip(*outs.values()):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


@pytest.mark.parametrize("V,h,w,k", ac.UNPROJECT_CASES)
def test_unproject_edge_cases_vs_float64_per_pixel(hip_device, V, h, w, k):
    from freesplat_amd.gaussian_adapter import _Unproject
    c = ac.build_unproject(V, h, w, k)
    dev = hip_device
    d = c["depths"].to(dev).requires_grad_(True)
    xyz = _Unproject.apply(d, c["E"].to(dev), c["k0"].to(dev), h, w)
    assert xyz.shape == (V, h * w, 3)
    xyz.backward(c["g_xyz"].to(dev))
    got = dict(xyz=xyz.detach().cpu().reshape(-1, 3), g_depths=d.grad.cpu().reshape(-1, 1))
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    f = ac.unproject_figures(got, ac.run_unproject(c))
    print(f"unproject {V} x {h} x {w}: worst figure / bound "
          + ", ".join(f"{n} {e / ac.ADAPTER_TOL_GPU['unproject'][n]:.3f} ({e:.2e})" for n, (e, _) in f.items()))
    for n, (e, row) in f.items():
        assert e <= ac.ADAPTER_TOL_GPU["unproject"][n], (n, row, e)


def _adapter(dev, degree=2):
    from freesplat_amd.gaussian_adapter import GaussianAdapter, GaussianAdapterCfg
    return GaussianAdapter(GaussianAdapterCfg(ac.SMIN, ac.SMAX, degree)).to(dev)


def test_adapter_with_intrinsics_per_gaussian_vs_float64_multiplier(hip_device):
    """GaussianAdapter.forward(fusion=False, coords=...) with a camera per Gaussian: the multiplier reaches the kernel per row
    (mult_stride 1).  Forward against the restatement with the float64 multiplier 0.1 (1 / (fx w) + 1 / (fy h)) of each row.
    The device's fp32 multiplier (a 2x2 inverse of a diagonal block, two products, 0.1 and a sum: under eight roundings of
    2^-24 each) may differ from it by MULT_REL = 4 * 2^-23, which the scales get once and the covariances twice on top of
    the plain class's bound.  The gradients are ill-conditioned in the multiplier where their terms cancel, so they are
    compared with the restatement fed the device's own multiplier, at the plain class's bound unchanged."""
    dev = hip_device
    MULT_REL = 4.0 * 2.0 ** -23
    case = ac.build_case("plain", 9, 300)
    M, h, w = case["M"], 24, 40
    gen = torch.Generator().manual_seed(5)
    K = torch.eye(3).repeat(M, 1, 1)
    K[:, 0, 0], K[:, 1, 1] = 0.5 + 1.5 * torch.rand(M, generator=gen), 0.5 + 1.5 * torch.rand(M, generator=gen)
    K[:, 0, 2], K[:, 1, 2] = 0.3, 0.6
    mult64 = 0.1 * (1.0 / (K[:, 0, 0].double() * w) + 1.0 / (K[:, 1, 1].double() * h))
    ad = _adapter(dev)
    assert torch.equal(ad.sh_mask.cpu(), case["mask"])
    raw, dep, E = (case[k].to(dev).requires_grad_(True) for k in ("raw", "dep", "E"))
    coords, opac = torch.randn(M, 3, generator=gen).to(dev), torch.rand(M, generator=gen).to(dev)
    Kd = K.to(dev).view(1, 1, M, 1, 1, 3, 3)
    out = ad(E.view(1, 1, M, 1, 1, 4, 4), Kd, None, dep.view(1, 1, M, 1, 1), opac.view(1, 1, M, 1, 1),
             raw.view(1, 1, M, 1, 1, 34), (h, w), fusion=False, coords=coords.view(1, 1, M, 1, 1, 3))
    mult_dev = ad.get_scale_multiplier(Kd, 1 / torch.tensor((w, h), dtype=torch.float32, device=dev)).reshape(-1)
    assert mult_dev.numel() == M
    assert float(((mult_dev.cpu().double() - mult64).abs() / mult64).max()) <= MULT_REL
    assert torch.equal(out.means.reshape(M, 3), coords) and torch.equal(out.opacities.reshape(M), opac)
    got = dict(cov=out.covariances.reshape(M, 3, 3), harmonics=out.harmonics.reshape(M, 3, 9), scales=out.scales.reshape(M, 3),
               rotations=out.rotations.reshape(M, 4))
    g = torch.autograd.grad([got["cov"], got["harmonics"], got["scales"], got["rotations"]], (raw, dep, E),
                            [case["g_" + k].to(dev) for k in OUTS])
    got.update(g_raw=g[0], g_depths=g[1], g_E=g[2])
    got = {k: t.detach().cpu() for k, t in got.items()}
    _exact_checks(case, OUTS, got, "adapter")
    tol = ac.ADAPTER_TOL_GPU["plain"]
    ref = ac.run_head(dict(case, mult=mult64), OUTS)           # (float64 multiplier: not the cached plain reference)
    for name, extra in (("cov", 2.0 * MULT_REL), ("scales", MULT_REL), ("rotations", 0.0)):
        e, row = ac.figure(got, ref, name)
        assert e <= tol[name] + extra, (name, row, e)
    ref = ac.run_head(dict(case, mult=mult_dev.cpu()), OUTS)
    f = ac.figures(got, ref)
    print("adapter, intrinsics per Gaussian: worst figure / bound " + ", ".join(f"{n} {e / tol[n]:.3f}" for n, (e, _) in f.items()))
    for name, (e, row) in f.items():
        assert e <= tol[name], (name, row, e)


def test_adapter_fusion_takes_view_0_intrinsics_of_each_batch_element(hip_device):
    """GaussianAdapter.forward(fusion=True) at b = 2, v = 3 with intrinsics that differ per batch element AND per view: the
    reference builds its Create_from_depth_map once per batch element from intrinsics[i, 0] and projects every view of that
    element with it (reference src/model/encoder/common/gaussian_adapter.py:178-186), so the expected means use view 0's
    intrinsics.  The normalised intrinsics are dyadic, so their pixel forms (fx w, fy h, cx w, cy h) are exact in fp32."""
    dev = hip_device
    b, v, h, w = 2, 3, 5, 7
    gen = torch.Generator().manual_seed(11)
    fx = torch.tensor([[0.875, 1.125, 1.5], [1.25, 0.75, 1.0]])
    fy = torch.tensor([[1.375, 0.625, 1.0], [0.9375, 1.75, 1.125]])
    cx = torch.tensor([[0.3125, 0.5, 0.4375], [0.28125, 0.5625, 0.5]])
    cy = torch.tensor([[0.625, 0.5, 0.5625], [0.59375, 0.4375, 0.5]])
    K = torch.eye(3).repeat(b, v, 1, 1)
    K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2] = fx, fy, cx, cy
    E = torch.eye(4).repeat(b, v, 1, 1) + 0.3 * torch.randn(b, v, 4, 4, generator=gen)
    depths = 0.5 + 4.5 * torch.rand(b, v, h * w, generator=gen)
    for i in range(b):
        for j in range(v):
            for n, x in enumerate(ac.UNPROJECT_DEPTHS):
                depths[i, j, (3 * j + 5 * i + 9 * n) % (h * w)] = x
    g_xyz = torch.randn(b, v, h * w, 3, generator=gen)
    d = depths.to(dev).requires_grad_(True)
    xyz = _adapter(dev)(E.to(dev)[:, :, None, None, None], K.to(dev)[:, :, None, None, None], None, d[..., None, None], None, None,
                        (h, w), fusion=True)
    assert xyz.shape == (b, v, h * w, 1, 1, 3)
    xyz.backward(g_xyz.to(dev)[:, :, :, None, None, :])
    got = dict(xyz=xyz.detach().cpu().reshape(-1, 3), g_depths=d.grad.cpu().reshape(-1, 1))

    def expected(view_of):
        xs, gs = [], []
        for i in range(b):
            d64 = depths[i].double().requires_grad_(True)
            rows = []
            for j in range(v):
                Kj = K[i, view_of(j)].double()
                k0 = torch.stack([Kj[0, 0] * w, Kj[1, 1] * h, Kj[0, 2] * w, Kj[1, 2] * h])
                rows.append(unproject64(d64[j:j + 1], E[i, j:j + 1].double(), k0, h, w)[0])
            x = torch.stack(rows)
            (x * g_xyz[i].double()).sum().backward()
            xs.append(x.detach())
            gs.append(d64.grad)
        return dict(xyz=torch.stack(xs).reshape(-1, 3), g_depths=torch.stack(gs).reshape(-1, 1))

    tol = ac.ADAPTER_TOL_GPU["unproject"]
    f = ac.unproject_figures(got, expected(lambda j: 0))
    own = ac.unproject_figures(got, expected(lambda j: j))
    print("fusion, view 0's intrinsics: worst figure / bound " + ", ".join(f"{n} {e / tol[n]:.3f}" for n, (e, _) in f.items())
          + "; against each view's own: " + ", ".join(f"{n} {e:.2e}" for n, (e, _) in own.items()))
    for n, (e, row) in f.items():
        assert e <= tol[n], (n, row, e)
        assert own[n][0] >= 1e3 * tol[n], "the case does not tell view 0's intrinsics from each view's own"
