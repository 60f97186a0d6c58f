"""GPU parity of the fused HIP cost volume (C ABI fs_cost_volume_forward) against (a) the
reference's own outputs (golden fixtures) and (b) the CPU oracle at larger / ragged sizes.
Tolerance: 1e-4 abs on O(1) outputs (fp32; the MLP runs on exact-fp32 MFMA, summation orders differ)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
pytestmark = pytest.mark.gpu
ATOL = 1e-4


def _load(name):
    z = np.load(os.path.join(HERE, "golden", name))
    return {k: torch.from_numpy(z[k]) if z[k].ndim else z[k].item() for k in z.files}


def _module_from_fixture(g, h4, w4, D, C, dev):
    from freesplat_amd.cost_volume import AVGFeatureVolumeManager
    m = AVGFeatureVolumeManager(matching_height=h4, matching_width=w4, num_depth_bins=D,
                                mlp_channels=[202, 32, 32, 1], matching_dim_size=C)
    sd = {k.replace("__", "."): v for k, v in g.items() if k.startswith(("mlp__", "linear_ramp", "backprojector", "projector"))}
    missing, unexpected = m.load_state_dict(sd, strict=True), None  # same keys as the reference module
    return m.to(dev)


@pytest.fixture(params=["by_K", "classic", "projected"])
def sweep(request, monkeypatch):
    """Which forward sweep the library runs: its own choice (projected first layer for K = 1; otherwise the general
    sweep on 16-pixel wavefronts, here "classic") or
    either one forced (FS_CV_PROJECTED is read at every call) -- both must meet the same bar at every K."""
    if request.param != "by_K":
        monkeypatch.setenv("FS_CV_PROJECTED", "1" if request.param == "projected" else "0")
    return request.param


def _run(m, kw, dev, **extra):
    args = {k: v.to(dev) for k, v in kw.items()}
    with torch.no_grad():
        return m(**args, **extra).cpu()


@pytest.mark.parametrize("name", ["cv_small_k1.npz", "cv_small_k2.npz", "cv_small_c16.npz"])
def test_matches_reference_golden(hip_device, name, sweep):
    g = _load(name)
    kw = {k: g[k] for k in ("cur_feats", "src_feats", "src_extrinsics", "src_poses", "src_Ks", "cur_invK",
                            "min_depth", "max_depth")}
    m = _module_from_fixture(g, 12, 16, int(g["D"]), g["cur_feats"].shape[1], hip_device)
    out = _run(m, kw, hip_device)
    assert out.shape == g["out"].shape
    assert (out - g["out"]).abs().max().item() <= ATOL


def test_native_size_vs_reference_statistics_and_oracle(hip_device, sweep):
    import inputs
    from oracle import cost_volume_oracle as cvo
    from freesplat_amd.cost_volume import AVGFeatureVolumeManager
    stat = json.load(open(os.path.join(HERE, "golden", "cv_native_stat.json")))
    h4, w4, D, C, V, K = 96, 128, 128, 48, 2, 1
    torch.manual_seed(stat["seed_module"])
    m = AVGFeatureVolumeManager(matching_height=h4, matching_width=w4, num_depth_bins=D,
                                mlp_channels=[202, 32, 32, 1], matching_dim_size=C)
    kw = inputs.cv_inputs(V, K, h4, w4, C, seed=stat["seed_inputs"])
    sd = {k.replace(".", "__"): v for k, v in m.state_dict().items()}
    ref = cvo.cost_volume(kw["cur_feats"], kw["src_feats"], kw["src_extrinsics"], kw["src_Ks"], kw["cur_invK"],
                          kw["min_depth"], kw["max_depth"], D, cvo.mlp_from_state(sd))
    out = _run(m.to(hip_device), kw, hip_device)
    assert (out - ref).abs().max().item() <= ATOL
    o = out.numpy()
    assert abs(o.mean() - stat["mean"]) < 1e-5 and abs(o.std() - stat["std"]) < 1e-5
    np.testing.assert_allclose(o[0, ::16, 40, 60], stat["probe"], atol=ATOL)


RAGGED_CASES = [(3, 2, 15, 21, 11, True, 48), (4, 3, 30, 40, 16, False, 48), (2, 1, 5, 7, 3, True, 48), (2, 1, 64, 64, 128, False, 48),
                (3, 2, 13, 19, 7, True, 16), (2, 1, 24, 32, 16, False, 16)]     # (shared with tests/test_memory_guards.py)


@pytest.mark.parametrize("V,K,h4,w4,D,behind,C", RAGGED_CASES)
def test_ragged_shapes_vs_oracle(hip_device, V, K, h4, w4, D, behind, C, sweep):
    """C = 16 is the module's (and SimpleRecon's) default matching dimension: its own kernel instantiations."""
    import inputs
    from oracle import cost_volume_oracle as cvo
    from freesplat_amd.cost_volume import AVGFeatureVolumeManager
    torch.manual_seed(V * 100 + K)
    m = AVGFeatureVolumeManager(matching_height=h4, matching_width=w4, num_depth_bins=D,
                                mlp_channels=[202, 32, 32, 1], matching_dim_size=C)
    kw = inputs.cv_inputs(V, K, h4, w4, C, seed=17 + V, behind=behind)
    sd = {k.replace(".", "__"): v for k, v in m.state_dict().items()}
    ref = cvo.cost_volume(kw["cur_feats"], kw["src_feats"], kw["src_extrinsics"], kw["src_Ks"], kw["cur_invK"],
                          kw["min_depth"], kw["max_depth"], D, cvo.mlp_from_state(sd))
    out = _run(m.to(hip_device), kw, hip_device)
    assert (out - ref).abs().max().item() <= ATOL


@pytest.mark.parametrize("V,K,h4,w4,D,C", [(3, 2, 15, 21, 11, 48), (4, 8, 24, 32, 16, 48), (2, 1, 13, 19, 7, 48), (3, 2, 13, 19, 7, 16)])
@pytest.mark.parametrize("which", ["both", "cur", "src"])
def test_channels_last_maps_are_read_in_place(hip_device, V, K, h4, w4, D, C, which):
    """channels_last feature maps (pixel-major records) take fs_cost_volume_forward_layout -- no re-layout pass -- and give the
    SAME volume bit for bit as the [C, h, w] maps through the 16-pixel sweep (FS_CV_PROJECTED=0: at K = 1 the default [C, h, w]
    path is the projected sweep, a different summation order); with autograd on, the maps go the contiguous way and gradients flow."""
    import inputs
    from freesplat_amd import cost_volume as cvm
    torch.manual_seed(V * 10 + K)
    m = cvm.AVGFeatureVolumeManager(matching_height=h4, matching_width=w4, num_depth_bins=D, mlp_channels=[202, 32, 32, 1],
                                    matching_dim_size=C).to(hip_device)
    kw = {k: v.to(hip_device) for k, v in inputs.cv_inputs(V, K, h4, w4, C, seed=5 + V).items()}
    os.environ["FS_CV_PROJECTED"] = "0"
    try:
        with torch.no_grad():
            ref = m(**kw)
    finally:
        del os.environ["FS_CV_PROJECTED"]
    cl = dict(kw)
    if which in ("both", "cur"):
        cl["cur_feats"] = kw["cur_feats"].contiguous(memory_format=torch.channels_last)
    if which in ("both", "src"):
        cl["src_feats"] = kw["src_feats"].permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)     # [B,K,C,h,w] view of [B,K,h,w,C] memory
        assert cvm._pixel_major(cl["src_feats"]) and not cl["src_feats"].is_contiguous()
    with torch.no_grad():
        out = m(**cl)
    assert torch.equal(out, ref)
    # the layout entry point really ran: the same call with grad enabled must NOT take it, and still agree
    g = dict(cl)
    g["cur_feats"] = cl["cur_feats"].clone().requires_grad_(True)
    out_g = m(**g)
    assert (out_g - ref).abs().max().item() <= ATOL
    out_g.sum().backward()
    assert g["cur_feats"].grad is not None and torch.isfinite(g["cur_feats"].grad).all()


def test_c3_scale_border_validity_flips_are_rare(hip_device):
    """242x324 (= 968x1296 / 4), K=2.  The reference's `dot != 0` validity count is discontinuous where
    a bilinear tap is a rounding error inside / outside the source image; different (all fp32-valid)
    projection roundings can flip it for isolated (pixel, plane) cells.  Everything else must agree."""
    import inputs
    from oracle import cost_volume_oracle as cvo
    from freesplat_amd.cost_volume import AVGFeatureVolumeManager
    V, K, h4, w4, D = 3, 2, 242, 324, 64
    torch.manual_seed(0)
    m = AVGFeatureVolumeManager(matching_height=h4, matching_width=w4, num_depth_bins=D,
                                mlp_channels=[202, 32, 32, 1], matching_dim_size=48)
    kw = inputs.cv_inputs(V, K, h4, w4, 48, seed=1)
    sd = {k.replace(".", "__"): v for k, v in m.state_dict().items()}
    ref = cvo.cost_volume(kw["cur_feats"], kw["src_feats"], kw["src_extrinsics"], kw["src_Ks"], kw["cur_invK"],
                          kw["min_depth"], kw["max_depth"], D, cvo.mlp_from_state(sd))
    err = (_run(m.to(hip_device), kw, hip_device) - ref).abs()
    assert int((err > ATOL).sum()) <= max(1, err.numel() // 1_000_000)
    assert float(err.flatten().kthvalue(err.numel() - err.numel() // 1_000_000 - 1).values) <= ATOL


def test_zero_features_exact_zero_semantics(hip_device, sweep):
    """All-zero source features: every dot is exactly 0 -> no valid source -> MLP of the zero vector."""
    import inputs
    from freesplat_amd.cost_volume import AVGFeatureVolumeManager
    torch.manual_seed(5)
    m = AVGFeatureVolumeManager(matching_height=8, matching_width=8, num_depth_bins=4,
                                mlp_channels=[202, 32, 32, 1], matching_dim_size=48)
    kw = inputs.cv_inputs(2, 1, 8, 8, 48, seed=3)
    kw["src_feats"] = torch.zeros_like(kw["src_feats"])
    with torch.no_grad():
        const = m.mlp.net(torch.zeros(1, 49)).item()
    out = _run(m.to(hip_device), kw, hip_device)
    assert (out - const).abs().max().item() <= 1e-6


def test_cpu_tensor_raises(hip_device):
    import inputs
    from freesplat_amd.cost_volume import AVGFeatureVolumeManager
    m = AVGFeatureVolumeManager(matching_height=8, matching_width=8, num_depth_bins=4,
                                mlp_channels=[202, 32, 32, 1], matching_dim_size=48)
    kw = inputs.cv_inputs(2, 1, 8, 8, 48, seed=3)
    with pytest.raises(RuntimeError):
        m(**kw)


@pytest.mark.parametrize("V,K,h4,w4,D,behind,C", [(2, 1, 12, 16, 8, False, 48), (3, 2, 15, 21, 6, True, 48),
                                                   (2, 1, 48, 64, 32, False, 48), (3, 2, 14, 18, 5, True, 16)])
def test_backward_matches_oracle_autograd(hip_device, V, K, h4, w4, D, behind, C):
    """Gradients w.r.t. both feature maps and all six MLP tensors vs torch autograd of the oracle."""
    import inputs
    from oracle import cost_volume_oracle as cvo
    from freesplat_amd.cost_volume import AVGFeatureVolumeManager
    torch.manual_seed(V * 10 + K)
    m = AVGFeatureVolumeManager(matching_height=h4, matching_width=w4, num_depth_bins=D,
                                mlp_channels=[202, 32, 32, 1], matching_dim_size=C)
    kw = inputs.cv_inputs(V, K, h4, w4, C, seed=23 + V, behind=behind)
    g = torch.randn(V, D, h4, w4, generator=torch.Generator().manual_seed(3))
    # oracle + autograd on CPU
    cur_c = kw["cur_feats"].clone().requires_grad_(True)
    src_c = kw["src_feats"].clone().requires_grad_(True)
    mlp = {k: v.detach().clone().requires_grad_(True) for k, v in
           cvo.mlp_from_state({k.replace(".", "__"): v for k, v in m.state_dict().items()}).items()}
    ref = cvo.cost_volume(cur_c, src_c, kw["src_extrinsics"], kw["src_Ks"], kw["cur_invK"], kw["min_depth"],
                          kw["max_depth"], D, mlp)
    (ref * g).sum().backward()
    # HIP
    m = m.to(hip_device)
    a = {k: v.to(hip_device) for k, v in kw.items()}
    a["cur_feats"].requires_grad_(True)
    a["src_feats"].requires_grad_(True)
    out = m(**a)
    assert (out.detach().cpu() - ref.detach()).abs().max().item() <= ATOL
    (out * g.to(hip_device)).sum().backward()
    net = m.mlp.net
    pairs = [(a["cur_feats"].grad, cur_c.grad, "cur_feats"), (a["src_feats"].grad, src_c.grad, "src_feats"),
             (net[0].weight.grad, mlp["w1"].grad, "w1"), (net[0].bias.grad, mlp["b1"].grad, "b1"),
             (net[2].weight.grad, mlp["w2"].grad, "w2"), (net[2].bias.grad, mlp["b2"].grad, "b2"),
             (net[4].weight.grad, mlp["w3"].grad, "w3"), (net[4].bias.grad, mlp["b3"].grad, "b3")]
    # LeakyReLU'(z) jumps at z = 0: a pre-activation within rounding of zero gets slope 1 in one
    # summation order and 0.01 in another (the reference has the same CPU-vs-GPU nondeterminism), which
    # perturbs a few isolated (pixel, plane) points out of millions.  So: tight bounds on the bulk
    # (99.5th percentile, mean), a loose one on the isolated outliers.
    for got, want, name in pairs:
        scale = want.abs().max().item() + 1e-20
        e = (got.cpu() - want).abs().flatten() / scale
        if e.numel() > 10000:   # feature-map gradients: isolated flipped points
            k = max(1, int(e.numel() * 0.995))
            assert e.kthvalue(k).values.item() < 1e-3, f"{name}: 99.5th pct {e.kthvalue(k).values.item()}"
            assert e.mean().item() < 2e-4, f"{name}: mean {e.mean().item()}"
            assert e.max().item() < 0.1, f"{name}: max {e.max().item()}"
        else:                   # parameter gradients: sums over all points, flips average out
            assert e.max().item() < 1e-2, f"{name}: max {e.max().item()}"
            assert e.mean().item() < 2e-3, f"{name}: mean {e.mean().item()}"


def _masked_grad_out(aux, g, h4, w4, eps_z=1e-4, eps_px=1e-3):
    """grad_out with the discontinuity points of the volume zeroed: a (pixel, plane) point whose hidden pre-activation
    lies within eps_z of a LeakyReLU kink (slope 1 vs 0.01 decided by the last bits of a summation order), or one of whose
    sources is sampled within eps_px of the position where its first / last bilinear tap enters the source image (the tap's
    weight is ~0 there, but `dot != 0` -- the validity count -- flips).  What is left is smooth in every input, so fp32
    results can be held to a tight bar against a float64 oracle."""
    B, D = g.shape[:2]
    kink = (aux["z1"].abs() < eps_z).any(-1) | (aux["z2"].abs() < eps_z).any(-1)                     # [B,D,N]
    edge = torch.zeros_like(kink)
    for pos, size in ((aux["ix"], w4), (aux["iy"], h4)):                                              # [B,K,D,N]
        near = ((pos + 1).abs() < eps_px) | ((pos - size).abs() < eps_px) | ((pos - (size - 1)).abs() < eps_px) | (pos.abs() < eps_px)
        edge |= near.any(1)
    keep = ~(kink | edge).reshape(B, D, h4, w4)
    return g * keep, int((~keep).sum())


BWD_CASES = {
    # (V, K, h4, w4, D, C, behind, which current views the float64 oracle differentiates)
    "k8_24x32": (9, 8, 24, 32, 16, 48, False, None),
    "k2_60x80": (3, 2, 60, 80, 32, 48, False, None),
    "k2_behind": (3, 2, 30, 40, 16, 48, True, None),
    "k3_c16": (4, 3, 28, 36, 12, 16, False, None),
    # one view turned by 1.2 rad: the planes' horizon crosses its image -- as a SOURCE its tiles straddle the horizon (the tile
    # sweep's whole-image fallback: 320 of 1 920 (tile, plane) cells, 128 more entirely behind), as the CURRENT view its rays
    # run parallel to the planes
    "k2_oblique": (3, 2, 30, 40, 16, 48, "oblique", None),
    "native_k1": (2, 1, 96, 128, 128, 48, False, (1,)),
}


_ORACLE_CACHE = {}


def _set_form(monkeypatch, form):
    """saved: the training forward keeps the MLP's inputs (FREESPLAT_CV_SAVE=1; the default from K = 5 sources up),
    two-pass backward (pass 1: the 16-pixel kernel from saved inputs); two_pass: the backward recomputes the forward
    (FREESPLAT_CV_SAVE=0; pass 1: the 16-pixel kernel); atomic: the one-kernel scatter form (FS_CV_BWD_ATOMIC=1)."""
    monkeypatch.setenv("FREESPLAT_CV_SAVE", "1" if form == "saved" else "0")
    if form == "atomic":
        monkeypatch.setenv("FS_CV_BWD_ATOMIC", "1")


@pytest.mark.parametrize("case", list(BWD_CASES))
@pytest.mark.parametrize("form", ["saved", "two_pass", "atomic"])
def test_backward_tight_vs_float64_oracle(hip_device, case, form, monkeypatch):
    """Every gradient of the volume (both feature maps, the six MLP tensors) against autograd of the reference-pinned
    oracle run in float64, at K = 8, K = 2, a turned-round source, C = 16 and the native 96x128 / D = 128 size, with the
    discontinuity points masked out of grad_out (identically on both sides): <= 1e-3 of max-abs everywhere, <= 1e-4 on
    average, for every tensor.  All three forms of the backward: from the training forward's saved MLP inputs, with the
    forward recomputed (both two-pass: records + source-tile sweep, no global float atomics), and the
    one-kernel scatter they replaced (FS_CV_BWD_ATOMIC=1)."""
    import inputs
    from oracle import cost_volume_oracle as cvo
    from freesplat_amd.cost_volume import AVGFeatureVolumeManager
    V, K, h4, w4, D, C, behind, views = BWD_CASES[case]
    _set_form(monkeypatch, form)
    torch.manual_seed(V * 10 + K)
    m = AVGFeatureVolumeManager(matching_height=h4, matching_width=w4, num_depth_bins=D,
                                mlp_channels=[202, 32, 32, 1], matching_dim_size=C)
    kw = (inputs.cv_inputs(V, K, h4, w4, C, seed=31 + V, oblique=1.2) if behind == "oblique" else
          inputs.cv_inputs(V, K, h4, w4, C, seed=31 + V, behind=behind))
    vs = list(range(V)) if views is None else list(views)
    kw = {k: (v[vs] if k not in ("min_depth", "max_depth") else v) for k, v in kw.items()}
    B = len(vs)
    g = torch.randn(B, D, h4, w4, generator=torch.Generator().manual_seed(3))
    # float64 oracle + autograd on the CPU (once per case: the three forms share it)
    if case not in _ORACLE_CACHE:
        torch.set_num_threads(min(32, os.cpu_count() or 1))
        dbl = lambda t: t.double()
        cur_c = dbl(kw["cur_feats"]).requires_grad_(True)
        src_c = dbl(kw["src_feats"]).requires_grad_(True)
        mlp = {k: v.detach().double().requires_grad_(True) for k, v in
               cvo.mlp_from_state({k.replace(".", "__"): v for k, v in m.state_dict().items()}).items()}
        ref, aux = cvo.cost_volume(cur_c, src_c, dbl(kw["src_extrinsics"]), dbl(kw["src_Ks"]), dbl(kw["cur_invK"]),
                                   kw["min_depth"], kw["max_depth"], D, mlp, return_pre=True)
        gm, n_masked = _masked_grad_out({k: v.detach() for k, v in aux.items()}, g, h4, w4)
        assert n_masked < 0.05 * g.numel(), n_masked
        (ref * gm.double()).sum().backward()
        _ORACLE_CACHE.clear()       # (one case at a time: the native one holds a few hundred MB)
        _ORACLE_CACHE[case] = (ref.detach(), gm, cur_c.grad, src_c.grad, {k: v.grad for k, v in mlp.items()})
    ref, gm, cur_g, src_g, mlp_g = _ORACLE_CACHE[case]
    # HIP
    m = m.to(hip_device)
    a = {k: v.to(hip_device) for k, v in kw.items()}
    a["cur_feats"].requires_grad_(True)
    a["src_feats"].requires_grad_(True)
    out = m(**a)
    err = (out.detach().cpu().double() - ref).abs()
    assert float(err.median()) < 1e-5 and int((err > 1e-4).sum()) <= max(2, err.numel() // 20000), (float(err.max()), int((err > 1e-4).sum()))
    (out * gm.to(hip_device)).sum().backward()
    net = m.mlp.net
    pairs = [(a["cur_feats"].grad, cur_g, "cur_feats"), (a["src_feats"].grad, src_g, "src_feats"),
             (net[0].weight.grad, mlp_g["w1"], "w1"), (net[0].bias.grad, mlp_g["b1"], "b1"),
             (net[2].weight.grad, mlp_g["w2"], "w2"), (net[2].bias.grad, mlp_g["b2"], "b2"),
             (net[4].weight.grad, mlp_g["w3"], "w3"), (net[4].bias.grad, mlp_g["b3"], "b3")]
    bad = []
    for got, want, name in pairs:
        scale = want.abs().max().item() + 1e-30
        e = (got.detach().cpu().double() - want).abs() / scale
        if not (e.max().item() < 1e-3 and e.mean().item() < 1e-4):
            bad.append((name, e.max().item(), e.mean().item()))
    assert not bad, (case, form, bad)


def test_backward_forms_agree_with_zero_features(hip_device, monkeypatch):
    """All-zero current features at some pixels and an all-zero source region: the scores there are EXACTLY zero, the
    source is not averaged, yet d dot / cnt (cnt = 1e-8 when no source counts) still reaches the current feature
    (cost_volume.py:589-598).  The two-pass backward handles that in its re-gather branch (from saved activations: behind
    the header flag the training forward raises): same gradients as the one-kernel form."""
    import inputs
    from freesplat_amd.cost_volume import AVGFeatureVolumeManager
    V, K, h4, w4, D, C = 3, 2, 24, 32, 8, 48
    torch.manual_seed(5)
    m = AVGFeatureVolumeManager(h4, w4, num_depth_bins=D, mlp_channels=[202, 32, 32, 1], matching_dim_size=C).to(hip_device)
    kw = inputs.cv_inputs(V, K, h4, w4, C, seed=77)
    kw["cur_feats"][:, :, 5:9, 7:15] = 0.0
    kw["src_feats"][:, 0, :, 10:20, 3:12] = 0.0
    g = torch.randn(V, D, h4, w4, generator=torch.Generator().manual_seed(4)).to(hip_device)
    res = {}
    for form in ("saved", "two_pass", "atomic"):
        _set_form(monkeypatch, form)
        a = {k: v.to(hip_device) for k, v in kw.items()}
        a["cur_feats"].requires_grad_(True)
        a["src_feats"].requires_grad_(True)
        m.zero_grad()
        (m(**a) * g).sum().backward()
        res[form] = [a["cur_feats"].grad.cpu(), a["src_feats"].grad.cpu()] + [p.grad.cpu().clone() for p in m.parameters()]
    for form in ("saved", "two_pass"):
        for x, y in zip(res[form], res["atomic"]):
            scale = y.abs().max().item() + 1e-30
            assert ((x - y).abs().max().item() / scale) < 1e-4, form


@pytest.mark.parametrize("form", ["two_pass", "saved", "atomic"])
def test_backward_matches_reference_gradients(hip_device, form, monkeypatch):
    """The HIP backward against gradients computed THROUGH THE REFERENCE'S OWN MODULE (tests/golden/cv_small_k2_grads.npz,
    make_golden.gen_backward): 3 views, 2 sources (one turned round), 12 x 16, D = 8.  Discontinuity points (LeakyReLU kinks,
    tap validity on the image border) are few at this size but not masked here -- the reference's fp32 summation order decides
    them on its side: bulk bars as tight as the float64 test's, a loose bar on isolated outliers."""
    _set_form(monkeypatch, form)
    g, gg = _load("cv_small_k2.npz"), _load("cv_small_k2_grads.npz")
    m = _module_from_fixture(g, 12, 16, int(g["D"]), 48, hip_device)
    a = {k: g[k].to(hip_device) for k in ("cur_feats", "src_feats", "src_extrinsics", "src_poses", "src_Ks", "cur_invK",
                                           "min_depth", "max_depth")}
    a["cur_feats"].requires_grad_(True)
    a["src_feats"].requires_grad_(True)
    out = m(**a)
    assert (out.detach().cpu() - gg["out"]).abs().max().item() <= ATOL
    (out * gg["grad_out"].to(hip_device)).sum().backward()
    net = m.mlp.net
    for got, key in ((a["cur_feats"].grad, "d_cur_feats"), (a["src_feats"].grad, "d_src_feats"), (net[0].weight.grad, "d_w1"),
                     (net[0].bias.grad, "d_b1"), (net[2].weight.grad, "d_w2"), (net[2].bias.grad, "d_b2"),
                     (net[4].weight.grad, "d_w3"), (net[4].bias.grad, "d_b3")):
        want = gg[key]
        e = (got.cpu() - want).abs().flatten() / (want.abs().max().item() + 1e-30)
        assert e.mean().item() < 1e-4 and e.max().item() < 2e-2, (key, e.max().item(), e.mean().item())
        if e.numel() > 1000:
            assert e.kthvalue(int(0.995 * e.numel())).values.item() < 1e-3, key


@pytest.mark.parametrize("chunks", ["1", "3", "16"])
def test_tile_sweep_plane_chunks_agree(hip_device, chunks, monkeypatch):
    """The source-tile sweep splits the planes of a tile over several workgroups when there are too few tiles to fill the
    chip (their tiles then leave through atomics into a zeroed map) and walks them in ONE workgroup otherwise (plain
    stores).  The parity cases above are small, i.e. all of the first kind; here the split is forced (FS_CV_SG_CHUNKS: 1 =
    the plain-store form of the full-size workloads, 3 = a ragged split, 16 = one plane per workgroup): same source-feature
    gradient as the library's own choice."""
    import inputs
    from freesplat_amd.cost_volume import AVGFeatureVolumeManager
    V, K, h4, w4, D, C = 4, 3, 27, 35, 16, 48
    torch.manual_seed(8)
    m = AVGFeatureVolumeManager(h4, w4, num_depth_bins=D, mlp_channels=[202, 32, 32, 1], matching_dim_size=C).to(hip_device)
    kw = inputs.cv_inputs(V, K, h4, w4, C, seed=91)
    g = torch.randn(V, D, h4, w4, generator=torch.Generator().manual_seed(6)).to(hip_device)
    monkeypatch.setenv("FREESPLAT_CV_SAVE", "0")
    res = []
    for forced in (None, chunks):
        if forced is not None:
            monkeypatch.setenv("FS_CV_SG_CHUNKS", forced)
        a = {k: v.to(hip_device) for k, v in kw.items()}
        a["src_feats"].requires_grad_(True)
        (m(**a) * g).sum().backward()
        res.append(a["src_feats"].grad.cpu())
    scale = res[0].abs().max().item()
    assert scale > 0 and (res[0] - res[1]).abs().max().item() <= 2e-6 * scale


@pytest.mark.parametrize("seed", list(range(12)))
def test_two_pass_backward_equals_scatter_form_on_random_shapes(hip_device, seed, monkeypatch):
    """Seeded random shapes (1 - 5 views, 1 - 4 sources, ragged sizes down to 5 x 9, 1 - 19 planes, C = 16 / 48, sources turned
    round or oblique, forced plane splits): the two-pass backward (records + source-tile sweep) and the one-kernel scatter form
    give the same gradients for every tensor -- the edge cases of the tile geometry (tiles clipped by the image border, boxes
    clipped by the current view, empty boxes, whole-image fallbacks, plane groups with fewer than four planes)."""
    import inputs
    from freesplat_amd.cost_volume import AVGFeatureVolumeManager
    rng = np.random.default_rng(1000 + seed)
    K = int(rng.integers(1, 5))
    V = K + 1 + int(rng.integers(0, 2))
    h4, w4 = int(rng.integers(5, 41)), int(rng.integers(9, 53))
    D = int(rng.integers(1, 20))
    C = 16 if seed % 3 == 0 else 48
    mode = seed % 4
    kw = inputs.cv_inputs(V, K, h4, w4, C, seed=500 + seed, behind=(mode == 1), oblique=(1.1 + 0.1 * (seed % 3) if mode == 2 else 0.0))
    torch.manual_seed(seed)
    m = AVGFeatureVolumeManager(h4, w4, num_depth_bins=D, mlp_channels=[202, 32, 32, 1], matching_dim_size=C).to(hip_device)
    g = torch.randn(V, D, h4, w4, generator=torch.Generator().manual_seed(seed)).to(hip_device)
    if mode == 3:
        monkeypatch.setenv("FS_CV_SG_CHUNKS", str(1 + seed % 5))
    res = {}
    for form in ("two_pass", "atomic"):
        _set_form(monkeypatch, form)
        a = {k: v.to(hip_device) for k, v in kw.items()}
        a["cur_feats"].requires_grad_(True)
        a["src_feats"].requires_grad_(True)
        m.zero_grad()
        (m(**a) * g).sum().backward()
        res[form] = [a["cur_feats"].grad.cpu(), a["src_feats"].grad.cpu()] + [p_.grad.cpu().clone() for p_ in m.parameters()]
    names = ["cur_feats", "src_feats", "w1", "b1", "w2", "b2", "w3", "b3"]
    for x, y, n in zip(res["two_pass"], res["atomic"], names):
        scale = y.abs().max().item() + 1e-30
        assert torch.isfinite(x).all() and (x - y).abs().max().item() / scale < 2e-4, (n, V, K, h4, w4, D, C, mode, (x - y).abs().max().item() / scale)


@pytest.mark.parametrize("D,near,far", [(128, 0.5, 15.0), (64, 0.25, 20.0), (7, 1.0, 3.0)])
def test_depth_planes_kernel_is_bitwise_generate_depth_planes(hip_device, D, near, far):
    """fs_cost_volume_depth_planes (what the module's forward uses for the reference's call, one launch) against
    cost_volume.py:116-125 evaluated op by op in IEEE float32 on the CPU (= the reference-pinned oracle's planes): identical
    bits; against the same ops as torch launches on the device (whose reciprocal is not correctly rounded): within an ulp;
    and the module leaves the reference's `depth_planes_bdhw` attribute (an expanded view of the same values)."""
    import inputs
    from freesplat_amd.cost_volume import AVGFeatureVolumeManager
    from oracle import cost_volume_oracle as cvo
    h4, w4, C = 12, 16, 48
    m = AVGFeatureVolumeManager(h4, w4, num_depth_bins=D, mlp_channels=[202, 32, 32, 1], matching_dim_size=C)
    cpu = m.generate_depth_planes(2, torch.tensor(near).view(1, 1, 1, 1), torch.tensor(far).view(1, 1, 1, 1)).clone()
    assert torch.equal(cpu[0, :, 0, 0], cvo.depth_planes(near, far, D))
    m = m.to(hip_device)
    kw = {k: v.to(hip_device) for k, v in inputs.cv_inputs(2, 1, h4, w4, C, seed=3).items()}
    kw["min_depth"] = torch.tensor(near, device=hip_device).view(1, 1, 1, 1)
    kw["max_depth"] = torch.tensor(far, device=hip_device).view(1, 1, 1, 1)
    with torch.no_grad():
        m(**kw)
        got = m.depth_planes_bdhw
        dev = m.generate_depth_planes(2, kw["min_depth"], kw["max_depth"])
    assert got.shape == cpu.shape == (2, D, h4, w4) and torch.equal(got.cpu(), cpu)
    assert ((got - dev).abs() <= 1.2e-7 * dev.abs()).all()


@pytest.mark.gpu
def test_saved_activation_forward_runs_only_when_a_backward_can_follow(hip_device, monkeypatch):
    """The activation-keeping forward (fs_cost_volume_forward_train) is taken from K = 4 sources up when a backward can follow
    -- decided in the module's forward, in the caller's grad mode -- and never under no_grad (rounds 4 - 5 tested
    torch.is_grad_enabled() inside the autograd Function, where it is always False: the path was dead; ctx.needs_input_grad
    alone would have saved 3 GB per inference call, it reports the parameters even under no_grad)."""
    import inputs
    from freesplat_amd import cost_volume as CV
    monkeypatch.delenv("FREESPLAT_CV_SAVE", raising=False)
    V, K, h4, w4, D, C = 5, 4, 24, 32, 16, 48
    torch.manual_seed(1)
    m = CV.AVGFeatureVolumeManager(h4, w4, num_depth_bins=D, mlp_channels=[202, 32, 32, 1], matching_dim_size=C).to(hip_device)
    a = {k: v.to(hip_device) for k, v in inputs.cv_inputs(V, K, h4, w4, C, seed=3).items()}
    n0 = CV.CALLS["forward_train"]
    with torch.no_grad():
        ref = m(**a)
    assert CV.CALLS["forward_train"] == n0                       # inference: the plain forward
    out = m(**a)                                                  # grad mode on, the MLP's parameters require grad
    assert CV.CALLS["forward_train"] == n0 + 1
    assert torch.equal(out.detach(), ref)                         # same volume either way
    out.sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    a2 = {k: (v[:, :2].contiguous() if k.startswith("src_") else v) for k, v in a.items()}    # K = 2: recomputing form
    m(**a2)
    assert CV.CALLS["forward_train"] == n0 + 1
