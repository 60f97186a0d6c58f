"""Where `encoder_forward` takes the fused skip branch (gaussian_adapter.skip_latents) and where it must not: the module
matcher on the host, the composed stand-in encoder with the real 7x7 layer on the GPU, and the float64 restatement the GPU
tests measure against (tests/skip_ref.py) checked against torch's autograd."""
import pytest
import torch
from torch import nn

import skip_ref as R


def _layer(**kw):
    a = dict(in_channels=3, out_channels=64, kernel_size=7, stride=1, padding=3)
    a.update(kw)
    return nn.Sequential(nn.Conv2d(**a), nn.ReLU())


def test_matcher_accepts_only_the_reference_layer(monkeypatch):
    from freesplat_amd.encoder_forward import fused_skip_layer
    monkeypatch.delenv("FREESPLAT_SKIP_FUSED", raising=False)
    ref = _layer()                                                  # encoder_freesplat.py:124-128, high_resolution_skip[0]
    assert fused_skip_layer(ref) is ref[0]
    assert fused_skip_layer(nn.Sequential(nn.Conv2d(3, 64, 7, 1, 3), nn.ReLU(inplace=True))) is not None
    assert fused_skip_layer(_layer(kernel_size=3, padding=1)) is None
    assert fused_skip_layer(_layer(bias=False)) is None
    assert fused_skip_layer(_layer(kernel_size=6, stride=2, padding=2)) is None       # high_resolution_skip[1]
    assert fused_skip_layer(_layer(stride=2)) is None
    assert fused_skip_layer(_layer(padding=2)) is None
    assert fused_skip_layer(_layer(out_channels=32)) is None
    assert fused_skip_layer(_layer(padding_mode="reflect")) is None
    assert fused_skip_layer(nn.Sequential(nn.Conv2d(3, 64, 7, 1, 3))) is None         # no ReLU
    assert fused_skip_layer(nn.Sequential(nn.Conv2d(3, 64, 7, 1, 3), nn.Tanh())) is None
    assert fused_skip_layer(nn.Conv2d(3, 64, 7, 1, 3)) is None                        # the composed test's bare stand-in
    assert fused_skip_layer(nn.Conv2d(3, 64, 3, padding=1)) is None
    assert fused_skip_layer(ref.double()) is None
    monkeypatch.setenv("FREESPLAT_SKIP_FUSED", "0")
    assert fused_skip_layer(_layer()) is None
    monkeypatch.setenv("FREESPLAT_SKIP_FUSED", "1")
    assert fused_skip_layer(_layer()) is not None


def test_skip_latents_has_no_host_path():
    from freesplat_amd.gaussian_adapter import skip_latents
    with pytest.raises(RuntimeError, match="no CPU path"):
        skip_latents(torch.zeros(1, 65, 8, 8), torch.zeros(1, 3, 8, 8), torch.zeros(64, 3, 7, 7), torch.zeros(64))


def test_reference_restatement_is_torch_autograd():
    """skip_ref.reference (bands of rows, analytic gradients) against the expression itself under torch's autograd, float64;
    bands that end inside the image and a pixel subset included."""
    V, h, w = 2, 21, 19
    a = R.make_inputs(V, h, w, seed=1)
    W, b, hd = (a[k].double().requires_grad_(True) for k in ("weight", "bias", "head"))
    lat = (hd[:, 1:] + torch.relu(torch.nn.functional.conv2d(a["img"].double(), W, b, padding=3))).reshape(V, 64, h * w)
    lat = lat.transpose(1, 2)
    (lat * a["g_lat"].double()).sum().backward()
    ref = R.reference(a["head"], a["img"], a["weight"], a["bias"], g_lat=a["g_lat"], band=8)
    assert torch.allclose(ref["lat"], lat.detach().reshape(-1, 64), rtol=0, atol=1e-13)
    assert torch.allclose(ref["g_weight"], W.grad, rtol=0, atol=1e-10) and torch.allclose(ref["g_bias"], b.grad, rtol=0, atol=1e-10)
    assert bool((ref["bound"] > 0).all()) and bool((ref["g_weight_bound"] >= 0).all()) and ref["ambiguous_share"] < 1e-3
    sel = torch.tensor([0, 5, h * w - 1, h * w, 2 * h * w - 1])
    sub = R.reference(a["head"], a["img"], a["weight"], a["bias"], select=sel, band=8)
    assert torch.equal(sub["lat"], ref["lat"][sel]) and torch.equal(sub["bound"], ref["bound"][sel])


@pytest.mark.gpu
def test_encoder_forward_takes_the_fused_path_and_agrees(hip_device, monkeypatch):
    """The composed stand-in encoder (tests/test_composed_dropin.py) with the real 7x7 skip layer, through `encoder_forward`
    with the switch on and off: the fused op runs exactly when it is on, and the latents the fold receives agree within twice
    the float64 forward bound (both paths carry it)."""
    import test_composed_dropin as T
    from freesplat_amd import gaussian_adapter as GA
    from freesplat_amd.encoder_forward import encoder_forward
    enc = T._Encoder(oracle=False)
    torch.manual_seed(3)
    enc.high_resolution_skip = nn.ModuleList([_layer()])
    enc = enc.to(hip_device)
    ctx, _, _ = T._context(1, hip_device)
    seen = {"latents": [], "head": [], "fused": 0}
    fold = enc.fuse_gaussians

    def spy_fold(*a, **k):
        seen["latents"].append(a[0][0].detach().clone())
        return fold(*a, **k)
    enc.fuse_gaussians = spy_fold

    def same_head(module, inputs, out):     # both paths get the FIRST call's head map, whatever the stand-in trunk's run-to-run noise
        if seen["head"]:
            out = dict(out)
            out["output_pred_s-1_b1hw"] = seen["head"][0]
            return out
        seen["head"].append(out["output_pred_s-1_b1hw"].detach().clone())
    enc.depth_decoder.register_forward_hook(same_head)
    real = GA.skip_latents

    def spy_skip(*a):
        seen["fused"] += 1
        return real(*a)
    monkeypatch.setattr(GA, "skip_latents", spy_skip)
    for flag, want in (("1", 1), ("0", 1)):
        monkeypatch.setenv("FREESPLAT_SKIP_FUSED", flag)
        with torch.no_grad():
            res = encoder_forward(enc, dict(ctx), 0)
        assert seen["fused"] == want and res["gaussians"][0].means.shape[1] > 0
    on, off = (t.cpu().double().reshape(-1, 64) for t in seen["latents"])
    conv = enc.high_resolution_skip[0][0]
    ref = R.reference(seen["head"][0].cpu(), ctx["image"][0].cpu(), conv.weight.detach().cpu(), conv.bias.detach().cpu())
    print(f"encoder_forward fused vs module path: worst / (2 bound) {float(((on - off).abs() / (2 * ref['bound'])).max()):.3f}")
    assert bool(((on - off).abs() <= 2 * ref["bound"]).all())
    assert bool(((on - ref["lat"]).abs() <= ref["bound"]).all()) and bool(((off - ref["lat"]).abs() <= ref["bound"]).all())
    # images that require a gradient keep the module path even with the switch on
    monkeypatch.setenv("FREESPLAT_SKIP_FUSED", "1")
    ctx_g = dict(ctx)
    ctx_g["image"] = ctx["image"].clone().requires_grad_(True)
    encoder_forward(enc, ctx_g, 0)
    assert seen["fused"] == 1
