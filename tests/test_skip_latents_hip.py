"""GPU checks of the fused skip branch (csrc/skip_conv.hip, gaussian_adapter.skip_latents) against the float64 restatement
of the reference expression in tests/skip_ref.py and against the torch chain it replaces.  Every bound is computed by the test
in float64 from the inputs (skip_ref's docstring derives them); none is tuned to what the kernel gives."""
import json
import os
import subprocess
import sys

import pytest
import torch

import skip_ref as R

pytestmark = pytest.mark.gpu

SIZES = [(2, 40, 56), (1, 121, 162), (3, 64, 80), (2, 45, 77)]      # the last: h, w multiples of neither tile edge (8 x 32)
AMBIGUOUS_CAP = 1e-3


def _run(a, dev, **grad):
    from freesplat_amd.gaussian_adapter import skip_latents
    d = {k: v.to(dev) for k, v in a.items()}
    for k in ("head", "weight", "bias"):
        d[k].requires_grad_(grad.get(k, True))
    lat, dens = skip_latents(d["head"], d["img"], d["weight"], d["bias"])
    return d, lat, dens


def _assert_forward(lat, ref, border, what):
    err = (lat.double() - ref["lat"]).abs()
    ratio = err / ref["bound"]
    print(f"{what}: forward worst |err| / bound {float(ratio.max()):.3f} (border {float(ratio[border].max()):.3f}), "
          f"largest bound {float(ref['bound'].max()):.2e}")
    assert bool((err[border] <= ref["bound"][border]).all()), f"{what}: border pixels off: padding fault"
    assert bool((err <= ref["bound"]).all()), f"{what}: interior pixels off"


def _assert_weight_grads(gw, gb, ref, what):
    assert ref["ambiguous_share"] <= AMBIGUOUS_CAP, f"{what}: ambiguous share {ref['ambiguous_share']}"
    ew, eb = (gw.double() - ref["g_weight"]).abs(), (gb.double() - ref["g_bias"]).abs()
    tiny = 1e-300                            # (a channel whose ReLU never fires has gradient and bound exactly 0)
    print(f"{what}: ambiguous share {ref['ambiguous_share']:.2e}, g_weight worst |err| / bound "
          f"{float((ew / (ref['g_weight_bound'] + tiny)).max()):.3e}, g_bias {float((eb / (ref['g_bias_bound'] + tiny)).max()):.3e}, "
          f"g_weight relative to its largest entry {float(ew.max() / ref['g_weight'].abs().max()):.2e}")
    assert bool((ew <= ref["g_weight_bound"]).all()), f"{what}: g_weight"
    assert bool((eb <= ref["g_bias_bound"]).all()), f"{what}: g_bias"


@pytest.mark.parametrize("V,h,w", SIZES)
def test_forward_matches_float64_reference(hip_device, V, h, w):
    a = R.make_inputs(V, h, w, seed=V * 1000 + h)
    ref = R.reference(a["head"], a["img"], a["weight"], a["bias"])
    with torch.no_grad():
        _, lat, dens = _run(a, hip_device)
    assert lat.shape == (V, h * w, 64) and lat.is_contiguous() and dens.shape == (V, h * w)
    assert torch.equal(dens.cpu(), a["head"][:, 0].reshape(V, h * w)), "dens must be head[:, 0] bit for bit"
    _assert_forward(lat.cpu().reshape(-1, 64), ref, R.border_mask(V, h, w), f"{V}x{h}x{w}")


@pytest.mark.parametrize("V,h,w", SIZES)
def test_backward_matches_float64_reference(hip_device, V, h, w):
    a = R.make_inputs(V, h, w, seed=V * 1000 + h)
    ref = R.reference(a["head"], a["img"], a["weight"], a["bias"], g_lat=a["g_lat"])
    d, lat, dens = _run(a, hip_device)
    ((lat * d["g_lat"]).sum() + (dens * d["g_dens"]).sum()).backward()
    g_head = d["head"].grad.cpu()
    assert torch.equal(g_head[:, 1:].reshape(V, 64, h * w), a["g_lat"].transpose(1, 2)), "g_head[:, 1:] is the transposed g_lat"
    assert torch.equal(g_head[:, 0].reshape(V, h * w), a["g_dens"]), "g_head[:, 0] is g_dens"
    _assert_weight_grads(d["weight"].grad.cpu(), d["bias"].grad.cpu(), ref, f"{V}x{h}x{w}")
    # only the latents carry a gradient: the density channel of g_head is written as zero, not left uninitialised
    d2, lat2, _ = _run(a, hip_device)
    (lat2 * d2["g_lat"]).sum().backward()
    assert bool((d2["head"].grad[:, 0] == 0).all()) and torch.equal(d2["head"].grad[:, 1:].cpu(), g_head[:, 1:])
    # a frozen layer: the head's gradient alone, nothing kept for the weights
    d3, lat3, _ = _run(a, hip_device, weight=False, bias=False)
    (lat3 * d3["g_lat"]).sum().backward()
    assert d3["weight"].grad is None and torch.equal(d3["head"].grad[:, 1:].cpu(), g_head[:, 1:])


def test_backward_is_bit_reproducible(hip_device):
    V, h, w = 3, 64, 80
    a = R.make_inputs(V, h, w, seed=7)
    d, lat, dens = _run(a, hip_device)
    loss = (lat * d["g_lat"]).sum() + (dens * d["g_dens"]).sum()
    first = torch.autograd.grad(loss, [d["weight"], d["bias"]], retain_graph=True)
    second = torch.autograd.grad(loss, [d["weight"], d["bias"]], retain_graph=True)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    d2, lat2, dens2 = _run(a, hip_device)           # and from a second forward
    third = torch.autograd.grad((lat2 * d2["g_lat"]).sum() + (dens2 * d2["g_dens"]).sum(), [d2["weight"], d2["bias"]])
    assert torch.equal(first[0], third[0]) and torch.equal(first[1], third[1])


def test_agrees_with_the_torch_chain_on_the_device(hip_device):
    """latents_pack(head, relu(conv(img))), the path this op replaces, forward and backward: both sides carry the float64
    bound, so they agree within twice it; the head gradient is pure data movement on both sides."""
    from freesplat_amd.gaussian_adapter import latents_pack
    V, h, w = 2, 40, 56
    a = R.make_inputs(V, h, w, seed=11)
    ref = R.reference(a["head"], a["img"], a["weight"], a["bias"], g_lat=a["g_lat"])
    assert ref["ambiguous_share"] <= AMBIGUOUS_CAP
    d, lat, dens = _run(a, hip_device)
    ((lat * d["g_lat"]).sum() + (dens * d["g_dens"]).sum()).backward()
    c = {k: v.to(hip_device) for k, v in a.items()}
    for k in ("head", "weight", "bias"):
        c[k].requires_grad_(True)
    lat_c, dens_c = latents_pack(c["head"], torch.relu(torch.nn.functional.conv2d(c["img"], c["weight"], c["bias"], padding=3)))
    ((lat_c * c["g_lat"]).sum() + (dens_c * c["g_dens"]).sum()).backward()
    dl = (lat.detach() - lat_c.detach()).abs().cpu().double().reshape(-1, 64)
    print(f"fused vs chain: latents worst / (2 bound) {float((dl / (2 * ref['bound'])).max()):.3f}")
    assert bool((dl <= 2 * ref["bound"]).all())
    assert torch.equal(dens, dens_c) and torch.equal(d["head"].grad, c["head"].grad)
    assert bool(((d["weight"].grad - c["weight"].grad).abs().cpu().double() <= 2 * ref["g_weight_bound"]).all())
    assert bool(((d["bias"].grad - c["bias"].grad).abs().cpu().double() <= 2 * ref["g_bias_bound"]).all())


def test_no_skip_map_is_kept_for_the_backward(hip_device):
    """Beyond its inputs and outputs the op keeps one bit per (pixel, channel): at most V*h*w*8 bytes rounded up to the
    allocator's 512-byte granule, by torch.cuda.memory_allocated(), where today's chain keeps V*64*h*w*4 (60 MB here).
    Measured by tests/skip_held_bytes.py in a process of its own, where the counter is not inflated by cached blocks of earlier
    tests (its docstring); the allocator's requested-bytes counter is held to V*h*w*8 exactly as well."""
    V, h, w = 3, 242, 324
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "skip_held_bytes.py")
    run = subprocess.run([sys.executable, script, str(V), str(h), str(w)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    got = json.loads(run.stdout.strip().splitlines()[-1])
    print(f"held between forward and backward at {V}x{h}x{w}: {got} (one skip map: {V * 64 * h * w * 4} B)")
    granule = lambda n: (n + 511) // 512 * 512
    assert got["fused"]["allocated"] <= granule(V * h * w * 8)
    assert got["fused"]["requested"] <= V * h * w * 8
    assert got["chain"]["allocated"] >= V * 64 * h * w * 4      # (what the fused op removes)


@pytest.mark.slow
def test_full_size_once(hip_device):
    """3 x 968x1296 (BASELINE config 3), forward + backward: the latents on a seeded random subset of 2^16 pixels, the weight
    and bias gradients against the float64 reference of the whole contraction (matrix products over bands of rows: about a
    minute on 16 CPU threads)."""
    V, h, w = 3, 968, 1296
    a = R.make_inputs(V, h, w, seed=5)
    sel = torch.randperm(V * h * w, generator=torch.Generator().manual_seed(6))[:1 << 16].sort().values
    ref = R.reference(a["head"], a["img"], a["weight"], a["bias"], g_lat=a["g_lat"], select=sel)
    d, lat, dens = _run(a, hip_device)
    assert torch.equal(dens.detach().cpu(), a["head"][:, 0].reshape(V, h * w))
    _assert_forward(lat.detach().reshape(-1, 64)[sel.to(hip_device)].cpu(), ref, R.border_mask(V, h, w)[sel], "full size")
    ((lat * d["g_lat"]).sum() + (dens * d["g_dens"]).sum()).backward()
    g_head = d["head"].grad
    assert torch.equal(g_head[:, 1:].reshape(V, 64, h * w), d["g_lat"].transpose(1, 2))
    assert torch.equal(g_head[:, 0].reshape(V, h * w), d["g_dens"])
    _assert_weight_grads(d["weight"].grad.cpu(), d["bias"].grad.cpu(), ref, "full size")


def test_abi_guards(hip_device):
    from freesplat_amd import _lib
    L = _lib.lib()
    V, h, w = 1, 16, 32
    t = lambda *s: torch.zeros(*s, device=hip_device)
    head, img, wt, b, lat, dens = t(V, 65, h, w), t(V, 3, h, w), t(64, 3, 7, 7), t(64), t(V, h * w, 64), t(V, h * w)
    saved = torch.zeros(L.fs_skip_latents_saved_bytes(V, h, w), dtype=torch.uint8, device=hip_device)
    scratch = torch.zeros(L.fs_skip_latents_scratch_bytes(V, h, w), dtype=torch.uint8, device=hip_device)
    assert saved.numel() == V * h * w * 8 and scratch.numel() > 0
    assert L.fs_skip_latents_saved_bytes(0, h, w) == 0 and L.fs_skip_latents_scratch_bytes(V, -1, w) == 0
    p, st = _lib.ptr, _lib.current_stream()
    fwd = lambda ci, co, k, hd=head: L.fs_skip_latents_forward(V, h, w, ci, co, k, p(hd), p(img), p(wt), p(b), p(lat), p(dens),
                                                               p(saved), st)
    assert fwd(3, 64, 7) == 0
    for ci, co, k in ((4, 64, 7), (3, 32, 7), (3, 64, 3), (3, 64, 6)):
        assert fwd(ci, co, k) == -3, (ci, co, k)
    assert fwd(3, 64, 7, hd=None) == -1 and fwd(3, 64, 0) == -1
    assert L.fs_skip_latents_forward(0, h, w, 3, 64, 7, p(head), p(img), p(wt), p(b), p(lat), p(dens), p(saved), st) == -1
    gw, gb, gh = t(64, 3, 7, 7), t(64), t(V, 65, h, w)
    bwd = lambda ci, co, k, im=img, sc=scratch, out=gw: L.fs_skip_latents_backward(
        V, h, w, ci, co, k, p(im), p(saved), p(lat), p(dens), p(gh), p(out), p(gb), p(sc), st)
    assert bwd(3, 64, 7) == 0
    assert bwd(3, 64, 5) == -3 and bwd(1, 64, 7) == -3
    assert bwd(3, 64, 7, im=None) == -1 and bwd(3, 64, 7, sc=None) == -1
    assert L.fs_skip_latents_backward(V, h, w, 3, 64, 7, p(img), p(saved), p(lat), p(dens), None, None, None, p(scratch), st) == -1
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="no CPU path"):
        from freesplat_amd.gaussian_adapter import skip_latents
        skip_latents(head.cpu(), img.cpu(), wt.cpu(), b.cpu())
    with pytest.raises(RuntimeError, match="no gradient"):
        skip_latents(head, img.clone().requires_grad_(True), wt, b)
