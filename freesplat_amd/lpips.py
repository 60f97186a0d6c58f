"""LPIPS (VGG-16) as FreeSplat uses it: the perceptual term of the training loss (src/loss/loss_lpips.py:27-55,
`MSE + 0.05 * LPIPS`) and the third evaluation metric (src/evaluation/metrics.py:22-34), without the third-party `lpips`
package.

The VGG-16 convolution stack is dense convolution and stays on torch / MIOpen.  Everything around it runs through
libfreesplat_hip.so (csrc/lpips.hip): the input side (optional 2x - 1, the scaling layer, prediction and target packed as
one batch) and the distance head (per tap layer: unit-normalise both feature maps over channels, square the difference,
weight by the learned `lin` vector, average over pixels; summed over the five taps), forward and backward, deterministic.
Device tensors only: there is no CPU / eager path.

Weights are never fetched.  `LPIPS(weights=...)` takes a path, a state dict, or a list of those (merged); without it the
path(s) in FREESPLAT_LPIPS_WEIGHTS (os.pathsep-separated) or what `set_default_weights()` / compat.patch_lpips() set.
Two key layouts are accepted, [3P-from-memory] both: the `lpips` package's own (`net.slice{1-5}.{N}.{weight,bias}`,
`lin{0-4}.model.1.weight`, optionally `lins.{k}.model.1.weight` and `scaling_layer.{shift,scale}`), and torchvision's
VGG-16 (`features.{N}.{weight,bias}`, `classifier.*` ignored) together with the package's linear-layer file
(`lin{k}.model.1.weight`).  The key names and the scaling layer's constants are written from memory of that package -- the
reference tree does not vendor it -- so a key that does not fit is a loud error that lists what was found.
"""
from __future__ import annotations

import functools
import math
import os
from typing import Optional

import torch
from torch import Tensor, nn

from . import _args, _lib

_device_f32 = functools.partial(_args.device_f32, name="freesplat_amd.lpips")

# VGG-16 `features`: (torchvision index, in, out) of every convolution of slice k; taps after relu1_2, relu2_2, relu3_3,
# relu4_3, relu5_3.  Slices 2-5 open with a 2x2 max-pool (torchvision indices 4, 9, 16, 23).  [3P-from-memory]
VGG_SLICES = (
    ((0, 3, 64), (2, 64, 64)),
    ((5, 64, 128), (7, 128, 128)),
    ((10, 128, 256), (12, 256, 256), (14, 256, 256)),
    ((17, 256, 512), (19, 512, 512), (21, 512, 512)),
    ((24, 512, 512), (26, 512, 512), (28, 512, 512)),
)
TAP_CHANNELS = tuple(s[-1][2] for s in VGG_SLICES)
# the scaling layer of the `lpips` package  [3P-from-memory]
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
ENV_WEIGHTS = "FREESPLAT_LPIPS_WEIGHTS"

_default_weights = None
_modules = {}            # device -> LPIPS built from the default weights (get_lpips)


def set_default_weights(weights) -> None:
    """What `LPIPS()` without a `weights` argument loads (before FREESPLAT_LPIPS_WEIGHTS): a path, a state dict, a list of
    those, "random", or None to clear.  compat.patch_lpips(weights) calls this."""
    global _default_weights
    _default_weights = weights
    _modules.clear()


# ---- the two library-backed autograd functions ----

class _Prepare(torch.autograd.Function):
    """in0, in1 [B, C, H, W] -> [2B, C, H, W] scaled (and 2x - 1 first with `normalize`), in0's images first."""

    @staticmethod
    def forward(ctx, in0, in1, shift, scale, normalize):
        B, C, H, W = in0.shape
        out = torch.empty(2 * B, C, H, W, device=in0.device)
        p = _lib.ptr
        _lib.launch("fs_lpips_prepare_forward", p(in0), p(in1), p(shift), p(scale), B, C, H, W, int(normalize), p(out))
        ctx.save_for_backward(scale)
        ctx.normalize = int(normalize)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        (scale,) = ctx.saved_tensors
        g_out = g_out.contiguous()
        B2, C, H, W = g_out.shape
        B = B2 // 2
        g0 = torch.empty(B, C, H, W, device=g_out.device) if ctx.needs_input_grad[0] else None
        g1 = torch.empty(B, C, H, W, device=g_out.device) if ctx.needs_input_grad[1] else None
        p = _lib.ptr
        _lib.launch("fs_lpips_prepare_backward", p(g_out), p(scale), B, C, H, W, ctx.normalize, p(g0), p(g1))
        return g0, g1, None, None, None


def _layer_forward(f0: Tensor, f1: Tensor, w: Tensor, dist: Tensor) -> Tensor:
    """dist[B] += this layer's distance; returns the per-pixel scalars the backward needs."""
    B, C, H, W = f0.shape
    L = _lib.lib()
    saved = torch.empty(L.fs_lpips_saved_bytes(B, C, H, W) // 4, device=f0.device)
    scratch = torch.empty(L.fs_lpips_scratch_bytes(B, C, H, W), dtype=torch.uint8, device=f0.device)
    p = _lib.ptr
    _lib.launch("fs_lpips_layer_forward", p(f0), p(f1), p(w), B, C, H, W, p(dist), p(saved), p(scratch))
    return saved


def _layer_backward(g_dist: Tensor, f0: Tensor, f1: Tensor, w: Tensor, saved: Tensor, g_f0: Optional[Tensor],
                    g_f1: Optional[Tensor]) -> None:
    B, C, H, W = f0.shape
    p = _lib.ptr
    _lib.launch("fs_lpips_layer_backward", p(g_dist), p(f0), p(f1), p(w), p(saved), B, C, H, W, p(g_f0), p(g_f1))


class _Head(torch.autograd.Function):
    """dist [B] = sum over layers of the normalised, `lin`-weighted squared feature distance.  Per layer either one packed
    [2B, C, H, W] map (first half against second half; its gradient is written in place into one packed tensor) or two
    [B, C, H, W] maps.  args = (n_layers, packed, w_0 .. w_{n-1}, then per layer one or two maps)."""

    @staticmethod
    def forward(ctx, n, packed, *args):
        ws, maps = args[:n], args[n:]
        pairs = []
        for k in range(n):
            if packed:
                f = maps[k].contiguous()
                B = f.shape[0] // 2
                pairs.append((f, f[:B], f[B:]))
            else:
                pairs.append((None, maps[2 * k].contiguous(), maps[2 * k + 1].contiguous()))
        B = pairs[0][1].shape[0]
        dist = torch.zeros(B, device=pairs[0][1].device)
        saved = [_layer_forward(f0, f1, w, dist) for (_, f0, f1), w in zip(pairs, ws)]
        ctx.n, ctx.packed = n, packed
        ctx.save_for_backward(*ws, *saved, *[t for pk, f0, f1 in pairs for t in ((pk,) if packed else (f0, f1))])
        return dist

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_dist):
        n, packed = ctx.n, ctx.packed
        t = ctx.saved_tensors
        ws, saved, maps = t[:n], t[n:2 * n], t[2 * n:]
        g_dist = g_dist.float().contiguous()
        need = ctx.needs_input_grad[2 + n:]
        grads = []
        for k in range(n):
            if packed:
                f = maps[k]
                B = f.shape[0] // 2
                if need[k]:
                    g = torch.empty_like(f)
                    _layer_backward(g_dist, f[:B], f[B:], ws[k], saved[k], g[:B], g[B:])
                    grads.append(g)
                else:
                    grads.append(None)
            else:
                f0, f1 = maps[2 * k], maps[2 * k + 1]
                g0 = torch.empty_like(f0) if need[2 * k] else None
                g1 = torch.empty_like(f1) if need[2 * k + 1] else None
                if g0 is not None or g1 is not None:
                    _layer_backward(g_dist, f0, f1, ws[k], saved[k], g0, g1)
                grads += [g0, g1]
        return (None, None) + (None,) * n + tuple(grads)


def lpips_head(feats0, feats1, lin_weights) -> Tensor:
    """The distance head on its own: lists of [B, C_k, H_k, W_k] device maps and [C_k] weights -> dist [B]."""
    f0 = [_device_f32(f, "feature map") for f in feats0]
    f1 = [_device_f32(f, "feature map") for f in feats1]
    ws = [_device_f32(w, "lin weight").reshape(-1) for w in lin_weights]
    if not (len(f0) == len(f1) == len(ws)) or not f0:
        raise ValueError("freesplat_amd.lpips: need as many feature maps of each side as lin weights")
    for a, b, w in zip(f0, f1, ws):
        if a.dim() != 4 or a.shape != b.shape or w.numel() != a.shape[1] or a.shape[0] != f0[0].shape[0]:
            raise ValueError(f"freesplat_amd.lpips: feature maps {tuple(a.shape)} / {tuple(b.shape)}, weights {tuple(w.shape)}")
    return _Head.apply(len(ws), False, *ws, *[t for pair in zip(f0, f1) for t in pair])


# ---- weights ----

def _slice_of(index: int) -> int:
    for k, convs in enumerate(VGG_SLICES):
        if any(index == i for i, _, _ in convs):
            return k + 1
    raise KeyError(index)


def expected_keys() -> dict:
    """canonical key (the `lpips` package's layout) -> shape"""
    keys = {}
    for k, convs in enumerate(VGG_SLICES):
        for i, cin, cout in convs:
            keys[f"net.slice{k + 1}.{i}.weight"] = (cout, cin, 3, 3)
            keys[f"net.slice{k + 1}.{i}.bias"] = (cout,)
        keys[f"lin{k}.model.1.weight"] = (1, TAP_CHANNELS[k], 1, 1)
    return keys


def canonical_state(state: dict) -> dict:
    """Map either accepted key layout onto the canonical one.  Unknown keys, missing keys and wrong shapes raise a KeyError /
    ValueError that names them and lists the keys that were found."""
    want = expected_keys()
    out, unknown = {}, []
    found = sorted(state)

    def put(key, value):
        value = torch.as_tensor(value).detach()
        if key in out and not torch.equal(out[key].cpu().float(), value.cpu().float()):
            raise ValueError(f"freesplat_amd.lpips: two different tensors for {key} in the given weights")
        out[key] = value

    for key, value in state.items():
        parts = key.split(".")
        if key in want or key in ("scaling_layer.shift", "scaling_layer.scale"):
            put(key, value)
        elif parts[0] == "features" and len(parts) == 3 and parts[1].isdigit() and parts[2] in ("weight", "bias"):
            try:
                put(f"net.slice{_slice_of(int(parts[1]))}.{parts[1]}.{parts[2]}", value)
            except KeyError:
                unknown.append(key)
        elif parts[0] == "lins" and len(parts) == 5 and f"lin{parts[1]}.{'.'.join(parts[2:])}" in want:
            put(f"lin{parts[1]}.{'.'.join(parts[2:])}", value)
        elif parts[0] == "classifier":          # the rest of torchvision's VGG-16: not part of LPIPS
            continue
        else:
            unknown.append(key)
    missing = [k for k in want if k not in out]
    if unknown or missing:
        raise KeyError(f"freesplat_amd.lpips: weights do not fit the VGG-16 LPIPS layout: missing {missing or 'nothing'}, "
                       f"unexpected {unknown or 'nothing'}; keys found: {found}")
    for key, shape in want.items():
        if tuple(out[key].shape) != shape:
            raise ValueError(f"freesplat_amd.lpips: {key} has shape {tuple(out[key].shape)}, expected {shape}")
    for key in ("scaling_layer.shift", "scaling_layer.scale"):
        if key in out and out[key].numel() != 3:
            raise ValueError(f"freesplat_amd.lpips: {key} has shape {tuple(out[key].shape)}, expected 3 values")
    return out


def random_state(seed: int = 0) -> dict:
    """He-initialised convolutions and non-negative `lin` vectors (tests and benchmarks), canonical keys, CPU float32."""
    gen = torch.Generator().manual_seed(seed)
    state = {}
    for key, shape in expected_keys().items():
        if key.startswith("lin"):
            state[key] = torch.rand(shape, generator=gen) / shape[1]
        elif key.endswith("bias"):
            state[key] = 0.1 * torch.randn(shape, generator=gen)
        else:
            state[key] = torch.randn(shape, generator=gen) * math.sqrt(2.0 / (shape[1] * 9))
    return state


def _load(weights) -> dict:
    if isinstance(weights, dict):
        return dict(weights)
    if isinstance(weights, (list, tuple)):
        merged = {}
        for w in weights:
            merged.update(_load(w))
        return merged
    if isinstance(weights, (str, os.PathLike)):
        path = os.fspath(weights)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"freesplat_amd.lpips: weights file {path} not found (weights are never fetched)")
        state = torch.load(path, map_location="cpu", weights_only=True)
        if isinstance(state, dict) and "state_dict" in state and isinstance(state["state_dict"], dict):
            state = state["state_dict"]
        if not isinstance(state, dict):
            raise ValueError(f"freesplat_amd.lpips: {path} does not hold a state dict")
        return dict(state)
    raise TypeError(f"freesplat_amd.lpips: weights must be a path, a state dict or a list of those, got {type(weights)}")


def resolve_weights(weights=None, seed: int = 0) -> dict:
    """`weights` -> canonical state dict; None: set_default_weights()'s value, then FREESPLAT_LPIPS_WEIGHTS, else ValueError."""
    if weights is None:
        weights = _default_weights
    if weights is None and os.environ.get(ENV_WEIGHTS):
        paths = [p for p in os.environ[ENV_WEIGHTS].split(os.pathsep) if p]
        weights = paths if len(paths) > 1 else paths[0]
    if weights is None:
        raise ValueError(
            "freesplat_amd.lpips: no LPIPS weights.  Pass LPIPS(weights=<path | state dict | list of those>), or set "
            f"{ENV_WEIGHTS} to the file(s) ({os.pathsep!r}-separated): either a state dict of the `lpips` package's "
            "LPIPS(net='vgg'), or torchvision's VGG-16 state dict plus the package's linear-layer file (lin{k}.model.1.weight)."
            "  Weights are never downloaded; weights='random' gives a seeded random network for tests and benchmarks.")
    if isinstance(weights, str) and weights == "random":
        return random_state(seed)
    return canonical_state(_load(weights))


# ---- the module ----

class _Lin(nn.Module):
    def __init__(self, channels: int):
        super().__init__()
        self.model = nn.Sequential(nn.Identity(), nn.Conv2d(channels, 1, 1, bias=False))   # (the package: Dropout, Conv2d)


class _ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(SHIFT)[None, :, None, None])
        self.register_buffer("scale", torch.tensor(SCALE)[None, :, None, None])


class _VGG16(nn.Module):
    def __init__(self):
        super().__init__()
        for k, convs in enumerate(VGG_SLICES):
            seq = nn.Sequential()
            first = convs[0][0]
            if k:
                seq.add_module(str(first - 1), nn.MaxPool2d(kernel_size=2, stride=2))
            for i, cin, cout in convs:
                seq.add_module(str(i), nn.Conv2d(cin, cout, 3, padding=1))
                seq.add_module(str(i + 1), nn.ReLU(inplace=False))
            setattr(self, f"slice{k + 1}", seq)

    def forward(self, x):
        taps = []
        for k in range(len(VGG_SLICES)):
            x = getattr(self, f"slice{k + 1}")(x)
            taps.append(x)
        return taps


def _to_buffers(module: nn.Module) -> None:
    """Every parameter becomes a (persistent) buffer: nothing of LPIPS is trainable, nothing reaches an optimiser."""
    for child in module.children():
        _to_buffers(child)
    for name, p in list(module.named_parameters(recurse=False)):
        value = p.detach().clone()
        delattr(module, name)
        module.register_buffer(name, value)


class LPIPS(nn.Module):
    """`lpips.LPIPS(net="vgg")` as FreeSplat calls it: forward(in0, in1, normalize=False) -> [B, 1, 1, 1].  Gradients flow to
    whichever of in0, in1 requires them.  State-dict keys are the `lpips` package's."""

    def __init__(self, net: str = "vgg", weights=None, seed: int = 0, **unused):
        super().__init__()
        if net != "vgg":
            raise NotImplementedError(f"freesplat_amd.lpips: net={net!r}; FreeSplat only ever builds LPIPS(net='vgg')")
        for k, v in unused.items():
            # the package's other switches at the values FreeSplat leaves them at
            if k not in ("pretrained", "version", "lpips", "spatial", "pnet_rand", "pnet_tune", "use_dropout", "eval_mode",
                         "verbose", "model_path") or (k == "spatial" and v) or (k == "lpips" and not v):
                raise NotImplementedError(f"freesplat_amd.lpips: LPIPS({k}={v!r}) is not supported")
        state = resolve_weights(weights, seed)
        self.scaling_layer = _ScalingLayer()
        self.net = _VGG16()
        for k, c in enumerate(TAP_CHANNELS):
            setattr(self, f"lin{k}", _Lin(c))
        _to_buffers(self)
        own = self.state_dict()
        for key, value in state.items():
            own[key].copy_(value.reshape(own[key].shape).to(own[key].dtype))
        self.eval()

    def lin_weights(self):
        return [getattr(self, f"lin{k}").model[1].weight.reshape(-1) for k in range(len(TAP_CHANNELS))]

    def forward(self, in0: Tensor, in1: Tensor, normalize: bool = False, retPerLayer: bool = False) -> Tensor:
        if retPerLayer:
            raise NotImplementedError("freesplat_amd.lpips: retPerLayer is not supported")
        in0 = _device_f32(in0, "in0")
        in1 = _device_f32(in1, "in1")
        if in0.dim() != 4 or in0.shape != in1.shape or in0.shape[1] != 3 or in0.shape[0] == 0:
            raise ValueError(f"freesplat_amd.lpips: expected two [B, 3, H, W] tensors of one shape, got {tuple(in0.shape)} and "
                             f"{tuple(in1.shape)}")
        if in0.device != in1.device or in0.device != self.scaling_layer.shift.device:
            raise ValueError(f"freesplat_amd.lpips: inputs on {in0.device} and {in1.device}, module on "
                             f"{self.scaling_layer.shift.device}")
        if min(in0.shape[2:]) < 16:
            raise ValueError(f"freesplat_amd.lpips: images of {in0.shape[2]}x{in0.shape[3]} vanish in VGG-16's four poolings")
        B = in0.shape[0]
        x = _Prepare.apply(in0, in1, self.scaling_layer.shift.reshape(-1), self.scaling_layer.scale.reshape(-1), normalize)
        ws = self.lin_weights()
        grad = torch.is_grad_enabled()
        need0, need1 = grad and in0.requires_grad, grad and in1.requires_grad
        if need0 == need1:
            # one pass of the convolutions over both halves; the head reads (and differentiates) the packed maps in place
            dist = _Head.apply(len(ws), True, *ws, *self.net(x))
        else:
            # training (only the prediction carries a gradient): the target's half runs without a graph, so its
            # activations are not kept and the convolutions' backward sees B images, not 2B
            with torch.no_grad():
                t_const = self.net(x[B:] if need0 else x[:B])
            t_grad = self.net(x[:B] if need0 else x[B:])
            pairs = zip(t_grad, t_const) if need0 else zip(t_const, t_grad)
            dist = _Head.apply(len(ws), False, *ws, *[t for pair in pairs for t in pair])
        return dist.reshape(B, 1, 1, 1)


# ---- the reference's two call sites ----

def get_lpips(device) -> LPIPS:
    """One module per device (src/evaluation/metrics.py:22-24), built from the default weights."""
    device = torch.device(device)
    if device not in _modules:
        _modules[device] = LPIPS(net="vgg").to(device)
    return _modules[device]


@torch.no_grad()
def compute_lpips(ground_truth: Tensor, predicted: Tensor) -> Tensor:
    """[batch] LPIPS of images in [0, 1] (metrics.py:27-34: normalize=True, no gradient)."""
    predicted = _device_f32(predicted, "predicted")
    value = get_lpips(predicted.device).forward(ground_truth, predicted, normalize=True)
    return value[:, 0, 0, 0]


def lpips_loss(prediction_color: Tensor, target_image: Tensor, weight: float, apply_after_step: int, global_step: int,
               module: Optional[LPIPS] = None) -> Tensor:
    """LossLpips.forward (loss_lpips.py:36-55): [b, v, 3, h, w] prediction and target -> weight * mean LPIPS (inputs taken as
    they are, normalize=False); a zero before `apply_after_step`, returned without touching the library."""
    if global_step < apply_after_step:
        return torch.tensor(0, dtype=torch.float32, device=target_image.device)
    if module is None:
        module = get_lpips(_device_f32(target_image, "target_image").device)
    loss = module.forward(prediction_color.flatten(0, 1), target_image.flatten(0, 1))
    return weight * loss.mean()
