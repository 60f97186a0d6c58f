"""Float64 torch restatement of LPIPS (VGG-16) for the tests: the distance head and the whole module, written from the
formula, differentiated by torch's autograd.  It is the checker of freesplat_amd/lpips.py and csrc/lpips.hip, never a
fallback of theirs.  (`dtype` lets the same code run in float32: that is the "eager torch head" whose own error against
float64 sets the tests' tolerances.)

There is no fixture from the reference for this feature: the reference imports LPIPS from a third-party package that is
not in its tree, so nothing here can be pinned to recorded reference output.

  head:    dist[b] = sum_k mean_{h,w} sum_c w_kc (f0_kc / (|f0_k| + eps) - f1_kc / (|f1_k| + eps))^2,  eps = 1e-10,
           |.| the L2 norm over the channels of a pixel
  module:  x -> (2x - 1 if normalize) -> (x - shift) / scale -> VGG-16 features, taps after relu1_2, relu2_2, relu3_3,
           relu4_3, relu5_3 -> head with the five `lin` vectors
"""
import torch
import torch.nn.functional as F

EPS = 1e-10
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# convolutions (torchvision `features` indices) of the five slices; slices 2-5 start with a 2x2 max-pool
SLICES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))


def normalize_tensor(f, eps=EPS):
    return f / (f.pow(2).sum(dim=1, keepdim=True).sqrt() + eps)


def layer(f0, f1, w, dtype=torch.float64):
    """[B, C, H, W] x 2, w [C] -> [B]"""
    f0, f1, w = f0.to(dtype), f1.to(dtype), w.to(dtype)
    d = (normalize_tensor(f0) - normalize_tensor(f1)).pow(2)
    return (d * w.reshape(1, -1, 1, 1)).sum(dim=1).mean(dim=(1, 2))


def head(feats0, feats1, ws, dtype=torch.float64):
    return sum(layer(a, b, w, dtype) for a, b, w in zip(feats0, feats1, ws))


def layer_grad_closed_form(f0, f1, w, g_dist):
    """The gradient with d|f|/df = 0 at zero-norm pixels (the library's rule), float64, from the closed form:
    g_f0 = gs (a q - u (q . u) / |f0|), q = 2 w (u - v), u = a f0, v = b f1, a = 1 / (|f0| + eps), gs = g_dist / (H W)."""
    f0, f1, w = f0.double(), f1.double(), w.double().reshape(1, -1, 1, 1)
    n0 = f0.pow(2).sum(1, keepdim=True).sqrt()
    n1 = f1.pow(2).sum(1, keepdim=True).sqrt()
    a, b = 1 / (n0 + EPS), 1 / (n1 + EPS)
    u, v = f0 * a, f1 * b
    q = 2 * w * (u - v)
    gs = g_dist.double().reshape(-1, 1, 1, 1) / (f0.shape[2] * f0.shape[3])
    r0 = torch.where(n0 > 0, (q * u).sum(1, keepdim=True) / n0.clamp_min(1e-300), torch.zeros_like(n0))
    r1 = torch.where(n1 > 0, (q * v).sum(1, keepdim=True) / n1.clamp_min(1e-300), torch.zeros_like(n1))
    return gs * (a * q - u * r0), gs * (v * r1 - b * q)


def vgg_taps(x, state, dtype=torch.float64):
    """state: canonical keys (net.slice{k}.{i}.weight / .bias)"""
    taps = []
    for k, convs in enumerate(SLICES):
        if k:
            x = F.max_pool2d(x, 2, 2)
        for i in convs:
            x = F.relu(F.conv2d(x, state[f"net.slice{k + 1}.{i}.weight"].to(dtype), state[f"net.slice{k + 1}.{i}.bias"].to(dtype),
                                padding=1))
        taps.append(x)
    return taps


def module(in0, in1, state, normalize=False, dtype=torch.float64):
    """-> [B]"""
    shift = torch.tensor(SHIFT, dtype=dtype, device=in0.device).reshape(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=dtype, device=in0.device).reshape(1, 3, 1, 1)

    def prep(x):
        x = x.to(dtype)
        if normalize:
            x = 2 * x - 1
        return (x - shift) / scale

    state = {k: v.to(in0.device) for k, v in state.items()}
    t0, t1 = vgg_taps(prep(in0), state, dtype), vgg_taps(prep(in1), state, dtype)
    ws = [state[f"lin{k}.model.1.weight"].reshape(-1) for k in range(5)]
    return head(t0, t1, ws, dtype)
