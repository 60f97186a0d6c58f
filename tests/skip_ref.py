"""Float64 restatement of the fused skip branch (encoder_freesplat.py:124-128, :302-316) with the error bounds its tests use.

    lat = rearrange(head[:, 1:] + relu(conv2d(img, W, b, padding=3)), "n c h w -> n (h w) c")

evaluated on the CPU in float64, in bands of image rows (im2col of a band, then matrix products), so that the full-size case
needs no [V, 64, H, W] float64 map and no autograd graph.  The gradients are the analytic ones of that expression;
tests/test_skip_wiring.py::test_reference_restatement_is_torch_autograd checks them against torch's autograd on conv2d.

Bounds (u = 2^-24, the unit roundoff of fp32):
  forward   |lat - lat64| <= 150 u (|b| + sum_k |W||x| + |head|): a 148-term fp32 dot product plus two adds;
  ambiguous a (pixel, channel) whose float64 pre-activation is within 150 u (|b| + sum_k |W||x|) of zero: its ReLU may
            legitimately switch the other way in fp32;
  weights   |g - g64| <= n u sum |g_lat x| + sum_{ambiguous} |g_lat x|, n = V h w: the sequential-summation bound, valid for
            any order, plus exactly the terms that may flip (the bias gradient: x = 1).
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
FWD_FACTOR = 150.0


def reference(head, img, weight, bias, g_lat=None, select=None, band=64):
    """head [V,65,h,w], img [V,3,h,w], weight [64,3,7,7], bias [64] (CPU, any float dtype), g_lat [V, h*w, 64] or None.
    select: None (every pixel) or a sorted 1-D int64 tensor of flat pixel ids v * h*w + p whose latents are wanted.
    Returns a dict: lat, bound [n_sel, 64] float64 (rows in the order of `select`), ambiguous_share, and with g_lat:
    g_weight [64,3,7,7], g_bias [64], g_weight_bound, g_bias_bound (float64)."""
    V, _, h, w = head.shape
    P = h * w
    W64, b64 = weight.double().reshape(64, 147), bias.double()
    Wabs, babs = W64.abs(), b64.abs()
    lat_rows, bound_rows = [], []
    n_amb = 0
    gW = torch.zeros(64, 147, dtype=torch.float64)
    gb = torch.zeros(64, dtype=torch.float64)
    t_w, t_b, a_w, a_b = torch.zeros_like(gW), torch.zeros_like(gb), torch.zeros_like(gW), torch.zeros_like(gb)
    for v in range(V):
        x = F.pad(img[v].double(), (3, 3, 3, 3))
        for r0 in range(0, h, band):
            r1 = min(h, r0 + band)
            n = (r1 - r0) * w
            pat = F.unfold(x[None, :, r0:r1 + 6], 7)[0]                    # [147, n], rows in (ci, ky, kx) order
            pabs = pat.abs()
            pre = W64 @ pat + b64[:, None]
            mag = Wabs @ pabs + babs[:, None]
            hd = head[v, 1:, r0:r1].reshape(64, n).double()
            amb = pre.abs() <= FWD_FACTOR * U * mag
            n_amb += int(amb.sum())
            lo, hi = v * P + r0 * w, v * P + r1 * w
            if select is None:
                cols = slice(None)
            else:
                cols = select[(select >= lo) & (select < hi)] - lo
            lat_rows.append((hd + pre.clamp_min(0))[:, cols].T)
            bound_rows.append((FWD_FACTOR * U * (mag + hd.abs()))[:, cols].T)
            if g_lat is not None:
                g = g_lat[v, r0 * w:r1 * w].double().T                     # [64, n]
                gm = g * (pre > 0)
                gW += gm @ pat.T
                gb += gm.sum(1)
                t_w += gm.abs() @ pabs.T
                t_b += gm.abs().sum(1)
                ga = g.abs() * amb
                a_w += ga @ pabs.T
                a_b += ga.sum(1)
    out = {"lat": torch.cat(lat_rows), "bound": torch.cat(bound_rows), "ambiguous_share": n_amb / (V * P * 64)}
    if g_lat is not None:
        n = V * P
        out.update(g_weight=gW.reshape(64, 3, 7, 7), g_bias=gb, g_weight_bound=(n * U * t_w + a_w).reshape(64, 3, 7, 7),
                   g_bias_bound=n * U * t_b + a_b)
    return out


def make_inputs(V, h, w, seed):
    """Image uniform in [0, 1), nn.Conv2d's default initialisation, a normal head map and normal output gradients."""
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(3, 64, 7, 1, 3)
    g = torch.Generator().manual_seed(seed + 1)
    return {"head": torch.randn(V, 65, h, w, generator=g), "img": torch.rand(V, 3, h, w, generator=g),
            "weight": conv.weight.detach().clone(), "bias": conv.bias.detach().clone(),
            "g_lat": torch.randn(V, h * w, 64, generator=g), "g_dens": torch.randn(V, h * w, generator=g)}


def border_mask(V, h, w):
    """[V * h*w] bool: pixels in the first / last 3 rows or columns (whose patches reach the zero padding)."""
    m = torch.zeros(h, w, dtype=torch.bool)
    m[:3] = m[-3:] = True
    m[:, :3] = m[:, -3:] = True
    return m.reshape(-1).repeat(V)
