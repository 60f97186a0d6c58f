"""Restatement of the fused Gaussian Adam step (csrc/gaussian_adam.hip, include/freesplat_amd_optim.h) in plain torch:
float64 on the CPU as the reference, and the same formulas in float32 on a device as the yardstick of fp32 rounding (the
`E` of the tests' bound).  It covers the chain rule through exp / sigmoid, the six learning-rate groups, row visibility
(sparse Adam: a row that is not visible keeps its parameters and moments, the step number t is global) and arrays without a
gradient.  Written from the definition of torch.optim.Adam (no weight decay, no amsgrad); tests/test_gaussian_adam_host.py
checks it against torch.optim.Adam itself.
"""
from __future__ import annotations

import torch

MEANS, SCALES, ROTATIONS, OPACITIES, SHS = range(5)
ARRAYS = ("means", "log_scales", "rotations", "logits", "shs")                      # raw parameters, the order of every list
GROUPS = ("means", "scales", "rotations", "opacity", "sh_dc", "sh_rest")
DEFAULT_LR = dict(means=1.6e-4, sh_dc=2.5e-3, sh_rest=1.25e-4, opacity=5e-2, scales=5e-3, rotations=1e-3)
N_SHAPES = (1, 3, 63, 64, 65, 257, 1031)
M_SHAPES = (1, 4, 9, 16)
K_STEPS = 5


def make_inputs(N: int, M: int, K: int = K_STEPS, seed: int = 0):
    """(raw, grads): raw = five float32 CPU tensors (means ~ N(0, 10), log-scales ~ N(0, 3), rotations ~ N(0, 1), logits ~
    N(0, 3) clamped to [-6, 6], shs ~ N(0, 1)); grads = K lists of five gradients with respect to the ACTIVATED values,
    |g| = |normal| * 10^U(-4, 2), fresh for every step."""
    gen = torch.Generator().manual_seed(1000 * N + 10 * M + seed)
    shapes = [(N, 3), (N, 3), (N, 4), (N,), (N, M, 3)]
    sigma = [10.0, 3.0, 1.0, 3.0, 1.0]
    raw = [s * torch.randn(shape, generator=gen) for s, shape in zip(sigma, shapes)]
    raw[OPACITIES].clamp_(-6.0, 6.0)
    grads = [[torch.randn(shape, generator=gen) * 10.0 ** (6.0 * torch.rand(shape, generator=gen) - 4.0) for shape in shapes]
             for _ in range(K)]
    return raw, grads


def radii_pattern(N: int, k: int) -> torch.Tensor:
    """int32 [N] with zeros, negatives and positives; runs of 1, 2, 3, 5 rows so that the changes fall inside 16-byte groups
    of the width-1, -3, -4 and -27 arrays.  `k` shifts the pattern."""
    i = torch.arange(N) + k
    r = torch.where((i % 11 < 5) | (i % 3 == 0), 7, 0)
    r = torch.where(i % 7 == 2, -3, r)
    return r.to(torch.int32)


class RefAdam:
    """The step on lists of tensors of `dtype` on `device`.  p: raw parameters; m, v: moments; t: steps taken."""

    def __init__(self, raw, lr=None, betas=(0.9, 0.999), eps=1e-15, dtype=torch.float64, device="cpu"):
        self.p = [t.detach().to(device=device, dtype=dtype).clone() for t in raw]
        self.m = [torch.zeros_like(t) for t in self.p]
        self.v = [torch.zeros_like(t) for t in self.p]
        self.t = 0
        self.lr = dict(DEFAULT_LR, **(lr or {}))
        self.betas, self.eps = betas, eps

    def _rate(self, k: int):
        if k != SHS:
            return self.lr[GROUPS[k]]
        M = self.p[SHS].shape[1]
        r = torch.full((1, M, 1), self.lr["sh_rest"], dtype=self.p[SHS].dtype, device=self.p[SHS].device)
        r[:, 0] = self.lr["sh_dc"]
        return r

    def activated(self):
        return torch.exp(self.p[SCALES]), torch.sigmoid(self.p[OPACITIES])

    def step(self, grads, visible=None) -> None:
        """grads: five gradients with respect to means, scales, rotations, opacities, shs (None: that array is left alone);
        visible: None or integer [N], rows with a value <= 0 are skipped (whatever their gradients hold)."""
        self.t += 1                                       # global: it advances whatever is visible
        b1, b2 = self.betas
        bc1, bc2 = 1.0 - b1 ** self.t, 1.0 - b2 ** self.t
        for k in range(5):
            if grads[k] is None:
                continue
            p, m, v = self.p[k], self.m[k], self.v[k]
            g = grads[k].to(device=p.device, dtype=p.dtype).reshape(p.shape)
            if k == SCALES:
                g = g * torch.exp(p)
            if k == OPACITIES:
                o = torch.sigmoid(p)
                g = g * o * (1.0 - o)
            m_new = b1 * m + (1.0 - b1) * g
            v_new = b2 * v + (1.0 - b2) * g * g
            p_new = p - (self._rate(k) / bc1) * (m_new / (v_new.sqrt() / bc2 ** 0.5 + self.eps))
            if visible is not None:
                on = (visible.to(p.device) > 0).reshape((-1,) + (1,) * (p.dim() - 1))
                p_new, m_new, v_new = torch.where(on, p_new, p), torch.where(on, m_new, m), torch.where(on, v_new, v)
            self.p[k], self.m[k], self.v[k] = p_new, m_new, v_new


def err(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max |got - ref| in float64 on the CPU."""
    ref = ref.detach().double().cpu()
    return float((got.detach().double().cpu().reshape(ref.shape) - ref).abs().max())


def bound(E: float, ref: torch.Tensor, K: int) -> float:
    """max(4 E, K 2^-23 max|ref|): E = the error of the fp32 restatement on the same device against the same float64
    result; the floor allows K roundings of the stored value (half an ulp each), doubled for the update's own arithmetic."""
    return max(4.0 * E, K * 2.0 ** -23 * float(ref.detach().abs().max()))
