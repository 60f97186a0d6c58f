"""The adapter kernels (csrc/adapter.hip: unprojection and Gaussian head) restated in torch ops.  The restatement runs in the
dtype of its inputs: float64 is the reference of the tests, fp32 is what fixes their bounds (adapter_cases.ADAPTER_F32_VS_F64).

`head64(..., mutate=k)` is the CPU mutation check's switch: each value is one plausible kernel mistake (MUTATIONS).  Nothing
broken ever runs on a device: the mutated restatement is compared with the unmutated one."""
import torch


class _SymmetrisedGrad(torch.autograd.Function):
    """Identity whose backward symmetrises the cotangent of a [.., 3, 3] tensor (mutation 8)."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return 0.5 * (g + g.transpose(-1, -2))


class _UpperMirroredGrad(torch.autograd.Function):
    """Identity whose backward reads the cotangent's upper triangle only and mirrors it (mutation 9)."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        u = torch.triu(g)
        return u + torch.triu(g, 1).transpose(-1, -2)


# mutate value -> (what the mistake is, the groups of adapter_cases.GROUPS it must show in).
#  3 follows the issue's first clause: the raw-scale gradient loses its `depth` factor (g_raw[:, :3] as if sc = f(raw) * mult);
#    the value and g_depths stay right.
#  8 cannot show: cov = Rc A Rc^T is symmetric for every input, so <d cov, G> = <d cov, (G + G^T) / 2> and every gradient is
#    unchanged (in the kernel: dRc = G^T B + G Rc A^T = (G + G^T) Rc A).  It is kept to pin that equivalence; 9 is the
#    mistake next to it that does show, a g_cov assumed symmetric and read from one triangle.
MUTATIONS = {
    1: ("quaternion divide with its norm detached (no projection term)", ("g_raw_q",)),
    2: ("row 0's multiplier used for every row", ("scales", "cov")),
    3: ("depth factor missing from the raw-scale gradient", ("g_raw_s",)),
    4: ("one off-diagonal sign of R flipped", ("cov", "g_raw_q")),
    5: ("Rc^T A Rc instead of Rc A Rc^T", ("cov", "g_E")),
    6: ("SH mask indexed by c // 3 instead of c % d_sh", ("harmonics", "g_raw_sh")),
    7: ("1e-8 of the quaternion divide dropped", ("rotations", "g_raw_q")),
    8: ("g_cov symmetrised before use (equivalent: see above)", ()),
    9: ("g_cov read from its upper triangle and mirrored", ("g_E", "g_raw_q")),
}


def head64(raw, dep, E, mult, mask, smin=0.5, smax=15.0, mutate=0):
    """The head (gaussian_adapter.py:151-172, common/gaussians.py:8-44) in torch ops at any d_sh = mask.numel():
    raw [M, 7 + 3 d_sh] -> cov [M,3,3], sh [M,3,d_sh], scales [M,3], rotations [M,4] (xyzw).  mult: a scalar, [1] or [M]."""
    d_sh = mask.numel()
    mu = mult.reshape(-1, 1)
    if mutate == 2:
        mu = mu[:1]
    f = smin + (smax - smin) * torch.sigmoid(raw[:, :3])
    if mutate == 3:     # value unchanged; d sc / d raw without the depth factor, d sc / d depth as it should be
        sc = f.detach() * dep[:, None] * mu + (f - f.detach()) * mu
    else:
        sc = f * dep[:, None] * mu
    rq = raw[:, 3:7]
    n = rq.norm(dim=-1, keepdim=True)
    q = rq / ((n.detach() if mutate == 1 else n) + (0.0 if mutate == 7 else 1e-8))
    i, j, k, r = q.unbind(-1)
    two_s = 2.0 / ((q * q).sum(-1) + 1e-8)
    r01 = two_s * (i * j + k * r) if mutate == 4 else two_s * (i * j - k * r)
    R = torch.stack([1 - two_s * (j * j + k * k), r01, two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)], -1).view(-1, 3, 3)
    Mm = R * sc[:, None, :]
    Rc = E[:, :3, :3]
    if mutate == 5:
        Rc = Rc.transpose(-1, -2)
    cov = Rc @ (Mm @ Mm.transpose(-1, -2)) @ Rc.transpose(-1, -2)
    if mutate == 8:
        cov = _SymmetrisedGrad.apply(cov)
    if mutate == 9:
        cov = _UpperMirroredGrad.apply(cov)
    if mutate == 6:
        sh = (raw[:, 7:] * mask[torch.arange(3 * d_sh) // 3]).reshape(-1, 3, d_sh)
    else:
        sh = raw[:, 7:].reshape(-1, 3, d_sh) * mask
    return cov, sh, sc, q


def unproject64(depths, E, k0, h, w):
    """The unprojection (gaussian_adapter.py:36-79, 174-188): depths [V, h*w], c2w E [V,4,4] (any 3x4 top, not assumed rigid),
    k0 = (fx, fy, cx, cy) in pixels -- ONE set for all V views -- and integer pixel coordinates without the half-pixel offset.
    Returns world xyz [V, h*w, 3]."""
    dt = depths.dtype
    ys, xs = torch.meshgrid(torch.arange(h, dtype=dt), torch.arange(w, dtype=dt), indexing="ij")
    px = ((xs - k0[2]) / k0[0]).reshape(1, -1)
    py = ((ys - k0[3]) / k0[1]).reshape(1, -1)
    cam = torch.stack([px * depths, py * depths, depths], -1)                 # [V, P, 3]
    return cam @ E[:, :3, :3].transpose(-1, -2) + E[:, None, :3, 3]
