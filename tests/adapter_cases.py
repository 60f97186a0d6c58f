"""The branch-edge rows of the adapter kernels (csrc/adapter.hip), in classes, with the figure and the bounds of the tests on
them (test_adapter_edges_host.py on the CPU, test_adapter_edges_hip.py on the device).

Each class is judged on its own with util_raster.per_gaussian_err: a row's error over that row's own largest entry, floored at
1e-4 of the class's largest.  So a class holds rows of ONE magnitude per group: the quaternion rows are split by their norm
(d raw_q ~ 1 / |q|: one class of norms 1e-3 ... 1e15 would judge every row but the shortest at the floor), the depths likewise.

Every class is laid out at M = 1 and M = 300 (one full 256-row workgroup and a ragged one at d_sh 1 / 4 / 9; two full 128-row
ones and a ragged one at d_sh 16).  The edge rows of a class repeat cyclically over the rows, shifted by the degree, so each
kind sits at the first row, either side of the boundaries (127 | 128, 255 | 256) and in the ragged tail; the other columns of
such a row are random."""
from math import isqrt

import numpy as np
import torch

from adapter_ref import head64, unproject64
from util_raster import per_gaussian_err

D_SHS = (1, 4, 9, 16)
MS = (1, 300)
CLASSES = ("plain", "scales", "quat_1e-3", "quat_1", "quat_1e3", "quat_1e15", "tiny_quat", "depth_small", "depth_large",
           "depth_mixed", "extrinsics", "extrinsics_off16")
COTANGENTS = ("cov", "sh", "scales", "rot")
COT_SETS = (COTANGENTS, ("cov",), ("sh",), ("scales",), ("rot",))
FWD_GROUPS = ("cov", "scales", "rotations")
BWD_GROUPS = ("g_raw_s", "g_raw_q", "g_depths", "g_E")
SMIN, SMAX = 0.5, 15.0
MULT_ONE = 0.0123


def sh_mask(d_sh):
    """GaussianAdapter.sh_mask (gaussian_adapter.py:127-133) at d_sh = (degree + 1)^2."""
    m = torch.ones(d_sh, dtype=torch.float32)
    for degree in range(1, isqrt(d_sh)):
        m[degree ** 2:(degree + 1) ** 2] = 0.1 * 0.25 ** degree
    return m


def _rotations(n, rng):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    i, j, k, r = q.T
    return np.stack([1 - 2 * (j * j + k * k), 2 * (i * j - k * r), 2 * (i * k + j * r),
                     2 * (i * j + k * r), 1 - 2 * (i * i + k * k), 2 * (j * k - i * r),
                     2 * (i * k - j * r), 2 * (j * k + i * r), 1 - 2 * (i * i + j * j)], -1).reshape(n, 3, 3)


# raw scale channels: sigmoid exactly 0 (-90) and exactly 1 (+20, +90) in fp32, a subnormal-free 2e-9 (-20), mixed within a row
_SCALE_ROWS = ((0.0, 5.0, -5.0), (0.0, 20.0, -20.0), (0.0, 90.0, -90.0), (5.0, 20.0, 90.0), (-5.0, -20.0, -90.0),
               (20.0, 0.0, -90.0), (90.0, -5.0, 20.0), (-20.0, 5.0, 0.0), (90.0, 90.0, -90.0), None)
# quaternion directions (xyzw), scaled to the class's norm: the axes, w < 0, one and two zero components, random
_QUAT_ROWS = ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (0, 0, 0, -1), "w_neg", "zero_1", "zero_2", "zero_w", None)
_TINY_ROWS = ("zero", "one_1e-20", 1e-9, 1e-8, 1e-7)
_E_ROWS = (None, "mean_of_two", "reflection", "three_times", "zero_block")

_cache = {}


def build_case(cls, d_sh, M):
    """One class at one degree and size: fp32 CPU tensors raw [M, 7 + 3 d_sh], dep [M], E [M,4,4], mult [1] | [M], mask [d_sh],
    the cotangents g_cov (never symmetric), g_sh, g_scales, g_rot, and e_offset: the floats by which the extrinsics are to be
    moved off the 16-byte grid where they are placed (place()).  Computed once and shared: read-only."""
    key = (cls, d_sh, M)
    if key in _cache:
        return _cache[key]
    assert cls in CLASSES and d_sh in D_SHS
    shift = D_SHS.index(d_sh)
    seed = 1000 * CLASSES.index(cls.replace("_off16", "")) + 10 * d_sh + (M > 1)
    gen = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    raw = rn(M, 7 + 3 * d_sh)
    dep = 1.0 + torch.rand(M, generator=gen)
    E = torch.eye(4).repeat(M, 1, 1) + 0.1 * rn(M, 4, 4)
    mult = torch.tensor([MULT_ONE])
    c = dict(cls=cls, d_sh=d_sh, M=M, e_offset=0, mask=sh_mask(d_sh), g_cov=rn(M, 3, 3), g_sh=rn(M, 3, d_sh),
             g_scales=rn(M, 3), g_rot=rn(M, 4))
    per_row_mult = lambda: 10.0 ** (-3.0 + 2.0 * torch.rand(M, generator=gen))      # two decades, 1e-3 ... 1e-1
    kind = lambda rows, m: rows[(m + shift) % len(rows)]
    if cls == "plain":
        mult = per_row_mult()
    elif cls == "scales":
        for m in range(M):
            k = kind(_SCALE_ROWS, m)
            if k is not None:
                raw[m, :3] = torch.tensor(k)
    elif cls.startswith("quat_"):
        norm = float(cls[5:])
        for m in range(M):
            k = kind(_QUAT_ROWS, m)
            q = rng.normal(size=4)
            if k == "w_neg":
                q[3] = -abs(q[3])
            elif k == "zero_1":
                q[m % 3] = 0.0
            elif k == "zero_w":
                q[3] = 0.0
            elif k == "zero_2":
                q[m % 4] = q[(m + 1 + m // 4 % 3) % 4] = 0.0
            elif k is not None:
                q = np.asarray(k, np.float64)
            q *= norm * rng.uniform(0.5, 2.0) / np.linalg.norm(q)
            raw[m, 3:7] = torch.from_numpy(q.astype(np.float32))
    elif cls == "tiny_quat":
        for m in range(M):
            k = kind(_TINY_ROWS, m)
            q = np.zeros(4)
            if k == "one_1e-20":
                q[m % 4] = 1e-20 * (-1.0) ** m
            elif k != "zero":
                q = rng.normal(size=4)
                q *= k / np.linalg.norm(q)
            raw[m, 3:7] = torch.from_numpy(q.astype(np.float32))
    elif cls == "depth_small":
        dep = 1e-3 * (0.5 + 1.5 * torch.rand(M, generator=gen))
        dep[shift % 2::2] = 1e-3
    elif cls == "depth_large":
        dep = 80.0 * (0.5 + 0.5 * torch.rand(M, generator=gen))
        dep[shift % 2::2] = 80.0
    elif cls == "depth_mixed":
        mult = per_row_mult()
        for m in range(M):
            dep[m] = (1e-3, 1.0, 80.0)[(m + shift) % 3] * (1.0 if m % 2 else float(dep[m]) / 2.0)
    else:       # extrinsics, extrinsics_off16: the same rows, the second given as a view one float into a larger buffer
        Ra, Rb = _rotations(M, rng), _rotations(M, rng)
        for m in range(M):
            k = kind(_E_ROWS, m)
            if k == "mean_of_two":
                B = 0.5 * (Ra[m] + Rb[m])
            elif k == "reflection":
                B = Ra[m] @ np.diag([1.0, 1.0, -1.0])
            elif k == "three_times":
                B = 3.0 * Ra[m]
            elif k == "zero_block":
                B = np.zeros((3, 3))
            else:
                continue
            E[m, :3, :3] = torch.from_numpy(B.astype(np.float32))
        c["e_offset"] = int(cls.endswith("_off16"))
    c.update(raw=raw, dep=dep, E=E.contiguous(), mult=mult)
    _cache[key] = c
    return c


def place(t, device="cpu", offset=0):
    """t on `device`, contiguous; offset > 0: as a view `offset` floats into a larger buffer, i.e. off the 16-byte grid."""
    if not offset:
        return t.to(device).contiguous()
    buf = torch.empty(t.numel() + offset + 3, dtype=t.dtype, device=device)
    v = buf[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def assert_cases_present(case, E_placed=None):
    """The properties the tests on a class rely on hold in fp32 (as util_raster.assert_edge_cases_present does for the
    rasterizer's scene), so that a change of the generator fails the tests instead of emptying them.  E_placed: the extrinsics
    as handed to the code under test.  Returns the counts."""
    cls, M, raw = case["cls"], case["M"], case["raw"]
    assert raw.dtype == torch.float32 and raw.shape == (M, 7 + 3 * case["d_sh"])
    sig = 1.0 / (1.0 + torch.exp(-raw[:, :3]))                  # the kernel's expression, fp32
    nq = (raw[:, 3:7] * raw[:, 3:7]).sum(-1).sqrt()
    g = case["g_cov"]
    n = dict(sig_0=int((sig == 0).sum()), sig_1=int((sig == 1).sum()), sig_dead=int(((sig * (1 - sig)) == 0).sum()),
             nq_0=int((nq == 0).sum()), nq_below_eps=int(((nq > 0) & (nq <= 1e-8)).sum()),
             mult_per_row=int(case["mult"].numel() == M), mult_one=int(case["mult"].numel() == 1),
             E_off_grid=int(E_placed is not None and E_placed.data_ptr() % 16 != 0),
             g_cov_asymmetric=int(((g - g.transpose(-1, -2)).abs().amax((1, 2)) > 1e-3).sum()))
    assert n["g_cov_asymmetric"] == M, n
    assert bool(torch.isfinite(raw).all()) and bool(torch.isfinite(raw[:, 3:7] ** 2).all())     # the squares fit fp32
    if cls in ("plain", "depth_mixed"):
        assert n["mult_per_row"] and (M == 1 or float(case["mult"].max() / case["mult"].min()) > 30.0), n
    else:
        assert n["mult_one"], n
    if cls == "extrinsics_off16":
        assert E_placed is not None and n["E_off_grid"] and E_placed.is_contiguous(), n
    elif E_placed is not None:
        assert not n["E_off_grid"], n
    if cls == "quat_1e15":
        assert float(nq.min()) >= 4e14 and float(nq.max()) <= 2.1e15
    big = M > 1
    if cls == "scales":
        assert n["sig_0"] >= (30 if big else 0) and n["sig_1"] >= (30 if big else 0) and n["sig_dead"] >= (60 if big else 0), n
        assert M > 1 or bool((raw[0, :3].abs() >= 5).any()), "the single row has no edge channel"
    if cls == "tiny_quat":
        assert float(nq.max()) <= 1.01e-7
        if big:
            assert n["nq_0"] >= 50 and n["nq_below_eps"] >= 100 and int((nq > 5e-8).sum()) >= 50, n
            assert int(((raw[:, 3:7] != 0).sum(-1) == 1).sum()) >= 50       # the one-component 1e-20 rows
    if cls == "extrinsics" or cls == "extrinsics_off16":
        if big:
            B = case["E"][:, :3, :3].double()
            det = torch.linalg.det(B)
            orth = (B @ B.transpose(-1, -2) - torch.eye(3, dtype=torch.float64)).abs().amax((1, 2))
            assert int((det < -0.99).sum()) >= 50 and int((det > 26.9).sum()) >= 50 and int((B.abs().amax((1, 2)) == 0).sum()) >= 50
            assert int((orth > 0.05).sum()) >= 200          # nothing but the reflections is orthonormal
    return n


# ------------------------------------------------------------------------------------------------------ reference and figure
def run_head(case, cots, dtype=torch.float64, mutate=0):
    """The restatement and its autograd on a case for the cotangent set `cots`, in `dtype`.  Returns the forward outputs and
    the gradients (zeros where none arrives) as a dict of CPU tensors.  float64, unmutated results of build_case's own cases are
    computed once and shared: read-only."""
    key = ("ref", case["cls"], case["d_sh"], case["M"], cots)
    shared = dtype == torch.float64 and not mutate and _cache.get(key[1:4]) is case     # (a modified copy of a case is not)
    if shared and key in _cache:
        return _cache[key]
    leaf = lambda t: t.to(dtype).clone().requires_grad_(True)
    r, d, e = leaf(case["raw"]), leaf(case["dep"]), leaf(case["E"])
    cov, sh, sc, q = head64(r, d, e, case["mult"].to(dtype), case["mask"].to(dtype), SMIN, SMAX, mutate=mutate)
    outs = dict(cov=cov, sh=sh, scales=sc, rot=q)
    loss = sum((outs[k] * case["g_" + k].to(dtype)).sum() for k in cots)
    g = torch.autograd.grad(loss, (r, d, e), allow_unused=True)
    g = [torch.zeros_like(t) if x is None else x for x, t in zip(g, (r, d, e))]
    res = dict(cov=cov.detach(), harmonics=sh.detach(), scales=sc.detach(), rotations=q.detach(), g_raw=g[0], g_depths=g[1],
               g_E=g[2])
    if shared:
        _cache[key] = res
    return res


def group(res, name):
    """The tensor of one judged group out of a result dict (run_head's keys)."""
    if name == "g_raw_s":
        return res["g_raw"][:, :3]
    if name == "g_raw_q":
        return res["g_raw"][:, 3:7]
    if name == "g_raw_sh":
        return res["g_raw"][:, 7:]
    if name == "g_E":
        return res["g_E"][:, :3, :3]
    if name == "g_depths":
        return res["g_depths"].reshape(-1, 1)
    return res[name]


def figure(got, ref, name):
    """(per_gaussian_err of group `name`, worst row); a result that is not finite reads inf."""
    a, b = group(got, name), group(ref, name)
    if not bool(torch.isfinite(a).all()):
        bad = (~torch.isfinite(a.reshape(a.shape[0], -1))).any(1)
        return float("inf"), int(bad.nonzero()[0])
    return per_gaussian_err(a, b)


def figures(got, ref, groups=FWD_GROUPS + BWD_GROUPS):
    return {name: figure(got, ref, name) for name in groups}


# ------------------------------------------------------------------------------------------------------------- unprojection
# (V, h, w, k): k picks which of the edge depths leads, so that the one-pixel case sees each of them
UNPROJECT_DEPTHS = (0.0, -1.5, 1e-3, 1e3)
UNPROJECT_CASES = ((1, 1, 1, 0), (1, 1, 1, 1), (1, 1, 1, 2), (1, 1, 1, 3), (3, 5, 7, 0), (2, 17, 31, 1))
UNPROJECT_GROUPS = ("xyz", "g_depths")


def build_unproject(V, h, w, k):
    """depths [V, h*w] (0, a negative value, 1e-3 and 1e3 at the first pixels of every view and at its last ones; 0.5 - 5
    elsewhere), per-view extrinsics I + 0.3 randn (not rigid), k0 = (fx, fy, cx, cy) in pixels with fx != fy and the principal
    point at 0.3 / 0.6 of the image, and the cotangent g_xyz.  (2, 17, 31): 527 pixels a view, the view boundary inside the
    third 256-thread workgroup."""
    key = ("unproject", V, h, w, k)
    if key in _cache:
        return _cache[key]
    gen = torch.Generator().manual_seed(7000 + 100 * V + h + k)
    P = h * w
    depths = 0.5 + 4.5 * torch.rand(V, P, generator=gen)
    for v in range(V):
        for j in range(min(4, P)):
            depths[v, j] = UNPROJECT_DEPTHS[(j + k + v) % 4]
            if P >= 8:
                depths[v, P - 1 - j] = UNPROJECT_DEPTHS[(j + k + v + 1) % 4]
    E = torch.eye(4).repeat(V, 1, 1) + 0.3 * torch.randn(V, 4, 4, generator=gen)
    k0 = torch.tensor([0.9 * w, 1.3 * h, 0.3 * w, 0.6 * h], dtype=torch.float32)
    c = dict(V=V, h=h, w=w, depths=depths, E=E, k0=k0, g_xyz=torch.randn(V, P, 3, generator=gen))
    assert float(k0[0]) != float(k0[1])
    if P >= 8:
        for x in UNPROJECT_DEPTHS:
            assert bool((depths == x).any(1).all()), x
    _cache[key] = c
    return c


def run_unproject(c, dtype=torch.float64):
    d = c["depths"].to(dtype).clone().requires_grad_(True)
    xyz = unproject64(d, c["E"].to(dtype), c["k0"].to(dtype), c["h"], c["w"])
    (xyz * c["g_xyz"].to(dtype)).sum().backward()
    return dict(xyz=xyz.detach().reshape(-1, 3), g_depths=d.grad.reshape(-1, 1))


def unproject_figures(got, ref):
    return {name: per_gaussian_err(got[name], ref[name]) for name in UNPROJECT_GROUPS}


# ------------------------------------------------------------------------------------------------------------------- bounds
# What fp32 torch autograd of the restatement reads against float64 (per_gaussian_err; per class and group the worst of d_sh
# 1 / 4 / 9 / 16, M = 1 / 300 and the five cotangent sets; CPU, x86-64 glibc; measure_f32_vs_f64() prints this table).
# The forward groups sit at one or two roundings.  The backward ones are set by each class's worst-conditioned row, not by the
# typical one (1e-7 - 1e-6): g_depths is ONE number a row, a sum of three signed terms that cancels to 1e-3 of its terms on
# some row of 300; d raw_q through the covariance vanishes as two scales of a row approach each other (the saturated rows of
# the scales class have two EQUAL scales, hence its 1.4e-4), and the covariance's cotangent alone reads highest.
ADAPTER_F32_VS_F64 = {
    "plain": dict(cov=6.89e-07, scales=1.65e-07, rotations=1.20e-07, g_raw_s=2.32e-06, g_raw_q=1.24e-05, g_depths=2.90e-05, g_E=9.85e-07),
    "scales": dict(cov=8.56e-07, scales=1.38e-07, rotations=1.23e-07, g_raw_s=8.70e-05, g_raw_q=1.44e-04, g_depths=3.22e-04, g_E=7.78e-07),
    "quat_1e-3": dict(cov=6.25e-07, scales=1.75e-07, rotations=1.38e-07, g_raw_s=3.76e-06, g_raw_q=2.42e-05, g_depths=3.38e-04, g_E=6.41e-07),
    "quat_1": dict(cov=6.57e-07, scales=1.76e-07, rotations=1.20e-07, g_raw_s=1.62e-06, g_raw_q=2.39e-05, g_depths=7.92e-05, g_E=7.55e-07),
    "quat_1e3": dict(cov=6.83e-07, scales=2.27e-07, rotations=1.15e-07, g_raw_s=1.02e-06, g_raw_q=6.05e-06, g_depths=3.01e-04, g_E=7.86e-07),
    "quat_1e15": dict(cov=6.36e-07, scales=1.76e-07, rotations=1.07e-07, g_raw_s=2.15e-06, g_raw_q=7.05e-06, g_depths=2.64e-04, g_E=6.30e-07),
    "tiny_quat": dict(cov=9.98e-07, scales=1.93e-07, rotations=1.24e-07, g_raw_s=1.12e-06, g_raw_q=1.95e-05, g_depths=2.52e-04, g_E=8.57e-07),
    "depth_small": dict(cov=7.57e-07, scales=2.04e-07, rotations=1.30e-07, g_raw_s=1.23e-06, g_raw_q=3.34e-05, g_depths=2.34e-04, g_E=7.41e-07),
    "depth_large": dict(cov=7.82e-07, scales=2.09e-07, rotations=1.22e-07, g_raw_s=2.28e-06, g_raw_q=1.88e-05, g_depths=1.39e-04, g_E=6.67e-07),
    "depth_mixed": dict(cov=6.79e-07, scales=1.94e-07, rotations=1.28e-07, g_raw_s=1.70e-06, g_raw_q=4.31e-06, g_depths=5.07e-05, g_E=7.99e-07),
    "extrinsics": dict(cov=6.80e-07, scales=2.12e-07, rotations=1.19e-07, g_raw_s=3.34e-06, g_raw_q=2.25e-05, g_depths=9.95e-05, g_E=9.52e-07),
    "extrinsics_off16": dict(cov=6.80e-07, scales=2.12e-07, rotations=1.19e-07, g_raw_s=3.34e-06, g_raw_q=2.25e-05, g_depths=9.95e-05, g_E=9.52e-07),
    "unproject": dict(xyz=1.92e-07, g_depths=1.57e-05),
}
# What the MI355X kernels read on the same cases (worst of the degrees, sizes and cotangent sets), for comparison; the forward
# groups equal the fp32 restatement's figure because the kernel rounds the same operations in the same order:
#   plain:            cov 6.89e-07, scales 1.65e-07, rotations 1.20e-07, g_raw_s 2.46e-06, g_raw_q 1.16e-05, g_depths 5.75e-05, g_E 9.85e-07
#   scales:           cov 8.56e-07, scales 1.38e-07, rotations 1.23e-07, g_raw_s 8.70e-05, g_raw_q 1.52e-04, g_depths 2.59e-04, g_E 7.78e-07
#   quat_1e-3:        cov 6.25e-07, scales 1.75e-07, rotations 1.38e-07, g_raw_s 3.94e-06, g_raw_q 1.23e-05, g_depths 2.70e-04, g_E 6.41e-07
#   quat_1:           cov 6.57e-07, scales 1.76e-07, rotations 1.20e-07, g_raw_s 1.62e-06, g_raw_q 2.60e-05, g_depths 6.39e-05, g_E 7.55e-07
#   quat_1e3:         cov 6.83e-07, scales 2.27e-07, rotations 1.15e-07, g_raw_s 9.38e-07, g_raw_q 9.83e-06, g_depths 3.86e-04, g_E 7.86e-07
#   quat_1e15:        cov 6.36e-07, scales 1.76e-07, g_raw_s 2.58e-06, g_raw_q 6.81e-06, g_depths 2.06e-04, g_E 6.30e-07, rotations 1.07e-07
#   tiny_quat:        cov 9.98e-07, scales 1.93e-07, g_raw_s 1.53e-06, g_raw_q 8.95e-06, g_depths 2.52e-04, g_E 8.57e-07, rotations 1.24e-07
#   depth_small:      cov 7.57e-07, scales 2.04e-07, rotations 1.30e-07, g_raw_s 1.23e-06, g_raw_q 3.08e-05, g_depths 2.34e-04, g_E 7.41e-07
#   depth_large:      cov 7.82e-07, scales 2.09e-07, rotations 1.22e-07, g_raw_s 2.60e-06, g_raw_q 2.41e-05, g_depths 9.88e-05, g_E 6.61e-07
#   depth_mixed:      cov 6.79e-07, scales 1.94e-07, rotations 1.28e-07, g_raw_s 1.70e-06, g_raw_q 3.93e-06, g_depths 1.82e-05, g_E 7.99e-07
#   extrinsics:       cov 6.80e-07, scales 2.12e-07, rotations 1.19e-07, g_raw_s 3.74e-06, g_raw_q 1.98e-05, g_depths 9.95e-05, g_E 9.52e-07
#   extrinsics_off16: cov 6.80e-07, scales 2.12e-07, rotations 1.19e-07, g_raw_s 3.74e-06, g_raw_q 1.98e-05, g_depths 9.95e-05, g_E 9.52e-07
#   unproject:        xyz 1.92e-07, g_depths 8.97e-06
ADAPTER_TOL_CPU = {c: {g: 2.0 * v for g, v in t.items()} for c, t in ADAPTER_F32_VS_F64.items()}   # platform libm differences
ADAPTER_TOL_GPU = {c: {g: 4.0 * v for g, v in t.items()} for c, t in ADAPTER_F32_VS_F64.items()}   # + the order of the kernel's sums


def measure_f32_vs_f64():
    """The table above, measured: {class: {group: figure}} and the unprojection's under "unproject"."""
    out = {}
    for cls in CLASSES:
        worst = dict.fromkeys(FWD_GROUPS + BWD_GROUPS, 0.0)
        for d_sh in D_SHS:
            for M in MS:
                case = build_case(cls, d_sh, M)
                for cots in COT_SETS:
                    f = figures(run_head(case, cots, torch.float32), run_head(case, cots))
                    worst = {g: max(worst[g], f[g][0]) for g in worst}
        out[cls] = worst
    worst = dict.fromkeys(UNPROJECT_GROUPS, 0.0)
    for args in UNPROJECT_CASES:
        c = build_unproject(*args)
        f = unproject_figures(run_unproject(c, torch.float32), run_unproject(c))
        worst = {g: max(worst[g], f[g][0]) for g in worst}
    out["unproject"] = worst
    return out


if __name__ == "__main__":
    for cls, t in measure_f32_vs_f64().items():
        print(f'    "{cls}": dict(' + ", ".join(f"{g}={v:.2e}" for g, v in t.items()) + "),")
