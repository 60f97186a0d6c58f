"""Restatement of adaptive density control (csrc/gaussian_density.hip, include/freesplat_amd_density.h) in NumPy / torch.

  accumulate   the three statistics over the visible rows, in any dtype (float64 reference, float32 yardstick).
  plan         the one-pass rules in fp32 comparisons -- exact: the kernel only compares and forms one fp32 product.
  source_map   the stable output -> (source row, j) map the plan implies.
  bits / uniforms / normals   the counter-based generator in uint32 arithmetic, Box-Muller in any dtype.
  apply        the gather: kept rows and clone originals with their moments, copies and children with none; the children's
               log-scales and means in any dtype (float64 on the CPU as the reference, float32 on a device as the yardstick E).
  sequence     the literal 3DGS order -- clone (append), split (append two children, remove the parent), prune on the grown
               set -- as a second, independent statement of which rows survive.
"""
from __future__ import annotations

import math

import numpy as np
import torch

DROPPED, KEPT, CLONE, SPLIT = range(4)
MEANS, SCALES, ROTATIONS, OPACITIES, SHS = range(5)
OUTPUTS = np.array([0, 1, 2, 2], np.uint32)
TWO_PI_F32 = float(np.float32(6.2831855))
LOG_SPLIT_F32 = float(np.float32(0.47000363))            # logf(1.6f), the constant the kernel subtracts


def thresholds(extent, grad_threshold=2e-4, min_opacity=0.005, percent_dense=0.01, max_screen_size=None, prune_big=False):
    """The host's mapping of densify()'s arguments to the six floats of fs_density_plan, each rounded once from double."""
    prune = 0.1 * float(extent) if prune_big else 0.0
    vals = (float(grad_threshold), float(percent_dense) * float(extent), float(min_opacity),
            0.0 if max_screen_size is None else float(max_screen_size), prune, 1.6 * prune)
    return tuple(np.float32(v) for v in vals)


def accumulate(stats, g, radii, dtype=torch.float64):
    """stats = (grad_accum, denom, max_radii) tensors of `dtype`; g [N,3] with anything in the rows that are not visible."""
    on = radii > 0
    g = g.to(stats[0].device, dtype)
    norm = torch.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1])
    z = torch.zeros_like(stats[0])
    return (stats[0] + torch.where(on, norm, z), stats[1] + on.to(dtype), torch.where(on, torch.maximum(stats[2], radii.to(dtype)), stats[2]))


def plan(grad_accum, denom, max_radii, scales, opacities, th):
    """float32 arrays in, (kind uint8 [N], offset uint32 [N], totals [4]) out."""
    f = lambda a: np.ascontiguousarray(np.asarray(a, np.float32))
    grad_accum, denom, max_radii, opacities = f(grad_accum).ravel(), f(denom).ravel(), f(max_radii).ravel(), f(opacities).ravel()
    grad_t, dense, min_op, screen, prune, child = (np.float32(t) for t in th)
    s_max = f(scales).reshape(-1, 3).max(1)
    with np.errstate(invalid="ignore"):
        product = grad_t * denom                          # float32 x float32 array: one fp32 product per row
    assert product.dtype == np.float32
    hot = (denom > 0) & (grad_accum >= product)
    split = hot & (s_max > dense)
    clone = hot & ~split
    drop = opacities < min_op
    if screen > 0:
        drop |= ~split & (max_radii > screen)
    if prune > 0:
        drop |= s_max > np.where(split, child, prune).astype(np.float32)
    kind = np.where(drop, DROPPED, np.where(split, SPLIT, np.where(clone, CLONE, KEPT))).astype(np.uint8)
    counts = OUTPUTS[kind]
    offset = (np.cumsum(counts, dtype=np.uint64) - counts).astype(np.uint32)
    totals = [int(counts.sum()), int((kind == CLONE).sum()), int((kind == SPLIT).sum()), int((kind == DROPPED).sum())]
    return kind, offset, totals


def source_map(kind):
    """(rows, j): output row o is output j (0 or 1) of source row rows[o]; stable."""
    counts = OUTPUTS[np.asarray(kind)]
    rows = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    first = np.cumsum(counts, dtype=np.int64) - counts
    return rows, np.arange(len(rows), dtype=np.int64) - first[rows]


# ---- the generator: uint32 arithmetic, wrapping ---------------------------------------------------------------------------

def _fmix(h):
    h = h.astype(np.uint32)
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def bits(seed, row, child, word):
    """uint32 arrays (broadcast) -> uint32: fmix(fmix(fmix(seed ^ 0x9E3779B9) ^ row) + 0x9E3779B1 * (8 child + word + 1))."""
    u = lambda x: np.asarray(x, dtype=np.uint64).astype(np.uint32)
    seed, row, child, word = u(int(seed) & 0xFFFFFFFF), u(row), u(child), u(word)
    with np.errstate(over="ignore"):
        h = _fmix(_fmix(np.atleast_1d(seed ^ np.uint32(0x9E3779B9))) ^ row)
        return _fmix(h + np.uint32(0x9E3779B1) * (np.uint32(8) * child + word + np.uint32(1)))


def uniforms(seed, rows, child):
    """float64 [n, 6] holding the kernel's fp32 uniforms exactly: words 0..5 of (seed, row, child), u = fl32((bits >> 8) + 0.5)
    2^-24 -- the sum is exact below 2^23 and rounds to even above, so u lies in (0, 1]."""
    b = bits(seed, np.asarray(rows)[:, None], np.asarray(child)[:, None], np.arange(6)[None, :])
    k = (b >> np.uint32(8)).astype(np.float32) + np.float32(0.5)
    assert k.dtype == np.float32
    return k.astype(np.float64) * 2.0 ** -24


def normals(seed, rows, child, dtype=torch.float64, device="cpu"):
    """[n, 3] standard normals: z[c] = sqrt(-2 log u[2c]) cos(6.2831855f u[2c+1]), evaluated in `dtype` on `device`."""
    u = torch.from_numpy(uniforms(seed, rows, child)).to(device=device, dtype=dtype)
    return torch.sqrt(-2.0 * torch.log(u[:, 0::2])) * torch.cos(TWO_PI_F32 * u[:, 1::2])


def rotation(q):
    """R(q / |q|) as rasterizer.build_cov3d defines it; q [n, 4] as (w, x, y, z)."""
    q = q / q.norm(dim=-1, keepdim=True)
    r, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


def children(means, log_scales, rotations, seed, rows, child, dtype=torch.float64, device="cpu"):
    """(means, log_scales) of the children `child` [n] of the parents in source rows `rows` [n], from the parents' float32
    raw values, evaluated in `dtype` on `device`."""
    d = lambda t: t[torch.as_tensor(rows)].to(device=device, dtype=dtype)
    m, ls, q = d(means), d(log_scales), d(rotations)
    z = normals(seed, rows, child, dtype, device)
    sz = torch.exp(ls) * z
    R = rotation(q)
    off = (R[:, :, 0] * sz[:, None, 0] + R[:, :, 1] * sz[:, None, 1]) + R[:, :, 2] * sz[:, None, 2]
    return m + off, ls - (LOG_SPLIT_F32 if dtype == torch.float32 else math.log(1.6))


def apply(raw, exp_avg, exp_avg_sq, kind, seed, dtype=torch.float64, device="cpu"):
    """raw / exp_avg / exp_avg_sq: five float32 CPU tensors each.  Returns dict(p, m, v: lists of five tensors of `dtype` with
    n_out rows; rows, j: the source map; copied: bool [n_out], rows whose parameters are bit copies of the source)."""
    kind = np.asarray(kind)
    rows, j = source_map(kind)
    k = kind[rows]
    idx = torch.from_numpy(rows)
    keep = torch.from_numpy((j == 0) & (k != SPLIT))
    gather = lambda t: t[idx].to(device=device, dtype=dtype)
    p = [gather(t) for t in raw]
    shape = lambda t: (-1,) + (1,) * (t.dim() - 1)
    m = [torch.where(keep.to(device).reshape(shape(t)), gather(t), torch.zeros((), dtype=dtype, device=device)) for t in exp_avg]
    v = [torch.where(keep.to(device).reshape(shape(t)), gather(t), torch.zeros((), dtype=dtype, device=device)) for t in exp_avg_sq]
    is_split = k == SPLIT
    if is_split.any():
        sel = torch.from_numpy(np.nonzero(is_split)[0]).to(device)
        cm, cs = children(raw[MEANS], raw[SCALES], raw[ROTATIONS], seed, rows[is_split], j[is_split], dtype, device)
        p[MEANS][sel], p[SCALES][sel] = cm, cs
    return dict(p=p, m=m, v=v, rows=rows, j=j, kind=k, copied=~is_split)


# ---- the literal 3DGS sequence --------------------------------------------------------------------------------------------

def sequence(grad_accum, denom, max_radii, scales, opacities, th):
    """Clone, then split, then prune on the grown set.  Rows carry (source row, tag) with tag 0 = the row itself, 1 = a
    clone's copy, 2 / 3 = the children of a split; a copy inherits opacity, scales and screen radius, a child inherits the
    opacity, has the scales / 1.6 and no screen radius yet.  Returns the sorted list of surviving (source row, tag).
    Float64 throughout, with the fp32 thresholds: inputs placed away from ties give the rows of the one-pass rules."""
    grad_t, dense, min_op, screen, prune, _ = (float(t) for t in th)
    ga, dn, mr, op = (np.asarray(a, np.float64).ravel() for a in (grad_accum, denom, max_radii, opacities))
    s_max = np.asarray(scales, np.float64).reshape(-1, 3).max(1)
    N = len(ga)
    with np.errstate(invalid="ignore", divide="ignore"):
        avg = ga / dn
    avg[np.isnan(avg)] = 0.0                              # never seen: 0 / 0
    table = [dict(src=i, tag=0, op=op[i], s=s_max[i], r=mr[i]) for i in range(N)]
    # clone: small and hot, the copy is appended
    for i in range(N):
        if avg[i] >= grad_t and s_max[i] <= dense:
            table.append(dict(table[i], tag=1))
    # split: large and hot (rows appended by the clone pass have no gradient: padded with zeros), two children appended, parents removed
    parents = [i for i in range(N) if avg[i] >= grad_t and s_max[i] > dense]
    for i in parents:
        for c in (2, 3):
            table.append(dict(src=i, tag=c, op=op[i], s=s_max[i] / 1.6, r=0.0))
    gone = set(parents)
    table = [row for k, row in enumerate(table) if not (k < N and k in gone)]
    # prune on the grown set
    out = []
    for row in table:
        drop = row["op"] < min_op
        if screen > 0:
            drop = drop or row["r"] > screen
        if prune > 0:
            drop = drop or row["s"] > prune
        if not drop:
            out.append((row["src"], row["tag"]))
    return sorted(out)


def one_pass_rows(kind):
    """The same multiset from the one-pass kinds."""
    out = []
    for i, k in enumerate(np.asarray(kind)):
        out += {DROPPED: [], KEPT: [(i, 0)], CLONE: [(i, 0), (i, 1)], SPLIT: [(i, 2), (i, 3)]}[int(k)]
    return sorted(out)


# ---- inputs -------------------------------------------------------------------------------------------------------------

def kind_pattern(N: int, k: int) -> np.ndarray:
    """uint8 [N] with every kind in runs of 1, 2, 3 and 5 rows, so that the kind boundaries fall inside 16-byte groups of the
    width-1, -3, -4 and -27 arrays; `k` shifts the pattern."""
    i = np.arange(N) + k
    kind = np.where((i % 11 < 5) | (i % 3 == 0), KEPT, CLONE)
    kind = np.where(i % 7 == 2, SPLIT, kind)
    kind = np.where(i % 13 == 5, DROPPED, kind)
    return kind.astype(np.uint8)


# exactly representable thresholds: ties in the statistics pin >=, > and <
TIE_K = 12
GRAD_T, DENSE, MIN_OP = 5.0 * 2.0 ** -TIE_K, 0.25, 0.0078125


def stats_for(kind, seed=0, ties=True):
    """Statistics, activated scales [N,3] and opacities [N] (float32 arrays) that make fs_density_plan with thresholds
    (GRAD_T, DENSE, MIN_OP, 0, 0, 0) produce `kind`.  Every third row of a kind sits exactly ON the deciding threshold:
    gradients (3, 4) 2^-k summed to exactly grad_threshold x denom (>= holds: hot), s_max == dense_scale (> fails: clone),
    opacity == min_opacity (< fails: kept); the other rows lie well inside (ties=False: all rows do)."""
    kind = np.asarray(kind)
    N = len(kind)
    rng = np.random.default_rng(seed + 17 * N)
    tie = (np.arange(N) % 3 == 0) & bool(ties)
    denom = rng.integers(1, 4, N).astype(np.float32)
    denom[(kind == KEPT) & (np.arange(N) % 5 == 1)] = 0.0                     # never seen
    hot = (kind == CLONE) | (kind == SPLIT)
    avg = np.where(hot, np.where(tie, GRAD_T, GRAD_T * 3.0), GRAD_T * 0.5)
    grad_accum = (avg * denom).astype(np.float32)
    grad_accum[denom == 0] = 0.0
    s_max = np.where(kind == SPLIT, DENSE * 2.0, np.where(tie, DENSE, DENSE * 0.5))
    scales = (s_max[:, None] * np.array([0.5, 1.0, 0.25])[None, :]).astype(np.float32)
    scales = np.take_along_axis(scales, np.argsort(rng.random((N, 3)), 1), 1)  # the largest in any column
    opacities = np.where(kind == DROPPED, MIN_OP * 0.5, np.where(tie, MIN_OP, 0.6)).astype(np.float32)
    max_radii = rng.integers(0, 40, N).astype(np.float32)
    return grad_accum, denom, max_radii, scales, opacities


def make_state(N: int, M: int, seed: int = 0):
    """(raw, exp_avg, exp_avg_sq): float32 CPU tensors; log-scales ~ N(-2, 1), non-zero moments in every row."""
    gen = torch.Generator().manual_seed(1000 * N + 10 * M + seed)
    shapes = [(N, 3), (N, 3), (N, 4), (N,), (N, M, 3)]
    raw = [s * torch.randn(shape, generator=gen) for s, shape in zip((10.0, 1.0, 1.0, 3.0, 1.0), shapes)]
    raw[SCALES] -= 2.0
    raw[OPACITIES].clamp_(-6.0, 6.0)
    m = [0.1 * torch.randn(shape, generator=gen) for shape in shapes]
    v = [0.01 * torch.rand(shape, generator=gen) + 1e-6 for shape in shapes]
    return raw, m, v


def err(got: torch.Tensor, ref: torch.Tensor) -> float:
    ref = ref.detach().double().cpu()
    if ref.numel() == 0:
        return 0.0
    return float((got.detach().double().cpu().reshape(ref.shape) - ref).abs().max())


def bound(E: float, ref: torch.Tensor, K: int) -> float:
    """max(4 E, K 2^-23 max|ref|), the project's rule (tests/gaussian_adam_ref.py)."""
    return max(4.0 * E, K * 2.0 ** -23 * (float(ref.detach().abs().max()) if ref.numel() else 0.0))
