"""Seeded inputs for the multi-view / scale-invariant depth loss tests, shared by tests/test_mv_depth_loss_host.py,
tests/test_mv_depth_loss_hip.py and smoke(): smooth depth fields at 1-4 m, current poses within 2 m / 0.5 rad, source poses
within 0.4 m / 0.25 rad of them, fx = 0.9 W, holes of every kind (NaN, +-inf, 0, negative) in `gt` and `src`, a `pred` with
non-positive and NaN pixels, an alpha that crosses alpha_floor, and one view without a valid pixel.

"Decidable": the kernels take their decisions (which source pixel, visible or not, z_p' > 0) in fp32 where the reference takes
them in float64.  A pixel one of whose decisions could flip is made a hole of `gt` WHEN THE CASE IS BUILT (build_case), so that
afterwards no pixel has to be left out of a comparison; assert_decidable() then checks the finished case, and that at most
MAX_HOLED of its pixels went that way.  The float64 reference values of a case are computed once (functools.lru_cache) and
shared by the tests.
"""
import functools
import math

import torch

import mv_depth_ref as MR

B = 2
FLOOR = 1e-3
MAX_HOLED = 0.01
MARGIN_PX, NEAR_PX, MARGIN_OCC, MARGIN_Z = 1e-3, 1.5, 1e-4, 1e-3
KW = dict(occlusion=1.05, min_depth=0.5, max_depth=3.75, alpha_floor=FLOOR)
SEED_1X1 = (9, 2)

# (H, W, Hs, Ws, K, with_alpha, pool, invalid_view, seed): 1 x 1; one row; W no multiple of 4; 33 x 130 crosses a workgroup's
# 1024-pixel span inside a row and from row to row; a source of another size; K = 1, 3, 16; the pool form (a repeated index, a
# -1, an index >= S_pool); invalid_view: the last view has no valid pixel.  The seeds of the 1 x 1 cases were picked so that the
# one pixel of each view is selected by a source.
CASES = [
    (1, 1, 1, 1, 1, False, False, False, SEED_1X1[0]),
    (1, 1, 1, 1, 3, True, False, False, SEED_1X1[1]),
    (1, 67, 1, 67, 3, True, False, False, 1),
    (1, 67, 1, 67, 1, False, False, True, 0),
    (37, 53, 37, 53, 3, True, False, True, 0),
    (37, 53, 37, 53, 16, False, False, False, 0),
    (37, 53, 37, 53, 1, True, False, False, 0),
    (33, 130, 33, 130, 3, True, False, False, 1),
    (33, 130, 33, 130, 16, True, False, False, 0),
    (33, 130, 33, 130, 1, False, False, True, 0),
    (5, 130, 7, 96, 3, True, False, False, 13),
    (5, 130, 7, 96, 1, False, False, False, 0),
    (5, 130, 7, 96, 4, True, True, False, 5),
    (37, 53, 37, 53, 4, False, True, False, 1),
]
POOL = 5                                       # maps in the pool of the pool-form cases
POOL_INDEX = [[3, 0, 3, -1], [1, POOL, 4, 2]]  # a repeated index, a -1 and an index >= S_pool


def field(H, W, gen, lo=1.0, hi=4.0):
    """A smooth depth field in (lo, hi)."""
    y = torch.arange(H, dtype=torch.float64).view(H, 1) / max(H, 8)
    x = torch.arange(W, dtype=torch.float64).view(1, W) / max(W, 8)
    p = torch.rand(6, generator=gen, dtype=torch.float64)
    s = torch.sin(2.0 * math.pi * ((0.5 + p[0]) * x + p[1])) * torch.cos(2.0 * math.pi * ((0.5 + p[2]) * y + p[3]))
    s = 0.7 * s + 0.25 * torch.sin(2.0 * math.pi * ((1.0 + p[4]) * (x + y) + p[5]))
    return 0.5 * (lo + hi) + 0.5 * (hi - lo) * s


def rotation(axis_angle):
    """Rodrigues, float64."""
    th = float(axis_angle.norm())
    if th == 0.0:
        return torch.eye(3, dtype=torch.float64)
    k = axis_angle / th
    Kx = torch.tensor([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(th) * Kx + (1.0 - math.cos(th)) * (Kx @ Kx)


def pose(gen, max_t, max_r):
    """A rigid transform with a translation within max_t and a rotation within max_r."""
    v = torch.randn(2, 3, generator=gen, dtype=torch.float64)
    v = v / v.norm(dim=1, keepdim=True) * torch.rand(2, 1, generator=gen, dtype=torch.float64)
    T = torch.eye(4, dtype=torch.float64)
    T[:3, :3] = rotation(v[0] * max_r)
    T[:3, 3] = v[1] * max_t
    return T


def intrinsics(H, W):
    return torch.tensor([0.9 * W, 0.9 * W, (W - 1) / 2.0, (H - 1) / 2.0], dtype=torch.float64)


def holes(t, gen, frac):
    """Every kind of hole, each over about frac / 5 of the elements."""
    u = torch.rand(t.shape, generator=gen)
    for i, v in enumerate((float("nan"), float("inf"), -float("inf"), 0.0, -1.5)):
        t = torch.where((u >= i * frac / 5) & (u < (i + 1) * frac / 5), torch.full_like(t, v), t)
    return t


def undecidable(c):
    """[B, H, W] bool, float64: a pixel with a valid gt one of whose decisions for one of its sources could flip in fp32."""
    gt, pairs = c["gt"].double(), c["pairs"].double()
    Bc, H, W = gt.shape
    K = pairs.shape[1]
    maps, on = MR._sources(c["src"].double(), c["src_index"], Bc, K)
    Hs, Ws = maps.shape[-2:]
    kw = c["kw"]
    V0 = MR.valid(gt, kw["min_depth"], kw["max_depth"])
    E, _ = MR.expected_depth(c["depth"].double(), None if c["alpha"] is None else c["alpha"].double(), MR.f32(kw["alpha_floor"]))
    x = torch.arange(W, dtype=torch.float64).view(1, 1, W).expand(Bc, H, W)
    y = torch.arange(H, dtype=torch.float64).view(1, H, 1).expand(Bc, H, W)
    pix = torch.stack([x, y, torch.ones_like(x)], 1)
    g = torch.where(V0, gt, torch.ones_like(gt))
    bad = torch.zeros(Bc, H, W, dtype=torch.bool)
    for k in range(K):
        A, t = pairs[:, k, :, :3], pairs[:, k, :, 3]
        ray = torch.einsum("bij,bjhw->bihw", A, pix)
        q = g[:, None] * ray + t[:, :, None, None]
        zq = q[:, 2] + MR.EPS
        b = zq.abs() < MARGIN_Z
        den = torch.where(b, torch.ones_like(zq), zq)
        u, v = q[:, 0] / den, q[:, 1] / den
        near = (u > -0.5 - NEAR_PX) & (u < Ws - 0.5 + NEAR_PX) & (v > -0.5 - NEAR_PX) & (v < Hs - 0.5 + NEAR_PX)
        for coord in (u, v):
            b = b | (near & (((coord - torch.floor(coord)) - 0.5).abs() < MARGIN_PX))
        ix, iy = torch.round(q[:, 0] / den), torch.round(q[:, 1] / den)
        inside = (ix >= 0) & (ix < Ws) & (iy >= 0) & (iy < Hs)
        flat = (torch.where(inside, iy, torch.zeros_like(iy)) * Ws + torch.where(inside, ix, torch.zeros_like(ix))).long()
        S = torch.gather(maps[:, k].reshape(Bc, Hs * Ws), 1, flat.view(Bc, H * W)).view(Bc, H, W)
        S_ok = inside & MR.valid(S, kw["min_depth"], kw["max_depth"])
        b = b | (S_ok & ((zq - kw["occlusion"] * S).abs() < MARGIN_OCC * zq.abs()))
        zp = E * ray[:, 2] + t[:, 2, None, None] + MR.EPS
        b = b | (torch.isfinite(zp) & (zp.abs() < MARGIN_Z))
        bad = bad | (b & on[:, k].view(Bc, 1, 1))
    return bad & V0


def raw_case(H, W, Hs, Ws, K, with_alpha, pool, invalid_view=False, seed=0, views=B, kw=None):
    """The inputs before any pixel is holed for decidability: fp32 tensors on the CPU."""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * H + 13 * W + K + (50 if with_alpha else 0) + (100 if pool else 0) + 3)
    # the pose deltas shrink with the smaller side of the images, so that a source of a few rows is still hit
    shrink = min(1.0, min(H, W, Hs, Ws) / 32.0)
    if K > 4:
        # every source adds two rounding decisions per pixel: with 16 generic sources 6 % of the pixels would lie within the
        # margin of one.  The many-source cases keep their sources within a third of a pixel of the current view (0.585 W
        # shrink is the largest shift a pose delta makes at 1 m), so that all K gathers hit and none is near a boundary; the
        # generic geometry is what the cases with K <= 4 are for.  For the same reason their sources' depths stay clear of the
        # occlusion threshold (below).
        shrink = min(shrink, 0.6 / max(H, W))
    clean = torch.stack([field(H, W, gen) for _ in range(views)])
    gt = holes(clean.float(), gen, 0.1)
    alpha = None
    depth = clean * torch.exp(0.05 * torch.randn(views, H, W, generator=gen, dtype=torch.float64))
    if with_alpha:
        alpha = (0.3 + 0.7 * torch.rand(views, H, W, generator=gen)).float()
        u = torch.rand(views, H, W, generator=gen)
        alpha = torch.where(u < 0.03, torch.full_like(alpha, 5e-4), alpha)         # below the floor
        alpha = torch.where((u >= 0.03) & (u < 0.05), torch.full_like(alpha, FLOOR), alpha)     # at the floor
        depth = depth * alpha.clamp_min(FLOOR).double()
    depth = depth.float()
    u = torch.rand(views, H, W, generator=gen)
    # (a predicted depth of 0 puts z_p' at t[2], which the near-identity sources of K > 4 leave at about 1e-3: undecidable)
    for i, v in enumerate((float("nan"), 0.0 if K <= 4 else -0.2, -0.7, float("inf"))):
        depth = torch.where((u >= 0.01 * i) & (u < 0.01 * (i + 1)), torch.full_like(depth, v), depth)
    if invalid_view and views > 1:
        gt[-1] = float("nan")
    n_src = POOL if pool else views * K
    if K > 4:                                  # (see `shrink`: such a source sees the current view's surface, 10-40 % deeper)
        assert not pool and (Hs, Ws) == (H, W)
        src = torch.stack([clean[i // K] * field(H, W, gen, 1.1, 1.4) for i in range(n_src)])
    else:
        src = torch.stack([field(Hs, Ws, gen) for _ in range(n_src)])
    src = holes(src.float(), gen, 0.1)
    c2w = torch.stack([pose(gen, 2.0, 0.5) for _ in range(views)])
    kc, ks = intrinsics(H, W), intrinsics(Hs, Ws)
    if pool:
        assert views == B and K == len(POOL_INDEX[0])
        index = torch.tensor(POOL_INDEX, dtype=torch.int32)
        owner = [0 if i in POOL_INDEX[0] else 1 for i in range(POOL)]              # the view a pool map is a neighbour of
        w2s = torch.stack([torch.linalg.inv(c2w[owner[i]] @ pose(gen, 0.4 * shrink, 0.25 * shrink)) for i in range(POOL)])
    else:
        index = None
        w2s = torch.stack([torch.stack([torch.linalg.inv(c2w[b] @ pose(gen, 0.4 * shrink, 0.25 * shrink)) for _ in range(K)])
                           for b in range(views)])
        src = src.view(views, K, Hs, Ws)
    pairs = MR.pair_transforms(kc, c2w, ks, w2s, index).float()
    return dict(depth=depth, gt=gt, alpha=alpha, src=src, src_index=index, pairs=pairs, kw=dict(KW if kw is None else kw),
                cams=dict(intr=kc, cam_to_world=c2w, src_intr=ks, src_world_to_cam=w2s))


def build_case(*args, **kwargs):
    """raw_case with every undecidable pixel's gt made a hole; c["holed"]: the fraction of pixels that went that way."""
    c = raw_case(*args, **kwargs)
    bad = undecidable(c)
    c["gt"] = torch.where(bad, torch.full_like(c["gt"], float("nan")), c["gt"])
    c["holed"] = float(bad.float().mean())
    return c


def assert_decidable(c):
    """No decision of the finished case can flip in fp32, and at most MAX_HOLED of its pixels were given up for that."""
    left = int(undecidable(c).sum())
    assert left == 0, f"{left} undecidable pixels are left"
    assert c["holed"] <= MAX_HOLED, f"{c['holed']:.4f} of the pixels were made holes for decidability (at most {MAX_HOLED})"


@functools.lru_cache(maxsize=None)
def case(H, W, Hs, Ws, K, with_alpha, pool, invalid_view, seed):
    """The case with its float64 reference: vals (sum, cnt, residuals), g_sum and the gradients for it ("terms") and through the
    scalar loss ("loss"); si_vals (s1, s2, n), g_si (g1, g2) and the same two families of gradients."""
    c = build_case(H, W, Hs, Ws, K, with_alpha, pool, invalid_view, seed)
    c["invalid_view"] = invalid_view
    gen = torch.Generator().manual_seed(H * W + K)
    c["vals"] = MR.mv_values(c)
    c["g_sum"] = torch.randn(B, K, generator=gen, dtype=torch.float64)
    loss, *lg = MR.mv_loss_grad(c)
    c["loss"], c["grads"] = loss, {"terms": MR.mv_grad(c, c["g_sum"]), "loss": tuple(lg)}
    c["si_vals"] = MR.si_values(c)
    c["g_si"] = tuple(torch.randn(B, generator=gen, dtype=torch.float64) for _ in range(2))
    si_loss, *sg = MR.si_loss_grad(c)
    c["si_loss"], c["si_grads"] = si_loss, {"terms": MR.si_grad(c, *c["g_si"]), "loss": tuple(sg)}
    return c


def golden_case(H, W, K, views, seed):
    """The small cases the reference's MVDepthLoss / ScaleInvariantLoss are run on (tests/golden/make_mv_depth_golden.py): NaN
    holes in gt; 0, negative and NaN holes in src (the reference has no thresholds and takes +-inf for a depth); a positive
    pred; no alpha; no empty source column."""
    c = build_case(H, W, H, W, K, False, False, seed=seed, views=views,
                   kw=dict(occlusion=1.05, min_depth=0.0, max_depth=math.inf, alpha_floor=FLOOR))
    gt, src, depth = c["gt"], c["src"], c["depth"]
    c["gt"] = torch.where(torch.isfinite(gt) & (gt > 0), gt, torch.full_like(gt, float("nan")))
    c["src"] = torch.where(torch.isinf(src), torch.zeros_like(src), src)
    c["depth"] = torch.where(torch.isfinite(depth) & (depth > 0), depth, torch.full_like(depth, 2.0))
    bad = undecidable(c)                                # (a pixel that was +-inf in src is 0 now: decide again)
    c["gt"] = torch.where(bad, torch.full_like(c["gt"], float("nan")), c["gt"])
    c["holed"] += float(bad.float().mean())
    return c
