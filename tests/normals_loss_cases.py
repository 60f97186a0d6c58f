"""The inputs of the normals-loss GPU cases (tests/test_normals_loss_hip.py), shared with tests/test_normals_loss_host.py, which
runs the same generator over every case on the CPU: a smooth surface at 1.5 - 3 m plus small noise seen through fx ~ fy ~ 0.8 W
with an off-centre principal point, each view with its own intrinsics.

No pixel is left out of a comparison on the GPU.  Instead `assert_decidable` asserts on the inputs themselves, in float64, that
every thresholded quantity is at least 1e-3 (relative) from its threshold -- E > 0, the alpha floor, min_depth / max_depth and
|Gx x Gy| against 1e-12 -- and `case` nudges the inputs until that holds."""
import functools
import math

import torch

import normals_loss_ref as NR
from freesplat_amd.normals_loss import TILE_H, TILE_W          # the kernels' tile extents

B = 2
STRADDLING = [(TILE_H + 1, TILE_W + 1), (2 * TILE_H - 1, 2 * TILE_W + 1)]
SHAPES = [(1, 1), (2, 3), (5, 7), (13, 9)] + STRADDLING        # the first four are at or below the backward's halo of 6
MASKS = ["valid", "holes", "view_invalid", "low_alpha"]        # low_alpha: only with alpha
SMOOTHINGS = [None, 2.0]
TARGETS = ["gt_depth", "gt_normals"]
HOLES = (float("nan"), float("inf"), 0.0, -1.0)
FLOOR = 1e-3
MARGIN = 1e-3
CASES = [(H, W, s, with_alpha, target, mask) for H, W in SHAPES for s in SMOOTHINGS for with_alpha in (False, True)
         for target in TARGETS for mask in MASKS if with_alpha or mask != "low_alpha"]
MAP_CASES = [(H, W, s, with_alpha, mask) for H, W in SHAPES for s in SMOOTHINGS for with_alpha in (False, True)
             for mask in ("valid", "holes", "low_alpha") if with_alpha or mask != "low_alpha"]


def thresholds(mask):
    return dict(min_depth=1.7, max_depth=2.9) if mask == "holes" else {}     # some finite, positive values are holes too


def intrinsics(H, W, views=B):
    """[views, 4] float32: fx ~ fy ~ 0.8 W, the principal point off-centre, another one per view."""
    rows = [(0.8 * W * (1.0 + 0.03 * v), 0.8 * W * (1.05 - 0.02 * v), 0.45 * W + 0.3 + 0.2 * v, 0.55 * H - 0.2 - 0.1 * v)
            for v in range(views)]
    return torch.tensor(rows, dtype=torch.float64).float()


def surface(H, W, views, g, bumps=0.01):
    """[views, H, W] float64 in 1.5 .. 3: two low-frequency waves plus noise of `bumps` m."""
    y = torch.arange(H, dtype=torch.float64).view(1, H, 1) / max(H, 8)
    x = torch.arange(W, dtype=torch.float64).view(1, 1, W) / max(W, 8)
    ph = 6.0 * torch.rand(views, 1, 1, generator=g, dtype=torch.float64)
    z = 2.25 + 0.4 * torch.sin(3.0 * x + ph) + 0.3 * torch.cos(2.5 * y - ph)
    return z + bumps * torch.randn(views, H, W, generator=g, dtype=torch.float64)


def blocky(H, W, views, g, p):
    """bool [views, H, W], about p of it True, in 3 x 3 blocks (so that windows of valid pixels remain)."""
    coarse = torch.rand(views, -(-H // 3), -(-W // 3), generator=g) < p
    return coarse.repeat_interleave(3, 1).repeat_interleave(3, 2)[:, :H, :W]


def raw_inputs(H, W, with_alpha, target, mask, seed, views=B):
    """float32 dict(depth, alpha | None, gt_depth | gt_normals, intr)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.rand(views, H, W, generator=g, dtype=torch.float64)
    intr = intrinsics(H, W, views)
    gt = surface(H, W, views, g)
    E = gt * (1.0 + 0.03 * torch.sin(5.0 * surface(H, W, views, g, 0.0))) + 0.01 * torch.randn(views, H, W, generator=g, dtype=torch.float64)
    holes = torch.tensor(HOLES, dtype=torch.float64)
    kind = lambda: holes[torch.randint(0, len(HOLES), (views, H, W), generator=g)]
    if mask == "holes":                                          # ... in the prediction too: those pixels must receive exactly 0
        E = torch.where(blocky(H, W, views, g, 0.1), kind(), E)
    alpha = None
    if with_alpha:
        alpha = 0.3 + 0.7 * r()
        if mask == "low_alpha":
            alpha = torch.where(r() < 0.1, 2e-4 + 6e-4 * r(), alpha)             # below the floor: E = depth / floor
            alpha[-1, -1, -1] = 5e-4
            zero = blocky(H, W, views, g, 0.1)                                    # nothing rendered: depth = alpha = 0
            zero[0, 0, 0], zero[-1, -1, -1] = True, False                         # (at least one pixel of each kind)
            alpha, E = torch.where(zero, torch.zeros_like(alpha), alpha), torch.where(zero, torch.zeros_like(E), E)
        depth = E * alpha.clamp_min(FLOOR)
    else:
        depth = E
    out = dict(depth=depth.float(), alpha=None if alpha is None else alpha.float(), intr=intr)
    if target == "gt_depth":
        if mask == "holes":
            gt = torch.where(blocky(H, W, views, g, 0.3), kind(), gt)
        if mask == "view_invalid":
            gt[-1] = holes[torch.arange(H * W) % len(HOLES)].view(H, W)
        out["gt_depth"] = gt.float()
    else:
        t = NR.depth_normals(gt, intr.double(), smoothing=None).nan_to_num(0.0)   # (borders included: every tap is valid)
        if H * W == 1:
            t = torch.tensor([0.1, -0.2, 0.97], dtype=torch.float64).view(1, 3, 1, 1).expand(views, 3, 1, 1).clone()
        bad = torch.tensor([float("nan"), float("inf"), float("-inf")], dtype=torch.float64)
        if mask == "holes":
            hole = blocky(H, W, views, g, 0.3)
            for c in range(3):
                hit = hole & (torch.randint(0, 3, (views, H, W), generator=g) <= c)
                t[:, c] = torch.where(hit, bad[torch.randint(0, 3, (views, H, W), generator=g)], t[:, c])
            t[:, 0] = torch.where(hole & torch.isfinite(t).all(1), bad[0], t[:, 0])
        if mask == "view_invalid":
            t[-1, 1] = bad[torch.arange(H * W) % 3].view(H, W)
        out["gt_normals"] = t.float()
    return out


def _kw(c, smoothing, mask):
    kw = dict(smoothing=smoothing, alpha_floor=FLOOR, **thresholds(mask))
    for name in ("gt_depth", "gt_normals"):
        if name in c:
            kw[name] = c[name]
    return kw


def undecided(c, smoothing, mask, for_map=False):
    """bool [views, H, W]: pixels next to a quantity that is within MARGIN (relative) of its threshold, float64."""
    d = c["depth"].double()
    a = None if c["alpha"] is None else c["alpha"].double()
    intr = c["intr"].double()
    bad = torch.zeros(d.shape, dtype=torch.bool)
    E = NR.expected_depth(d, a, FLOOR)
    if a is not None:
        bad |= (a - FLOOR).abs() < MARGIN * FLOOR
    bad |= (E != 0) & (E.abs() < MARGIN * 1.0)                                   # E is an exact 0 or well away from it
    th = thresholds(mask)
    edged = [E] if for_map else ([c["gt_depth"].double()] if "gt_depth" in c else [])
    for x in edged:
        fin = torch.isfinite(x)
        for edge in th.values():
            bad |= fin & ((x - edge).abs() < MARGIN * max(abs(edge), 1.0))
    lo = max(th.get("min_depth", 0.0), 0.0) if for_map else 0.0
    hi = th.get("max_depth", math.inf) if for_map else math.inf
    maps = [NR.with_nans(E, lo, hi)]
    if "gt_depth" in c and not for_map:
        maps.append(NR.with_nans(c["gt_depth"].double(), th.get("min_depth", 0.0), th.get("max_depth", math.inf)))
    for m in maps:
        S = NR.smooth(m, smoothing)
        _, M = NR.normals_of(S, intr)
        Gx, Gy = NR.sobel_vectors(torch.where(torch.isfinite(S), S, torch.ones_like(S)), intr)
        norm = torch.cross(Gx, Gy, dim=1).norm(dim=1)
        bad |= M & (norm != 0) & (norm < NR.EPS * 1e3)                           # |Gx x Gy| is an exact 0 or far above the floor
    return bad


def settle(c, smoothing, mask, seed, for_map=False):
    """Nudges the depth (and alpha) of the pixels `undecided` names until it names none."""
    g = torch.Generator().manual_seed(seed + 1000)
    for _ in range(100):
        bad = undecided(c, smoothing, mask, for_map)
        if not bool(bad.any()):
            return c
        c = dict(c)
        c["depth"] = torch.where(bad, c["depth"] * (1.0 + 0.05 * torch.randn(bad.shape, generator=g)).float(), c["depth"])
        if c["alpha"] is not None:
            c["alpha"] = torch.where(bad & (c["alpha"] > 0), c["alpha"] * 1.01, c["alpha"])
        if "gt_depth" in c:
            c["gt_depth"] = torch.where(bad & torch.isfinite(c["gt_depth"]) & (c["gt_depth"] > 0), c["gt_depth"] * 1.004, c["gt_depth"])
    raise AssertionError("the inputs did not settle: choose another seed")


def assert_decidable(c, smoothing, mask, for_map=False):
    """What the GPU comparisons rely on, asserted on the inputs themselves."""
    assert not bool(undecided(c, smoothing, mask, for_map).any()), "a thresholded quantity is within 1e-3 of its threshold"
    for t in (c["depth"], c["alpha"], c["intr"]):
        assert t is None or t.dtype == torch.float32
    assert bool(torch.isfinite(c["intr"]).all()) and bool((c["intr"][:, :2] > 0).all())


def _seed(H, W, smoothing, with_alpha, target, mask):
    return 1000 * H + 10 * W + (3 if smoothing else 0) + (5 if with_alpha else 0) + MASKS.index(mask) * 100000 + \
        (target == "gt_normals") * 50000


@functools.lru_cache(maxsize=None)
def case(H, W, smoothing, with_alpha, target, mask):
    """Inputs, cotangents and every float64 reference of one loss case, computed once and shared (never modified)."""
    seed = _seed(H, W, smoothing, with_alpha, target, mask)
    c = settle(raw_inputs(H, W, with_alpha, target, mask, seed), smoothing, mask, seed)
    kw = _kw(c, smoothing, mask)
    g_sum = torch.randn(B, generator=torch.Generator().manual_seed(seed + 1))
    c = dict(c, kw=kw, g_sum=g_sum, smoothing=smoothing, mask=mask)
    c["vals"] = NR.values(c["depth"], c["intr"], c["alpha"], **kw)
    c["grads"] = {"terms": NR.grad(c["depth"], c["intr"], c["alpha"], g_sum, **kw)}
    loss, gd, ga = NR.loss_grad(c["depth"], c["intr"], c["alpha"], **kw)
    c["loss"] = loss
    c["grads"]["loss"] = (gd, ga)
    return c


@functools.lru_cache(maxsize=None)
def map_case(H, W, smoothing, with_alpha, mask):
    """The same for depth_normals: the float64 map and the gradients for a random [B, 3, H, W] cotangent."""
    seed = _seed(H, W, smoothing, with_alpha, "gt_depth", mask) + 7
    c = raw_inputs(H, W, with_alpha, "gt_depth", mask, seed)
    c.pop("gt_depth")
    c = settle(c, smoothing, mask, seed, for_map=True)
    kw = dict(smoothing=smoothing, alpha_floor=FLOOR, **thresholds(mask))
    g = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed + 1))
    c = dict(c, kw=kw, g=g, smoothing=smoothing, mask=mask)
    c["normals"] = NR.normals_values(c["depth"], c["intr"], c["alpha"], **kw)
    c["grads"] = NR.normals_grad(c["depth"], c["intr"], c["alpha"], g, **kw)
    return c
