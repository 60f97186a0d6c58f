"""Shared case generator of tests/test_exposure_host.py and tests/test_exposure_hip.py: shapes, id patterns, inputs and fit
cases, seeded, float32 on the CPU, each with its float64 reference (tests/exposure_ref.py) computed once and cached.

Every fit case handed out satisfies, in float64, kappa(M + ridge cnt I) <= 1e7 for every view with a valid pixel (the bound of
the GPU test is linear in kappa); a draw that does not is redrawn with the next seed."""
import functools

import torch

import exposure_ref as R

CHUNK = 4096                                   # freesplat_amd.exposure.CHUNK (asserted by the host test)
KAPPA_MAX = 1e7
B = 3

_W = 93
# odd pixel counts for the scalar head / tail; 64 x 64: every plane 16-byte aligned; the last: three workgroups per image, a
# pixel count that is neither a multiple of a workgroup's nor of four
SHAPES = [(1, 1), (2, 3), (5, 7), (13, 9), (17, 33), (31, 65), (64, 64), (-(-(2 * CHUNK + 1) // _W), _W)]
LARGE = SHAPES[-1]

# name -> (view_ids, V)
PATTERNS = {"none": (None, 3), "dup": ([2, 0, 2], 4), "oor": ([0, 7, -1], 2)}

MASKS = ("none", "blocks", "view_masked")
RIDGES = (1e-6, 0.0)
RIDGE0_MIN_PIXELS = 35                          # ridge = 0 only where every view keeps enough pixels for kappa(M) <= 1e7


def gen(*seed):
    return torch.Generator().manual_seed(hash(tuple(seed)) % (2 ** 31))


def draw_params(V, g):
    A = torch.eye(3) + 0.2 * torch.randn(V, 3, 3, generator=g)
    return torch.cat([A, 0.1 * torch.randn(V, 3, 1, generator=g)], 2).contiguous()


def blocky(H, W, n, g, p, cell=4):
    """[n, H, W] bool, True with probability p in cell x cell blocks."""
    coarse = torch.rand(n, -(-H // cell), -(-W // cell), generator=g) < p
    return coarse.repeat_interleave(cell, 1).repeat_interleave(cell, 2)[:, :H, :W]


@functools.lru_cache(maxsize=None)
def apply_case(H, W, pattern):
    """image, g_out [B, 3, H, W], params [V, 3, 4] float32, ids, V and the float64 references with their absolute-term sums."""
    ids, V = PATTERNS[pattern]
    g = gen(H, W, len(pattern), 1)
    image = torch.rand(B, 3, H, W, generator=g)
    params = draw_params(V, g)
    g_out = torch.randn(B, 3, H, W, generator=g)
    c = dict(image=image, params=params, g_out=g_out, ids=ids, V=V)
    c["out"], c["out_abs"] = R.apply(image, params, ids), R.apply(image, params, ids, absolute=True)
    c["g_image"], c["g_params"], c["n"] = R.apply_grad(image, params, ids, g_out)
    c["g_image_abs"], c["g_params_abs"], _ = R.apply_grad(image, params, ids, g_out, absolute=True)
    return c


def fit_cases(H, W):
    """The (mask, nonfinite, ridge) combinations of a shape."""
    ridges = RIDGES if H * W >= RIDGE0_MIN_PIXELS else RIDGES[:1]
    return [(m, nf, r) for m in MASKS for nf in (False, True) for r in ridges]


def _draw_fit(H, W, pattern, mask_kind, nonfinite, seed):
    ids, V = PATTERNS[pattern]
    g = gen(H, W, len(pattern), len(mask_kind), int(nonfinite), seed)
    pred = torch.rand(B, 3, H, W, generator=g)
    true = draw_params(V, g)
    idl = R.resolve_ids(ids, B, V)
    per_entry = torch.stack([true[v] if 0 <= v < V else R.identity(1, torch.float32)[0] for v in idl])
    target = R.eager_apply(pred, per_entry) + 0.02 * torch.randn(B, 3, H, W, generator=g)
    mask = None
    if mask_kind != "none":
        mask = ~blocky(H, W, B, g, 0.3)
        if mask_kind == "view_masked":                                         # every entry of the first entry's view
            mask[[b for b, v in enumerate(idl) if v == idl[0]]] = False
    if nonfinite:                                                              # under the mask and outside it
        bad = torch.tensor([float("nan"), float("inf"), -float("inf")])
        for t in (pred, target):
            hit = torch.rand(B, 3, H, W, generator=g) < 0.04
            t[hit] = bad[torch.randint(0, 3, (int(hit.sum()),), generator=g)]
    return dict(pred=pred, target=target, mask=mask, ids=ids, V=V, true=true)


@functools.lru_cache(maxsize=None)
def fit_case(H, W, pattern, mask_kind, nonfinite, ridge):
    for seed in range(50):
        c = _draw_fit(H, W, pattern, mask_kind, nonfinite, seed)
        c["params"], c["count"], c["solved"], c["kappa"] = R.fit(c["pred"], c["target"], c["mask"], c["ids"], c["V"], ridge)
        live = c["count"] > 0
        if not bool(live.any()) or float(c["kappa"][live].max()) <= KAPPA_MAX:
            c["ridge"], c["seed"] = ridge, seed
            assert_kappa(c)
            return c
    raise AssertionError(f"no draw of {(H, W, pattern, mask_kind, nonfinite, ridge)} met kappa <= {KAPPA_MAX:g}")


def assert_kappa(c):
    live = c["count"] > 0
    assert bool((c["kappa"][live] <= KAPPA_MAX).all()), c["kappa"]
    assert bool((c["solved"] == live).all()), (c["solved"], c["count"])       # at this kappa every pivot is positive
