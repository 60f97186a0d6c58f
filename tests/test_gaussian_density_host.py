"""CPU checks of adaptive density control: the one-pass rules against the literal 3DGS sequence (tests/gaussian_density_ref.py),
the generator's statistics, and the C boundary of include/freesplat_amd_density.h (exports, binding table, revision, argument
validation with fake pointers -- nothing may launch).  No GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gaussian_density_ref as D  # noqa: E402
from util_abi import declared_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the text of the header under test: the restatement's constants are checked against it, so that the two cannot drift apart
HEADER = open(os.path.join(ROOT, "include", "freesplat_amd_density.h")).read()
EXPECTED = ["fs_density_accumulate", "fs_density_api_version", "fs_density_apply", "fs_density_plan",
            "fs_density_plan_scratch_bytes", "fs_density_reset_opacity"]


@pytest.mark.parametrize("screen,prune_big", [(None, False), (20.0, False), (None, True), (20.0, True)])
def test_one_pass_rules_give_the_rows_of_the_literal_sequence(screen, prune_big):
    """N = 1031 random rows: every kind, rows never seen, rows on both sides of prune_scale and of 1.6 prune_scale (and none
    within rounding of a threshold: the sequence divides by 1.6 in float64 where the rules compare with (float)(1.6 p))."""
    N, extent = 1031, 10.0
    rng = np.random.default_rng(3)
    th = D.thresholds(extent, grad_threshold=2e-4, min_opacity=0.05, percent_dense=0.01, max_screen_size=screen, prune_big=prune_big)
    denom = rng.integers(0, 4, N).astype(np.float32)
    grad_accum = (denom * 2e-4 * 10.0 ** rng.uniform(-1.0, 1.0, N)).astype(np.float32)
    # s_max from 0.02 to 5: below / above dense_scale = 0.1, prune_scale = 1.0 and 1.6
    scales = (10.0 ** rng.uniform(-1.7, 0.7, (N, 1)) * rng.uniform(0.2, 1.0, (N, 3))).astype(np.float32)
    opacities = rng.uniform(0.0, 1.0, N).astype(np.float32) ** 3
    max_radii = rng.integers(0, 40, N).astype(np.float32)
    kind, offset, totals = D.plan(grad_accum, denom, max_radii, scales, opacities, th)
    for k, name in enumerate(("DROPPED", "KEPT", "CLONE", "SPLIT")):                  # the kinds are the header's
        assert re.search(r"#define\s+FS_DENSITY_%s\s+%d\b" % (name, k), HEADER) and getattr(D, name) == k
    s_max = scales.max(1)
    for t in (0.1, 1.0, 1.6):
        assert (s_max < 0.99 * t).any() and (s_max > 1.01 * t).any() and not (np.abs(s_max / t - 1.0) < 1e-5).any()
    assert not (np.abs(grad_accum / np.maximum(denom, 1) / 2e-4 - 1.0) < 1e-5).any()
    assert (denom == 0).sum() > 100 and set(kind.tolist()) == {D.DROPPED, D.KEPT, D.CLONE, D.SPLIT}
    if prune_big:       # split parents on both sides of 1.6 prune_scale, unsplit rows on both sides of prune_scale
        hot = (denom > 0) & (grad_accum >= th[0] * denom) & (opacities >= th[2])
        assert (kind[hot & (s_max > 1.0) & (s_max < 1.6)] == D.SPLIT).all() and (hot & (s_max > 1.0) & (s_max < 1.6)).any()
        assert (kind[hot & (s_max > 1.6)] == D.DROPPED).all() and (hot & (s_max > 1.6)).any()
        assert (kind[~hot & (s_max > 1.0)] == D.DROPPED).all() and (~hot & (s_max > 1.0) & (s_max < 1.6)).any()
    assert D.one_pass_rows(kind) == D.sequence(grad_accum, denom, max_radii, scales, opacities, th)
    assert totals[0] == len(D.one_pass_rows(kind)) == int(D.OUTPUTS[kind].sum())
    assert totals[1] + totals[2] + totals[3] + int((kind == D.KEPT).sum()) == N
    rows, j = D.source_map(kind)
    assert np.array_equal(offset[rows] + j, np.arange(totals[0]))               # stable: outputs of row i at offset[i], offset[i] + 1


def test_ties_pin_the_comparisons():
    """Rows exactly on a threshold: >= (hot), > (split), < (min_opacity)."""
    from freesplat_amd import refine
    assert refine._STATS == ("grad_accum", "denom", "max_radii")                      # the order of stats_for and of the plan's inputs
    kind = D.kind_pattern(257, 0)
    got, _, _ = D.plan(*D.stats_for(kind), (D.GRAD_T, D.DENSE, D.MIN_OP, 0.0, 0.0, 0.0))
    assert np.array_equal(got, kind)
    ga, dn, mr, sc, op = D.stats_for(kind)
    tie = np.arange(257) % 3 == 0
    assert (ga[tie & (dn > 0) & (kind >= D.CLONE)] == (np.float32(D.GRAD_T) * dn)[tie & (dn > 0) & (kind >= D.CLONE)]).all()
    assert (sc.max(1)[tie & (kind != D.SPLIT)] == np.float32(D.DENSE)).all() and (op[tie & (kind != D.DROPPED)] == np.float32(D.MIN_OP)).all()


def test_generator_statistics_on_the_cpu():
    """The restated normals of the 4099-row all-split case (24 594 values): |mean| < 0.05, std in [0.95, 1.05] -- about 8
    and 11 standard errors; the uniforms lie in (0, 1] and are fp32 values; seeds, rows, children and words
    all change the bits."""
    for constant in ("0x85EBCA6B", "0xC2B2AE35", "0x9E3779B9", "0x9E3779B1", "6.2831855f", "8 * child + word + 1"):
        assert constant in HEADER, f"{constant}: the header's statement of the generator and the restatement differ"
    N = 4099
    rows = np.repeat(np.arange(N), 2)
    child = np.tile(np.arange(2), N)
    z = D.normals(0, rows, child).numpy()
    assert z.shape == (2 * N, 3) and z.size == 24594
    print(f"generator: mean {z.mean():+.4f} std {z.std():.4f} max |z| {np.abs(z).max():.2f}")
    assert abs(z.mean()) < 0.05 and 0.95 <= z.std() <= 1.05
    for c in range(3):
        assert abs(z[:, c].mean()) < 0.05 and 0.95 <= z[:, c].std() <= 1.05
    u = D.uniforms(0, rows, child)
    assert u.min() > 0.0 and u.max() <= 1.0 and np.array_equal(u.astype(np.float32).astype(np.float64), u)
    assert abs(u.mean() - 0.5) < 0.01 and abs(np.corrcoef(z[0::2].ravel(), z[1::2].ravel())[0, 1]) < 0.03   # the two children
    b = D.bits(0, rows[:, None], child[:, None], np.arange(6)[None, :])
    assert len(np.unique(b)) > 0.999 * b.size
    assert not np.array_equal(b, D.bits(1, rows[:, None], child[:, None], np.arange(6)[None, :]))
    # a known answer, so that a change of the function is seen here before it is seen on a device
    for args, want in (((0, 0, 0, 0), 0xF07CDF35), ((7, 4098, 1, 5), 0x89C1DC8E), ((0xFFFFFFFF, 123456789, 0, 3), 0xE9B8172E)):
        assert int(D.bits(args[0], [args[1]], [args[2]], [args[3]])[0]) == want, args
    assert int(D._fmix(np.array([1], np.uint32))[0]) == 0x514E28B7                                          # murmur3 fmix32(1)


def test_density_header_is_exported_and_bound():
    from freesplat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    names = declared_names("freesplat_amd_density.h")
    assert names == EXPECTED
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/freesplat_amd_density.h but not exported"
        assert n in _lib.DENSITY_SIGNATURES, f"{n} has no ctypes signature in freesplat_amd/_lib.py"
    assert set(_lib.DENSITY_SIGNATURES) == set(names)
    assert _lib.lib().fs_density_api_version() == 1 == _lib.DENSITY_API_VERSION
    text = open(os.path.join(ROOT, "include", "freesplat_amd_density.h")).read()
    assert re.search(r"#define\s+FS_DENSITY_API_VERSION\s+1\b", text)
    for k, name in enumerate(("DROPPED", "KEPT", "CLONE", "SPLIT")):
        assert re.search(r"#define\s+FS_DENSITY_%s\s+%d\b" % (name, k), text) and getattr(D, name) == k


P = 4096      # a fake non-NULL pointer: nothing may launch with it
vp = lambda x: None if x is None else C.c_void_p(x)
table = lambda t: None if t == "null" else (C.c_void_p * 5)(*(t if t is not None else [P] * 5))


def _plan_call(L, N=8, ptrs=None, th=(2e-4, 0.1, 0.005, 0.0, 0.0, 0.0)):
    ptrs = [P] * 10 if ptrs is None else ptrs
    return L.fs_density_plan(N, *[vp(x) for x in ptrs[:5]], *th, *[vp(x) for x in ptrs[5:]], None)


def _apply_call(L, N=8, M=4, N_out=8, src=P, tables=None, out_scales=P, out_opacities=P):
    tables = [None] * 6 if tables is None else tables
    return L.fs_density_apply(N, M, N_out, vp(src), *[table(t) for t in tables], vp(out_scales), vp(out_opacities), 0, None)


def test_entry_points_validate_before_touching_a_device():
    from freesplat_amd import _lib
    L = _lib.lib()
    nan, inf = float("nan"), float("inf")
    # accumulate
    assert L.fs_density_accumulate(0, *[vp(P)] * 5, None) == 0 and L.fs_density_accumulate(0, *[None] * 5, None) == 0
    assert L.fs_density_accumulate(-1, *[vp(P)] * 5, None) == -1
    for k in range(5):
        assert L.fs_density_accumulate(8, *[None if i == k else vp(P) for i in range(5)], None) == -1, k
    # plan
    assert L.fs_density_plan_scratch_bytes(0) == 0 and L.fs_density_plan_scratch_bytes(-5) == 0
    assert L.fs_density_plan_scratch_bytes(1) >= 16 and L.fs_density_plan_scratch_bytes(1 << 20) >= 16 * 1024
    assert L.fs_density_plan_scratch_bytes(1025) >= 32
    assert _plan_call(L, N=0) == 0 and _plan_call(L, N=0, ptrs=[None] * 10) == 0
    assert _plan_call(L, N=-1) == -1 and _plan_call(L, N=2 ** 30) == -1       # src[] keeps bit 31 for the split flag
    for k in range(10):
        assert _plan_call(L, ptrs=[None if i == k else P for i in range(10)]) == -1, k
    for k in range(6):
        for bad in (-1.0, nan, -inf):
            th = [2e-4, 0.1, 0.005, 0.0, 0.0, 0.0]
            th[k] = bad
            assert _plan_call(L, th=th) == -1, (k, bad)
            assert _plan_call(L, N=0, th=th) == -1, (k, bad)
    # apply
    assert _apply_call(L, N=0, N_out=0) == 0 and _apply_call(L, N_out=0) == 0 and _apply_call(L, N=0, N_out=0, src=None, tables=["null"] * 6) == 0
    assert _apply_call(L, N=-1) == -1 and _apply_call(L, N_out=-1) == -1 and _apply_call(L, N=8, N_out=17) == -1
    for M in (0, 2, 3, 5, 8, 15, 17, 25, -1):
        assert _apply_call(L, M=M) == -1, M
    assert _apply_call(L, N=(2 ** 31) // 48 + 1, M=16) == -1 and _apply_call(L, N=2 ** 31 - 1, M=1) == -1
    assert _apply_call(L, N=(2 ** 31) // 48 - 8, M=16, N_out=(2 ** 31) // 48 + 1) == -1
    for name in ("src", "out_scales", "out_opacities"):
        assert _apply_call(L, **{name: None}) == -1, name
    for t in range(6):
        assert _apply_call(L, tables=["null" if i == t else None for i in range(6)]) == -1, t
        for k in range(5):
            entry = [None if i == k else P for i in range(5)]
            assert _apply_call(L, tables=[entry if i == t else None for i in range(6)]) == -1, (t, k)
    # reset_opacity
    p = vp(P)
    assert L.fs_density_reset_opacity(0, 0.01, p, p, p, p, None) == 0 and L.fs_density_reset_opacity(0, 0.01, None, None, None, None, None) == 0
    assert L.fs_density_reset_opacity(-1, 0.01, p, p, p, p, None) == -1
    for bad in (0.0, 1.0, -0.5, 1.5, nan):
        assert L.fs_density_reset_opacity(8, bad, p, p, p, p, None) == -1, bad
    for k in range(4):
        assert L.fs_density_reset_opacity(8, 0.01, *[None if i == k else p for i in range(4)], None) == -1, k


def test_python_layer_has_the_density_interface():
    """What needs no device: the methods exist with the documented defaults, and the docstring names the host sync."""
    import inspect
    from freesplat_amd.refine import GaussianAdam
    sig = inspect.signature(GaussianAdam.densify)
    want = dict(grad_threshold=2e-4, min_opacity=0.005, percent_dense=0.01, max_screen_size=None, prune_big=False, seed=None,
                max_gaussians=None)
    assert {k: v.default for k, v in sig.parameters.items() if k in want} == want and "extent" in sig.parameters
    assert inspect.signature(GaussianAdam.reset_opacity).parameters["max_opacity"].default == 0.01
    assert "host synchronisation" in GaussianAdam.densify.__doc__ and "captur" in GaussianAdam.densify.__doc__
    assert callable(GaussianAdam.accumulate)
