"""Host checks of the exposure compensation (no GPU): the float64 restatement (tests/exposure_ref.py) against known answers and
against torch.autograd, the C boundary of include/freesplat_amd_exposure.h without a device, the Python layer's argument errors
and the case generator's kappa condition over every case the GPU test uses."""
import ctypes as C
import os
import re

import pytest
import torch

import exposure_cases as EC
import exposure_ref as ER
from util_abi import declared_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = ["fs_exposure_api_version", "fs_exposure_scratch_bytes", "fs_exposure_apply_forward", "fs_exposure_apply_backward",
            "fs_exposure_fit"]


# ---- the restatement against known answers ---------------------------------------------------------------------------------

def test_identity_parameters_return_the_image():
    g = torch.Generator().manual_seed(0)
    x = torch.rand(3, 3, 5, 7, generator=g)
    assert torch.equal(ER.apply(x, ER.identity(3)), x.double())
    assert torch.equal(ER.apply(x, ER.identity(4), [2, 0, 2]), x.double())
    assert torch.equal(ER.apply(x, 5.0 * ER.identity(1), [4, -1, 1]), x.double())          # out of range: passed through


def test_a_pure_gain_and_offset():
    x = torch.rand(2, 3, 4, 4, generator=torch.Generator().manual_seed(1)).double()
    q = ER.identity(2)
    q[0, :, :3] *= 2.0
    q[0, :, 3] = torch.tensor([0.1, 0.2, 0.3])
    q[1, 0, 1] = 0.5                                                         # red gets half of green
    out = ER.apply(x, q)
    assert torch.allclose(out[0], 2.0 * x[0] + torch.tensor([0.1, 0.2, 0.3]).view(3, 1, 1).double(), rtol=0, atol=1e-15)
    assert torch.allclose(out[1, 0], x[1, 0] + 0.5 * x[1, 1], rtol=0, atol=1e-15) and torch.equal(out[1, 1:], x[1, 1:])


def test_an_exact_affine_target_is_recovered_by_the_fit():
    g = torch.Generator().manual_seed(2)
    x = torch.rand(3, 3, 9, 11, generator=g).double()
    true = EC.draw_params(4, g).double()
    ids = [2, 0, 2]
    y = ER.apply(x, true, ids)
    for ridge, tol in ((0.0, 1e-11), (1e-6, 1e-4)):
        params, count, solved, kappa = ER.fit(x, y, None, ids, 4, ridge)
        assert count.tolist() == [99, 0, 198, 0] and solved.tolist() == [True, False, True, False]
        assert float((params[[0, 2]] - true[[0, 2]]).abs().max()) <= tol
        assert torch.equal(params[[1, 3]], ER.identity(2))                  # unreferenced views: the identity exactly
        assert float(kappa[[0, 2]].max()) < 1e3


def test_a_masked_out_view_gives_the_identity_unsolved():
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 3, 6, 6, generator=g)
    y = torch.rand(2, 3, 6, 6, generator=g)
    mask = torch.ones(2, 6, 6)
    mask[1] = 0
    params, count, solved, _ = ER.fit(x, y, mask)
    assert count.tolist() == [36, 0] and solved.tolist() == [True, False] and torch.equal(params[1], ER.identity(1)[0])
    y[0, 1, 2, 3] = float("nan")                                             # a non-finite value takes its pixel out
    x[0, 0, 0, 0] = float("inf")
    assert ER.fit(x, y, mask)[1].tolist() == [34, 0]
    # ridge 0 on a rank-deficient system: a pivot that is not positive, the identity
    one = torch.rand(1, 3, 1, 1, generator=g)
    p0, c0, s0, _ = ER.fit(one, one, ridge=0.0)
    assert c0.tolist() == [1] and s0.tolist() == [False] and torch.equal(p0, ER.identity(1))
    p1, _, s1, k1 = ER.fit(one, one, ridge=1e-6)
    assert s1.tolist() == [True] and float(k1) < EC.KAPPA_MAX


@pytest.mark.parametrize("pattern", list(EC.PATTERNS))
def test_the_apply_gradient_equals_autograd(pattern):
    ids, V = EC.PATTERNS[pattern]
    g = torch.Generator().manual_seed(4)
    x = torch.rand(EC.B, 3, 5, 7, generator=g, dtype=torch.float64).requires_grad_(True)
    q = EC.draw_params(V, g).double().requires_grad_(True)
    cot = torch.randn(EC.B, 3, 5, 7, generator=g, dtype=torch.float64)
    rows = []
    for b, v in enumerate(ER.resolve_ids(ids, EC.B, V)):                       # the definition, written for autograd
        rows.append(x[b] if not 0 <= v < V else torch.einsum("ck,khw->chw", q[v, :, :3], x[b]) + q[v, :, 3].view(3, 1, 1))
    out = torch.stack(rows)
    assert float((out.detach() - ER.apply(x.detach(), q.detach(), ids)).abs().max()) <= 1e-12
    want = torch.autograd.grad(out, [x, q], cot)
    got = ER.apply_grad(x.detach(), q.detach(), ids, cot)
    for a, b in zip(got[:2], want):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    referenced = {v for v in ER.resolve_ids(ids, EC.B, V) if 0 <= v < V}
    for v in range(V):
        assert (v in referenced) == bool(got[1][v].any()) and int(got[2][v]) == 35 * sum(1 for i in ER.resolve_ids(ids, EC.B, V) if i == v)


# ---- the C boundary --------------------------------------------------------------------------------------------------------

def test_exposure_header_is_exported_and_bound():
    from freesplat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    names = declared_names("freesplat_amd_exposure.h")
    assert names == sorted(EXPECTED)
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/freesplat_amd_exposure.h but not exported"
    assert set(_lib.EXPOSURE_SIGNATURES) == set(names)
    assert _lib.lib().fs_exposure_api_version() == 1 == _lib.EXPOSURE_API_VERSION
    text = open(os.path.join(ROOT, "include", "freesplat_amd_exposure.h")).read()
    assert re.search(r"#define\s+FS_EXPOSURE_API_VERSION\s+1\b", text)


P = C.c_void_p(4096)      # a fake non-NULL pointer: nothing may launch with it


def _fwd(L, B=2, V=2, H=16, W=16, ptrs=None):
    ptrs = [P, P, None, P] if ptrs is None else ptrs                  # image, params, view_ids | out
    return L.fs_exposure_apply_forward(B, V, H, W, *ptrs, None)


def _bwd(L, B=2, V=2, H=16, W=16, ptrs=None):
    ptrs = [P, P, None, P, P, P, P] if ptrs is None else ptrs         # image, params, view_ids, g_out | g_image, g_params, scratch
    return L.fs_exposure_apply_backward(B, V, H, W, *ptrs, None)


def _fit(L, B=2, V=2, H=16, W=16, ptrs=None, ridge=1e-6):
    ptrs = [P, P, None, None, P, P, P, P] if ptrs is None else ptrs   # pred, target, mask, view_ids | params, count, solved, scratch
    return L.fs_exposure_fit(B, V, H, W, *ptrs[:4], ridge, *ptrs[4:], None)


def test_entry_points_validate_before_touching_a_device():
    """FS_ERR_INVALID_ARG (-1) from every int-returning entry point for NULL pointers with positive sizes; 0 or -1 with zero sizes;
    -1 for non-positive sizes, a missing required pointer, B != V without ids, a bad ridge; FS_ERR_UNSUPPORTED (-3) for an H * W
    beyond the 32-bit pixel index -- all but the first with fake non-NULL pointers, so nothing may launch."""
    from freesplat_amd import _lib
    L = _lib.lib()
    checked = 0
    for name, (rt, at) in _lib.EXPOSURE_SIGNATURES.items():
        if rt is not C.c_int or not at:
            continue
        for size in (1, 16):
            args = [size if a is C.c_int32 else (1e-6 if a is C.c_double else None) for a in at]
            assert getattr(L, name)(*args) == -1, name
        zero = [0 if a is C.c_int32 else (1e-6 if a is C.c_double else None) for a in at]
        assert getattr(L, name)(*zero) in (0, -1), name
        zero = [0 if a is C.c_int32 else (1e-6 if a is C.c_double else P) for a in at]
        assert getattr(L, name)(*zero) in (0, -1), name
        checked += 1
    assert checked == 3
    for call in (_fwd, _bwd, _fit):
        for bad in (dict(B=0, V=0), dict(B=-1, V=-1), dict(V=0), dict(H=0), dict(W=-3), dict(B=2, V=3)):
            assert call(L, **bad) == -1, (call.__name__, bad)
        assert call(L, H=46341, W=46341) == -3, call.__name__                 # H * W > 2^31 - 1
        assert call(L, B=2 ** 30, V=2 ** 30, H=128, W=128) == -3, call.__name__     # the workgroup count
    for i in (0, 1, 3):
        assert _fwd(L, ptrs=[None if k == i else v for k, v in enumerate([P, P, None, P])]) == -1, i
    base = [P, P, None, P, P, P, P]
    for i in (1, 3):                                                         # params, g_out
        assert _bwd(L, ptrs=[None if k == i else v for k, v in enumerate(base)]) == -1, i
    assert _bwd(L, ptrs=[P, P, None, P, None, None, P]) == -1                # neither gradient
    assert _bwd(L, ptrs=[None, P, None, P, P, P, P]) == -1                   # g_params without the image
    assert _bwd(L, ptrs=[P, P, None, P, P, P, None]) == -1                   # g_params without scratch
    base = [P, P, None, None, P, P, P, P]
    for i in (0, 1, 4, 5, 6, 7):
        assert _fit(L, ptrs=[None if k == i else v for k, v in enumerate(base)]) == -1, i
    for ridge in (-1e-9, float("nan"), float("inf"), -float("inf")):
        assert _fit(L, ridge=ridge) == -1, ridge


def test_scratch_bytes():
    """One row of 22 doubles per workgroup, rounded up to 256; monotone in every size; 0 for what the entry points refuse."""
    from freesplat_amd import _lib, exposure as E
    L = _lib.lib()
    assert E.CHUNK == EC.CHUNK
    al = lambda x: (x + 255) // 256 * 256
    for B, H, W in ((1, 1, 1), (2, 13, 9), (4, 968, 1296), (3, 64, 64), (3, 64, 65), (3,) + EC.LARGE):
        assert L.fs_exposure_scratch_bytes(B, H, W) == al(22 * 8 * B * -(-H * W // E.CHUNK)) > 0
    sizes = [1, 2, 7, 64, 65, 500, 4096]
    for a, b in zip(sizes, sizes[1:]):
        assert L.fs_exposure_scratch_bytes(a, 64, 64) <= L.fs_exposure_scratch_bytes(b, 64, 64)
        assert L.fs_exposure_scratch_bytes(3, a, 64) <= L.fs_exposure_scratch_bytes(3, b, 64)
        assert L.fs_exposure_scratch_bytes(3, 64, a) <= L.fs_exposure_scratch_bytes(3, 64, b)
    for bad in ((0, 16, 16), (1, 0, 16), (1, 16, -1), (-2, 16, 16), (1, 46341, 46341), (2 ** 30, 128, 128)):
        assert L.fs_exposure_scratch_bytes(*bad) == 0


# ---- the Python layer --------------------------------------------------------------------------------------------------------

def test_python_layer_refuses_what_it_cannot_run():
    """The error cases that need no device."""
    import freesplat_amd
    from freesplat_amd import exposure as E
    assert freesplat_amd.apply_exposure is E.apply_exposure and freesplat_amd.fit_exposure is E.fit_exposure
    assert freesplat_amd.color_corrected is E.color_corrected and freesplat_amd.Exposure is E.Exposure
    x = torch.rand(2, 3, 4, 4)
    q = ER.identity(2, torch.float32)
    for fn in (lambda: E.apply_exposure(x, q), lambda: E.fit_exposure(x, x), lambda: E.color_corrected(x, x),
               lambda: E.Exposure(2)(x), lambda: E.Exposure(2).fit_(x, x)):
        with pytest.raises(ValueError, match=r"freesplat_amd\.exposure: .*HIP device"):
            fn()
    for ridge in (-1.0, float("nan"), float("inf"), True):
        with pytest.raises(ValueError, match=r"freesplat_amd\.exposure: ridge"):
            E.fit_exposure(x, x, ridge=ridge)
    with pytest.raises(ValueError, match="num_views"):
        E.Exposure(0)
    cpu = torch.device("cpu")
    # the id check that runs on the host
    for bad in ([0, 2], [0, -1], [0], [0, 1, 1], [0.0, 1.0], [[0, 1]], torch.tensor([True, False])):
        with pytest.raises(ValueError, match=r"freesplat_amd\.exposure: view_ids"):
            E._view_ids(bad, 2, 2, cpu)
    with pytest.raises(ValueError, match="one entry per view"):
        E._view_ids(None, 2, 3, cpu)
    assert E._view_ids(None, 2, 2, cpu) is None
    got = E._view_ids([1, 0], 2, 2, cpu)
    assert got.dtype == torch.int64 and got.tolist() == [1, 0]
    assert E._view_ids(torch.tensor([1, 1], dtype=torch.int32), 2, 2, cpu).dtype == torch.int64
    m = E.Exposure(3)
    assert isinstance(m.params, torch.nn.Parameter) and torch.equal(m.params.detach(), ER.identity(3, torch.float32))
    assert "torch.optim.Adam([exposure.params]" in E.Exposure.__doc__


# ---- the GPU cases' inputs ---------------------------------------------------------------------------------------------------

def test_case_grid():
    from freesplat_amd.exposure import CHUNK
    H, W = EC.LARGE
    assert -(-H * W // CHUNK) >= 3 and (H * W) % CHUNK and (H * W) % 4
    assert EC.SHAPES[:7] == [(1, 1), (2, 3), (5, 7), (13, 9), (17, 33), (31, 65), (64, 64)] and len(EC.SHAPES) == 8
    assert EC.PATTERNS == {"none": (None, 3), "dup": ([2, 0, 2], 4), "oor": ([0, 7, -1], 2)}
    assert len(EC.fit_cases(1, 1)) == 6 and len(EC.fit_cases(5, 7)) == 12


@pytest.mark.parametrize("H,W", EC.SHAPES)
def test_every_fit_case_meets_the_kappa_condition(H, W):
    """kappa(M + ridge cnt I) <= 1e7 in float64 for every view with a valid pixel, of every case the GPU test compares; such a
    view is solved, a view without a pixel is the identity."""
    worst = 0.0
    for pattern in EC.PATTERNS:
        for mask_kind, nonfinite, ridge in EC.fit_cases(H, W):
            c = EC.fit_case(H, W, pattern, mask_kind, nonfinite, ridge)
            EC.assert_kappa(c)
            live = c["count"] > 0
            assert torch.equal(c["params"][~live], ER.identity(int((~live).sum())))
            if mask_kind == "view_masked":
                assert not bool(live.all())
            if nonfinite and H * W >= 35:
                assert not bool(torch.isfinite(c["pred"]).all()) and not bool(torch.isfinite(c["target"]).all())
            if bool(live.any()):
                worst = max(worst, float(c["kappa"][live].max()))
    print(f"{H} x {W}: largest kappa {worst:.3g}")
    assert worst <= EC.KAPPA_MAX
