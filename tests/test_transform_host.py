"""Host checks of the similarity transform of Gaussians (no GPU): the float64 restatement (tests/transform_ref.py) against the
defining identities and against the dense float64 renderer (the rendering invariance, with negative controls), the C boundary of
include/freesplat_amd_transform.h without a device, the Python layer's argument errors and the adapter's coords=None path."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import transform_cases as TC
import transform_ref as TR
from oracle.raster_dense_torch import _sh_color, render_dense
from util_abi import declared_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = ["fs_transform_api_version", "fs_transform_prepare", "fs_sh_rotate", "fs_gaussians_transform_forward",
            "fs_gaussians_transform_backward"]
F64 = torch.float64


def _rot(seed):
    return TR.random_rotation(torch.Generator().manual_seed(seed))


# ---- the restatement ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("l", [0, 1, 2, 3])
def test_the_restatement_satisfies_the_defining_identities(l):
    g = torch.Generator().manual_seed(10 + l)
    R1, R2 = TR.random_rotation(g), TR.random_rotation(g)
    d = torch.randn(200, 3, dtype=F64, generator=g)
    d = d / d.norm(dim=1, keepdim=True)                                   # fresh directions, not the 64 of the fit
    D1, D2 = TR.sh_matrix(l, R1), TR.sh_matrix(l, R2)
    n = 2 * l + 1
    assert float((TR.band(l, d @ R1.T) - TR.band(l, d) @ D1.T).abs().max()) <= 1e-12            # b_l(R d) = D_l b_l(d)
    assert float((TR.sh_matrix(l, torch.eye(3, dtype=F64)) - torch.eye(n, dtype=F64)).abs().max()) <= 1e-12    # D(I) = I
    assert float((TR.sh_matrix(l, R1 @ R2) - D1 @ D2).abs().max()) <= 1e-12                     # D(R1 R2) = D(R1) D(R2)
    assert float((D1.T @ D1 - torch.eye(n, dtype=F64)).abs().max()) <= 1e-12                    # orthogonal
    if l:
        assert float((D1 - torch.eye(n, dtype=F64)).abs().max()) > 0.1                          # (and not the identity)


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_rotated_coefficients_give_the_same_colour_in_the_rotated_direction(deg):
    g = torch.Generator().manual_seed(20 + deg)
    R = TR.random_rotation(g)
    M = (deg + 1) ** 2
    c = torch.randn(50, M, 3, dtype=F64, generator=g)
    d = torch.randn(50, 3, dtype=F64, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    want = _sh_color(deg, d, c)
    got = _sh_color(deg, d @ R.T, TR.rotate_sh(c, R[None]))
    assert float((got - want).abs().max()) <= 1e-12
    cm = TR.rotate_sh(c.transpose(1, 2), R[None], layout="channel_major").transpose(1, 2)      # the other layout, the same numbers
    assert float((cm - TR.rotate_sh(c, R[None])).abs().max()) <= 1e-14
    back = TR.rotate_sh(TR.rotate_sh(c, R[None]), R[None], transpose=True)
    assert float((back - c).abs().max()) <= 1e-12
    if deg:
        assert float((_sh_color(deg, d @ R.T, c) - want).abs().max()) > 1e-2                    # unrotated coefficients do differ


def test_quaternion_and_package_matrices_agree_with_the_restatement():
    from freesplat_amd.transform import compose, sh_rotation_matrices, similarity_inverse, similarity_matrix, transform_cameras
    g = torch.Generator().manual_seed(30)
    for k in range(8):
        R = TR.random_rotation(g)
        q = TR.matrix_to_quat(R)
        assert float(q[0]) >= 0 and abs(float(q.norm()) - 1) <= 1e-14 and float((TR.quat_to_matrix(q) - R).abs().max()) <= 1e-13
        R2 = TR.random_rotation(g)
        assert float((TR.quat_to_matrix(TR.quat_mul(q, TR.matrix_to_quat(R2))) - R @ R2).abs().max()) <= 1e-13
        for l, D in enumerate(sh_rotation_matrices(R, 3)):                  # the quadrature form against the least-squares form
            assert D.dtype == F64 and float((D - TR.sh_matrix(l, R)).abs().max()) <= 1e-12
    s, R, t = 1.7, TR.random_rotation(g), torch.randn(3, dtype=F64, generator=g)
    T = similarity_matrix(s, R, t)
    x = torch.randn(5, 3, dtype=F64, generator=g)
    y = s * x @ R.T + t
    Ti = similarity_inverse(T)
    assert float((y @ Ti[:3, :3].T + Ti[:3, 3] - x).abs().max()) <= 1e-13
    si, Ri, ti = similarity_inverse((s, R, t))
    assert float((similarity_matrix(si, Ri, ti) - Ti).abs().max()) <= 1e-14
    assert float((compose(Ti, T) - torch.eye(4, dtype=F64)).abs().max()) <= 1e-13
    T2 = similarity_matrix(0.5, TR.random_rotation(g), torch.randn(3, dtype=F64, generator=g))
    assert float((compose(T2, T) - T2 @ T).abs().max()) <= 1e-13
    c2w = torch.eye(4, dtype=F64)
    c2w[:3, :3], c2w[:3, 3] = TR.random_rotation(g), torch.randn(3, dtype=F64, generator=g)
    got = transform_cameras(c2w[None], T)[0]
    assert float((got - TR.transform_cameras(c2w, s, R, t)).abs().max()) <= 1e-13
    assert float((got[:3, :3].T @ got[:3, :3] - torch.eye(3, dtype=F64)).abs().max()) <= 1e-13   # rigid: no scale in the rotation


# ---- the rendering invariance -------------------------------------------------------------------------------------------------

def _render(sc, means, scales, rotations, shs, c2w, discrete):
    from freesplat_amd.rasterizer import build_cov3d
    H, W = 24, 32
    view, proj, campos, tx, ty = TC.camera_matrices(c2w, sc["near"], sc["far"])
    cov6 = build_cov3d(scales, rotations, 1.0)
    if discrete is None:
        from oracle import raster_oracle as ro
        n = lambda t: t.float().numpy()
        st = ro.forward(H, W, tx, ty, np.zeros(3, np.float32), n(view), n(proj), sc["sh_degree"], n(campos), n(means), n(cov6),
                        n(sc["opacities"]), shs=n(shs))
        order = torch.from_numpy(np.lexsort((np.arange(st["N"]), st["depths"].view(np.uint32))).astype(np.int64))
        discrete = dict(rect=torch.from_numpy(st["rect"]), radii=torch.from_numpy(st["radii"]), order=order)
    color, depth, _ = render_dense(H, W, tx, ty, torch.tensor([0.2, 0.3, 0.1], dtype=F64), view, proj, sc["sh_degree"], campos,
                                   means, cov6, sc["opacities"], shs=shs, **discrete)
    return color, depth, discrete


@pytest.mark.parametrize("s", [2.0, 0.5])
def test_rendering_the_transformed_scene_from_the_transformed_camera_gives_the_same_image(s):
    """24 x 32, 100 Gaussians, degree 3, float64 through render_dense with the discrete inputs of the C oracle's forward of the
    ORIGINAL scene for both renders.  Colour within 1e-9, depth' = s depth within 1e-9 of the largest depth (depths are about
    1000 units: transform_cases.invariance_scene says why).  Rounding sits near 1e-13; a wrong convention moves pixels by 1e-3
    and more, which the three negative controls show on this very scene."""
    sc = TC.invariance_scene()
    g = torch.Generator().manual_seed(41)
    R, t = TR.random_rotation(g), 300.0 * torch.randn(3, dtype=F64, generator=g)
    xf = torch.cat([s * R, t[:, None]], 1)[None]
    color, depth, discrete = _render(sc, sc["means"], sc["scales"], sc["rotations"], sc["shs"], sc["c2w"], None)
    assert int((discrete["radii"] > 0).sum()) >= 90 and float(depth.max()) > 500.0
    assert float(color.std()) > 0.05                                        # (an image, not a flat background)
    m, scl, q, _, sh = TR.transform(xf, None, sc["means"], sc["scales"], sc["rotations"], None, sc["shs"])
    c2w = TR.transform_cameras(sc["c2w"], s, R, t)
    color2, depth2, _ = _render(sc, m, scl, q, sh, c2w, discrete)
    err_c = float((color2 - color).abs().max())
    err_d = float((depth2 - s * depth).abs().max() / (s * depth).abs().max())
    print(f"s = {s}: colour {err_c:.3e}, depth (relative to the largest) {err_d:.3e}")
    assert err_c <= 1e-9 and err_d <= 1e-9
    # negative controls: each must be visible, by orders of magnitude
    sh_inverse = TR.rotate_sh(sc["shs"], R.T[None])
    q_swapped = TR.quat_mul(sc["rotations"], TR.matrix_to_quat(R)[None])
    for name, args in (("D(R^T)", (m, scl, q, sh_inverse)), ("SH left unrotated", (m, scl, q, sc["shs"])),
                       ("q (x) q_R", (m, scl, q_swapped, sh))):
        bad = float((_render(sc, *args, c2w, discrete)[0] - color).abs().max())
        print(f"  control {name}: {bad:.3e}")
        assert bad > 1e-4, name


# ---- the C boundary -----------------------------------------------------------------------------------------------------------

def test_transform_header_is_exported_and_bound():
    from freesplat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    names = declared_names("freesplat_amd_transform.h")
    assert names == sorted(EXPECTED)
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/freesplat_amd_transform.h but not exported"
    assert set(_lib.TRANSFORM_SIGNATURES) == set(names)
    assert _lib.lib().fs_transform_api_version() == 1 == _lib.TRANSFORM_API_VERSION
    text = open(os.path.join(ROOT, "include", "freesplat_amd_transform.h")).read()
    assert re.search(r"#define\s+FS_TRANSFORM_API_VERSION\s+1\b", text)
    for name, value in (("TABLE_FLOATS", 100), ("S", 0), ("R", 1), ("T", 10), ("Q", 13), ("D1", 17), ("D2", 26), ("D3", 51),
                        ("SH_CHANNEL_MAJOR", 1), ("SH_TRANSPOSE", 2), ("QUAT_XYZW", 4), ("COV_FULL", 8)):
        assert re.search(rf"#define\s+FS_TRANSFORM_{name}\s+{value}\b", text), name
        assert getattr(_lib, "TRANSFORM_" + name) == value
    assert TR.TABLE_FLOATS == 100 and TR.OFF == dict(s=0, R=1, t=10, q=13, D1=17, D2=26, D3=51)


P = C.c_void_p(4096)      # a fake non-NULL pointer: nothing may launch with it


def _prepare(L, V=1, ptrs=(P, P)):
    return L.fs_transform_prepare(V, *ptrs, None)


def _rotate(L, N=8, M=16, V=1, flags=0, ptrs=(P, P, None, P)):              # sh_in, table, ids | sh_out
    return L.fs_sh_rotate(N, M, V, flags, *ptrs, None)


def _xform(L, which, N=8, M=16, V=1, flags=0, table=P, ids=None, ins=(P,) * 5, outs=(P,) * 5):
    return getattr(L, "fs_gaussians_transform_" + which)(N, M, V, flags, table, ids, *ins, *outs, None)


def test_entry_points_validate_before_touching_a_device():
    """FS_ERR_INVALID_ARG (-1) from every int-returning entry point, with fake non-NULL pointers wherever a pointer is given, so
    nothing may launch: all-NULL pointers, sizes <= 0, M outside {1, 4, 9, 16}, ids NULL with V != 1, unknown flag bits, a
    missing required pointer, an input without its output, all five arrays NULL."""
    from freesplat_amd import _lib
    L = _lib.lib()
    checked = 0
    for name, (rt, at) in _lib.TRANSFORM_SIGNATURES.items():
        if rt is not C.c_int or not at:
            continue
        for size in (1, 16):
            assert getattr(L, name)(*[size if a is C.c_int32 else None for a in at]) == -1, name
        assert getattr(L, name)(*[0 if a is C.c_int32 else P for a in at]) == -1, name
        checked += 1
    assert checked == 4
    for V in (0, -1):
        assert _prepare(L, V=V) == -1
    assert _prepare(L, ptrs=(None, P)) == -1 and _prepare(L, ptrs=(P, None)) == -1
    for bad in (dict(N=0), dict(N=-5), dict(V=0), dict(V=-1), dict(M=0), dict(M=2), dict(M=3), dict(M=25), dict(M=-1), dict(V=2),
                dict(flags=4), dict(flags=8), dict(flags=16), dict(flags=-1)):
        assert _rotate(L, **bad) == -1, bad
    for i in (0, 1, 3):
        assert _rotate(L, ptrs=[None if k == i else v for k, v in enumerate((P, P, None, P))]) == -1, i
    for which in ("forward", "backward"):
        for bad in (dict(N=0), dict(N=-5), dict(V=0), dict(V=-1), dict(M=0), dict(M=2), dict(M=15), dict(M=17), dict(V=2),
                    dict(flags=2), dict(flags=16), dict(flags=-1), dict(table=None), dict(ins=(None,) * 5),
                    dict(ins=(None,) * 5, outs=(None,) * 5)):
            assert _xform(L, which, **bad) == -1, (which, bad)
        for i in range(5):                                                   # an input without its output
            assert _xform(L, which, outs=tuple(None if k == i else P for k in range(5))) == -1, (which, i)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------

def test_a_host_transform_that_is_no_similarity_is_rejected():
    """Sheared, non-uniformly scaled, reflected, zero or negative scale, a projective last row, non-finite: ValueError naming the
    defect, raised before any tensor is looked at (so it needs no device)."""
    from freesplat_amd.transform import transform_gaussians
    R = _rot(50)
    x = torch.zeros(4, 3)                                                    # a CPU tensor: never reached
    T = torch.eye(4, dtype=F64)
    T[:3, :3], T[:3, 3] = 1.5 * R, torch.tensor([1.0, 2.0, 3.0], dtype=F64)
    shear = T.clone()
    shear[0, 1] += 1e-3
    squash = T.clone()
    squash[:3, :3] = R @ torch.diag(torch.tensor([1.0, 1.0, 1.01], dtype=F64))
    mirror = T.clone()
    mirror[:3, :3] = T[:3, :3] @ torch.diag(torch.tensor([1.0, 1.0, -1.0], dtype=F64))
    zero = T.clone()
    zero[:3, :3] = 0.0
    proj = T.clone()
    proj[3, 0] = 0.1
    nan = T.clone()
    nan[0, 3] = float("nan")
    for name, bad in (("shear", shear), ("squash", squash), ("mirror", mirror), ("zero", zero), ("projective", proj), ("nan", nan),
                      ("s = 0", (0.0, R, torch.zeros(3))), ("s < 0", (-1.0, R, torch.zeros(3))),
                      ("tuple mirror", (1.0, -R, torch.zeros(3))), ("tuple shear", (1.0, shear[:3, :3] / 1.5, torch.zeros(3))),
                      ("numpy shear", shear.numpy())):
        with pytest.raises(ValueError, match="similarity|scale|last row|finite"):
            transform_gaussians(None, bad, means=x)
    # a good host transform gets past the check and stops at the CPU tensor instead
    with pytest.raises(ValueError, match="HIP device"):
        transform_gaussians(None, T, means=x)
    with pytest.raises(ValueError, match="HIP device"):
        transform_gaussians(None, T.float(), means=x)                        # fp32 entries pass the orthogonality tolerance
    with pytest.raises(ValueError, match="transform"):
        transform_gaussians(None, None, means=x)


def test_the_adapter_without_coords_no_longer_refuses():
    """fusion=False, coords=None used to end in NotImplementedError.  On the host: the view table the path builds has one
    rotation per camera and one id per Gaussian, and the call now gets as far as the device check (values: the GPU tests)."""
    from freesplat_amd.gaussian_adapter import GaussianAdapter, GaussianAdapterCfg
    b, v, h, w = 2, 3, 4, 5
    ad = GaussianAdapter(GaussianAdapterCfg(0.5, 15.0, 2))
    g = torch.Generator().manual_seed(60)
    E = torch.eye(4).repeat(b, v, 1, 1)
    for i in range(b):
        for j in range(v):
            E[i, j, :3, :3] = _rot(61 + 3 * i + j).float()
    lead = (b, v, h * w, 1, 1)
    M = b * v * h * w
    rot, ids = GaussianAdapter._view_rotations(E[:, :, None, None, None], lead, M)
    assert tuple(rot.shape) == (b * v, 3, 3) and torch.equal(rot, E.reshape(-1, 4, 4)[:, :3, :3])
    assert ids.dtype == torch.int64 and torch.equal(ids, torch.arange(b * v).repeat_interleave(h * w))
    rot, ids = GaussianAdapter._view_rotations(E[0, 0], lead, M)             # one camera for everything
    assert tuple(rot.shape) == (1, 3, 3) and not bool(ids.any())
    per = torch.eye(4).expand(*lead, 4, 4)                                   # no broadcast structure: a row per Gaussian
    rot, ids = GaussianAdapter._view_rotations(per, lead, M)
    assert tuple(rot.shape) == (M, 3, 3) and torch.equal(ids, torch.arange(M))
    K = torch.tensor([[0.9, 0, 0.5], [0, 1.2, 0.5], [0, 0, 1]]).expand(b, v, 1, 1, 1, 3, 3)
    try:
        ad(E[:, :, None, None, None], K, None, 1 + torch.rand(lead, generator=g), torch.rand(lead, generator=g),
           torch.randn(*lead, ad.d_in, generator=g), (h, w), fusion=False, coords=None)
    except NotImplementedError:
        pytest.fail("GaussianAdapter.forward(fusion=False, coords=None) still raises NotImplementedError")
    except RuntimeError as e:
        assert "HIP device" in str(e)                                        # CPU tensors: there is no CPU path
