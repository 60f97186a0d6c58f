"""Host checks of the pose and transform gradients (no GPU): the SH generators of the library against the float64 restatement
(tests/pose_ref.py), the camera identity through the dense float64 renderer with negative controls, the transform's ambient
gradient against central differences of tests/transform_ref.py, sim3_exp and Poses, and the C boundary of
include/freesplat_amd_pose.h without a device.  Every case prints its worst error / bound ratio."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import pose_ref as PR
import transform_cases as TC
import transform_ref as TR
from oracle.raster_dense_torch import render_dense
from util_abi import declared_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = ["fs_pose_api_version", "fs_sim3_tangent_scratch_bytes", "fs_sim3_sh_generators", "fs_sim3_tangent"]
F64 = torch.float64


def _lib():
    from freesplat_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        L.build()
    return L


# ---- 1. the generators --------------------------------------------------------------------------------------------------------

def test_the_library_generators_match_the_restatement():
    """fs_sim3_sh_generators against autograd of the restatement's D_l(exp([omega]x)) at 0: entrywise within 1e-12, antisymmetric
    to 1e-15, exactly zero where the restatement is below 1e-14; and G_{l,k} b_l(d) = grad b_l(d) . (e_k x d) on fresh directions."""
    L = _lib()
    buf = (C.c_double * (3 * 83))()
    assert L.lib().fs_sim3_sh_generators(buf) == 0
    got = torch.tensor(list(buf), dtype=F64).reshape(3, 83)
    want = PR.generator_table()
    err = float((got - want).abs().max())
    small = want.abs() < 1e-14
    print(f"generators: worst error / bound {err / 1e-12:.3e}; {int((~small).sum())} nonzero entries")
    assert err <= 1e-12
    assert not bool(got[small].any()) and int((~small).sum()) == 48
    for k in range(3):
        for l, off in ((1, 0), (2, 9), (3, 34)):
            n = 2 * l + 1
            G = got[k, off:off + n * n].reshape(n, n)
            assert float((G + G.T).abs().max()) <= 1e-15, (k, l)
            d = torch.randn(50, 3, dtype=F64, generator=torch.Generator().manual_seed(7 + l)).requires_grad_(True)
            b = TR.band(l, d)
            e = torch.eye(3, dtype=F64)[k].expand(50, 3)
            jvp = torch.stack([torch.autograd.grad(b[:, i].sum(), d, retain_graph=True)[0] for i in range(n)], 1)     # [50, n, 3]
            lhs = torch.einsum("nic,nc->ni", jvp, torch.linalg.cross(e, d.detach()))
            assert float((lhs - b.detach() @ G.T).abs().max()) <= 1e-12, (k, l)


# ---- 2. the camera identity ---------------------------------------------------------------------------------------------------

def _discrete(sc, H, W):
    from freesplat_amd.rasterizer import build_cov3d
    from oracle import raster_oracle as ro
    view, proj, campos, tx, ty = TC.camera_matrices(sc["c2w"], sc["near"], sc["far"])
    n = lambda t: t.float().numpy()
    st = ro.forward(H, W, tx, ty, np.zeros(3, np.float32), n(view), n(proj), sc["sh_degree"], n(campos), n(sc["means"]),
                    n(build_cov3d(sc["scales"], sc["rotations"], 1.0)), n(sc["opacities"]), shs=n(sc["shs"]))
    order = torch.from_numpy(np.lexsort((np.arange(st["N"]), st["depths"].view(np.uint32))).astype(np.int64))
    return dict(rect=torch.from_numpy(st["rect"]), radii=torch.from_numpy(st["radii"]), order=order)


def _loss(sc, E, a, weights, discrete, H, W):
    from freesplat_amd.rasterizer import build_cov3d
    view, proj, campos, tx, ty = TC.camera_matrices(E, sc["near"], sc["far"])
    color, depth, _ = render_dense(H, W, tx, ty, torch.tensor([0.2, 0.3, 0.1], dtype=F64), view, proj, sc["sh_degree"], campos,
                                   a["means"], build_cov3d(a["scales"], a["rotations"], 1.0), sc["opacities"], shs=a["shs"], **discrete)
    return (weights[0] * color).sum() + (weights[1] * depth).sum() / float(sc["far"])


def _chain_camera(G, E):
    """<G, E hat(e_k)> for the six rigid tangent directions."""
    return torch.stack([(G * (E @ PR.hat(torch.eye(7, dtype=F64)[k]))).sum() for k in range(6)])


@pytest.mark.parametrize("depth", [1000.0, 4.0])
def test_the_camera_gradient_is_the_pulled_back_tangent_of_the_gaussian_gradients(depth):
    """24 x 32, 100 Gaussians, degree 3, unnormalised quaternions, random weights on colour and depth, the discrete inputs of
    the C oracle: camera_ambient of the restatement's reduction of the Gaussian gradients, chained to eps in E Exp(eps), against
    torch.autograd of render_dense with respect to eps.  Relative error <= 1e-10; leaving out the SH term, leaving out the
    quaternion term and flipping the sign each move the result by more than 1e-2."""
    from freesplat_amd.pose import camera_ambient
    H, W = 24, 32
    sc = TC.invariance_scene(depth=depth)
    discrete = _discrete(sc, H, W)
    assert int((discrete["radii"] > 0).sum()) >= 90
    g = torch.Generator().manual_seed(90)
    weights = (torch.randn(3, H, W, dtype=F64, generator=g), torch.randn(H, W, dtype=F64, generator=g))
    a = {k: sc[k].clone().requires_grad_(True) for k in ("means", "scales", "rotations", "shs")}
    eps = torch.zeros(6, dtype=F64, requires_grad=True)
    E = sc["c2w"] @ torch.linalg.matrix_exp(PR.hat(torch.cat([eps, torch.zeros(1, dtype=F64)])))
    loss = _loss(sc, E, a, weights, discrete, H, W)
    want, *grads = torch.autograd.grad(loss, [eps] + [a[k] for k in ("means", "scales", "rotations", "shs")])
    grads = dict(zip(("means", "scales", "rotations", "shs"), grads))
    assert float(want.abs().min()) > 0
    vals = {k: v.detach() for k, v in a.items()}
    scale = float(want.norm())

    def chained(which, sign=1.0):
        tau, _ = PR.tangent(1, None, {k: vals[k] for k in which}, {k: grads[k] for k in which})
        return _chain_camera(camera_ambient(sc["c2w"], sign * tau[0]), sc["c2w"])

    err = float((chained(("means", "scales", "rotations", "shs")) - want).norm()) / scale
    print(f"depth {depth}: relative error {err:.3e}, error / bound {err / 1e-10:.3e}")
    assert err <= 1e-10
    for name, got in (("no SH term", chained(("means", "scales", "rotations"))), ("no quaternion term", chained(("means", "scales", "shs"))),
                      ("sign flipped", chained(("means", "scales", "rotations", "shs"), -1.0))):
        moved = float((got - want).norm()) / scale
        print(f"  control {name}: {moved:.3e}")
        assert moved > 1e-2, name


# ---- 3. the transform's gradient ----------------------------------------------------------------------------------------------

def _transform_case(V):
    N, M = 37, 16
    g = torch.Generator().manual_seed(17 + V)
    a = {k: v.double() for k, v in TC.arrays(N, M, 5 + V, False, "coeff_major").items()}
    cot = {k: torch.randn(v.shape, dtype=F64, generator=g) for k, v in a.items()}
    T0 = torch.eye(4, dtype=F64).repeat(V, 1, 1)
    for v in range(V):
        T0[v, :3, :3] = (1.7 if v == 0 else 0.6 + 0.5 * v) * TR.random_rotation(g)
        T0[v, :3, 3] = torch.randn(3, dtype=F64, generator=g)
    ids = None
    if V > 1:
        ids = torch.randint(0, V, (N,), generator=g)
        ids[1], ids[N - 2], ids[N // 2] = -1, V, -1
    return a, cot, T0, ids


def _transform_loss(T, ids, a, cot):
    out = TR.transform(T[:, :3], ids, a["means"], a["scales"], a["rotations"], a["cov"], a["shs"], "wxyz", "coeff_major")
    return sum((o * cot[k]).sum() for o, k in zip(out, PR.ARRAYS))


@pytest.mark.parametrize("V", [1, 3])
def test_the_transform_gradient_matches_central_differences(V):
    """N = 37, M = 16, all five arrays, s = 1.7 (V = 3: three transforms, ids with -1 and V): transform_ambient of the
    restatement's reduction over the inputs and the input gradients, chained through T0 sim3_exp(xi), against central differences
    of transform_ref.transform at h = 1e-5, relative error <= 1e-8; the matrix and the (s, R) form of transform_ambient agree, and
    chained through xf = (s R | t) by autograd they give tau_sigma / s, s G_A and G_t."""
    from freesplat_amd.pose import sim3_exp, transform_ambient
    a, cot, T0, ids = _transform_case(V)
    leaves = {k: v.clone().requires_grad_(True) for k, v in a.items()}
    g_in = dict(zip(PR.ARRAYS, torch.autograd.grad(_transform_loss(T0, ids, leaves, cot), [leaves[k] for k in PR.ARRAYS])))
    tau, _ = PR.tangent(V, ids, a, g_in)
    h, fd = 1e-5, torch.zeros(V, 7, dtype=F64)
    for v in range(V):
        for e in range(7):
            xi = torch.zeros(V, 7, dtype=F64)
            xi[v, e] = h
            fd[v, e] = (_transform_loss(T0 @ sim3_exp(xi), ids, a, cot) - _transform_loss(T0 @ sim3_exp(-xi), ids, a, cot)) / (2 * h)
    s, R, t = TR.split_xf(T0[:, :3])
    G = transform_ambient(T0, tau)
    assert tuple(G.shape) == (V, 3, 4)
    assert float((G - transform_ambient((s, R), tau)).abs().max()) <= 1e-12 * float(G.abs().max())
    chained = torch.stack([torch.stack([(G[v] * (T0[v] @ PR.hat(torch.eye(7, dtype=F64)[e]))[:3]).sum() for e in range(7)]) for v in range(V)])
    scale = fd.norm(dim=1, keepdim=True)
    err_tau = float(((chained - tau).norm(dim=1, keepdim=True) / scale).max())
    err = float(((chained - fd).norm(dim=1, keepdim=True) / scale).max())
    print(f"V = {V}: chained ambient against tau {err_tau:.3e}, against central differences {err:.3e}; error / bound {err / 1e-8:.3e}")
    assert err_tau <= 1e-13 and err <= 1e-8
    # the tuple form: xf built from (s, R, t) by torch operations
    s_, R_, t_ = (x.clone().requires_grad_(True) for x in (s, R, t))
    xf = torch.cat([s_[:, None, None] * R_, t_[:, :, None]], 2)
    gs, gR, gt = torch.autograd.grad((G * xf).sum(), [s_, R_, t_])
    assert float((gs - tau[:, 6] / s).abs().max()) <= 1e-12 * float(gs.abs().max())
    assert float((gR - s[:, None, None] * G[:, :, :3]).abs().max()) <= 1e-12 * float(gR.abs().max())
    assert torch.equal(gt, G[:, :, 3])


# ---- 4. sim3_exp and Poses ----------------------------------------------------------------------------------------------------

def test_sim3_exp_and_poses():
    """sim3_exp against [[e^sigma Rodrigues(omega), V u], [0, 1]] with V summed as a power series; the six-number form is the
    seven-number one at sigma = 0; Poses.matrices() before and after fold_() within 1e-12, with a base that stays rigid."""
    from freesplat_amd.pose import Poses, sim3_exp, sim3_hat
    g = torch.Generator().manual_seed(23)
    xi = torch.randn(5, 7, dtype=F64, generator=g) * torch.tensor([2.0, 2, 2, 0.7, 0.7, 0.7, 0.3], dtype=F64)
    T = sim3_exp(xi)
    for k in range(5):
        w, th = xi[k, 3:6], float(xi[k, 3:6].norm())
        K = PR.skew(w / th)
        Rod = torch.eye(3, dtype=F64) + math.sin(th) * K + (1 - math.cos(th)) * K @ K
        A = xi[k, 6] * torch.eye(3, dtype=F64) + PR.skew(w)
        Vm, term = torch.zeros(3, 3, dtype=F64), torch.eye(3, dtype=F64)
        for j in range(40):
            Vm = Vm + term                                                   # term = A^j / (j + 1)!
            term = term @ A / (j + 2)
        want = torch.eye(4, dtype=F64)
        want[:3, :3], want[:3, 3] = math.exp(float(xi[k, 6])) * Rod, Vm @ xi[k, :3]
        assert float((T[k] - want).abs().max()) <= 1e-12
        assert float((sim3_hat(xi[k]) - PR.hat(xi[k])).abs().max()) == 0.0
    six = xi[:, :6]
    assert float((sim3_exp(six) - sim3_exp(torch.cat([six, torch.zeros(5, 1, dtype=F64)], 1))).abs().max()) <= 1e-15
    with pytest.raises(ValueError):
        sim3_hat(torch.zeros(5))
    base = torch.eye(4, dtype=F64).repeat(4, 1, 1)
    for v in range(4):
        base[v, :3, :3], base[v, :3, 3] = TR.random_rotation(g), 3.0 * torch.randn(3, dtype=F64, generator=g)
    poses = Poses(base)
    assert tuple(poses.delta.shape) == (4, 6) and not bool(poses.delta.any()) and torch.equal(poses.matrices(), base)
    with torch.no_grad():
        poses.delta.copy_(0.1 * torch.randn(4, 6, dtype=F64, generator=g))
    before = poses.matrices().detach()
    assert float((before - base).abs().max()) > 1e-2
    assert torch.equal(poses.matrices([2, 0]), before[[2, 0]])
    poses.fold_()
    after = poses.matrices().detach()
    err = float((after - before).abs().max())
    print(f"fold_: {err:.3e}, error / bound {err / 1e-12:.3e}")
    assert err <= 1e-12 and not bool(poses.delta.any()) and torch.equal(after, poses.base)
    Rb = poses.base[:, :3, :3]
    assert float((Rb.transpose(1, 2) @ Rb - torch.eye(3, dtype=F64)).abs().max()) <= 1e-15
    assert bool((torch.linalg.det(Rb) > 0).all()) and torch.equal(poses.base[:, 3], torch.tensor([0.0, 0, 0, 1], dtype=F64).expand(4, 4))
    assert tuple(Poses(base, scale=True).delta.shape) == (4, 7)
    loss = (poses.matrices() * torch.randn(4, 4, 4, dtype=F64, generator=g)).sum()        # delta is trainable
    loss.backward()
    assert poses.delta.grad is not None and float(poses.delta.grad.abs().min()) > 0


# ---- 5. the C boundary --------------------------------------------------------------------------------------------------------

def test_pose_header_is_exported_and_bound():
    L_ = _lib()
    L = C.CDLL(L_.LIB_PATH)
    names = declared_names("freesplat_amd_pose.h")
    assert names == sorted(EXPECTED)
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/freesplat_amd_pose.h but not exported"
    assert set(L_.POSE_SIGNATURES) == set(names)
    assert L_.lib().fs_pose_api_version() == 1 == L_.POSE_API_VERSION
    text = open(os.path.join(ROOT, "include", "freesplat_amd_pose.h")).read()
    for name, value in (("POSE_API_VERSION", 1), ("SIM3_MAX_ROWS", 64), ("SIM3_TANGENT_DIM", 7), ("SIM3_SH_GENERATOR_DOUBLES", 83)):
        assert re.search(rf"#define\s+FS_{name}\s+{value}\b", text), name
    assert (L_.SIM3_MAX_ROWS, L_.SIM3_TANGENT_DIM, L_.SIM3_SH_GENERATOR_DOUBLES) == (64, 7, 83)


P = C.c_void_p(4096)      # a fake non-NULL pointer: nothing may launch with it
BIG = 1 << 30


def _tangent(L, N=8, M=16, V=1, flags=0, ids=None, values=(P,) * 5, grads=(P,) * 5, out=P, scratch=P, nbytes=BIG):
    return L.fs_sim3_tangent(N, M, V, flags, ids, *values, *grads, out, scratch, nbytes, None)


def test_entry_points_validate_before_touching_a_device():
    """FS_ERR_INVALID_ARG (-1), with fake non-NULL pointers wherever a pointer is given, so nothing may launch: sizes <= 0, M
    outside {1, 4, 9, 16}, V = 0 and V = 65, ids NULL with V != 1, unknown flag bits (the transpose bit among them), values
    without their gradient, a gradient other than that of the means without its values, no gradient at all, out or scratch NULL,
    a scratch that is too small; the size query answers 0 for invalid sizes."""
    L = _lib().lib()
    for name, (rt, at) in _lib().POSE_SIGNATURES.items():
        if rt is not C.c_int or not at:
            continue
        for size in (1, 16):
            assert getattr(L, name)(*[size if a in (C.c_int32, C.c_size_t) else None for a in at]) == -1, name
        if name == "fs_sim3_tangent":
            assert getattr(L, name)(*[0 if a in (C.c_int32, C.c_size_t) else P for a in at]) == -1, name
    assert L.fs_sim3_sh_generators(None) == -1
    for bad in (dict(N=0), dict(N=-5), dict(M=0), dict(M=2), dict(M=15), dict(M=17), dict(V=0), dict(V=-1), dict(V=65, ids=P),
                dict(V=2), dict(flags=2), dict(flags=16), dict(flags=-1), dict(out=None), dict(scratch=None), dict(nbytes=0),
                dict(nbytes=7 * 8 - 1), dict(grads=(None,) * 5), dict(values=(None,) * 5, grads=(None,) * 5)):
        assert _tangent(L, **bad) == -1, bad
    for i in range(5):
        only = tuple(P if k == i else None for k in range(5))
        without = tuple(None if k == i else P for k in range(5))
        assert _tangent(L, values=(P,) * 5, grads=without) == -1, ("values without their gradient", i)
        assert _tangent(L, values=only, grads=(None,) * 5) == -1, ("values alone", i)
        if i:
            assert _tangent(L, values=without, grads=(P,) * 5) == -1, ("a gradient without its values", i)
    assert L.fs_sim3_tangent_scratch_bytes(0, 1) == 0 and L.fs_sim3_tangent_scratch_bytes(8, 0) == 0
    assert L.fs_sim3_tangent_scratch_bytes(8, 65) == 0 and L.fs_sim3_tangent_scratch_bytes(-1, 1) == 0
    assert L.fs_sim3_tangent_scratch_bytes(1024, 1) == 56 and L.fs_sim3_tangent_scratch_bytes(1025, 3) == 3 * 2 * 56


def test_the_python_layer_rejects_bad_arguments_without_a_device():
    from freesplat_amd.pose import camera_ambient, observe, sim3_tangent, transform_ambient
    x = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="HIP device"):
        sim3_tangent(means=x, grads=dict(means=x))
    with pytest.raises(ValueError, match="no gradients"):
        sim3_tangent(means=x)
    with pytest.raises(ValueError, match="needs scales"):
        sim3_tangent(grads=dict(scales=x))
    with pytest.raises(ValueError, match="grads may hold"):
        sim3_tangent(means=x, grads=dict(opacities=x))
    with pytest.raises(ValueError, match="HIP device"):
        observe(torch.eye(4), means=x)
    with pytest.raises(ValueError, match=r"\[4, 4\]"):
        camera_ambient(torch.eye(3), torch.zeros(7))
    with pytest.raises(ValueError, match="tau"):
        camera_ambient(torch.eye(4), torch.zeros(6))
    with pytest.raises(ValueError, match="transform"):
        transform_ambient(torch.zeros(5, 5), torch.zeros(7))
