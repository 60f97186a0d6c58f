"""CPU checks of the fused Gaussian Adam step: the float64 restatement (tests/gaussian_adam_ref.py) against torch.optim.Adam
itself, and the C boundary of include/freesplat_amd_optim.h (exports, binding table, revision, argument validation with
fake pointers -- nothing may launch).  No GPU."""
import ctypes as C
import os
import re

import pytest
import torch

import gaussian_adam_ref as R
from util_abi import declared_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("N,M", [(65, 4), (7, 1), (33, 16)])
def test_restatement_equals_torch_adam_in_float64(N, M):
    """All rows visible: six parameter groups of torch.optim.Adam, autograd through exp / sigmoid, 5 steps, to 1e-12."""
    raw, grads = R.make_inputs(N, M, K=5, seed=1)
    ref = R.RefAdam(raw)
    leaves = [t.double().clone().requires_grad_(True) for t in (raw[0], raw[1], raw[2], raw[3], raw[4][:, :1], raw[4][:, 1:])]
    names = ("means", "scales", "rotations", "opacity", "sh_dc", "sh_rest")
    live = [(p, n) for p, n in zip(leaves, names) if p.numel()]            # M = 1: no sh_rest parameters
    opt = torch.optim.Adam([dict(params=[p], lr=R.DEFAULT_LR[n]) for p, n in live], betas=(0.9, 0.999), eps=1e-15)
    for g in grads:
        ref.step(g)
        opt.zero_grad()
        acts = (leaves[0], torch.exp(leaves[1]), leaves[2], torch.sigmoid(leaves[3]), torch.cat([leaves[4], leaves[5]], 1))
        sum((a * w.double()).sum() for a, w in zip(acts, g)).backward()
        opt.step()
    want = [leaves[0], leaves[1], leaves[2], leaves[3], torch.cat([leaves[4], leaves[5]], 1)]
    moments = {key: [opt.state[p][key] if p.numel() else p.detach() for p in leaves] for key in ("exp_avg", "exp_avg_sq")}
    for k in range(5):
        assert R.err(ref.p[k], want[k]) <= 1e-12, R.ARRAYS[k]
    for got, key in ((ref.m, "exp_avg"), (ref.v, "exp_avg_sq")):
        mo = moments[key]
        for k, w in enumerate(mo[:4] + [torch.cat(mo[4:], 1)]):
            assert R.err(got[k], w) <= 1e-12 * max(1.0, float(w.abs().max())), (key, R.ARRAYS[k])
    assert ref.t == 5


def test_restatement_visibility_and_missing_gradients():
    """A row that is not visible keeps p, m, v (NaN gradients there reach nothing) while t advances; visible rows follow the
    dense formulas with that global t; an array without a gradient is left alone."""
    N, M = 37, 4
    raw, grads = R.make_inputs(N, M, K=2, seed=2)
    vis = R.radii_pattern(N, 0)
    assert bool((vis > 0).any()) and bool((vis == 0).any()) and bool((vis < 0).any())
    dense, sparse = R.RefAdam(raw), R.RefAdam(raw)
    poisoned = [torch.where((vis > 0).reshape((-1,) + (1,) * (g.dim() - 1)), g, torch.full_like(g, float("nan"))) for g in grads[0]]
    dense.step(grads[0])
    sparse.step(poisoned, vis)
    on = vis > 0
    for k in range(5):
        for a, b, start in ((sparse.p, dense.p, raw[k].double()), (sparse.m, dense.m, 0.0), (sparse.v, dense.v, 0.0)):
            assert torch.equal(a[k][on], b[k][on]) and bool(torch.isfinite(a[k]).all())
            assert bool((a[k][~on] == start[~on] if isinstance(start, torch.Tensor) else a[k][~on] == 0.0).all())
    # second step, everything visible: rows skipped in step 1 take their FIRST update with t = 2
    sparse.step(grads[1], torch.ones(N, dtype=torch.int32))
    assert sparse.t == 2
    k, row = R.MEANS, int((~on).nonzero()[0])
    g = grads[1][k][row].double()
    m, v = 0.1 * g, 0.001 * g * g
    want = raw[k][row].double() - R.DEFAULT_LR["means"] / (1 - 0.9 ** 2) * (m / (v.sqrt() / (1 - 0.999 ** 2) ** 0.5 + 1e-15))
    assert float((sparse.p[k][row] - want).abs().max()) <= 1e-14
    skip = R.RefAdam(raw)
    skip.step([grads[0][0], None, grads[0][2], None, None])
    for k in (1, 3, 4):
        assert torch.equal(skip.p[k], raw[k].double()) and not bool(skip.m[k].any()) and not bool(skip.v[k].any())
    for k in (0, 2):
        assert torch.equal(skip.p[k], dense.p[k])


def test_optim_header_is_exported_and_bound():
    from freesplat_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    names = declared_names("freesplat_amd_optim.h")
    assert names == ["fs_gaussian_activate", "fs_gaussian_adam_step", "fs_optim_api_version"]
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/freesplat_amd_optim.h but not exported"
        assert n in _lib.OPTIM_SIGNATURES, f"{n} has no ctypes signature in freesplat_amd/_lib.py"
    assert set(_lib.OPTIM_SIGNATURES) == set(names)
    assert _lib.lib().fs_optim_api_version() == 1 == _lib.OPTIM_API_VERSION
    text = open(os.path.join(ROOT, "include", "freesplat_amd_optim.h")).read()
    assert re.search(r"#define\s+FS_OPTIM_API_VERSION\s+1\b", text)
    from freesplat_amd import refine
    for k, name in enumerate(("MEANS", "SCALES", "ROTATIONS", "OPACITIES", "SH_DC", "SH_REST")):
        assert re.search(r"#define\s+FS_OPTIM_LR_%s\s+%d\b" % (name, k), text)
    assert refine.GROUPS == R.GROUPS and refine.DEFAULT_LR == R.DEFAULT_LR


def _step_call(L, N=8, M=4, p=None, g=None, m=None, v=None, visible=None, lr=4096, step=4096, beta1=0.9, beta2=0.999,
               eps=1e-15, out_scales=4096, out_opacities=4096):
    """fs_gaussian_adam_step with fake non-NULL pointers (4096) wherever an argument is not given."""
    table = lambda t: None if t == "null" else (C.c_void_p * 5)(*(t if t is not None else [4096] * 5))
    vp = lambda x: None if x is None else C.c_void_p(x)
    return L.fs_gaussian_adam_step(N, M, table(p), table(g), table(m), table(v), vp(visible), vp(lr), vp(step), beta1, beta2, eps,
                                   vp(out_scales), vp(out_opacities), None)


def test_entry_points_validate_before_touching_a_device():
    from freesplat_amd import _lib
    L = _lib.lib()
    assert _step_call(L, N=0) == 0                                        # an empty job: nothing launched
    assert _step_call(L, N=0, g=[None] * 5) == 0 and _step_call(L, N=0, p="null", lr=None) == 0
    assert _step_call(L, N=-1) == -1
    for M in (0, 2, 3, 5, 8, 15, 17, 25, -1):
        assert _step_call(L, M=M) == -1, M
    for kw in (dict(beta1=1.0), dict(beta2=1.0), dict(beta1=-0.1), dict(beta2=1.5), dict(eps=-1e-8), dict(beta1=float("nan")),
               dict(eps=float("nan"))):
        assert _step_call(L, **kw) == -1, kw
    # each required pointer NULL in turn: the four tables, every p / exp_avg / exp_avg_sq entry, lr, step, the two outputs
    for name in ("p", "g", "m", "v"):
        assert _step_call(L, **{name: "null"}) == -1, name
    for name in ("p", "m", "v"):
        for k in range(5):
            assert _step_call(L, **{name: [None if i == k else 4096 for i in range(5)]}) == -1, (name, k)
    for name in ("lr", "step", "out_scales", "out_opacities"):
        assert _step_call(L, **{name: None}) == -1, name
    assert _step_call(L, g=[None] * 5) == -1                             # no gradient at all
    # 32-bit element indices: 3 M N must stay below 2^31
    assert _step_call(L, N=(2 ** 31) // 48 + 1, M=16) == -1 and _step_call(L, N=2 ** 31 - 1, M=1) == -1
    # fs_gaussian_activate
    p = C.c_void_p(4096)
    assert L.fs_gaussian_activate(0, p, p, p, p, None) == 0 and L.fs_gaussian_activate(0, None, None, None, None, None) == 0
    assert L.fs_gaussian_activate(-1, p, p, p, p, None) == -1
    for k in range(4):
        assert L.fs_gaussian_activate(8, *[None if i == k else p for i in range(4)], None) == -1, k


def test_python_layer_refuses_what_it_cannot_run():
    """The error cases that need no device: CPU tensors."""
    from freesplat_amd.refine import GaussianAdam
    N = 4
    args = [torch.rand(N, 3), torch.rand(N, 3) + 0.1, torch.randn(N, 4), torch.rand(N) * 0.5 + 0.2, torch.randn(N, 4, 3)]
    with pytest.raises(ValueError, match="HIP device"):
        GaussianAdam(*args)
    with pytest.raises(ValueError, match="HIP device"):
        GaussianAdam(*args, sparse=True)
