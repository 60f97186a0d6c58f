"""Deterministic backwards of the cost volume, the PTF fold and the depth tail (ABI 9: fs_cost_volume_backward_det,
fs_ptf_*_backward_det, fs_depth_tail_backward_det).  CPU: the boundary (revision, symbols, size queries, argument checks).
GPU: bitwise repeatability, independence of the batch and the environment, agreement with the default mode and the oracle."""
import ctypes as C
import os
import re
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))

NEW = ("fs_cost_volume_backward_det_bytes", "fs_cost_volume_backward_det", "fs_ptf_backward_det_bytes",
       "fs_ptf_write_state_backward_det", "fs_ptf_gru_inputs_backward_det", "fs_depth_tail_backward_det")


# ---------------------------------------------------------------- CPU: the boundary

def test_abi_revision_9_declares_exports_and_binds_the_det_entry_points():
    from freesplat_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION == 9 and L.fs_abi_version() == 9
    header = open(os.path.join(ROOT, "include", "freesplat_amd.h")).read()
    assert re.search(r"#define FS_ABI_VERSION 9\b", header)
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name) is not None


def test_det_size_queries():
    from freesplat_amd import _lib
    L = _lib.lib()
    q = L.fs_cost_volume_backward_det_bytes
    for bad in ((0, 2, 48, 24, 32, 64), (2, 0, 48, 24, 32, 64), (2, 2, 32, 24, 32, 64), (2, 2, 48, 0, 32, 64),
                (2, 2, 48, 24, 0, 64), (2, 2, 48, 24, 32, 0), (2, 17, 48, 24, 32, 64), (-1, 2, 48, 24, 32, 64)):
        assert q(*bad) == 0, bad
    base = q(2, 2, 48, 24, 32, 64)
    assert base > 0 and base % 256 == 0
    assert q(3, 2, 48, 24, 32, 64) > base                  # B
    assert q(2, 2, 48, 24, 32, 128) > base                 # D (more plane slices and chunks at this small size)
    assert q(2, 2, 48, 24, 32, 128) >= q(2, 2, 48, 24, 32, 64) >= q(2, 2, 48, 24, 32, 8)
    assert q(2, 2, 16, 24, 32, 64) < base                  # C
    p = L.fs_ptf_backward_det_bytes
    assert p(-1, 100) == 0 and p(10, 0) == 0 and p(10, -5) == 0
    assert 0 < p(0, 100) < p(10, 100) < p(1000, 100)       # n_fuse
    assert p(10, 100) < p(10, 10000)


def test_existing_size_queries_unchanged():
    """Values of the parent revision: the deterministic form adds its own query and leaves these alone."""
    from freesplat_amd import _lib
    L = _lib.lib()
    want = {(3, 2, 48, 242, 324, 128): (6292740608, 270978560), (10, 8, 48, 96, 128, 128): (3570773760, 424677120),
            (2, 2, 16, 13, 21, 8): (525824, 209920)}
    for a, (full, scatter) in want.items():
        assert L.fs_cost_volume_backward_workspace_bytes(*a) == full
        assert L.fs_cost_volume_backward_workspace_bytes_for(*a, 0) == full
        assert L.fs_cost_volume_backward_workspace_bytes_for(*a, 1) == scatter
    assert L.fs_ptf_fold_scratch_bytes(5000, 48, 64) == 3124224
    # the PTF fold's four queries over M x (h, w), V x (h, w) and n_fuse x P, recorded before their layouts became named structs
    match = {(0, 7, 9): 1536, (0, 48, 64): 16384, (1, 7, 9): 1536, (1, 48, 64): 16384, (1000, 7, 9): 9984,
             (1000, 48, 64): 24832, (5000, 7, 9): 46336, (5000, 48, 64): 61184}
    step = {(0, 7, 9): 3840, (0, 48, 64): 42752, (1, 7, 9): 3840, (1, 48, 64): 42752, (1000, 7, 9): 80384,
            (1000, 48, 64): 1033984, (5000, 7, 9): 148736, (5000, 48, 64): 3124224}
    fold = {(2, 7, 9): 68864, (2, 48, 64): 3287808, (3, 7, 9): 69888, (3, 48, 64): 3340032, (5, 7, 9): 72192,
            (5, 48, 64): 3444736}
    det = {(0, 63): 768, (0, 3072): 37120, (10, 63): 4096, (10, 3072): 40448, (3072, 63): 836352, (3072, 3072): 872704}
    for fn, table in ((L.fs_ptf_scratch_bytes, match), (L.fs_ptf_fold_scratch_bytes, step), (L.fs_ptf_fold_bytes, fold),
                      (L.fs_ptf_backward_det_bytes, det)):
        for a, want_bytes in table.items():
            assert fn(*a) == want_bytes, (a, want_bytes)


def _call(name, size, ptr=None, **over):
    from freesplat_amd import _lib
    _, at = _lib.SIGNATURES[name]
    args = [size if a in (C.c_int32, C.c_int64, C.c_int) else ptr for a in at]
    for i, v in over.items():
        args[int(i[1:])] = v
    return getattr(_lib.lib(), name)(*args)


def test_det_entry_points_validate_before_touching_a_device():
    for name in ("fs_cost_volume_backward_det", "fs_ptf_write_state_backward_det", "fs_ptf_gru_inputs_backward_det",
                 "fs_depth_tail_backward_det"):
        assert _call(name, 0) in (0, -1), name
        assert _call(name, 1) == -1, name
    # non-NULL dummy pointers (never dereferenced): K = 17 and per-pixel planes are FS_ERR_UNSUPPORTED, nothing launched
    dummy = C.c_void_p(0x1000)
    args = dict(a0=2, a1=2, a2=48, a3=24, a4=32, a5=64, a12=0, a13=1, a14=0)
    assert _call("fs_cost_volume_backward_det", 1, dummy, **{**args, "a1": 17}) == -3
    assert _call("fs_cost_volume_backward_det", 1, dummy, **{**args, "a14": 1}) == -3
    assert _call("fs_cost_volume_backward_det", 1, dummy, **{**args, "a2": 32}) == -3
    # ... and a missing det scratch is an argument error
    assert _call("fs_cost_volume_backward_det", 1, dummy, **{**args, "a31": None}) == -1


# ---------------------------------------------------------------- GPU helpers

def _det(on):
    from freesplat_amd import rasterizer as R
    R.DETERMINISTIC = bool(on)


@pytest.fixture(autouse=True)
def _restore_mode():
    from freesplat_amd import rasterizer as R
    saved = R.DETERMINISTIC
    yield
    R.DETERMINISTIC = saved
    torch.use_deterministic_algorithms(False)


def _cv_case(B, K, C_, h, w, D, seed):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import inputs
    kw = inputs.cv_inputs(max(B, K + 1), K, h, w, C_, seed=seed)
    for k in ("cur_feats", "src_feats", "src_extrinsics", "src_poses", "src_Ks", "cur_invK"):
        kw[k] = kw[k][:B].contiguous()
    return kw


def _cv_run(kw, C_, D, dev, rows=None, seed=0):
    """One forward + backward of the HIP cost volume on views `rows`; returns {name: gradient}."""
    from freesplat_amd.cost_volume import AVGFeatureVolumeManager
    h, w = kw["cur_feats"].shape[-2:]
    torch.manual_seed(seed)
    m = AVGFeatureVolumeManager(matching_height=h, matching_width=w, num_depth_bins=D, mlp_channels=[202, 32, 32, 1],
                                matching_dim_size=C_).to(dev)
    sel = slice(None) if rows is None else rows
    a = {k: (v[sel] if torch.is_tensor(v) and v.dim() > 2 and k not in ("min_depth", "max_depth") else v).to(dev)
         for k, v in kw.items()}
    a["cur_feats"] = a["cur_feats"].clone().requires_grad_(True)
    a["src_feats"] = a["src_feats"].clone().requires_grad_(True)
    out = m(**a)
    B = kw["cur_feats"].shape[0]
    g = torch.randn((B,) + tuple(out.shape[1:]), generator=torch.Generator().manual_seed(seed + 7))[sel].to(dev)
    (out * g).sum().backward()
    torch.cuda.synchronize()
    net = m.mlp.net
    return {"cur": a["cur_feats"].grad.clone(), "src": a["src_feats"].grad.clone(), "w1": net[0].weight.grad.clone(),
            "b1": net[0].bias.grad.clone(), "w2": net[2].weight.grad.clone(), "b2": net[2].bias.grad.clone(),
            "w3": net[4].weight.grad.clone(), "b3": net[4].bias.grad.clone()}


def _bitwise(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def _close(a, b, rel):
    for k in a:
        s = float(b[k].abs().max()) + 1e-30
        e = (a[k] - b[k]).abs().flatten() / s
        q = float(e.kthvalue(max(1, int(0.995 * e.numel()))).values)
        assert q < rel and float(e.mean()) < rel / 5, (k, q, float(e.mean()))


CV_CASES = [(1, 1, 48, 24, 32, 128), (2, 2, 48, 24, 32, 128), (3, 8, 48, 20, 28, 128), (3, 2, 48, 61, 81, 128),
            (2, 2, 16, 13, 21, 8),
            (3, 2, 48, 242, 324, 128)]      # config-3 scale: one plane slice and one chunk (direct stores, weight rows only)


@pytest.mark.gpu
@pytest.mark.parametrize("save", ["1", "0"])          # the training forward's saved MLP inputs, or the recomputing backward
@pytest.mark.parametrize("B,K,C_,h,w,D", CV_CASES)
def test_cost_volume_det_repeatable_batch_independent_and_close_to_default(hip_device, monkeypatch, B, K, C_, h, w, D, save):
    monkeypatch.setenv("FREESPLAT_CV_SAVE", save)
    kw = _cv_case(B, K, C_, h, w, D, seed=B * 10 + K)
    _det(True)
    runs = [_cv_run(kw, C_, D, hip_device) for _ in range(3)]
    assert _bitwise(runs[0], runs[1]) and _bitwise(runs[0], runs[2]), "deterministic cost volume backward changed bits"
    # the environment's chunk / scatter switches are ignored
    for env in (("FS_CV_SG_CHUNKS", "1"), ("FS_CV_SG_CHUNKS", "4"), ("FS_CV_BWD_ATOMIC", "1")):
        monkeypatch.setenv(*env)
        r = _cv_run(kw, C_, D, hip_device)
        monkeypatch.delenv(env[0])
        assert _bitwise(runs[0], r), env
    # view 0 alone: the same bits as inside the batch; weight gradients = fp32 sum of the views', in view order
    if B > 1:
        one = [_cv_run(kw, C_, D, hip_device, rows=slice(v, v + 1)) for v in range(B)]
        assert torch.equal(one[0]["cur"][0], runs[0]["cur"][0]) and torch.equal(one[0]["src"][0], runs[0]["src"][0])
        for k in ("w1", "b1", "w2", "b2", "w3", "b3"):
            acc = one[0][k].clone()
            for v in range(1, B):
                acc = acc + one[v][k]
            assert torch.equal(acc, runs[0][k]), k
    # against the default (atomic) mode
    _det(False)
    ref = _cv_run(kw, C_, D, hip_device)
    _close(runs[0], ref, 1e-4)


@pytest.mark.gpu
def test_cost_volume_det_two_views_sum_exactly(hip_device):
    kw = _cv_case(2, 2, 48, 24, 32, 128, seed=5)
    _det(True)
    both = _cv_run(kw, 48, 128, hip_device)
    a, b = (_cv_run(kw, 48, 128, hip_device, rows=slice(v, v + 1)) for v in range(2))
    for k in ("w1", "b1", "w2", "b2", "w3", "b3"):
        assert torch.equal(both[k], a[k] + b[k]), k
    assert torch.equal(both["src"][1], b["src"][0]) and torch.equal(both["cur"][1], b["cur"][0])


@pytest.mark.gpu
def test_cost_volume_det_matches_the_oracle(hip_device):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import inputs
    from oracle import cost_volume_oracle as cvo
    from freesplat_amd.cost_volume import AVGFeatureVolumeManager
    h4, w4, D = 24, 32, 16
    torch.manual_seed(0)
    m = AVGFeatureVolumeManager(matching_height=h4, matching_width=w4, num_depth_bins=D, mlp_channels=[202, 32, 32, 1],
                                matching_dim_size=48)
    kw = inputs.cv_inputs(2, 1, h4, w4, 48, seed=1)
    sd = {k.replace(".", "__"): v for k, v in m.state_dict().items()}
    cur_c, src_c = kw["cur_feats"].clone().requires_grad_(True), kw["src_feats"].clone().requires_grad_(True)
    ref = cvo.cost_volume(cur_c, src_c, kw["src_extrinsics"], kw["src_Ks"], kw["cur_invK"], kw["min_depth"], kw["max_depth"],
                          D, cvo.mlp_from_state(sd))
    g = torch.randn(ref.shape, generator=torch.Generator().manual_seed(2))
    (ref * g).sum().backward()
    a = {k: v.to(hip_device) for k, v in kw.items()}
    a["cur_feats"].requires_grad_(True)
    a["src_feats"].requires_grad_(True)
    _det(True)
    out = m.to(hip_device)(**a)
    (out * g.to(hip_device)).sum().backward()
    for got, want in ((a["cur_feats"].grad, cur_c.grad), (a["src_feats"].grad, src_c.grad)):
        e = (got.cpu() - want).abs().flatten() / (want.abs().max() + 1e-30)
        assert float(e.kthvalue(int(0.995 * e.numel())).values) < 1e-3 and float(e.mean()) < 2e-4


@pytest.mark.gpu
def test_cost_volume_det_raises_for_k17_and_warns_under_warn_only(hip_device):
    kw = _cv_case(1, 17, 16, 9, 11, 8, seed=3)
    _det(True)
    with pytest.raises(RuntimeError, match="cost volume backward"):
        _cv_run(kw, 16, 8, hip_device)
    _det(False)
    torch.use_deterministic_algorithms(True, warn_only=True)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        r = _cv_run(kw, 16, 8, hip_device)
    assert any("cost volume backward" in str(x.message) for x in rec)
    assert torch.isfinite(r["src"]).all()


# ---------------------------------------------------------------- depth tail

@pytest.mark.gpu
@pytest.mark.parametrize("D", [128, 160, 256])
def test_depth_tail_det_repeatable_and_close(hip_device, D):
    from oracle.depth_tail_oracle import depth_tail
    from freesplat_amd.depth_tail import depth_regression_tail
    B, h2, w2 = 2, 19, 27
    gen = torch.Generator().manual_seed(D)
    logits = 2.0 * torch.randn(B, D, h2, w2, generator=gen)
    cand = torch.log(torch.tensor(0.5)) + torch.linspace(0, 1, D) * torch.log(torch.tensor(30.0))
    keys = ("coarse", "depth", "depth_map", "depth_weights")
    lc = logits.double().clone().requires_grad_(True)
    r = depth_tail(lc, cand.double(), True)
    up = torch.nn.functional.interpolate(torch.softmax(logits.double(), 1), scale_factor=2, mode="bilinear", align_corners=True)
    top2 = up.topk(2, dim=1).values
    clear = ((top2[:, 0] - top2[:, 1]) > 1e-5)[:, None]
    gs = {k: torch.randn(r[k].shape, generator=gen) for k in keys}
    gs["depth_weights"] = gs["depth_weights"] * clear
    sum((r[k] * gs[k].double()).sum() for k in keys).backward()

    def run(det):
        _det(det)
        lg = logits.to(hip_device).requires_grad_(True)
        o = depth_regression_tail(lg, cand.to(hip_device), True)
        sum((o[k] * gs[k].to(hip_device)).sum() for k in keys).backward()
        torch.cuda.synchronize()
        return lg.grad.clone()

    runs = [run(True) for _ in range(5)]
    assert all(torch.equal(runs[0], x) for x in runs[1:])
    e = (runs[0].cpu().double() - lc.grad).abs()
    assert e.max().item() <= 2e-5 * lc.grad.abs().max().item()
    dflt = run(False)
    assert (runs[0] - dflt).abs().max().item() <= 2e-5 * dflt.abs().max().item()


# ---------------------------------------------------------------- PTF fold with exact z ties

def _tied_fold_inputs(V=4, h=16, w=24, seed=0):
    """V views from ONE camera.  Each view's points come in groups of four with the SAME world position (exact z-buffer ties
    in every later view), the four rows of a group a quarter of the view apart (different workgroups of the fused list)."""
    rng = np.random.default_rng(seed)
    P = h * w
    fx, fy, cx, cy = 0.9, 1.2, 0.5, 0.5
    E = np.eye(4, dtype=np.float32)
    lat = rng.normal(size=(V, P, 64)).astype(np.float32)
    xyz = np.zeros((V, P, 3), np.float32)
    depth = np.zeros((V, P), np.float32)
    n4 = P // 4
    pix = rng.permutation(P)[:n4]                          # the pixel each group lands on
    z = (2.0 + 0.3 * rng.random(n4)).astype(np.float32)
    u, v = (pix % w + 0.5) / w, (pix // w + 0.5) / h
    base = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1).astype(np.float32)
    for i in range(V):
        for q in range(4):
            xyz[i, q * n4:(q + 1) * n4] = base
        depth[i] = 9.0
        depth[i, pix] = z
    dens = rng.random((V, P)).astype(np.float32) + 0.5
    wemb = rng.random((V, P)).astype(np.float32)
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)
    return dict(lat=lat, xyz=xyz, depth=depth.reshape(V, 1, h, w), dens=dens, wemb=wemb,
                E=np.repeat(E[None], V, 0), K=np.repeat(K[None], V, 0), hw=(h, w))


def _fold_grads(d, dev, seed=1):
    from freesplat_amd.ptf import PixelwiseTripletFusion
    torch.manual_seed(seed)
    m = PixelwiseTripletFusion().to(dev)
    V = d["lat"].shape[0]
    P = d["lat"].shape[1]
    t = lambda a: torch.from_numpy(a).to(dev)
    leaves = [t(d["lat"])[None].requires_grad_(True), t(d["xyz"]).view(1, V, P, 1, 1, 3).requires_grad_(True),
              t(d["dens"]).view(1, V, P, 1, 1).requires_grad_(True), t(d["wemb"]).view(1, V, P, 1, 1).requires_grad_(True),
              t(d["depth"]).requires_grad_(True)]
    out = m.fuse_gaussians([leaves[0]], [leaves[1]], leaves[2], leaves[3], leaves[4], t(d["E"])[None], t(d["K"])[None],
                           d["hw"])
    gen = torch.Generator().manual_seed(seed + 3)
    loss = sum((o * torch.randn(o.shape, generator=gen).to(dev)).sum() for o in out)
    loss.backward()
    torch.cuda.synchronize()
    return [x.grad.clone() for x in leaves] + [q.grad.clone() for q in m.gru.parameters()], out[0].shape[1]


@pytest.mark.gpu
@pytest.mark.parametrize("V", [3, 4])
def test_ptf_det_repeatable_with_exact_ties(hip_device, V):
    from freesplat_amd import ptf
    d = _tied_fold_inputs(V=V)
    _det(True)
    runs = [_fold_grads(d, hip_device) for _ in range(5)]
    counts = ptf.LAST_FOLD_COUNTS.cpu().numpy()
    assert counts[1:, 1].min() > 0, counts                 # every step fused rows
    # ... and the first step's fuse list really has 3- and 4-way exact ties (the tie-sum path runs)
    h, w = d["hw"]
    Kv = d["K"][1]
    kpix = torch.tensor([Kv[0, 0] * w, Kv[1, 1] * h, Kv[0, 2] * w, Kv[1, 2] * h], device=hip_device)
    w2c = ptf.world_to_camera(torch.from_numpy(d["E"][1:2]).to(hip_device)).view(4, 4)
    _, _, fpix, _ = ptf.match_view(torch.from_numpy(d["xyz"][0]).to(hip_device), w2c, kpix,
                                   torch.from_numpy(d["depth"][1]).reshape(-1).to(hip_device), h, w)
    per_pixel = torch.bincount(fpix)
    assert int(per_pixel.max()) >= 3 and int((per_pixel >= 3).sum()) >= 16, per_pixel.max()
    for r in runs[1:]:
        assert r[1] == runs[0][1]
        assert all(torch.equal(a, b) for a, b in zip(runs[0][0], r[0]))
    _det(False)
    ref = _fold_grads(d, hip_device)
    for a, b in zip(runs[0][0], ref[0]):
        assert (a - b).abs().max().item() <= 1e-4 * (b.abs().max().item() + 1e-30)
    # against the oracle's CPU autograd (same GRU parameters, same cotangents)
    from oracle import ptf_oracle as po
    from freesplat_amd.ptf import PixelwiseTripletFusion
    torch.manual_seed(1)
    m = PixelwiseTripletFusion()
    params = {k: v.detach().clone().requires_grad_(True) for k, v in m.gru.state_dict().items()}
    P = d["lat"].shape[1]
    t_ = torch.from_numpy
    cpu_in = [t_(d["lat"])[None].clone().requires_grad_(True), t_(d["xyz"]).view(1, V, P, 1, 1, 3).clone().requires_grad_(True),
              t_(d["dens"]).view(1, V, P, 1, 1).clone().requires_grad_(True),
              t_(d["wemb"]).view(1, V, P, 1, 1).clone().requires_grad_(True), t_(d["depth"]).clone().requires_grad_(True)]
    out = po.fuse_gaussians(params, *cpu_in, t_(d["E"])[None], t_(d["K"])[None], d["hw"])
    assert out[0].shape[1] == runs[0][1]
    gen = torch.Generator().manual_seed(1 + 3)
    sum((o * torch.randn(o.shape, generator=gen)).sum() for o in out).backward()
    want = [x.grad for x in cpu_in] + [params[k].grad for k, _ in m.gru.named_parameters()]
    for got, wt in zip(runs[0][0], want):
        if wt is None:
            continue
        assert (got.cpu() - wt).abs().max().item() <= 2e-3 * (wt.abs().max().item() + 1e-30)


# ---------------------------------------------------------------- torch glue under the library's switch alone

@pytest.mark.gpu
def test_glue_source_pick_is_order_fixed_under_the_library_switch(hip_device):
    """FREESPLAT_DETERMINISTIC alone (torch's switch off): prepare_cost_volume_inputs -> cost volume; the matching features'
    gradient (every view is a source of the three others) is the same bits run after run."""
    from freesplat_amd.cost_volume import AVGFeatureVolumeManager
    from freesplat_amd.encoder_glue import prepare_cost_volume_inputs
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import inputs
    V, h, w, C_, D = 4, 24, 32, 48, 32
    E, Kn = inputs.cameras(V, 4 * h, 4 * w, baseline=0.3, seed=5)
    feats0 = torch.randn(V, C_, h, w, generator=torch.Generator().manual_seed(3))
    assert not torch.are_deterministic_algorithms_enabled()
    _det(True)

    def run():
        torch.manual_seed(0)
        m = AVGFeatureVolumeManager(h, w, num_depth_bins=D, mlp_channels=[202, 32, 32, 1], matching_dim_size=C_).to(hip_device)
        feats = feats0.to(hip_device).requires_grad_(True)
        kw = prepare_cost_volume_inputs(E.to(hip_device)[None], Kn.to(hip_device)[None], feats,
                                        torch.full((1, V), 0.5, device=hip_device), torch.full((1, V), 15.0, device=hip_device),
                                        (4 * h, 4 * w), num_context_views=V)
        vol = m(**kw)
        (vol * torch.randn(vol.shape, generator=torch.Generator().manual_seed(4)).to(hip_device)).sum().backward()
        torch.cuda.synchronize()
        return feats.grad.clone()

    runs = [run() for _ in range(3)]
    assert all(torch.equal(runs[0], r) for r in runs[1:])
    _det(False)
    dflt = run()
    assert (runs[0] - dflt).abs().max().item() <= 1e-4 * dflt.abs().max().item()


# ---------------------------------------------------------------- composed chain

def _chain(dev, seed=0):
    """The library's part of a training step, from leaf tensors (no convolutions in between): glue -> cost volume -> depth
    tail -> unprojection (fs_unproject) -> PTF fold -> Gaussian head -> render_views (DecoderSplattingCUDA) -> MSE.  Returns
    the gradient of every leaf and parameter."""
    from freesplat_amd.cost_volume import AVGFeatureVolumeManager
    from freesplat_amd.decoder import DecoderSplattingCUDA, Gaussians
    from freesplat_amd.depth_tail import depth_regression_tail
    from freesplat_amd.encoder_glue import prepare_cost_volume_inputs
    from freesplat_amd.gaussian_adapter import GaussianAdapter, GaussianAdapterCfg
    from freesplat_amd.ptf import PixelwiseTripletFusion
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import inputs
    V, C_, h, w, D = 3, 48, 16, 24, 32
    H, W = 2 * h, 2 * w                                     # the depth tail's x2 map is the Gaussians' resolution
    near, far = 0.5, 15.0
    E, Kn = inputs.cameras(V, H, W, baseline=0.3, seed=5)
    tgt = inputs.cameras(2, H, W, baseline=0.2, seed=9)[0]
    gen = torch.Generator().manual_seed(seed + 1)
    d = lambda t: t.to(dev)
    feats = d(torch.randn(V, C_, h, w, generator=gen)).requires_grad_(True)
    lat = d(torch.randn(1, V, H * W, 64, generator=gen)).requires_grad_(True)
    dens = d(torch.rand(1, V, H * W, 1, 1, generator=gen) * 0.8 + 0.1).requires_grad_(True)
    target = d(torch.rand(1, 2, 3, H, W, generator=gen))
    torch.manual_seed(seed)
    cvm = AVGFeatureVolumeManager(h, w, num_depth_bins=D, mlp_channels=[202, 32, 32, 1], matching_dim_size=C_).to(dev)
    fold = PixelwiseTripletFusion().to(dev)
    lin = torch.nn.Linear(64, 36).to(dev)
    ad = GaussianAdapter(GaussianAdapterCfg(0.5, 15.0, 2)).to(dev)
    kw = prepare_cost_volume_inputs(d(E)[None], d(Kn)[None], feats, torch.full((1, V), near, device=dev),
                                    torch.full((1, V), far, device=dev), (4 * h, 4 * w), num_context_views=V)
    vol = cvm(**kw)                                                          # [V, D, h, w]
    cand = torch.log(torch.linspace(1.3, 1.8, D, device=dev))
    r = depth_regression_tail(vol, cand, True)                               # depth_map, depth_weights [V, 1, H, W]
    depth = r["depth_map"]
    xyz = ad(d(E)[None, :, None, None, None], d(Kn)[None, :, None, None, None], None, depth.reshape(1, V, H * W, 1, 1), None,
             None, (H, W), fusion=True)
    wts = r["depth_weights"].reshape(1, V, H * W, 1, 1)
    g_lat, X, Ex, Dp = fold.fuse_gaussians([lat], [xyz], dens, wts, depth, d(E)[None], d(Kn)[None], (H, W))
    raw = lin(torch.relu(g_lat))
    M = raw.shape[1]
    g = ad(Ex.view(1, 1, M, 1, 1, 4, 4), d(Kn)[0].view(1, 1, 1, 1, 1, 3, 3).expand(1, 1, M, 1, 1, 3, 3), None,
           Dp.view(1, 1, M, 1, 1), torch.sigmoid(raw[..., :1]).view(1, 1, M, 1, 1), raw[..., 2:].view(1, 1, M, 1, 1, 34), (H, W),
           fusion=False, coords=X.view(1, 1, M, 1, 1, 3))
    gs = Gaussians(g.means.reshape(1, M, 3), g.covariances.reshape(1, M, 3, 3), g.harmonics.reshape(1, M, 3, 9),
                   g.opacities.reshape(1, M))
    n = tgt.shape[0]
    out = DecoderSplattingCUDA((0.0, 0.0, 0.0)).to(dev)(gs, d(tgt)[None], d(Kn[:1]).expand(n, 3, 3)[None],
                                                        torch.full((1, n), near, device=dev), torch.full((1, n), far, device=dev),
                                                        (H, W), depth_mode="depth")
    loss = ((out.color - target) ** 2).mean() + 0.01 * r["coarse"].square().mean()
    loss.backward()
    torch.cuda.synchronize()
    leaves = [feats, lat, dens] + list(cvm.parameters()) + list(fold.parameters()) + list(lin.parameters())
    return [x.grad.clone() if x.grad is not None else None for x in leaves], M


@pytest.mark.gpu
@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("switch", ["torch", "env"])
def test_composed_chain_is_bitwise_repeatable(hip_device, switch, streams):
    from freesplat_amd import rasterizer as R
    saved = R.NUM_STREAMS
    R.NUM_STREAMS = streams
    try:
        if switch == "torch":
            torch.use_deterministic_algorithms(True)
        else:
            _det(True)
        runs = [_chain(hip_device) for _ in range(3)]
    finally:
        R.NUM_STREAMS = saved
    assert runs[0][1] > 100                                 # Gaussians after the fold
    for r in runs[1:]:
        assert r[1] == runs[0][1]
        for a, b in zip(runs[0][0], r[0]):
            assert a is not None and b is not None
            assert torch.equal(a, b)
