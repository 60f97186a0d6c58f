"""Deterministic rasterizer backward (include/freesplat_amd.h FS_RASTER_DETERMINISTIC).

CPU: the scratch size query and the argument checks of the three backward entry points with the flag set.
GPU: the gradients of the deterministic mode are the same bits on every run, for every stream count and instance capacity,
whichever switch turns it on; they equal the default (atomic) mode's up to the order of the fp32 sums and match the oracle
through the existing backward tests."""
import ctypes as C

import numpy as np
import pytest
import torch

from freesplat_amd import _lib, synthetic
from util_raster import hip_forward, small_scene, view_inputs


def _dims(N, H, W, flags):
    d = _lib.RasterDims()
    d.N, d.M, d.H, d.W, d.sh_degree, d.tanfovx, d.tanfovy, d.flags = N, 9, H, W, 2, 0.5, 0.5, flags
    return d


def test_scratch_bytes_without_the_flag_are_the_old_sizes():
    L = _lib.lib()
    al = lambda x: (x + 255) // 256 * 256
    for N, H, W in ((1, 1, 1), (1000, 64, 80), (1_000_000, 968, 1296), (300_001, 480, 640)):
        for flags in (0, _lib.RASTER_TILE_CULL | _lib.RASTER_FAST_EXP):
            d = _dims(N, H, W, flags)
            for cap in (0, 1 << 20, 8 * N):
                for ns in (0, 1, 2, 4):
                    assert L.fs_raster_backward_scratch_bytes(C.byref(d), 0, ns, cap) == N * 12 * 4
                    for v in (1, 2, 16):
                        assert L.fs_raster_backward_scratch_bytes(C.byref(d), v, ns, cap) == v * al(N * 48)
    d = _dims(10, 8, 8, _lib.RASTER_DETERMINISTIC)
    assert L.fs_raster_backward_scratch_bytes(None, 1, 1, 100) == 0
    assert L.fs_raster_backward_scratch_bytes(C.byref(d), -1, 1, 100) == 0
    assert L.fs_raster_backward_scratch_bytes(C.byref(d), 1, 1, -1) == 0


def test_scratch_bytes_with_the_flag_grow_with_capacity_views_and_streams():
    L = _lib.lib()
    al = lambda x: (x + 255) // 256 * 256
    for N, H, W in ((1000, 64, 80), (1_000_000, 968, 1296)):
        d = _dims(N, H, W, _lib.RASTER_DETERMINISTIC)
        q = lambda v, ns, cap: L.fs_raster_backward_scratch_bytes(C.byref(d), v, ns, cap)
        for v in (0, 1, 4, 16):
            base = N * 48 if v == 0 else v * al(N * 48)
            prev = base
            for cap in sorted({1, 1000, 1 << 20, 8 * N, 20_000_000}):
                n = q(v, 2, cap)
                assert n > prev and n >= base + cap * 4 * 40, (v, cap)   # at least the slab: cap x 4 quadrants x 40 B
                prev = n
        cap = 8 * N
        sizes = [q(v, 2, cap) for v in (1, 2, 3, 8, 16)]
        assert all(a < b for a, b in zip(sizes, sizes[1:]))
        # one region per stream in flight: a second stream adds one, more streams than views add none
        assert q(4, 2, cap) > q(4, 1, cap) and q(4, 0, cap) == q(4, 1, cap) and q(2, 4, cap) == q(2, 2, cap)
        # ~1.7 GB per stream at 1 M Gaussians and the default capacity (cap x 4 x 40 B slab, index, per-position sums)
        if N == 1_000_000:
            assert 1.6e9 < q(1, 1, cap) - al(N * 48) < 1.8e9


def test_backward_entry_points_refuse_null_arguments_with_the_flag():
    L = _lib.lib()
    d = _dims(100, 32, 32, _lib.RASTER_DETERMINISTIC | _lib.RASTER_TILE_CULL)
    strides = (C.c_size_t * 3)(1 << 20, 1 << 20, 1 << 20)
    assert L.fs_raster_backward(C.byref(d), *([None] * 24), 0, None) == -1
    assert L.fs_raster_backward_views(C.byref(d), 2, *([None] * 15), strides, *([None] * 9), 0, 0, None, None) == -1
    assert L.fs_raster_backward_views_rows(C.byref(d), 2, *([None] * 15), strides, *([None] * 9), 0, 0, None, None,
                                           0, 100, 1) == -1
    assert L.fs_raster_backward(None, *([None] * 24), 0, None) == -1
    assert _lib.ABI_VERSION == L.fs_abi_version() >= 7


# ---------------------------------------------------------------------------------------------------------------- GPU
def _mode(monkeypatch, on):
    from freesplat_amd import rasterizer as R
    monkeypatch.setattr(R, "DETERMINISTIC", on)


def _single_view_grads(vi, dev, with_depth, runs=1, seed=5):
    """One forward of the drop-in rasterizer, `runs` backward passes of it: lists of the five gradients per run."""
    (color, radii, depth, alpha), leaves = hip_forward(vi, dev, requires_grad=True)
    rng = np.random.default_rng(seed)
    H, W = vi["H"], vi["W"]
    loss = (color * torch.from_numpy(rng.normal(size=(3, H, W)).astype(np.float32)).to(dev)).sum()
    if with_depth:
        loss = loss + (depth * torch.from_numpy((0.25 * rng.normal(size=(H, W))).astype(np.float32)).to(dev)).sum()
    names = [k for k in ("means3D", "means2D", "cov3D", "shs", "colors_precomp", "opacities") if leaves.get(k) is not None]
    out = []
    for _ in range(runs):
        g = torch.autograd.grad(loss, [leaves[k] for k in names], retain_graph=True)
        out.append({k: t.detach().clone() for k, t in zip(names, g)})
    return out


def _views_grads(scene, cams, H, W, dev, with_depth, runs=1, seed=9):
    from freesplat_amd.decoder import render_views
    v = cams["extrinsics"].shape[0]
    g = {k: scene[k].to(dev).requires_grad_(True) for k in ("means", "covariances", "harmonics", "opacities")}
    cam = {k: t.to(dev) for k, t in cams.items()}
    color, depth = render_views(cam["extrinsics"], cam["intrinsics"], cam["near"], cam["far"], (H, W),
                                torch.full((v, 3), 0.2, device=dev), g["means"], g["covariances"], g["harmonics"],
                                g["opacities"])
    rng = np.random.default_rng(seed)
    loss = (color * torch.from_numpy(rng.normal(size=tuple(color.shape)).astype(np.float32)).to(dev)).sum()
    if with_depth:
        loss = loss + (depth * torch.from_numpy(rng.normal(size=tuple(depth.shape)).astype(np.float32)).to(dev)).sum()
    out = []
    for _ in range(runs):
        gr = torch.autograd.grad(loss, list(g.values()), retain_graph=True)
        out.append({k: t.detach().clone() for k, t in zip(g, gr)})
    return out


def _assert_bitwise(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs (max {float((a[k] - b[k]).abs().max()):.3e})"


def _assert_close_to_default(det, ref, what, tol=1e-5):
    """The two modes differ only in the order of the fp32 sums: 1e-5 of each gradient's max-abs."""
    for k in det:
        scale = float(ref[k].abs().max()) + 1e-20
        err = float((det[k] - ref[k]).abs().max()) / scale
        assert err < tol, f"{what}: {k} deterministic vs default {err:.3e} of max-abs"


def _fixed_capacity(monkeypatch, cap):
    from freesplat_amd import rasterizer as R
    monkeypatch.setattr(R, "default_capacity", lambda N, st, H=0, W=0: cap)


def _check_single_view(dev, monkeypatch, vi, with_depth, caps, tol=1e-5):
    _mode(monkeypatch, True)
    with monkeypatch.context() as m:
        _fixed_capacity(m, caps[0])
        runs = _single_view_grads(vi, dev, with_depth, runs=3)
    _assert_bitwise(runs[0], runs[1], "run 2")
    _assert_bitwise(runs[0], runs[2], "run 3")
    for cap in caps[1:]:   # the instance capacity sizes the slab only
        with monkeypatch.context() as m:
            _fixed_capacity(m, cap)
            _assert_bitwise(runs[0], _single_view_grads(vi, dev, with_depth)[0], f"capacity {cap}")
    _mode(monkeypatch, False)
    _assert_close_to_default(runs[0], _single_view_grads(vi, dev, with_depth)[0], "single view", tol)
    assert any(bool(t.any()) for t in runs[0].values())


def _check_views(dev, monkeypatch, scene, cams, H, W, with_depth, caps, tol=1e-5):
    from freesplat_amd import rasterizer as R
    _mode(monkeypatch, True)
    monkeypatch.setattr(R, "NUM_STREAMS", 2)
    with monkeypatch.context() as m:
        _fixed_capacity(m, caps[0])
        runs = _views_grads(scene, cams, H, W, dev, with_depth, runs=3)
        _assert_bitwise(runs[0], runs[1], "run 2")
        _assert_bitwise(runs[0], runs[2], "run 3")
        for ns in (1, 3):
            m.setattr(R, "NUM_STREAMS", ns)
            _assert_bitwise(runs[0], _views_grads(scene, cams, H, W, dev, with_depth)[0], f"{ns} streams")
    monkeypatch.setattr(R, "NUM_STREAMS", 2)
    for cap in caps[1:]:
        with monkeypatch.context() as m:
            _fixed_capacity(m, cap)
            _assert_bitwise(runs[0], _views_grads(scene, cams, H, W, dev, with_depth)[0], f"capacity {cap}")
    _mode(monkeypatch, False)
    _assert_close_to_default(runs[0], _views_grads(scene, cams, H, W, dev, with_depth)[0], "render_views", tol)


@pytest.mark.gpu
@pytest.mark.parametrize("with_depth", [False, True])
def test_single_view_repeatable_small(hip_device, monkeypatch, with_depth):
    scene, cams = small_scene(N=8000, H=128, W=160, seed=13)
    vi = view_inputs(scene, cams, 1, 128, 160, bg=(0.3, 0.5, 0.1))
    _check_single_view(hip_device, monkeypatch, vi, with_depth, caps=(1 << 20, 3 << 20))


@pytest.mark.gpu
@pytest.mark.fast_exp
def test_single_view_repeatable_fast_exp(hip_device, monkeypatch):
    from freesplat_amd import rasterizer as R
    assert R.FAST_EXP
    scene, cams = small_scene(N=8000, H=128, W=160, seed=14)
    vi = view_inputs(scene, cams, 0, 128, 160)
    _check_single_view(hip_device, monkeypatch, vi, True, caps=(1 << 20,))


@pytest.mark.gpu
@pytest.mark.parametrize("with_depth", [False, True])
def test_render_views_repeatable_streams_and_capacity(hip_device, monkeypatch, with_depth):
    H, W = 96, 128
    scene, cams = small_scene(N=6000, H=H, W=W, seed=31, n_views=5)
    _check_views(hip_device, monkeypatch, scene, cams, H, W, with_depth, caps=(1 << 20, 5 << 20))


@pytest.mark.gpu
@pytest.mark.fast_exp
def test_render_views_repeatable_fast_exp(hip_device, monkeypatch):
    H, W = 96, 128
    scene, cams = small_scene(N=6000, H=H, W=W, seed=32, n_views=4)
    _check_views(hip_device, monkeypatch, scene, cams, H, W, True, caps=(3 << 20,))


@pytest.mark.gpu
def test_torch_deterministic_switch_equals_explicit_switch(hip_device, monkeypatch):
    H, W = 96, 128
    scene, cams = small_scene(N=6000, H=H, W=W, seed=41, n_views=4)
    vi = view_inputs(scene, cams, 1, H, W)
    _mode(monkeypatch, True)
    want_v = _views_grads(scene, cams, H, W, hip_device, True)[0]
    want_s = _single_view_grads(vi, hip_device, True)[0]
    _mode(monkeypatch, False)
    saved = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(True, warn_only=True)
        got_v = _views_grads(scene, cams, H, W, hip_device, True)[0]
        got_s = _single_view_grads(vi, hip_device, True)[0]
    finally:
        torch.use_deterministic_algorithms(saved[0], warn_only=saved[1])
    _assert_bitwise(want_v, got_v, "render_views")
    _assert_bitwise(want_s, got_s, "single view")


@pytest.mark.gpu
def test_chunked_rows_and_view_by_view_paths(hip_device, monkeypatch):
    """fs_raster_backward_views_rows (the chunked gradient exchange) and the view-by-view fallback (a re-rendered view)
    give the bits of the one-call deterministic backward."""
    from freesplat_amd import decoder as D, rasterizer as R
    H, W = 96, 128
    scene, cams = small_scene(N=6000, H=H, W=W, seed=43, n_views=4)
    _mode(monkeypatch, True)
    want = _views_grads(scene, cams, H, W, hip_device, True)[0]

    class Hook:   # three chunks of rows, handed over as they are ready (no exchange: one process)
        def begin(self, N):
            pass

        def chunk_rows(self, N):
            b = [0, N // 3, 2 * N // 3, N]
            return list(zip(b[:-1], b[1:]))

        def chunk_ready(self, c0, c1, tensors):
            pass

    monkeypatch.setattr(D, "GRAD_EXCHANGE_HOOK", Hook())
    _assert_bitwise(want, _views_grads(scene, cams, H, W, hip_device, True)[0], "chunked rows")
    monkeypatch.setattr(D, "GRAD_EXCHANGE_HOOK", None)
    # the view-by-view backward: sums the views in view order through `accumulate`, which is not the per-Gaussian pass's
    # register sum -- same bits on every run, close to the one-call result
    real = R.default_capacity
    monkeypatch.setattr(R, "default_capacity", lambda N, st, H=0, W=0: 64)    # every view overflows and is re-rendered
    a = _views_grads(scene, cams, H, W, hip_device, True, runs=2)
    monkeypatch.setattr(R, "default_capacity", real)
    R._state(hip_device).retry_cap = 0                                         # (drop the overflow history)
    _assert_bitwise(a[0], a[1], "view by view")
    _assert_close_to_default(a[0], want, "view by view")


@pytest.mark.gpu
def test_overflowed_view_gives_zero_gradients(hip_device, monkeypatch):
    import test_raster_hip as base
    _mode(monkeypatch, True)
    base.test_deferred_overflow_backward_is_safe(hip_device, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("precomp,with_depth,H,W,N", [(False, True, 48, 64, 500), (True, False, 40, 40, 300),
                                                      (False, False, 128, 160, 8000)])
def test_matches_oracle_small(hip_device, monkeypatch, precomp, with_depth, H, W, N):
    import test_raster_hip as base
    _mode(monkeypatch, True)
    base.test_backward_matches_oracle(hip_device, precomp, with_depth, H, W, N)


@pytest.mark.gpu
@pytest.mark.slow
@pytest.mark.parametrize("workload", ["c2_640x480_300k", "c3_968x1296_1M"])
def test_matches_oracle_full_size(hip_device, monkeypatch, workload):
    import test_raster_hip as base
    _mode(monkeypatch, True)
    base.test_full_size_forward_backward_gradients(hip_device, workload)


@pytest.mark.gpu
@pytest.mark.slow
def test_closeup_repeatable_single_view_and_views(hip_device, monkeypatch):
    """The close-up workload (19.6 M instances, the most contended rows): bitwise repeatable, for two capacities and for
    one and two streams, single view and four views, with and without a depth gradient."""
    workload = "c3_closeup_968x1296_1M"
    H, W, N = synthetic.WORKLOADS[workload]
    scene = synthetic.workload_scene(workload)
    cams = synthetic.target_cameras(4)
    vi = view_inputs(scene, cams, 0, H, W)
    # (capacities whose key areas hold the close-up's longest tile lists: no overflow retry, which would change the path)
    # (cov3D of the close-up: a difference of large moment sums over ~20 tiles per Gaussian; the order of its fp32 sums moves
    # it by up to ~1.3e-5 of its max-abs -- the bar of the default mode's own run-to-run spread, printed here)
    _mode(monkeypatch, False)
    d0, d1 = _single_view_grads(vi, hip_device, True, runs=2)
    print("close-up default mode, run-to-run:", {k: float((d0[k] - d1[k]).abs().max() / (d0[k].abs().max() + 1e-20)) for k in d0})
    _check_single_view(hip_device, monkeypatch, vi, True, caps=(40 << 20, 64 << 20), tol=3e-5)
    _check_views(hip_device, monkeypatch, scene, cams, H, W, False, caps=(40 << 20, 48 << 20), tol=3e-5)


@pytest.mark.gpu
def test_deterministic_backward_hipgraph_capture_and_replay(hip_device, monkeypatch):
    """The deterministic backward allocates from the capacity and never syncs: forward + backward of render_views record
    into one hipGraph, and replays give the eager bits."""
    from freesplat_amd.decoder import check_deferred, render_views
    _mode(monkeypatch, True)
    H, W, v = 96, 128, 4
    dev = hip_device
    scene, cams = small_scene(N=6000, H=H, W=W, seed=51, n_views=v)
    g = {k: scene[k].to(dev).requires_grad_(True) for k in ("means", "covariances", "harmonics", "opacities")}
    cam = {k: t.to(dev) for k, t in cams.items()}
    bg = torch.zeros(v, 3, device=dev)
    gc = torch.from_numpy(np.random.default_rng(3).normal(size=(v, 3, H, W)).astype(np.float32)).to(dev)

    def step():
        color, _ = render_views(cam["extrinsics"], cam["intrinsics"], cam["near"], cam["far"], (H, W), bg, g["means"],
                                g["covariances"], g["harmonics"], g["opacities"], check="deferred")
        return torch.autograd.grad((color * gc).sum(), list(g.values()))

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(); check_deferred()                       # warm-up outside capture (side streams, caches)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        grads = step()
    from freesplat_amd import decoder as _D
    _D._pending_checks.clear()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in grads]
        want = step(); check_deferred()
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    assert any(bool(t.any()) for t in got)
