"""Guard-band and poisoned-scratch tests: every HIP entry point that takes a device buffer runs through its Python path with
every torch.empty / torch.zeros of the package replaced by a guarded block (tests/guarded_alloc.py).

Each GPU case runs the operation four times -- unguarded (baseline), then guarded with the scratch / saved / output buffers
pre-filled with 0xFF bytes (NaN, int -1), with zeros, and with finite garbage of magnitude 1e3 -- with the inputs inside blocks
whose surroundings are NaN, and asserts
  * no byte within 64 KiB before or after any buffer changed (after the forward, and again after the backward),
  * no non-finite value in any output or gradient,
  * the four runs agree: bit for bit wherever the path is deterministic (every forward; the backwards under
    rasterizer.DETERMINISTIC; skip conv, LPIPS, GRU, metrics always), within the operation's own existing oracle bound for the
    default atomic backwards.
They do not re-derive correctness (the per-operation files do); the baseline is the only value reference.

Entry point -> guarded case (checked against include/freesplat_amd.h by test_every_entry_point_is_in_the_table):
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

from guarded_alloc import FILLS, GUARD, PAD, Arena, GuardViolation, guarded  # noqa: E402

COVERAGE = {
    # rasterizer and decoder
    "fs_raster_forward": "test_rasterizer_single_view",
    "fs_raster_backward_alpha": "test_rasterizer_single_view",
    "fs_raster_backward": "test_rasterizer_backward_entry_points_without_alpha",
    "fs_raster_forward_views": "test_render_views",
    "fs_raster_backward_views": "test_render_views",
    "fs_raster_backward_views_alpha": "test_rasterizer_backward_entry_points_without_alpha",
    "fs_raster_backward_views_rows": "test_render_views_chunked_rows",
    "fs_raster_backward_views_rows_alpha": "test_rasterizer_backward_entry_points_without_alpha",
    "fs_raster_cov3d_from_scale_rot": "test_cov3d_from_scale_rot",
    "fs_frame_views": "test_frame_views_and_render_depth",
    # cost volume
    "fs_cost_volume_depth_planes": "test_cost_volume",
    "fs_cost_volume_forward": "test_cost_volume",
    "fs_cost_volume_forward_layout": "test_cost_volume",
    "fs_cost_volume_forward_train": "test_cost_volume",
    "fs_cost_volume_backward": "test_cost_volume",
    "fs_cost_volume_backward_train": "test_cost_volume",
    "fs_cost_volume_backward_det": "test_cost_volume",
    # PTF
    "fs_ptf_match": "test_match_view_and_write_state",
    "fs_ptf_gru_inputs": "test_match_view_and_write_state",
    "fs_ptf_write_state": "test_match_view_and_write_state",
    "fs_ptf_gru_forward": "test_gru_rows",
    "fs_ptf_gru_backward": "test_gru_rows",
    "fs_ptf_gru_weight_grads": "test_gru_rows",
    "fs_ptf_fold": "test_inference_fold",
    "fs_ptf_fold_step": "test_training_fold",
    "fs_ptf_fold_step_save": "test_training_fold",
    "fs_ptf_cameras": "test_training_fold",
    "fs_ptf_gru_backward_saved": "test_training_fold",
    "fs_ptf_write_state_backward": "test_training_fold",
    "fs_ptf_write_state_backward_det": "test_training_fold",
    "fs_ptf_gru_inputs_backward": "test_training_fold_with_tied_pixels",
    "fs_ptf_gru_inputs_backward_det": "test_training_fold_with_tied_pixels",
    "fs_invert_4x4": "test_world_to_camera",
    # adapter
    "fs_unproject_forward": "test_unproject",
    "fs_unproject_backward": "test_unproject",
    "fs_gaussian_head_forward_sh": "test_gaussian_head",
    "fs_gaussian_head_backward_sh": "test_gaussian_head",
    "fs_gaussian_head_forward": "test_gaussian_head_degree_2_entry_points",
    "fs_gaussian_head_backward": "test_gaussian_head_degree_2_entry_points",
    "fs_latents_pack_forward": "test_latents_pack",
    "fs_latents_pack_backward": "test_latents_pack",
    "fs_skip_latents_forward": "test_skip_latents",
    "fs_skip_latents_backward": "test_skip_latents",
    # depth tail
    "fs_depth_tail_forward": "test_depth_tail",
    "fs_depth_tail_backward": "test_depth_tail",
    "fs_depth_tail_backward_det": "test_depth_tail",
    # metrics, LPIPS
    "fs_image_metrics": "test_image_metrics",
    "fs_depth_metrics": "test_depth_metrics",
    "fs_lpips_layer_forward": "test_lpips_head",
    "fs_lpips_layer_backward": "test_lpips_head",
    "fs_lpips_prepare_forward": "test_lpips_prepare",
    "fs_lpips_prepare_backward": "test_lpips_prepare",
}
EXEMPT = {
    "fs_version": "returns a host string",
    "fs_abi_version": "returns an integer",
    "fs_last_error": "returns a host string",
    "fs_profile_enable": "host-side switch", "fs_profile_collect": "writes host arrays only", "fs_profile_stage_name": "host string",
    "fs_raster_buffer_sizes": "size query (host out[4]); its sizes are what the guarded rasterizer cases allocate",
    "fs_raster_scratch_slots": "size query", "fs_raster_backward_scratch_bytes": "size query",
    "fs_cost_volume_workspace_bytes": "size query", "fs_cost_volume_saved_bytes": "size query",
    "fs_cost_volume_backward_workspace_bytes": "size query", "fs_cost_volume_backward_workspace_bytes_for": "size query",
    "fs_cost_volume_backward_det_bytes": "size query",
    "fs_ptf_scratch_bytes": "size query", "fs_ptf_fold_scratch_bytes": "size query", "fs_ptf_fold_bytes": "size query",
    "fs_ptf_backward_det_bytes": "size query", "fs_ptf_gru_weight_grads_bytes": "size query",
    "fs_ptf_gru_table_rows": "layout query", "fs_ptf_gru_table_layout": "layout query", "fs_ptf_gru_table_t_rows": "layout query",
    "fs_ptf_gru_stream_rows": "layout query", "fs_ptf_gru_stream_layout": "layout query",
    "fs_ptf_gru_stream_chunk_rows": "layout query", "fs_ptf_gru_stream_t_rows": "layout query",
    "fs_ptf_gru_side_cols": "layout query", "fs_ptf_gru_act_cols": "layout query", "fs_ptf_gru_grad_floats": "layout query",
    "fs_ptf_fold_step_lists": "pointer arithmetic on the host: launches nothing, touches no device memory",
    "fs_image_metrics_scratch_bytes": "size query", "fs_depth_metrics_scratch_bytes": "size query",
    "fs_lpips_scratch_bytes": "size query", "fs_lpips_saved_bytes": "size query",
    "fs_skip_latents_saved_bytes": "size query", "fs_skip_latents_scratch_bytes": "size query",
    "fs_raster_tile_ranges": "debug accessor: returns a pointer into a buffer, launches nothing",
    "fs_raster_point_list": "debug accessor", "fs_raster_geom_records": "debug accessor", "fs_raster_final_T": "debug accessor",
    "fs_raster_n_contrib": "debug accessor",
}


# =====================================================================================================================
# Host tests: the helper itself
# =====================================================================================================================

def _header_entry_points():
    text = open(os.path.join(os.path.dirname(HERE), "include", "freesplat_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fs_\w+)\s*\(", text)))


def test_every_entry_point_is_in_the_table():
    names = _header_entry_points()
    assert len(names) > 80 and "fs_raster_forward" in names and "fs_skip_latents_backward" in names
    missing = [n for n in names if n not in COVERAGE and n not in EXEMPT]
    assert not missing, f"entry points of include/freesplat_amd.h with neither a guarded case nor an exemption: {missing}"
    stale = [n for n in list(COVERAGE) + list(EXEMPT) if n not in names]
    assert not stale, f"table rows for entry points the header no longer declares: {stale}"
    assert not set(COVERAGE) & set(EXEMPT)
    me = sys.modules[__name__]
    for n, t in COVERAGE.items():
        fn = getattr(me, t, None)
        assert callable(fn), f"{n}: the table names {t}, which this file does not define"
        marks = [m.name for m in getattr(fn, "pytestmark", [])]
        assert "gpu" in marks, f"{n}: {t} is not a GPU case"
    for n, why in EXEMPT.items():
        assert why, n


@pytest.mark.parametrize("fill", FILLS)
def test_replacements_return_what_the_originals_return(fill):
    x = torch.arange(6, dtype=torch.float64).reshape(2, 3)
    with guarded(fill) as arena:
        made = [torch.empty(5, 7), torch.empty((5, 7)), torch.empty([3], dtype=torch.int32), torch.empty(2, 3, 4, dtype=torch.float16, device="cpu"),
                torch.empty(torch.Size([9]), dtype=torch.uint8), torch.empty(3, dtype=torch.int64), torch.empty_like(x),
                torch.empty_like(x, dtype=torch.float32), x.new_empty(4, 2), x.new_empty((4, 2), dtype=torch.int32),
                torch.zeros(5, 7), torch.zeros((3,), dtype=torch.int32), torch.zeros_like(x), x.new_zeros(2, 2), x.new_zeros((7,))]
        want = [((5, 7), torch.float32), ((5, 7), torch.float32), ((3,), torch.int32), ((2, 3, 4), torch.float16), ((9,), torch.uint8),
                ((3,), torch.int64), ((2, 3), torch.float64), ((2, 3), torch.float32), ((4, 2), torch.float64), ((4, 2), torch.int32),
                ((5, 7), torch.float32), ((3,), torch.int32), ((2, 3), torch.float64), ((2, 2), torch.float64), ((7,), torch.float64)]
        assert len(arena.records) == len(made)
        for t, (shape, dtype), r in zip(made, want, arena.records):
            assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous() and t.device.type == "cpu"
            assert (t.data_ptr() - r.base.data_ptr()) == GUARD and GUARD % 256 == 0      # the block's own alignment is kept
            assert r.base.numel() == 2 * GUARD + -(-r.nbytes // 256) * 256 and r.nbytes == t.numel() * t.element_size()
            assert bool((r.base[:GUARD] == PAD).all()) and bool((r.base[GUARD + r.nbytes:] == PAD).all())
            assert "test_memory_guards.py" in r.site
        for t in made[10:]:
            assert bool((t == 0).all())
        raw = lambda t: t.view(torch.uint8) if t.dtype != torch.uint8 else t
        if fill == "ff":
            assert all(bool((raw(t) == 0xFF).all()) for t in made[:10]) and bool(made[0].isnan().all()) and bool((made[2] == -1).all())
        elif fill == "zero":
            assert all(bool((raw(t) == 0).all()) for t in made[:10])
        else:
            assert bool(made[0].isfinite().all()) and 400 < float(made[0].abs().min()) and float(made[0].abs().max()) < 2100
        # forms the package does not use fall through to the originals, unrecorded
        n = len(arena.records)
        assert torch.empty(0).numel() == 0 and torch.zeros(3, requires_grad=True).requires_grad
        assert torch.empty_like(x.t()).stride() == x.t().stride()
        assert torch.zeros_like(x, memory_format=torch.preserve_format).shape == x.shape
        assert len(arena.records) == n
        arena.check()
    assert torch.empty.__module__ != "guarded_alloc" and "new_empty" not in torch.Tensor.__dict__


def test_garbage_is_seeded():
    with guarded("garbage", seed=3) as a:
        x = torch.empty(1000)
    with guarded("garbage", seed=3) as b:
        y = torch.empty(1000)
    with guarded("garbage", seed=4) as c:
        z = torch.empty(1000)
    assert torch.equal(x, y) and not torch.equal(x, z)
    del a, b, c


@pytest.mark.parametrize("side", ["before", "after"])
def test_a_write_one_element_outside_is_reported(side):
    with guarded("zero") as arena:
        torch.empty(8)
        t = torch.empty(3, 5, dtype=torch.float32)           # 60 bytes: the slack up to 256 is guarded too
        torch.zeros(4)
        arena.check()
        base = arena.records[1].base                          # memory this test owns: the overrun stays inside the block
        whole = torch.as_strided(base.view(torch.float32), (base.numel() // 4,), (1,))
        first = GUARD // 4
        assert whole[first:first + 15].data_ptr() == t.data_ptr()
        whole[first - 1 if side == "before" else first + 15] = 1.0
        with pytest.raises(GuardViolation) as e:
            arena.check("forward")
    msg = str(e.value)
    assert "allocation #1 " in msg and "shape (3, 5)" in msg and "torch.float32" in msg and "test_memory_guards.py" in msg
    assert f"  {side} allocation" in msg and "(forward)" in msg and "#0" not in msg and "#2" not in msg
    assert ("bytes -4 .. -1 relative" in msg) if side == "before" else ("bytes +0 .. +3 past the buffer's 60 bytes" in msg)


def test_place_surrounds_an_input_with_nan():
    src = torch.arange(10, dtype=torch.float32).reshape(2, 5)
    arena = Arena("zero")
    t = arena.place(src.t())                                  # (a non-contiguous input is placed as its contiguous copy)
    assert torch.equal(t, src.t()) and t.is_contiguous() and not t.requires_grad
    base = arena.records[0].base
    around = torch.as_strided(base.view(torch.float32), (base.numel() // 4,), (1,))
    assert bool(around[: GUARD // 4].isnan().all()) and bool(around[GUARD // 4 + 10:].isnan().all())
    arena.check()
    around[GUARD // 4 + 10] = 0.0
    with pytest.raises(GuardViolation, match="after allocation #0 .input."):
        arena.check()


def test_the_patch_is_removed_after_an_exception():
    orig = (torch.empty, torch.empty_like, torch.zeros, torch.zeros_like, torch.Tensor.new_empty, torch.Tensor.new_zeros)
    with pytest.raises(KeyError):
        with guarded("ff"):
            assert torch.empty is not orig[0]
            raise KeyError("boom")
    assert (torch.empty, torch.empty_like, torch.zeros, torch.zeros_like, torch.Tensor.new_empty, torch.Tensor.new_zeros) == orig
    with pytest.raises(ValueError):
        with guarded("other"):
            pass
    assert torch.empty is orig[0]


# =====================================================================================================================
# GPU cases
# =====================================================================================================================

gpu = pytest.mark.gpu


def _clear_caches():
    from freesplat_amd import ptf, rasterizer, view_sharding
    ptf._fold_scratch.clear()
    for st in rasterizer._states.values():
        st.scratch.clear()
        st.last_instances = 0
        st.retry_cap = 0
    view_sharding._buckets.clear()


def _once(op, dev, fill, clear=True):
    """One run of `op(place) -> (outputs, backward | None)`; backward() -> gradients.  -> (outputs, gradients), detached."""
    if clear:
        _clear_caches()
    if fill is None:
        outs, bwd = op(lambda t, rg=False: t.to(dev).requires_grad_(rg))
        grads = list(bwd()) if bwd is not None else []
        torch.cuda.synchronize()
    else:
        with guarded(fill) as arena:
            outs, bwd = op(lambda t, rg=False: arena.place(t.to(dev)).requires_grad_(rg))
            torch.cuda.synchronize()
            arena.check("after the forward")
            grads = list(bwd()) if bwd is not None else []
            torch.cuda.synchronize()
            arena.check("after the backward")
    det = lambda ts: [None if t is None else t.detach() for t in ts]
    return det(outs), det(grads)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a == b) | ((a != a) & (b != b))).all())


def _agree(base, got, what, finite=True, close=None):
    """outputs: always the same bits; gradients: the same bits, or `close(a, b, k)` where the backward uses float atomics."""
    for part, (bs, gs) in (("output", (base[0], got[0])), ("gradient", (base[1], got[1]))):
        assert len(bs) == len(gs), (what, part)
        for k, (a, b) in enumerate(zip(bs, gs)):
            assert (a is None) == (b is None), (what, part, k)
            if a is None:
                continue
            if finite and b.is_floating_point():
                assert bool(b.isfinite().all()), f"{what}: {part} {k} holds a non-finite value"
            if part == "gradient" and close is not None:
                assert a.shape == b.shape and close(a, b, k), f"{what}: {part} {k} differs from the unguarded run beyond the bound"
            else:
                assert _same(a, b), f"{what}: {part} {k} differs from the unguarded run"


def _four(op, dev, what="", finite=True, close=None):
    base = _once(op, dev, None)
    for k, t in enumerate(base[0] + base[1]):
        if finite and t is not None and t.is_floating_point():
            assert bool(t.isfinite().all()), f"{what}: baseline tensor {k} is not finite: choose other inputs"
    for fill in FILLS:
        _agree(base, _once(op, dev, fill), f"{what} [fill {fill}]", finite, close)
    return base


def _rel_close(bound):
    return lambda a, b, k: float((a.double() - b.double()).abs().max()) <= bound * (float(a.double().abs().max()) + 1e-20)


@pytest.fixture
def det(monkeypatch):
    """Switches the deterministic backwards on / off (rasterizer.DETERMINISTIC is what every module's deterministic() reads)."""
    from freesplat_amd import rasterizer as R

    def set_(on):
        monkeypatch.setattr(R, "DETERMINISTIC", bool(on))
    return set_


# ---- adapter ---------------------------------------------------------------------------------------------------------

def _sh_mask(d_sh):
    m = torch.ones(d_sh)
    for degree in range(1, int(round(d_sh ** 0.5))):
        m[degree ** 2: (degree + 1) ** 2] = 0.1 * 0.25 ** degree
    return m


HEAD_M = [1, 127, 128, 129, 255, 257, 2000]


@gpu
@pytest.mark.parametrize("d_sh", [1, 4, 9, 16])
def test_gaussian_head(hip_device, d_sh):
    """_Head at every M around the 128-row blocks, with all 15 non-empty subsets of the four cotangents (absent = NULL)."""
    from freesplat_amd.gaussian_adapter import _Head
    for M in HEAD_M:
        gen = torch.Generator().manual_seed(M * 31 + d_sh)
        raw, dep = torch.randn(M, 7 + 3 * d_sh, generator=gen), 1.0 + torch.rand(M, generator=gen)
        E = torch.eye(4).repeat(M, 1, 1) + 0.1 * torch.randn(M, 4, 4, generator=gen)
        cots = [torch.randn(M, 3, 3, generator=gen), torch.randn(M, 3, d_sh, generator=gen), torch.randn(M, 3, generator=gen),
                torch.randn(M, 4, generator=gen)]

        def op(place):
            r, d, e = place(raw, True), place(dep, True), place(E, True)
            o = _Head.apply(r, d, e, place(torch.tensor([0.0123])), place(_sh_mask(d_sh)), 0.5, 15.0)
            c = [place(t) for t in cots]

            def bwd():
                res = []
                for bits in range(1, 16):
                    sel = [k for k in range(4) if bits >> k & 1]
                    res += torch.autograd.grad([o[k] for k in sel], [r, d, e], [c[k] for k in sel], retain_graph=True)
                return res
            return list(o), bwd
        _four(op, hip_device, f"gaussian head M={M} d_sh={d_sh}")


@gpu
def test_gaussian_head_degree_2_entry_points(hip_device):
    """fs_gaussian_head_forward / _backward (the d_sh = 9 entry points of ABI <= 8, which the Python layer no longer calls):
    the same buffers as _Head makes, the same bits as the _sh entry points."""
    from freesplat_amd import _lib
    from freesplat_amd.gaussian_adapter import _Head
    L, p = _lib.lib(), _lib.ptr
    for M in (1, 129, 2000):
        gen = torch.Generator().manual_seed(M)
        raw, dep = torch.randn(M, 34, generator=gen), 1.0 + torch.rand(M, generator=gen)
        E = torch.eye(4).repeat(M, 1, 1) + 0.1 * torch.randn(M, 4, 4, generator=gen)
        cots = [torch.randn(M, 3, 3, generator=gen), torch.randn(M, 3, 9, generator=gen), torch.randn(M, 3, generator=gen),
                torch.randn(M, 4, generator=gen)]

        def op(place, sh=False):
            r, d, e, mult, mask = place(raw), place(dep), place(E), place(torch.tensor([0.0123])), place(_sh_mask(9))
            c = [place(t) for t in cots]
            if sh:
                r, d, e = (t.requires_grad_(True) for t in (r, d, e))
                o = _Head.apply(r, d, e, mult, mask, 0.5, 15.0)
                return list(o), lambda: torch.autograd.grad(o, [r, d, e], c)
            dev = r.device
            o = [torch.empty(M, 3, 3, device=dev), torch.empty(M, 3, 9, device=dev), torch.empty(M, 3, device=dev), torch.empty(M, 4, device=dev)]
            _lib.check(L.fs_gaussian_head_forward(M, p(r), p(d), p(e), p(mult), 0, p(mask), C.c_float(0.5), C.c_float(15.0),
                                                  *[p(t) for t in o], _lib.current_stream()), "fs_gaussian_head_forward")

            def bwd():
                g = [torch.empty_like(r), torch.empty_like(d), torch.empty_like(e)]
                _lib.check(L.fs_gaussian_head_backward(M, p(r), p(d), p(e), p(mult), 0, p(mask), C.c_float(0.5), C.c_float(15.0),
                                                       *[p(t) for t in c], *[p(t) for t in g], _lib.current_stream()),
                           "fs_gaussian_head_backward")
                return g
            return o, bwd
        base = _four(op, hip_device, f"fs_gaussian_head_forward / _backward M={M}")
        _agree(base, _once(lambda place: op(place, sh=True), hip_device, None), "against the _sh entry points")


@gpu
@pytest.mark.parametrize("V,h,w", [(1, 7, 9), (3, 37, 41)])
def test_unproject(hip_device, V, h, w):
    from freesplat_amd.gaussian_adapter import _Unproject
    import inputs
    gen = torch.Generator().manual_seed(V + h)
    E, Kn = inputs.cameras(V, h, w, seed=3)
    dep = 1.0 + torch.rand(V, h * w, generator=gen)
    k0 = torch.tensor([0.9 * w, 1.2 * h, 0.49 * w, 0.51 * h])
    cot = torch.randn(V, h * w, 3, generator=gen)

    def op(place):
        d = place(dep, True)
        xyz = _Unproject.apply(d, place(E), place(k0), h, w)
        c = place(cot)
        return [xyz], lambda: torch.autograd.grad(xyz, [d], c)
    _four(op, hip_device, "unproject")


PACK_SHAPES = [(1, 8, 8), (3, 37, 41), (2, 64, 96), (1, 5, 7)]      # the last two of test_latents_pack's + one with h*w % 4 = 3


@gpu
@pytest.mark.parametrize("N,h,w", PACK_SHAPES)
def test_latents_pack(hip_device, N, h, w):
    from freesplat_amd.gaussian_adapter import latents_pack
    gen = torch.Generator().manual_seed(N * 1000 + h)
    head, skip = torch.randn(N, 65, h, w, generator=gen), torch.randn(N, 64, h, w, generator=gen)
    g_lat, g_dens = torch.randn(N, h * w, 64, generator=gen), torch.randn(N, h * w, generator=gen)

    def op(place):
        hd, sk = place(head, True), place(skip, True)
        lat, dens = latents_pack(hd, sk)
        gl, gd = place(g_lat), place(g_dens)
        return [lat, dens], lambda: (list(torch.autograd.grad([lat, dens], [hd, sk], [gl, gd], retain_graph=True))
                                     + list(torch.autograd.grad([lat], [hd, sk], [gl], retain_graph=True))
                                     + list(torch.autograd.grad([dens], [hd], [gd], retain_graph=True)))
    _four(op, hip_device, "latents_pack")


@gpu
@pytest.mark.parametrize("N,h,w", PACK_SHAPES)
def test_skip_latents(hip_device, N, h, w):
    from freesplat_amd.gaussian_adapter import skip_latents
    gen = torch.Generator().manual_seed(N * 1000 + w)
    head, img = torch.randn(N, 65, h, w, generator=gen), torch.rand(N, 3, h, w, generator=gen)
    weight, bias = 0.1 * torch.randn(64, 3, 7, 7, generator=gen), 0.1 * torch.randn(64, generator=gen)
    g_lat, g_dens = torch.randn(N, h * w, 64, generator=gen), torch.randn(N, h * w, generator=gen)

    def op(place):
        hd, wt, b = place(head, True), place(weight, True), place(bias, True)
        lat, dens = skip_latents(hd, place(img), wt, b)
        gl, gd = place(g_lat), place(g_dens)
        return [lat, dens], lambda: (list(torch.autograd.grad([lat, dens], [hd, wt, b], [gl, gd], retain_graph=True))
                                     + list(torch.autograd.grad([lat], [wt, b], [gl], retain_graph=True))
                                     + list(torch.autograd.grad([dens], [hd], [gd], retain_graph=True)))
    _four(op, hip_device, "skip_latents")          # (deterministic always: per-workgroup partial sums in a fixed order)

    def inference(place):
        with torch.no_grad():
            return list(skip_latents(place(head), place(img), place(weight), place(bias))), None
    _four(inference, hip_device, "skip_latents without a mask")


# ---- cost volume -----------------------------------------------------------------------------------------------------

def _cv_cases():
    from test_cost_volume_hip import BWD_CASES, RAGGED_CASES
    out = [pytest.param(V, K, h4, w4, D, C, behind, None, 17 + V, id=f"ragged_{V}_{K}_{h4}x{w4}_D{D}_C{C}")
           for V, K, h4, w4, D, behind, C in RAGGED_CASES]
    out += [pytest.param(V, K, h4, w4, D, C, behind, views, 31 + V, id=name) for name, (V, K, h4, w4, D, C, behind, views) in BWD_CASES.items()]
    return out


@gpu
@pytest.mark.parametrize("V,K,h4,w4,D,C,behind,views,seed", _cv_cases())
def test_cost_volume(hip_device, monkeypatch, det, V, K, h4, w4, D, C, behind, views, seed):
    """Inference on [C, h, w] and on channels-last maps; the training forward with and without saved activations; the saved,
    two-pass and atomic backwards and the deterministic one (from saved activations and recomputing).  The generated planes go
    through fs_cost_volume_depth_planes (D = 7, 3, 11, ... among the cases)."""
    import inputs
    from freesplat_amd.cost_volume import AVGFeatureVolumeManager
    torch.manual_seed(V * 10 + K)
    m = AVGFeatureVolumeManager(matching_height=h4, matching_width=w4, num_depth_bins=D, mlp_channels=[202, 32, 32, 1],
                                matching_dim_size=C).to(hip_device)
    kw = (inputs.cv_inputs(V, K, h4, w4, C, seed=seed, oblique=1.2) if behind == "oblique" else
          inputs.cv_inputs(V, K, h4, w4, C, seed=seed, behind=behind))
    if views is not None:
        kw = {k: (v[list(views)] if k not in ("min_depth", "max_depth") else v) for k, v in kw.items()}
    B = kw["cur_feats"].shape[0]
    g = torch.randn(B, D, h4, w4, generator=torch.Generator().manual_seed(3))
    params = list(m.mlp.parameters())

    def infer(place, channels_last=False):
        a = {k: place(v) for k, v in kw.items()}
        if channels_last:
            # (pixel-major memory under the [.., C, h, w] shape: made from the placed copy, so these two maps are not NaN-ringed)
            a["cur_feats"] = a["cur_feats"].contiguous(memory_format=torch.channels_last)
            a["src_feats"] = a["src_feats"].permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
        with torch.no_grad():
            return [m(**a)], None

    def train(place):
        a = {k: place(v) for k, v in kw.items()}
        a["cur_feats"].requires_grad_(True)
        a["src_feats"].requires_grad_(True)
        out = m(**a)
        go = place(g)
        return [out], lambda: torch.autograd.grad(out, [a["cur_feats"], a["src_feats"]] + params, go)

    monkeypatch.delenv("FS_CV_BWD_ATOMIC", raising=False)
    monkeypatch.delenv("FS_CV_PROJECTED", raising=False)
    det(False)
    _four(infer, hip_device, "cost volume inference")
    _four(lambda place: infer(place, True), hip_device, "cost volume inference, channels-last maps")
    # the bound of tests/test_cost_volume_hip.py::test_backward_tight_vs_float64_oracle for every gradient of every form:
    # 1e-3 of the tensor's max-abs at the worst element, 1e-4 on average
    bound = lambda a, b, k: (float((a - b).abs().max()) < 1e-3 * (float(a.abs().max()) + 1e-30)
                             and float((a - b).abs().mean()) < 1e-4 * (float(a.abs().max()) + 1e-30))
    for form in ("saved", "two_pass", "atomic"):
        monkeypatch.setenv("FREESPLAT_CV_SAVE", "1" if form == "saved" else "0")
        if form == "atomic":
            monkeypatch.setenv("FS_CV_BWD_ATOMIC", "1")
        _four(train, hip_device, f"cost volume training, {form} backward", close=bound)
    monkeypatch.delenv("FS_CV_BWD_ATOMIC", raising=False)
    det(True)
    for save in ("1", "0"):
        monkeypatch.setenv("FREESPLAT_CV_SAVE", save)
        _four(train, hip_device, f"cost volume training, deterministic backward, FREESPLAT_CV_SAVE={save}")


# ---- depth tail ------------------------------------------------------------------------------------------------------

def _tail_shapes():
    from test_depth_tail import SEEDED_SHAPES
    return [(B, D, h2, w2, which) for B, D, h2, w2, _lp, which in SEEDED_SHAPES]


@gpu
@pytest.mark.parametrize("log_planes", [True, False])
@pytest.mark.parametrize("B,D,h2,w2,which", sorted(set(_tail_shapes())))
def test_depth_tail(hip_device, det, B, D, h2, w2, which, log_planes):
    from freesplat_amd.depth_tail import depth_regression_tail
    gen = torch.Generator().manual_seed(B * 1000 + D)
    logits = 2.0 * torch.randn(B, D, h2, w2, generator=gen)
    lo, hi = 0.5, 15.0
    cand = (torch.log(torch.tensor(lo)) + torch.linspace(0, 1, D) * torch.log(torch.tensor(hi / lo))) if log_planes \
        else (1.0 / hi + torch.linspace(0, 1, D) * (1.0 / lo - 1.0 / hi))
    names = ("coarse", "depth", "depth_map", "depth_weights")
    shapes = dict(coarse=(B, 1, h2, w2), depth=(B, 1, h2, w2), depth_map=(B, 1, 2 * h2, 2 * w2), depth_weights=(B, 1, 2 * h2, 2 * w2))
    gs = {k: torch.randn(shapes[k], generator=gen) for k in names}
    keys = {"all": names, "weights": ("depth_weights",), "map": ("depth_map",), "coarse": ("coarse", "depth")}[which]

    def op(place):
        lg = place(logits, True)
        o = depth_regression_tail(lg, place(cand), log_planes)
        c = [place(gs[k]) for k in keys]
        return [o[k] for k in names], lambda: torch.autograd.grad([o[k] for k in keys], [lg], c)

    def coarse_only(place):
        with torch.no_grad():
            o = depth_regression_tail(place(logits), place(cand), log_planes, upsample=False)
        return [o["coarse"], o["depth"]], None
    det(True)
    _four(op, hip_device, "depth tail, deterministic backward")
    _four(coarse_only, hip_device, "depth tail without the x2 outputs")
    det(False)
    # tests/test_depth_tail.py::test_hip_forward_and_backward_on_seeded_shapes: 2e-5 of the gradient's max-abs
    _four(op, hip_device, "depth tail, default backward", close=_rel_close(2e-5))


# ---- PTF -------------------------------------------------------------------------------------------------------------

def _match_inputs(h, w, M, seed):
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = 0.9 * w, 1.2 * h, 0.49 * w, 0.51 * h
    u, v = rng.uniform(-0.1 * w, 1.1 * w, M), rng.uniform(-0.1 * h, 1.1 * h, M)
    z = 2.0 + 0.05 * rng.normal(size=M)
    xyz = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1).astype(np.float32)
    xyz[: M // 10] = xyz[M // 10: 2 * (M // 10)][: M // 10]
    w2c = np.array([[np.cos(0.03), 0, np.sin(0.03), 0.01], [0, 1, 0, -0.02], [-np.sin(0.03), 0, np.cos(0.03), 0.03], [0, 0, 0, 1]], np.float32)
    t = torch.from_numpy
    return t(xyz), t(w2c), torch.tensor([fx, fy, cx, cy], dtype=torch.float32), t((2.0 + 0.05 * rng.normal(size=h * w)).astype(np.float32))


@gpu
@pytest.mark.parametrize("h,w,M,seed", [(7, 9, 5, 4), (24, 32, 768, 1), (8, 8, 0, 2)])
def test_match_view_and_write_state(hip_device, h, w, M, seed):
    """match_view (fs_ptf_match), then the step's data movement through the entry points the fold no longer calls one by one:
    fs_ptf_gru_inputs -> fs_ptf_gru_forward -> fs_ptf_write_state on the lists of the match."""
    from freesplat_amd import _lib
    from freesplat_amd.ptf import GRU, gru_tables, match_view
    L, p = _lib.lib(), _lib.ptr
    xyz, w2c, kpix, depth = _match_inputs(h, w, M, seed)
    P = h * w
    gen = torch.Generator().manual_seed(seed)
    state = [torch.randn(M, 64, generator=gen), xyz, torch.rand(M, generator=gen), torch.rand(M, generator=gen),
             torch.randn(M, 16, generator=gen), 2.0 + torch.rand(M, generator=gen)]
    view = [torch.randn(P, 64, generator=gen), torch.randn(P, 3, generator=gen), torch.rand(P, generator=gen), torch.rand(P, generator=gen),
            depth, torch.randn(16, generator=gen)]
    torch.manual_seed(1)
    gru = GRU().to(hip_device)

    def op(place):
        lists = match_view(place(xyz), place(w2c), place(kpix), place(depth), h, w)
        keep, fuse, fpix, app = lists
        if M == 0:
            return list(lists), None
        nk, nf, na = keep.numel(), fuse.numel(), app.numel()
        G, X, R, O, E, D = (place(t) for t in state)
        g_i, x_i, rho_i, om_i, d_i, E_i = (place(t) for t in view)
        dev = G.device
        st = _lib.current_stream()
        cat = torch.empty(max(nf, 1), 176, device=dev)
        fused = torch.empty(max(nf, 1), 64, device=dev)
        if nf:
            _lib.check(L.fs_ptf_gru_inputs(nf, p(fuse), p(fpix), p(G), p(R), p(O), p(g_i), p(rho_i), p(om_i), p(cat), st), "fs_ptf_gru_inputs")
            _lib.check(L.fs_ptf_gru_forward(nf, p(cat), p(gru_tables(gru)), p(fused), st), "fs_ptf_gru_forward")
        n = nk + nf + na
        out = [torch.empty(n, k, device=dev) for k in (64, 3, 1, 1, 16, 1)]
        _lib.check(L.fs_ptf_write_state(nk, nf, na, p(keep), p(fuse), p(fpix), p(app), p(G), p(X), p(R), p(O), p(E), p(D), p(g_i),
                                        p(x_i), p(rho_i), p(om_i), p(d_i), p(E_i), p(fused), *[p(t) for t in out], st), "fs_ptf_write_state")
        return list(lists) + [cat[:nf], fused[:nf]] + out, None
    base = _four(op, hip_device, "match_view + write_state")
    assert M == 0 or base[0][1].numel() > 0 or M < 10


def _fold_scene(V, h, w, seed):
    from test_ptf_hip import _scene
    return _scene(V, h, w, seed=seed)


@gpu
@pytest.mark.parametrize("V", [2, 3, 5])
def test_inference_fold(hip_device, V):
    """fs_ptf_fold: V = 2 uses one state set; odd and even V end in different sets."""
    from freesplat_amd.ptf import PixelwiseTripletFusion
    h, w = 24, 32
    E, Kn, depths, lat, dens, wts, coords = _fold_scene(V, h, w, 60 + V)
    torch.manual_seed(2)
    m = PixelwiseTripletFusion().to(hip_device)

    def op(place):
        with torch.no_grad():
            out = m.fuse_gaussians([place(lat)], [place(coords)], place(dens), place(wts), place(depths), place(E)[None], place(Kn)[None], (h, w))
        return list(out), None
    base = _four(op, hip_device, "inference fold")
    assert base[0][0].shape[1] < V * h * w          # something fused


def _train_fold_op(m, scene, h, w, gru_grads=True):
    E, Kn, depths, lat, dens, wts, coords = scene

    def op(place):
        ins = [place(t, True) for t in (lat, coords, dens, wts, depths)]
        out = m.fuse_gaussians([ins[0]], [ins[1]], ins[2], ins[3], ins[4], place(E)[None], place(Kn)[None], (h, w))
        cot = [place(torch.randn(o.shape, generator=torch.Generator().manual_seed(11 + k))) for k, o in enumerate(out)]
        leaves = ins + (list(m.gru.parameters()) if gru_grads else [])
        return list(out), lambda: torch.autograd.grad(out, leaves, cot, allow_unused=True)
    return op


# tests/test_ptf_hip.py::test_fold_vs_oracle_and_gradients: input gradients within 1e-3, GRU tensors (k >= 5) within 2e-3 of max-abs
_FOLD_BOUND = lambda a, b, k: _rel_close(1e-3 if k < 5 else 2e-3)(a, b, k)


@gpu
@pytest.mark.parametrize("trim", [False, True])
@pytest.mark.parametrize("keep_act", [True, False])
@pytest.mark.parametrize("V", [3, 4])
def test_training_fold(hip_device, monkeypatch, det, V, keep_act, trim):
    """_PtfFold forward and backward: with kept GRU activations (fs_ptf_fold_step_save / fs_ptf_gru_backward_saved) and without
    (fs_ptf_fold_step / fs_ptf_gru_inputs + fs_ptf_gru_backward), with the states trimmed and as views of the worst-case buffers."""
    from freesplat_amd import ptf as P
    h, w = 24, 32
    scene = _fold_scene(V, h, w, 40 + V)
    torch.manual_seed(9)
    m = P.PixelwiseTripletFusion().to(hip_device)
    monkeypatch.setenv("FREESPLAT_GRU_SAVE", "1" if keep_act else "0")
    monkeypatch.setattr(P, "_KEEP_BYTES_ENV", "0" if trim else str(1 << 40))
    op = _train_fold_op(m, scene, h, w)
    det(True)
    _four(op, hip_device, "training fold, deterministic backward")
    det(False)
    _four(op, hip_device, "training fold, default backward", close=_FOLD_BOUND)


@gpu
@pytest.mark.parametrize("keep_act", [True, False])
def test_training_fold_with_tied_pixels(hip_device, monkeypatch, det, keep_act):
    """ptf_tie.npz: two fused rows share a pixel, so fs_ptf_gru_inputs_backward and fs_ptf_write_state_backward add twice into
    one row of the view's gradients (float atomics; in row order in the deterministic forms)."""
    from freesplat_amd import ptf as P
    from test_ptf_hip import _load
    g, gru = _load("ptf_tie.npz")
    m = P.PixelwiseTripletFusion()
    m.gru.load_state_dict(gru, strict=True)
    m = m.to(hip_device)
    monkeypatch.setenv("FREESPLAT_GRU_SAVE", "1" if keep_act else "0")
    h, w = int(g["h"]), int(g["w"])
    scene = (g["extrinsics"], g["intrinsics"], g["depths"], g["latents"], g["densities"], g["weights"], g["coords"])
    op = _train_fold_op(m, scene, h, w)
    det(True)
    _four(op, hip_device, "tied fold, deterministic backward")
    det(False)
    # tests/test_ptf_hip.py::test_fold_backward_with_tied_winners: 1e-3 of max-abs (GRU tensors: the 2e-3 of the fold's oracle test)
    _four(op, hip_device, "tied fold, default backward", close=_FOLD_BOUND)


@gpu
@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 33, 130, 4097])
def test_gru_rows(hip_device, n):
    """GRU.forward on its own (fs_ptf_gru_forward) and its backward (gru_backward: fs_ptf_gru_backward + fs_ptf_gru_weight_grads)
    around the 16-pair groups; the weight gradients are summed in a fixed order, so everything is bitwise."""
    from freesplat_amd.ptf import GRU
    torch.manual_seed(5)
    gru = GRU().to(hip_device)
    gen = torch.Generator().manual_seed(n)
    x, hid = torch.randn(n, 64, generator=gen), torch.randn(n, 64, generator=gen)
    xe, he = torch.randn(n, 24, generator=gen), torch.randn(n, 24, generator=gen)
    cot = torch.randn(n, 64, generator=gen)

    def op(place):
        ins = [place(t, True) for t in (x, hid, xe, he)]
        out = gru(*ins)
        c = place(cot)
        return [out], lambda: torch.autograd.grad(out, ins + list(gru.parameters()), c)
    _four(op, hip_device, f"GRU rows n={n}")


@gpu
@pytest.mark.parametrize("n", [1, 13])
def test_world_to_camera(hip_device, n):
    from freesplat_amd.ptf import world_to_camera
    gen = torch.Generator().manual_seed(n)
    E = torch.eye(4).repeat(n, 1, 1) + 0.1 * torch.randn(n, 4, 4, generator=gen)
    _four(lambda place: ([world_to_camera(place(E))], None), hip_device, "world_to_camera")


# ---- rasterizer and decoder ------------------------------------------------------------------------------------------

# tests/test_raster_hip.py (module docstring and every backward test): the atomic backward is held to 2e-4 of the gradient's max-abs
_RASTER_BOUND = _rel_close(2e-4)
RASTER_SIZES = [(16, 16, 50, 1), (17, 33, 300, 61), (72, 100, 3000, 3)]
RASTER_FORMS = [("cov", 3, "fp32"), ("scale_rot", 0, "fp32"), ("cov", 2, "fp16"), ("scale_rot", 0, "precomp")]


def _raster_op(vi, form, colour, cots, gen_seed=0):
    """-> op for one GaussianRasterizer call.  form: cov | scale_rot; colour: fp32 | fp16 | precomp; cots: subset of 'cda'."""
    from freesplat_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    N, H, W = vi["means3D"].shape[0], vi["H"], vi["W"]
    gen = torch.Generator().manual_seed(gen_seed + N)
    scales = (0.02 + 0.05 * torch.rand(N, 3, generator=gen)) * float(vi["means3D"].abs().mean())
    rots = torch.randn(N, 4, generator=gen)
    pre = torch.rand(N, 3, generator=gen)
    g = dict(c=torch.randn(3, H, W, generator=gen), d=torch.randn(H, W, generator=gen), a=torch.randn(H, W, generator=gen))

    def op(place):
        means, opac = place(vi["means3D"], True), place(vi["opacities"][:, None], True)
        leaves = [means, opac]
        kw = {}
        if form == "cov":
            kw["cov3D_precomp"] = place(vi["cov3D"], True)
            leaves.append(kw["cov3D_precomp"])
        else:
            kw["scales"], kw["rotations"] = place(scales, True), place(rots, True)
            leaves += [kw["scales"], kw["rotations"]]
        if colour == "precomp":
            kw["colors_precomp"] = place(pre, True)
            leaves.append(kw["colors_precomp"])
        else:
            kw["shs"] = place(vi["shs"].half() if colour == "fp16" else vi["shs"], True)
            leaves.append(kw["shs"])
        means2D = place(torch.zeros(N, 3), True)
        leaves.append(means2D)
        s = GaussianRasterizationSettings(H, W, vi["tanfovx"], vi["tanfovy"], place(vi["bg"]), 1.0, place(vi["viewmatrix"]),
                                          place(vi["projmatrix"]), vi["sh_degree"], place(vi["campos"]), False, False)
        color, radii, depth, alpha = GaussianRasterizer(s)(means3D=means, means2D=means2D, opacities=opac, **kw)
        outs = dict(c=color, d=depth, a=alpha)
        cot = {k: place(g[k]) for k in cots}
        return [color, radii, depth, alpha], lambda: torch.autograd.grad([outs[k] for k in cots], leaves, [cot[k] for k in cots], allow_unused=True)
    return op


def _view(H, W, N, seed, sh_degree=2, scale=1.0):
    from util_raster import small_scene, view_inputs
    scene, cams = small_scene(N=N, H=H, W=W, seed=seed, sh_degree=sh_degree)
    scene["covariances"] = scene["covariances"] * scale
    return view_inputs(scene, cams, 1, H, W, bg=(0.1, 0.2, 0.3))


@gpu
@pytest.mark.parametrize("form,degree,colour", RASTER_FORMS)
@pytest.mark.parametrize("H,W,N,seed", RASTER_SIZES)
def test_rasterizer_single_view(hip_device, det, H, W, N, seed, form, degree, colour):
    vi = _view(H, W, N, seed, sh_degree=degree, scale=30.0 if (H, W) == (17, 33) else 1.0)
    for cots in ("cda", "a"):            # colour + depth + alpha cotangents; alpha alone (dL_dcolor = the zeros the layer makes)
        op = _raster_op(vi, form, colour, cots)
        det(True)
        _four(op, hip_device, f"rasterizer {form} {colour} cotangents {cots}, deterministic backward")
        det(False)
        _four(op, hip_device, f"rasterizer {form} {colour} cotangents {cots}, default backward", close=_RASTER_BOUND)


@gpu
def test_rasterizer_empty_and_all_culled(hip_device, det):
    vi = _view(32, 32, 100, 2)
    behind = dict(vi)
    behind["means3D"] = vi["means3D"] * torch.tensor([1.0, 1.0, -1.0])
    det(True)
    base = _four(_raster_op(behind, "cov", "fp32", "cd"), hip_device, "all-culled scene")
    assert bool((base[0][1] == 0).all()) and all(g is None or bool((g == 0).all()) for g in base[1])
    empty = dict(vi)
    for k, shape in (("means3D", (0, 3)), ("cov3D", (0, 6)), ("shs", (0, 9, 3)), ("opacities", (0,))):
        empty[k] = torch.zeros(shape)

    def op(place):
        with torch.no_grad():
            return _raster_op(empty, "cov", "fp32", "")(place)[0], None
    _four(op, hip_device, "empty scene")


@gpu
def test_rasterizer_capacity_overflow_retry(hip_device, monkeypatch, det):
    """The retry's larger buffers are guarded too (the monkeypatch of tests/test_raster_hip.py::test_capacity_overflow_retry)."""
    from freesplat_amd import rasterizer as R
    vi = _view(64, 64, 3000, 8)
    det(True)
    base = _once(_raster_op(vi, "cov", "fp32", "cd"), hip_device, None)
    monkeypatch.setattr(R, "default_capacity", lambda N, st, H=0, W=0: 100)
    again = _four(_raster_op(vi, "cov", "fp32", "cd"), hip_device, "capacity-overflow retry")
    _agree(base, again, "retried forward against the one that fitted")


def _views_inputs(H, W, N, seed, v):
    from freesplat_amd import synthetic
    scene = synthetic.make_scene(N, n_context=2, seed=seed, sh_degree=2, ctx_hw=(H, W))
    cams = synthetic.target_cameras(v, seed=seed)
    return scene, cams


def _render_views_op(scene, cams, H, W, v, check="now"):
    from freesplat_amd.decoder import render_views
    gen = torch.Generator().manual_seed(v)
    gc, gd = torch.randn(v, 3, H, W, generator=gen), torch.randn(v, 1, H, W, generator=gen)

    def op(place):
        g = [place(scene[k], True) for k in ("means", "covariances", "harmonics", "opacities")]
        cam = {k: place(t) for k, t in cams.items()}
        color, depth = render_views(cam["extrinsics"], cam["intrinsics"], cam["near"], cam["far"], (H, W), place(torch.full((v, 3), 0.2)), *g,
                                    check=check)
        c, d = place(gc), place(gd)
        return [color, depth], lambda: torch.autograd.grad([color, depth], g, [c, d])
    return op


@gpu
@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("H,W,N,v", [(17, 33, 300, 3), (72, 100, 3000, 2)])
def test_render_views(hip_device, monkeypatch, det, H, W, N, v, streams):
    from freesplat_amd import rasterizer as R
    monkeypatch.setattr(R, "NUM_STREAMS", streams)
    scene, cams = _views_inputs(H, W, N, 5, v)
    op = _render_views_op(scene, cams, H, W, v)
    det(True)
    base = _four(op, hip_device, "render_views, deterministic backward")
    det(False)
    _four(op, hip_device, "render_views, default backward", close=_RASTER_BOUND)
    # one view overflows its capacity and is re-rendered on its own: forward and backward then go view by view
    det(True)
    monkeypatch.setattr(R, "default_capacity", lambda N, st, H=0, W=0: 64)
    again = _four(op, hip_device, "render_views with re-rendered views")
    _agree((base[0], []), (again[0], []), "re-rendered views against the batch that fitted")


class _Chunks:
    """The object decoder.GRAD_EXCHANGE_HOOK expects, without the exchange: three chunks of rows."""

    def begin(self, n):
        self.n = n

    def chunk_rows(self, n):
        from freesplat_amd.view_sharding import chunk_row_ranges
        return chunk_row_ranges(n, 3)

    def chunk_ready(self, c0, c1, grads):
        pass


@gpu
def test_render_views_chunked_rows(hip_device, monkeypatch, det):
    """fs_raster_backward_views_rows: the per-Gaussian pass in three chunks of rows gives the bits of the one-call backward."""
    from freesplat_amd import decoder as Dm
    H, W, N, v = 17, 33, 300, 2
    scene, cams = _views_inputs(H, W, N, 6, v)
    op = _render_views_op(scene, cams, H, W, v)
    det(True)
    whole = _once(op, hip_device, None)
    monkeypatch.setattr(Dm, "GRAD_EXCHANGE_HOOK", _Chunks())
    _agree(whole, _four(op, hip_device, "render_views, chunked per-Gaussian pass"), "chunked against whole")


@gpu
def test_rasterizer_backward_entry_points_without_alpha(hip_device, monkeypatch, det):
    """fs_raster_backward is fs_raster_backward_alpha with dL_dalpha = NULL, and fs_raster_backward_views(_rows)_alpha with NULL
    are fs_raster_backward_views(_rows) (include/freesplat_amd.h): the Python layer calls one of each pair, this case routes its
    calls to the other one and asks for the same bits."""
    from freesplat_amd import _lib, decoder as Dm
    L = _lib.lib()
    vi = _view(17, 33, 300, 61, scale=30.0)
    det(True)
    single = _raster_op(vi, "cov", "fp32", "cd")
    scene, cams = _views_inputs(17, 33, 300, 6, 2)
    views = _render_views_op(scene, cams, 17, 33, 2)
    want_single, want_views = _once(single, hip_device, None), _once(views, hip_device, None)
    orig = (L.fs_raster_backward_alpha, L.fs_raster_backward_views, L.fs_raster_backward_views_rows)
    called = []

    def no_alpha(*a):
        assert a[18] is None
        called.append("fs_raster_backward")
        return L.fs_raster_backward(*a[:18], *a[19:])

    def with_alpha(name, fn):
        def f(*a):
            called.append(name)
            return fn(*a[:20], None, *a[20:])
        return f
    monkeypatch.setattr(L, "fs_raster_backward_alpha", no_alpha, raising=False)
    monkeypatch.setattr(L, "fs_raster_backward_views", with_alpha("views_alpha", L.fs_raster_backward_views_alpha), raising=False)
    monkeypatch.setattr(L, "fs_raster_backward_views_rows", with_alpha("rows_alpha", L.fs_raster_backward_views_rows_alpha), raising=False)
    _agree(want_single, _four(single, hip_device, "fs_raster_backward"), "fs_raster_backward against _alpha")
    _agree(want_views, _four(views, hip_device, "fs_raster_backward_views_alpha"), "views_alpha against views")
    monkeypatch.setattr(Dm, "GRAD_EXCHANGE_HOOK", _Chunks())
    _agree(want_views, _four(views, hip_device, "fs_raster_backward_views_rows_alpha"), "rows_alpha against views")
    assert {"fs_raster_backward", "views_alpha", "rows_alpha"} <= set(called)
    monkeypatch.undo()
    assert (L.fs_raster_backward_alpha, L.fs_raster_backward_views, L.fs_raster_backward_views_rows) == orig


@gpu
@pytest.mark.parametrize("N", [1, 63, 257])
def test_cov3d_from_scale_rot(hip_device, N):
    from freesplat_amd import _lib
    gen = torch.Generator().manual_seed(N)
    rows = torch.cat([0.1 + torch.rand(N, 3, generator=gen), torch.randn(N, 4, generator=gen)], 1)

    def op(place):
        r = place(rows)
        out = torch.empty(N, 6, device=r.device)
        _lib.check(_lib.lib().fs_raster_cov3d_from_scale_rot(N, _lib.ptr(r), _lib.ptr(out), _lib.current_stream()), "fs_raster_cov3d_from_scale_rot")
        return [out], None
    _four(op, hip_device, "fs_raster_cov3d_from_scale_rot")


@gpu
def test_frame_views_and_render_depth(hip_device):
    from freesplat_amd.decoder import frame_views, render_depth_cuda
    H, W, N, v = 17, 33, 300, 3
    scene, cams = _views_inputs(H, W, N, 7, v)

    def frame(place):
        cam = {k: place(t) for k, t in cams.items()}
        return list(frame_views(cam["extrinsics"], cam["intrinsics"], cam["near"], cam["far"])), None
    _four(frame, hip_device, "frame_views")

    def depth(place):
        cam = {k: place(t) for k, t in cams.items()}
        rep = lambda t: place(t[None].expand(v, *t.shape))
        with torch.no_grad():
            return [render_depth_cuda(cam["extrinsics"], cam["intrinsics"], cam["near"], cam["far"], (H, W), rep(scene["means"]),
                                      rep(scene["covariances"]), rep(scene["opacities"]))], None
    _four(depth, hip_device, "render_depth_cuda")


# ---- metrics and LPIPS -----------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("B,C,H,W", [(1, 1, 11, 11), (2, 3, 13, 300), (5, 3, 96, 128)])
def test_image_metrics(hip_device, B, C, H, W):
    from freesplat_amd.metrics import image_metrics
    gen = torch.Generator().manual_seed(H * W + C)
    gt = torch.rand(B, C, H, W, generator=gen)
    pred = (gt + 0.1 * torch.randn(B, C, H, W, generator=gen)).clamp(-0.2, 1.2)
    _four(lambda place: (list(image_metrics(place(gt), place(pred), return_map=True)), None), hip_device, "image_metrics")
    _four(lambda place: (list(image_metrics(place(gt), place(pred))), None), hip_device, "image_metrics without the map")


@gpu
@pytest.mark.parametrize("case", ["mixed", "single", "empty"])
def test_depth_metrics(hip_device, case):
    """(`empty`: views without a valid pixel give NaN by definition, so only the bits are compared.)"""
    from freesplat_amd.metrics import depth_metrics
    z = np.load(os.path.join(HERE, "golden", "depth_metrics.npz"))      # (the fixture of tests/test_metrics_hip.py)
    gt, pred = torch.from_numpy(z[f"{case}__gt"]), torch.from_numpy(z[f"{case}__pred"])
    keys = ("abs_diff", "abs_rel", "delta_25", "delta_10")

    def op(place):
        m = depth_metrics(place(gt), place(pred))
        return [m[k] for k in keys], None
    _four(op, hip_device, f"depth_metrics {case}", finite=False)


def _lpips_maps(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.relu(torch.randn(B, C, H, W, generator=g)) + 1e-3, torch.relu(torch.randn(B, C, H, W, generator=g)) + 1e-3,
            torch.rand(C, generator=g))


def _lpips_cases():
    from test_lpips_hip import CASES
    return CASES


@gpu
@pytest.mark.parametrize("B,C,H,W", _lpips_cases())
def test_lpips_head(hip_device, B, C, H, W):
    """One layer forward and backward, both maps with a gradient, then the prediction's map alone (g_f1 = NULL)."""
    from freesplat_amd.lpips import lpips_head
    f0, f1, w = _lpips_maps(B, C, H, W, B * 1000 + C + H)
    g_dist = torch.rand(B, generator=torch.Generator().manual_seed(5)) + 0.5

    def op(place):
        a, b = place(f0, True), place(f1, True)
        dist = lpips_head([a], [b], [place(w)])
        g = place(g_dist)
        return [dist], lambda: (list(torch.autograd.grad([dist], [a, b], [g], retain_graph=True))
                                + list(torch.autograd.grad([dist], [a], [g], retain_graph=True)))
    _four(op, hip_device, "LPIPS head")

    def target_without_gradient(place):
        a = place(f0, True)
        dist = lpips_head([a], [place(f1)], [place(w)])
        g = place(g_dist)
        return [dist], lambda: torch.autograd.grad([dist], [a], [g])
    _four(target_without_gradient, hip_device, "LPIPS head, g_f1 = NULL")


@gpu
def test_lpips_five_layers_into_one_dist(hip_device):
    from freesplat_amd.lpips import lpips_head
    shapes = [(64, 32, 48), (128, 16, 24), (256, 8, 12), (512, 4, 6), (512, 2, 3)]
    layers = [_lpips_maps(2, C, H, W, 20 + i) for i, (C, H, W) in enumerate(shapes)]

    def op(place):
        a = [place(l[0], True) for l in layers]
        b = [place(l[1]) for l in layers]
        dist = lpips_head(a, b, [place(l[2]) for l in layers])
        g = place(torch.tensor([0.7, 1.3]))
        return [dist], lambda: torch.autograd.grad([dist], a, [g])
    _four(op, hip_device, "LPIPS head, five layers")


@gpu
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("B,H,W", [(1, 3, 5), (2, 37, 53)])
def test_lpips_prepare(hip_device, B, H, W, normalize):
    from freesplat_amd.lpips import _Prepare
    gen = torch.Generator().manual_seed(B + H)
    in0, in1 = torch.rand(B, 3, H, W, generator=gen), torch.rand(B, 3, H, W, generator=gen)
    shift, scale = torch.tensor([-.030, -.088, -.188]), torch.tensor([.458, .448, .450])
    cot = torch.randn(2 * B, 3, H, W, generator=gen)

    def op(place):
        a, b = place(in0, True), place(in1, True)
        out = _Prepare.apply(a, b, place(shift), place(scale), normalize)
        c = place(cot)
        return [out], lambda: (list(torch.autograd.grad([out], [a, b], [c], retain_graph=True))
                               + list(torch.autograd.grad([out], [a], [c], retain_graph=True)))
    _four(op, hip_device, "LPIPS prepare")


# ---- cache reuse -----------------------------------------------------------------------------------------------------

@gpu
def test_cached_scratch_carries_nothing_between_calls(hip_device, monkeypatch, det):
    """The inference fold keeps its scratch per (device, stream, V, h, w) and the rasterizer one key-area scratch per stream:
    larger call, smaller call, the first again, with the cached tensors overwritten in between (0xFF, then garbage) -- every
    result equals the one a fresh cache gives, bit for bit."""
    from freesplat_amd import ptf, rasterizer as R
    from freesplat_amd.ptf import PixelwiseTripletFusion
    monkeypatch.setattr(R, "NUM_STREAMS", 1)
    det(True)
    torch.manual_seed(2)
    m = PixelwiseTripletFusion().to(hip_device)

    def fold_op(V, h, w):
        E, Kn, depths, lat, dens, wts, coords = _fold_scene(V, h, w, 70 + V)

        def op(place):
            with torch.no_grad():
                return list(m.fuse_gaussians([place(lat)], [place(coords)], place(dens), place(wts), place(depths), place(E)[None],
                                             place(Kn)[None], (h, w))), None
        return op
    big_f, small_f = fold_op(3, 24, 32), fold_op(3, 12, 16)
    # (the key-area scratch that is kept per stream is the single-view path's; render_views allocates its own per call)
    big_r, small_r = _raster_op(_view(72, 100, 3000, 3), "cov", "fp32", "cd"), _raster_op(_view(17, 33, 300, 61), "cov", "fp32", "cd")
    big_v = _render_views_op(*_views_inputs(72, 100, 3000, 5, 2), 72, 100, 2)
    small_v = _render_views_op(*_views_inputs(17, 33, 300, 5, 2), 17, 33, 2)
    ops = [big_f, big_r, big_v, small_f, small_r, small_v, big_f, big_r, big_v]
    fresh = [_once(op, hip_device, None) for op in ops]            # (caches cleared before each)
    _clear_caches()
    torch.manual_seed(0)
    for k, (op, want) in enumerate(zip(ops, fresh)):
        cached = list(ptf._fold_scratch.values()) + [t for st in R._states.values() for t in st.scratch.values()]
        assert k == 0 or cached, "nothing is cached: this test no longer poisons anything"
        for t in cached:
            if k % 2:
                t.fill_(0xFF)
            else:
                t[: t.numel() // 4 * 4].view(torch.float32).normal_(0.0, 1e3)
        _agree(want, _once(op, hip_device, None, clear=False), f"call {k} on a poisoned cache")
