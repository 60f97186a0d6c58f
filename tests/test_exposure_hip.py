"""GPU checks of the exposure compensation (freesplat_amd/exposure.py on fs_exposure_apply_forward / _backward and
fs_exposure_fit) against the float64 restatement (tests/exposure_ref.py) fed the device's own fp32 inputs.

The bounds follow from the arithmetic the definitions prescribe, with u = 2^-24; none is tuned:
  out, g_image   |err| <= 4u (sum of the |A x| terms + |b|) per element: three fused multiply-adds
  g_params       |err| <= 2u |ref| + n 2^-52 sum |terms|: an fp64 sum of n exact products in any fixed order, one rounding
  fit            |params - ref| <= (2u + kappa cnt 2^-50) max(max |ref|, 1) per view: the final rounding plus the fp64 summation
                 order through the solve; count, solved and the identity rows exactly
Every comparison prints its largest error / bound ratio ("RATIO <family> <value>"); DESIGN.md records the largest seen.

Besides: autograd through apply_exposure, determinism (runs, streams, batch composition, alignment), graph capture, guard bands
and the path from the rasterizer through apply_exposure to photometric_loss."""
import sys

import pytest
import torch

import exposure_cases as EC
import exposure_ref as ER
from exposure_cases import B

gpu = pytest.mark.gpu
U = 2.0 ** -24


def _ids(ids, dev):
    """Device ids: the host never reads them, so out-of-range values are legal."""
    return None if ids is None else torch.tensor(ids, dtype=torch.int64, device=dev)


def _ratio(family, got, want, bound):
    err = (got.detach().double().cpu() - want).abs()
    assert bool(torch.isfinite(err).all()), family
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"RATIO {family} {ratio:.4f}")
    return ratio


def _lib_backward(image, params, ids, g_out, want_image=True, want_params=True):
    """fs_exposure_apply_backward itself, on fresh buffers."""
    from freesplat_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    Bn, _, H, W = g_out.shape
    dev = g_out.device
    g_image = torch.empty_like(g_out) if want_image else None
    g_params = torch.empty_like(params) if want_params else None
    scratch = torch.empty(L.fs_exposure_scratch_bytes(Bn, H, W), dtype=torch.uint8, device=dev) if want_params else None
    _lib.check(L.fs_exposure_apply_backward(Bn, params.shape[0], H, W, p(image if want_params else None), p(params), p(ids), p(g_out),
                                            p(g_image), p(g_params), p(scratch), _lib.current_stream()), "fs_exposure_apply_backward")
    return g_image, g_params


@gpu
@pytest.mark.parametrize("pattern", list(EC.PATTERNS))
@pytest.mark.parametrize("H,W", EC.SHAPES)
def test_apply_and_gradients_vs_float64(hip_device, H, W, pattern):
    from freesplat_amd import exposure as E
    c = EC.apply_case(H, W, pattern)
    ids, V = _ids(c["ids"], hip_device), c["V"]
    image = c["image"].to(hip_device).requires_grad_(True)
    params = c["params"].to(hip_device).requires_grad_(True)
    out = E.apply_exposure(image, params, ids)
    assert out.dtype == torch.float32 and out.shape == image.shape and out.requires_grad
    g_image, g_params = torch.autograd.grad(out, [image, params], c["g_out"].to(hip_device))
    assert g_image.dtype == g_params.dtype == torch.float32 and g_params.shape == params.shape
    worst = [_ratio("apply", out, c["out"], 4 * U * c["out_abs"]),
             _ratio("apply", g_image, c["g_image"], 4 * U * c["g_image_abs"]),
             _ratio("g_params", g_params, c["g_params"],
                    2 * U * c["g_params"].abs() + c["n"].double().view(-1, 1, 1) * 2.0 ** -52 * c["g_params_abs"])]
    idl = ER.resolve_ids(c["ids"], B, V)
    for b, v in enumerate(idl):
        if not 0 <= v < V:                                                    # out of range: passed through, bit for bit
            assert torch.equal(out[b].detach().cpu(), c["image"][b]) and torch.equal(g_image[b].cpu(), c["g_out"][b])
    for v in range(V):
        if v not in idl:
            assert not bool(g_params[v].any()), "a view that no entry references gets exactly 0"
        else:
            assert bool(g_params[v].any())
    # identity parameters: the image itself
    eye = ER.identity(V, torch.float32).to(hip_device)
    with torch.no_grad():
        assert torch.equal(E.apply_exposure(image, eye, ids), image.detach())
    assert max(worst) <= 1.0, worst


@gpu
@pytest.mark.parametrize("pattern", list(EC.PATTERNS))
@pytest.mark.parametrize("H,W", EC.SHAPES)
def test_fit_vs_float64(hip_device, H, W, pattern):
    from freesplat_amd import exposure as E
    worst = 0.0
    for mask_kind, nonfinite, ridge in EC.fit_cases(H, W):
        c = EC.fit_case(H, W, pattern, mask_kind, nonfinite, ridge)
        V = c["V"]
        mask = None if c["mask"] is None else c["mask"].to(hip_device)
        params, count, solved = E.fit_exposure(c["pred"].to(hip_device), c["target"].to(hip_device), mask, _ids(c["ids"], hip_device), V,
                                               ridge)
        assert params.dtype == torch.float32 and tuple(params.shape) == (V, 3, 4)
        assert count.dtype == torch.int64 and solved.dtype == torch.bool
        assert torch.equal(count.cpu(), c["count"]) and torch.equal(solved.cpu(), c["solved"]), (mask_kind, nonfinite, ridge)
        dead = ~c["solved"]
        assert torch.equal(params.cpu()[dead], ER.identity(int(dead.sum()), torch.float32)), "identity rows are exact"
        if bool(c["solved"].any()):
            live = c["solved"]
            ref = c["params"][live]
            scale = ref.abs().amax((1, 2)).clamp_min(1.0)
            bound = (2 * U + c["kappa"][live] * c["count"][live].double() * 2.0 ** -50) * scale
            worst = max(worst, _ratio("fit", params[live.to(hip_device)], ref, bound.view(-1, 1, 1).expand_as(ref)))
        if mask is not None:                                                  # the mask as uint8 and as float: the same bits
            for m in (mask.to(torch.uint8) * 3, mask.float() * 0.25):
                again = E.fit_exposure(c["pred"].to(hip_device), c["target"].to(hip_device), m, _ids(c["ids"], hip_device), V, ridge)
                assert all(torch.equal(a, b) for a, b in zip(again, (params, count, solved)))
    assert worst <= 1.0, worst


@gpu
def test_autograd_asks_for_what_is_needed_and_holds_nothing(hip_device, monkeypatch):
    """The gradients through apply_exposure are the library's; each needs_input_grad combination allocates (= writes) only what
    is asked; nothing outlives a call under no_grad or without an input that requires a gradient, and a pending backward holds
    references to the inputs only."""
    from freesplat_amd import _lib, exposure as E
    H, W = EC.LARGE
    c = EC.apply_case(H, W, "dup")
    ids, V = _ids(c["ids"], hip_device), c["V"]
    image, params, g_out = (c[k].to(hip_device) for k in ("image", "params", "g_out"))
    want_image, want_params = _lib_backward(image, params, ids, g_out)
    made, real = [], torch.empty

    def counting(*a, **k):
        t = real(*a, **k)
        made.append(t.numel() * t.element_size())
        return t
    monkeypatch.setattr(E.torch, "empty", counting)
    one = image.numel() * 4
    scratch = int(_lib.lib().fs_exposure_scratch_bytes(B, H, W))
    for rg_image, rg_params in ((True, True), (True, False), (False, True)):
        x, q = image.clone().requires_grad_(rg_image), params.clone().requires_grad_(rg_params)
        torch.cuda.synchronize()
        before, made[:] = torch.cuda.memory_allocated(hip_device), []
        out = E.apply_exposure(x, q, ids)
        torch.cuda.synchronize()
        assert out.grad_fn is not None and made == [one]
        assert torch.cuda.memory_allocated(hip_device) - before <= one + 4096     # the output alone: references, no copies
        made[:] = []
        grads = torch.autograd.grad(out, [t for t, rg in ((x, rg_image), (q, rg_params)) if rg], g_out)
        assert made == ([one] if rg_image else []) + ([V * 48, scratch] if rg_params else [])
        if rg_image:
            assert torch.equal(grads[0], want_image)
        if rg_params:
            assert torch.equal(grads[-1], want_params)
    alone = _lib_backward(image, params, ids, g_out, want_params=False)[0], _lib_backward(image, params, ids, g_out, want_image=False)[1]
    assert torch.equal(alone[0], want_image) and torch.equal(alone[1], want_params)
    x = image.clone().requires_grad_(True)
    torch.cuda.synchronize()
    before, made[:] = torch.cuda.memory_allocated(hip_device), []
    plain = E.apply_exposure(image, params, ids)                               # no input requires a gradient
    with torch.no_grad():
        quiet = E.apply_exposure(x, params.clone().requires_grad_(True), ids)  # grad mode off
    torch.cuda.synchronize()
    assert plain.grad_fn is None and quiet.grad_fn is None and not quiet.requires_grad and made == [one, one]
    del plain, quiet
    assert torch.cuda.memory_allocated(hip_device) - before <= V * 48 + 4096  # (the clone of the parameters may linger)


def _run_all(image, params, ids, g_out, pred, target, mask, V, ridge=1e-6):
    """Every output of the three entry points through the Python layer."""
    from freesplat_amd import exposure as E
    x, q = image.clone().requires_grad_(True), params.clone().requires_grad_(True)
    out = E.apply_exposure(x, q, ids)
    return (out.detach(),) + torch.autograd.grad(out, [x, q], g_out) + E.fit_exposure(pred, target, mask, ids, V, ridge)


@gpu
@pytest.mark.parametrize("H,W", [EC.SHAPES[3], EC.LARGE])
def test_determinism_runs_streams_and_batches(hip_device, H, W):
    """Two runs and a side stream: bit-equal in all outputs.  With distinct ids, each entry's out / g_image and each view's
    g_params / fitted row are bit-equal whether the batch is processed whole or one entry at a time."""
    a, f = EC.apply_case(H, W, "none"), EC.fit_case(H, W, "none", "blocks", True, 1e-6)
    V = 5
    ids = torch.tensor([3, 0, 4], dtype=torch.int64, device=hip_device)        # distinct, two views unreferenced
    params = EC.draw_params(V, EC.gen(H, W, 77)).to(hip_device)
    image, g_out, pred, target, mask = (t.to(hip_device) for t in (a["image"], a["g_out"], f["pred"], f["target"], f["mask"]))
    first = _run_all(image, params, ids, g_out, pred, target, mask, V)
    assert all(bool(t.any()) for t in first) and int(first[4].min()) == 0 and int(first[4].max()) > 0
    for x, y in zip(first, _run_all(image, params, ids, g_out, pred, target, mask, V)):
        assert torch.equal(x, y)
    side = torch.cuda.Stream(device=hip_device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = _run_all(image, params, ids, g_out, pred, target, mask, V)
    torch.cuda.current_stream().wait_stream(side)
    for x, y in zip(first, third):
        assert torch.equal(x, y)
    for k in range(B):
        s, v = slice(k, k + 1), int(ids[k])
        alone = _run_all(image[s], params, ids[s], g_out[s], pred[s], target[s], mask[s], V)
        assert torch.equal(alone[0], first[0][s]) and torch.equal(alone[1], first[1][s])
        for i in (2, 3, 4, 5):                                                # g_params, fitted params, count, solved: the view's row
            assert torch.equal(alone[i][v], first[i][v]), (k, i)


def _offset(t, elems=1):
    """A contiguous copy of `t` whose first element sits `elems` elements past a 256-byte aligned address."""
    buf = torch.empty(t.numel() + 64, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 256 == 0
    view = buf[elems: elems + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + elems * t.element_size()
    return view


@gpu
@pytest.mark.parametrize("H,W", [EC.SHAPES[6], EC.LARGE])
def test_arrays_4_bytes_off_a_16_byte_boundary_give_the_same_bits(hip_device, H, W):
    """The three entry points on buffers that start 4 bytes (the mask: 1 byte) past an aligned address, inputs and outputs
    alike, against the aligned run.  64 x 64 takes the vector path alone when aligned and the dword path alone when not."""
    from freesplat_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    a, f = EC.apply_case(H, W, "dup"), EC.fit_case(H, W, "dup", "blocks", True, 1e-6)
    V = a["V"]
    ids = _ids(a["ids"], hip_device)
    src = [t.to(hip_device) for t in (a["image"], a["params"], a["g_out"], f["pred"], f["target"], f["mask"].to(torch.uint8))]
    nbytes = L.fs_exposure_scratch_bytes(B, H, W)

    def run(place):
        image, params, g_out, pred, target, mask = (place(t) for t in src)
        out, g_image = place(torch.zeros_like(image)), place(torch.zeros_like(image))
        g_params, fitted = place(torch.zeros_like(params)), place(torch.zeros_like(params))
        count, solved = torch.zeros(V, dtype=torch.int64, device=hip_device), place(torch.zeros(V, dtype=torch.uint8, device=hip_device))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=hip_device)
        st = _lib.current_stream()
        _lib.check(L.fs_exposure_apply_forward(B, V, H, W, p(image), p(params), p(ids), p(out), st), "forward")
        _lib.check(L.fs_exposure_apply_backward(B, V, H, W, p(image), p(params), p(ids), p(g_out), p(g_image), p(g_params), p(scratch),
                                                st), "backward")
        _lib.check(L.fs_exposure_fit(B, V, H, W, p(pred), p(target), p(mask), p(ids), 1e-6, p(fitted), p(count), p(solved), p(scratch),
                                     st), "fit")
        torch.cuda.synchronize()
        return out, g_image, g_params, fitted, count, solved

    base = run(lambda t: t.clone())
    assert all(t.data_ptr() % 16 == 0 for t in base[:4]) and all(bool(t.any()) for t in base)
    assert torch.equal(base[4].cpu(), f["count"])
    for x, y in zip(base, run(_offset)):
        assert torch.equal(x, y)


@gpu
def test_graph_capture(hip_device):
    """Forward, backward and fit record into one graph (device ids: the host reads nothing) and replay to the same bits."""
    H, W = EC.LARGE
    a, f = EC.apply_case(H, W, "oor"), EC.fit_case(H, W, "oor", "blocks", True, 1e-6)
    V, ids = a["V"], _ids(a["ids"], hip_device)
    args = [t.to(hip_device) for t in (a["image"], a["params"])] + [ids] + \
           [t.to(hip_device) for t in (a["g_out"], f["pred"], f["target"], f["mask"])] + [V]
    step = lambda: _run_all(*args)
    side = torch.cuda.Stream(device=hip_device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                         # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        outs = step()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        got = [t.detach().clone() for t in outs]
        for x, y in zip(got, step()):
            assert torch.equal(x, y.detach())
    assert all(bool(t.any()) for t in got)


@gpu
def test_error_cases(hip_device):
    """The argument errors that need a device, and what legal inputs go through."""
    from freesplat_amd import exposure as E
    x = torch.rand(2, 3, 8, 9, device=hip_device)
    q = ER.identity(2, torch.float32).to(hip_device)
    bad_calls = [lambda: E.apply_exposure(x.cpu(), q), lambda: E.apply_exposure(x, q.cpu()), lambda: E.apply_exposure(x.double(), q),
                 lambda: E.apply_exposure(x, q.double()), lambda: E.apply_exposure(x[:, :2], q), lambda: E.apply_exposure(x[0], q),
                 lambda: E.apply_exposure(x, q[:, :, :3]), lambda: E.apply_exposure(x, q[:1]), lambda: E.apply_exposure(x[:0], q),
                 lambda: E.apply_exposure(x, q, [0, 2]), lambda: E.apply_exposure(x, q, [0, -1]), lambda: E.apply_exposure(x, q, [0]),
                 lambda: E.apply_exposure(x, q, torch.tensor([0, 5])), lambda: E.apply_exposure(x, q, torch.zeros(2, device=hip_device)),
                 lambda: E.apply_exposure(x, q, torch.zeros(3, dtype=torch.long, device=hip_device)),
                 lambda: E.fit_exposure(x, x[:, :, :7]), lambda: E.fit_exposure(x, x.cpu()), lambda: E.fit_exposure(x, x, x[:, 0].cpu()),
                 lambda: E.fit_exposure(x, x, x[:, 0, :7]), lambda: E.fit_exposure(x, x, ridge=-1.0),
                 lambda: E.fit_exposure(x, x, view_ids=torch.zeros(2, dtype=torch.long, device=hip_device)),
                 lambda: E.fit_exposure(x, x, num_views=3), lambda: E.fit_exposure(x, x, view_ids=[0, 1], num_views=0),
                 lambda: E.color_corrected(x, x.double())]
    if torch.cuda.device_count() > 1:
        bad_calls.append(lambda: E.apply_exposure(x, q.to("cuda:1")))
    for k, call in enumerate(bad_calls):
        with pytest.raises(ValueError, match=r"^freesplat_amd\.exposure: "):
            call()
            pytest.fail(f"call {k} was accepted")
    want = E.apply_exposure(x, q * 2.0, [1, 0])
    assert torch.equal(want, E.apply_exposure(x, q * 2.0, torch.tensor([1, 0], dtype=torch.int32, device=hip_device)))
    xt = x.transpose(2, 3).contiguous().transpose(2, 3)
    assert not xt.is_contiguous() and torch.equal(E.apply_exposure(xt, q * 2.0, (1, 0)), want)
    params, count, solved = E.fit_exposure(x, x * 0.5 + 0.1, view_ids=[1, 1])       # num_views from host ids
    assert tuple(params.shape) == (2, 3, 4) and count.tolist() == [0, 144] and solved.tolist() == [False, True]
    m = E.Exposure(3).to(hip_device)
    before = m.params.detach().clone()
    cnt = m.fit_(x, x * 0.5 + 0.1, view_ids=[2, 0])
    assert cnt.tolist() == [72, 0, 72] and torch.equal(m.params[1], before[1]) and m.params.requires_grad
    assert float((m.params[0, :, :3].detach() - 0.5 * torch.eye(3, device=hip_device)).abs().max()) < 1e-3
    assert float((m.params[2, :, 3].detach() - 0.1).abs().max()) < 1e-3


# ---- from the rasterizer to the photometric loss ---------------------------------------------------------------------------

@gpu
def test_through_the_rasterizer_and_the_photometric_loss(hip_device):
    """A 64-Gaussian scene at 32 x 32 in the (scales, rotations) form whose target is the render under a known gain / offset:
    fit_exposure recovers it within the fit bound, twenty Adam steps on Exposure.params alone through apply_exposure ->
    photometric_loss lower the loss monotonically after the first step, color_corrected raises the PSNR."""
    from freesplat_amd import exposure as E
    from freesplat_amd.metrics import compute_psnr
    from freesplat_amd.ssim_loss import photometric_loss
    from test_raster_scale_rot_alpha import _render, _scale_rot_for
    from util_raster import small_scene, view_inputs
    H = W = 32
    scene, cams = small_scene(N=64, H=H, W=W, seed=11)
    vi = view_inputs(scene, cams, 0, H, W)
    sc, rq = _scale_rot_for(vi, 4)
    (color, _, _, _), _ = _render(vi, hip_device, scales=sc, rotations=rq)
    render = color.detach()[None].contiguous()
    assert tuple(render.shape) == (1, 3, H, W) and float(render.std()) > 0.01
    gain = torch.tensor([[1.3, 0.05, 0.04], [-0.04, 0.8, 0.1], [0.05, 0.06, 1.2]])
    offset = torch.tensor([0.08, -0.06, 0.05])
    known = torch.cat([gain, offset[:, None]], 1)[None]
    target = E.apply_exposure(render, known.to(hip_device))
    # the fit against the restatement on the same fp32 images, and against what was put in
    params, count, solved = E.fit_exposure(render, target)
    ref, ref_count, ref_solved, kappa = ER.fit(render.cpu(), target.cpu())
    assert count.tolist() == ref_count.tolist() == [H * W] and solved.tolist() == ref_solved.tolist() == [True]
    bound = (2 * U + float(kappa[0]) * H * W * 2.0 ** -50) * max(float(ref.abs().max()), 1.0)
    err = float((params.double().cpu() - ref).abs().max())
    print(f"RATIO fit {err / bound:.4f} (kappa {float(kappa[0]):.3g})")
    assert err <= bound
    assert float((ref - known.double()).abs().max()) <= 1e-6 * float(kappa[0])    # the ridge pulls by about ridge * kappa at most
    # colour-corrected PSNR
    plain = compute_psnr(target.clamp(0, 1), render.clamp(0, 1))
    fixed = compute_psnr(target.clamp(0, 1), E.color_corrected(render, target).clamp(0, 1))
    assert float(fixed) > float(plain) + 10.0, (float(plain), float(fixed))
    # training the exposure alone
    m = E.Exposure(1).to(hip_device)
    opt = torch.optim.Adam([m.params], lr=1e-3)        # 20 steps move a parameter by 0.02 at most: none reaches its target
    losses = []
    for _ in range(21):
        loss = photometric_loss(m(render), target)
        losses.append(float(loss.detach()))
        opt.zero_grad()
        loss.backward()
        opt.step()
    assert all(b < a for a, b in zip(losses[1:], losses[2:])), losses
    assert losses[-1] < 0.9 * losses[0]


# ---- guard bands (tests/guarded_alloc.py, the harness of tests/test_memory_guards.py) ----

GUARDED = {
    "fs_exposure_apply_forward": "test_guard_bands",
    "fs_exposure_apply_backward": "test_guard_bands",
    "fs_exposure_fit": "test_guard_bands",
}


@gpu
@pytest.mark.parametrize("pattern", ["oor", "dup"])
@pytest.mark.parametrize("H,W", [EC.SHAPES[0], EC.SHAPES[2], EC.SHAPES[4], EC.SHAPES[6], EC.LARGE])
def test_guard_bands(hip_device, H, W, pattern):
    """All three entry points unguarded and under the fills ("ff", "zero", "garbage"): no guard byte changes, nothing non-finite,
    the same bits -- on the tail shapes, with the out-of-range ids and each subset of the gradients."""
    from freesplat_amd import exposure as E
    from test_memory_guards import _four
    a, f = EC.apply_case(H, W, pattern), EC.fit_case(H, W, pattern, "blocks", True, 1e-6)
    V = a["V"]
    ids = torch.tensor(a["ids"], dtype=torch.int64)

    def apply(place):
        x, q = place(a["image"], True), place(a["params"], True)
        out = E.apply_exposure(x, q, place(ids))
        g = place(a["g_out"])

        def bwd():
            return list(torch.autograd.grad(out, [x, q], g, retain_graph=True)) + list(torch.autograd.grad(out, [x], g, retain_graph=True)) + \
                list(torch.autograd.grad(out, [q], g))
        return [out], bwd
    base = _four(apply, hip_device, f"exposure apply {pattern} {H}x{W}")
    assert torch.equal(base[1][0], base[1][2]) and torch.equal(base[1][1], base[1][3])

    def fit(place):
        # (the inputs hold NaN and inf on purpose; the results are finite)
        return list(E.fit_exposure(place(f["pred"]), place(f["target"]), place(f["mask"]), place(ids), V)), None
    base = _four(fit, hip_device, f"exposure fit {pattern} {H}x{W}")
    assert torch.equal(base[0][1].cpu(), f["count"])

    def fit_without_mask(place):
        return list(E.fit_exposure(place(f["pred"]), place(f["target"]), None, place(ids), V)), None
    _four(fit_without_mask, hip_device, f"exposure fit without a mask {pattern} {H}x{W}")


def test_every_exposure_entry_point_with_a_device_buffer_has_a_guarded_case():
    from freesplat_amd import _lib
    with_buffers = sorted(n for n, (_, args) in _lib.EXPOSURE_SIGNATURES.items() if any(a is _lib._VP for a in args))
    assert with_buffers == sorted(GUARDED) and len(with_buffers) == 3
    me = sys.modules[__name__]
    for n, t in GUARDED.items():
        fn = getattr(me, t, None)
        assert callable(fn), (n, t)
        assert "gpu" in [m.name for m in getattr(fn, "pytestmark", [])], f"{n}: {t} is not a GPU case"
