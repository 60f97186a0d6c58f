"""GPU checks of TSDF fusion and mesh extraction (include/freesplat_amd_tsdf.h, csrc/tsdf.hip, freesplat_amd/tsdf.py) against the
fp32 restatement tests/tsdf_ref.py, bit for bit: integrate on every case of tests/tsdf_cases.py (one call and one call per
view), the extraction (live everywhere, unobserved regions, past the first scan level, empty, one cube), the same bits on
every run, on a side stream, at a 4-byte offset, with the brick-level view skip off and among views that do not see the
volume, graph capture, guard bands and poisoned buffers, and grid points no view reaches."""
import numpy as np
import pytest
import torch

import tsdf_cases as TC
import tsdf_ref as R
from guarded_alloc import guarded

pytestmark = pytest.mark.gpu
ALL = TC.CASES + [TC.BIG]
IDS = lambda cs: TC.case(*cs)["name"]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _same_bits(t, a):
    return np.array_equal(_bits(t), np.ascontiguousarray(a, np.float32).view(np.int32))


def _volume(c, dev, like=None):
    from freesplat_amd.tsdf import TSDFVolume
    v = c["vol"]
    vol = TSDFVolume(v["origin"], v["voxel_size"], v["dims"], v["trunc"], v["color"] is not None, v["max_weight"], device=dev)
    if like is not None:                                                     # start from the given arrays instead of an empty volume
        vol.tsdf.copy_(torch.from_numpy(like["tsdf"]))
        vol.weight.copy_(torch.from_numpy(like["weight"]))
        if vol.color is not None:
            vol.color.copy_(torch.from_numpy(like["color"]))
    return vol


def _integrate(vol, c, dev, lo=0, hi=None, place=lambda t: t, device_extrinsics=False, flags=0):
    views = TC.view_slice(c["views"], lo, hi)
    t = lambda k: None if views[k] is None else place(torch.from_numpy(views[k]).to(dev))
    E = torch.from_numpy(c["c2w"][lo:hi])
    vol.integrate(t("depth"), t("intrinsics"), E.to(dev) if device_extrinsics else E, image=t("image"), alpha=t("alpha"), _flags=flags,
                  **{k: views[k] for k in TC.SCALARS})


def _assert_volume(vol, want, what):
    assert _same_bits(vol.tsdf, want["tsdf"]), f"{what}: tsdf"
    assert _same_bits(vol.weight, want["weight"]), f"{what}: weight"
    if want["color"] is not None:
        assert _same_bits(vol.color, want["color"]), f"{what}: color"


def _shifted(t, device):
    """A copy of t that starts one float past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 5, dtype=torch.float32, device=device)
    off = 1 + (-(buf.data_ptr() // 4) % 4)
    assert (buf.data_ptr() + 4 * off) % 16 == 4
    v = buf[off: off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


# ---- 1. integrate ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cs", ALL, ids=IDS)
def test_integrate_matches_the_restatement_bit_for_bit(hip_device, cs):
    """One call with all V views (V = MAX + 1: two library calls through the Python layer's chunking) and V one-view calls."""
    c = TC.case(*cs)
    want, _, _ = TC.fused(cs)
    assert float(want["weight"].max()) > 0
    vol = _volume(c, hip_device)
    _integrate(vol, c, hip_device)
    _assert_volume(vol, want, "one call")
    vol.reset()
    for v in range(cs[2]):
        _integrate(vol, c, hip_device, v, v + 1)
    _assert_volume(vol, want, "one call per view")


# ---- 2. extract -----------------------------------------------------------------------------------------------------------------

def _extract_and_compare(vol_np, dev, min_weight=1.0):
    from freesplat_amd.tsdf import extract_mesh
    d = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)
    verts, cols = extract_mesh(d(vol_np["tsdf"]), d(vol_np["weight"]), d(vol_np["color"]), vol_np["origin"], vol_np["voxel_size"], min_weight)
    want_v, want_c = R.extract(vol_np, min_weight)
    assert tuple(verts.shape) == tuple(want_v.shape), (tuple(verts.shape), want_v.shape)
    assert _same_bits(verts, want_v), "vertices"
    assert (cols is None) == (want_c is None)
    if cols is not None:
        assert tuple(cols.shape) == tuple(want_c.shape) and _same_bits(cols, want_c), "colours"
    return verts, cols


@pytest.mark.parametrize("cs", [TC.CASES[-1], TC.CASES[5], TC.CASES[3], TC.BIG], ids=IDS)
def test_extract_matches_the_restatement_bit_for_bit_and_in_order(hip_device, cs):
    """The fused volumes of the cases: exact zeros on grid points (zero-area triangles), colour, unobserved regions, and a volume
    whose block counts need the scan's second level."""
    vol, _, _ = TC.fused(cs)
    verts, _ = _extract_and_compare(vol, hip_device)
    assert verts.shape[0] > 0 and bool((vol["weight"] == 0).any())
    if cs is TC.CASES[-1]:
        a, b, c = (verts[:, i].cpu().double() for i in range(3))
        assert int((torch.linalg.cross(b - a, c - a).norm(dim=1) == 0).sum()) > 0


def test_extract_live_everywhere_empty_and_one_cube(hip_device):
    rng = np.random.default_rng(5)
    live = R.new_volume((0.3, -0.2, 1.0), 0.07, (37, 10, 6), 0.2, 64.0, True)
    live["tsdf"] = rng.uniform(-1, 1, live["tsdf"].shape).astype(np.float32)
    live["weight"] = rng.integers(1, 4, live["weight"].shape).astype(np.float32)
    live["color"] = rng.random(live["color"].shape).astype(np.float32)
    verts, _ = _extract_and_compare(live, hip_device)
    assert verts.shape[0] > 36 * 9 * 5                                          # (a random field cuts nearly every cube)
    starved = dict(live, weight=live["weight"].copy())
    assert _extract_and_compare(starved, hip_device, min_weight=2.0)[0].shape[0] < verts.shape[0]
    for empty in (dict(live, tsdf=np.abs(live["tsdf"]) + 0.1), dict(live, weight=np.zeros_like(live["weight"])),
                  dict(live, tsdf=np.zeros_like(live["tsdf"]))):               # all outside; nothing observed; exact zeros: outside
        v, c = _extract_and_compare(empty, hip_device)
        assert tuple(v.shape) == (0, 3, 3) and tuple(c.shape) == (0, 3, 3)
    for dims in ((2, 2, 2), (1, 5, 4), (5, 1, 1)):
        one = R.new_volume((0.0, 0.0, 0.0), 0.5, dims, 1.0, 64.0, False)
        one["tsdf"] = rng.uniform(-1, 1, one["tsdf"].shape).astype(np.float32)
        one["tsdf"].reshape(-1)[0] = -0.5
        one["tsdf"].reshape(-1)[-1] = 0.5
        one["weight"][...] = 1.0
        v, _ = _extract_and_compare(one, hip_device)
        assert (v.shape[0] > 0) == (dims == (2, 2, 2))


def test_weld_on_the_device_gives_a_closed_mesh(hip_device):
    """A sphere's analytic field (no fusion): extract, weld and drop on the device; every directed edge once, its reverse once."""
    from freesplat_amd.tsdf import extract_mesh, weld
    n, r = 20, 6.3
    vol = R.new_volume((0.0, 0.0, 0.0), 1.0, (n, n, n), 3.0, 64.0, True)
    g = np.arange(n, dtype=np.float64)
    dist = np.sqrt((g[None, None, :] - 9.37) ** 2 + (g[None, :, None] - 9.62) ** 2 + (g[:, None, None] - 9.45) ** 2) - r
    vol["tsdf"] = np.clip(dist / 3.0, -1, 1).astype(np.float32)
    vol["weight"][...] = 1.0
    vol["color"] = np.random.default_rng(6).random(vol["color"].shape).astype(np.float32)
    verts, cols = _extract_and_compare(vol, hip_device)
    V, F, Cc = weld(verts, cols)
    assert V.is_cuda and F.is_cuda and Cc.shape == V.shape
    rep = R.mesh_report(V.cpu().numpy(), F.cpu().numpy())
    print(f"sphere of radius {r} voxels: {verts.shape[0]} triangles, {F.shape[0]} faces after weld, {rep}")
    assert rep["bad_edges"] == 0 and rep["euler"] == 2 and rep["volume"] > 0
    Vr, Fr = R.weld(verts.cpu().numpy())
    assert V.shape[0] == Vr.shape[0] and np.array_equal(V.cpu().numpy()[F.cpu().numpy()], Vr[Fr])


# ---- 3. the same bits across conditions -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("cs", [TC.CASES[1], TC.CASES[3], TC.CASES[4], TC.CASES[5]], ids=IDS)
def test_runs_streams_alignments_the_skip_and_added_views_give_the_same_bits(hip_device, cs):
    from freesplat_amd import _lib
    c = TC.case(*cs)
    want, _, _ = TC.fused(cs)
    shift = lambda t: _shifted(t, hip_device)

    vol = _volume(c, hip_device)
    _integrate(vol, c, hip_device)
    _assert_volume(vol, want, "a second run")

    vol = _volume(c, hip_device)
    _integrate(vol, c, hip_device, flags=_lib.TSDF_NO_BRICK_SKIP)
    _assert_volume(vol, want, "without the brick-level view skip")

    vol = _volume(c, hip_device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _integrate(vol, c, hip_device)
    torch.cuda.current_stream().wait_stream(side)
    _assert_volume(vol, want, "another stream")

    vol = _volume(c, hip_device)
    vol.tsdf, vol.weight = shift(vol.tsdf), shift(vol.weight)
    if vol.color is not None:
        vol.color = shift(vol.color)
    _integrate(vol, c, hip_device, place=shift)
    _assert_volume(vol, want, "every array one float past a 16-byte boundary")

    # the same views among added ones that do not see the volume: one looks away, one looks at it from the side with its
    # principal point far off the map
    V = cs[2]
    if V + 2 <= TC.MAX_VIEWS:
        views, c2w = dict(c["views"]), c["c2w"]
        away = c2w[0].copy()
        away[:3, 0], away[:3, 2] = -away[:3, 0], -away[:3, 2]
        order = [V, *range(V), V + 1]
        more = dict(c, c2w=np.concatenate([c2w, away[None], c2w[:1]])[order])
        k_off = views["intrinsics"][0].copy()
        k_off[2] += 1e4
        pick = lambda a, extra: None if a is None else np.concatenate([a, a[:1], extra])[order]
        views["world_to_cam"] = pick(views["world_to_cam"], views["world_to_cam"][:1])      # (not read: the layer takes c2w)
        views["intrinsics"] = pick(views["intrinsics"], k_off[None])
        for k in ("depth", "alpha", "image"):
            views[k] = pick(views[k], None if views[k] is None else views[k][:1])
        more["views"] = views
        vol = _volume(c, hip_device)
        _integrate(vol, more, hip_device)
        _assert_volume(vol, want, "among views that do not see the volume")


# ---- 4. graph capture -----------------------------------------------------------------------------------------------------------

def test_integrate_is_capturable(hip_device):
    """integrate with device extrinsics (no host synchronisation) captured in a graph and replayed on new depth values: the bits
    of the restatement for the new values (world_to_cam as the layer's device path forms it)."""
    from freesplat_amd.tsdf import world_to_cam
    cs = TC.CASES[4]
    c = TC.case(*cs)
    views = c["views"]
    depth2 = (views["depth"] * np.float32(1.01)).astype(np.float32)
    E = torch.from_numpy(c["c2w"]).to(hip_device)
    w2c = world_to_cam(E, hip_device).cpu().numpy()
    want = R.copy_volume(c["vol"])
    R.integrate(want, dict(views, depth=depth2, world_to_cam=w2c))
    first = R.copy_volume(c["vol"])
    R.integrate(first, dict(views, world_to_cam=w2c))
    assert not np.array_equal(first["tsdf"], want["tsdf"])

    vol = _volume(c, hip_device)
    depth = torch.from_numpy(views["depth"]).to(hip_device)
    intr, image = torch.from_numpy(views["intrinsics"]).to(hip_device), torch.from_numpy(views["image"]).to(hip_device)
    run = lambda: vol.integrate(depth, intr, E, image=image, **{k: views[k] for k in TC.SCALARS})
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _assert_volume(vol, first, "eager, device extrinsics")
    graph = torch.cuda.CUDAGraph()
    vol.reset()
    with torch.cuda.graph(graph):
        run()
    vol.reset()
    depth.copy_(torch.from_numpy(depth2))
    graph.replay()
    torch.cuda.synchronize()
    _assert_volume(vol, want, "replayed on new depth values")
    vol.reset()
    graph.replay()
    torch.cuda.synchronize()
    _assert_volume(vol, want, "replayed again")


# ---- 5. guard bands -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fill", ["ff", "garbage"])
@pytest.mark.parametrize("cs", [TC.CASES[0], TC.CASES[1], TC.CASES[2], TC.CASES[3], TC.CASES[5]], ids=IDS)
def test_nothing_is_written_outside_a_buffer(hip_device, fill, cs):
    """fs_tsdf_integrate, fs_tsdf_mesh_plan and fs_tsdf_mesh_emit with every buffer the Python layer allocates (the volume, the
    scratch, the total, the soup) between guard bands and poisoned, inputs between NaN guards: no guard byte changes, and the
    results are the restatement's bits (no poison reaches them)."""
    from freesplat_amd.tsdf import extract_mesh
    c = TC.case(*cs)
    want, _, _ = TC.fused(cs)
    with guarded(fill) as arena:
        vol = _volume(c, hip_device)                                         # (reset() overwrites the poison, as for any caller)
        _integrate(vol, c, hip_device, place=arena.place)
        torch.cuda.synchronize()
        arena.check("fs_tsdf_integrate")
        _assert_volume(vol, want, "guarded")
        verts, cols = vol.extract_mesh()
        torch.cuda.synchronize()
        arena.check("fs_tsdf_mesh_plan / fs_tsdf_mesh_emit")
        want_v, want_c = R.extract(want)
        assert tuple(verts.shape) == tuple(want_v.shape) and _same_bits(verts, want_v)
        if want_c is not None:
            assert _same_bits(cols, want_c)
        d = lambda a: None if a is None else arena.place(torch.from_numpy(np.array(a)).to(hip_device))
        verts2, _ = extract_mesh(d(want["tsdf"]), d(want["weight"]), d(want["color"]), want["origin"], want["voxel_size"])
        torch.cuda.synchronize()
        arena.check("extract_mesh on placed inputs")
        assert _same_bits(verts2, want_v)
    assert len(arena.records) >= 6


def test_the_python_layer_refuses_what_it_cannot_fuse(hip_device):
    """The argument errors of integrate that need a volume on a device, and from_bounds."""
    from freesplat_amd.tsdf import TSDFVolume
    vol = TSDFVolume.from_bounds((-0.5, 0.0, 1.0), (0.5, 0.35, 1.21), 0.1, color=True, device=hip_device)
    assert vol.dims == (11, 5, 4) and vol.trunc == float(np.float32(4 * np.float32(0.1))) and vol.color.shape == (3, 4, 5, 11)
    assert float(vol.tsdf.min()) == 1.0 and not bool(vol.weight.any()) and not bool(vol.color.any())
    assert torch.equal(vol.grid_points()[0, 0, :, 0].cpu(), torch.tensor(R.grid_axes(dict(origin=vol.origin, voxel_size=vol.voxel_size,
                                                                                          dims=vol.dims), np.float32)[0]))
    d, im = torch.ones(2, 6, 8, device=hip_device), torch.ones(2, 3, 6, 8, device=hip_device)
    k, E = (8.0, 8.0, 3.5, 2.5), torch.eye(4).repeat(2, 1, 1)
    vol.integrate(d, k, E, image=im)
    assert float(vol.weight.max()) == 2.0
    for bad in (lambda: vol.integrate(d, k, E), lambda: vol.integrate(d.cpu(), k, E, image=im), lambda: vol.integrate(d[0], k, E, image=im),
                lambda: vol.integrate(d, k, E, image=im[:, :2]), lambda: vol.integrate(d, k, E, image=im, alpha=d[:1]),
                lambda: vol.integrate(d, (8.0, 8.0, 3.5), E, image=im), lambda: vol.integrate(d, k, E[:1], image=im),
                lambda: vol.integrate(d, k, E, image=im, alpha_floor=0.0), lambda: vol.integrate(d, k, E, image=im, near=float("nan")),
                lambda: vol.integrate(d, k, E, image=im, max_depth=float("nan"))):
        with pytest.raises(ValueError, match="freesplat_amd.tsdf"):
            bad()
    with pytest.raises(RuntimeError, match="depth gets no gradient"):
        vol.integrate(d.clone().requires_grad_(True), k, E, image=im)
    plain = TSDFVolume((0, 0, 0), 0.1, (4, 4, 4), device=hip_device)
    with pytest.raises(ValueError, match="colour"):
        plain.integrate(d, k, E, image=im)
    assert float(vol.weight.max()) == 2.0                                    # (a refused call fuses nothing)


# ---- 6. grid points no view reaches ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cs", [TC.CASES[3], TC.CASES[4], TC.CASES[-1]], ids=IDS)
def test_a_grid_point_no_view_updates_keeps_its_bits(hip_device, cs):
    """The volume pre-filled with a pattern (finite values of both signs, -0.0, weights 0 .. 3): after the call the restatement's
    bits everywhere, and where no view updated a point the pattern's bits."""
    c = TC.case(*cs)
    _, codes, _ = TC.fused(cs)
    rng = np.random.default_rng(7)
    start = R.copy_volume(c["vol"])
    start["tsdf"] = rng.uniform(-3, 3, start["tsdf"].shape).astype(np.float32)
    start["tsdf"].reshape(-1)[::5] = -0.0
    start["weight"] = rng.integers(0, 4, start["weight"].shape).astype(np.float32)
    if start["color"] is not None:
        start["color"] = rng.uniform(-1, 2, start["color"].shape).astype(np.float32)
    want = R.copy_volume(start)
    R.integrate(want, c["views"])
    vol = _volume(c, hip_device, like=start)
    _integrate(vol, c, hip_device)
    _assert_volume(vol, want, "pre-filled")
    untouched = ~(codes == R.UPDATED).any(0)
    assert bool(untouched.any()) and not bool(untouched.all())
    pat = start["tsdf"].view(np.int32)
    assert np.array_equal(_bits(vol.tsdf)[untouched], pat[untouched])
    assert np.array_equal(_bits(vol.weight)[untouched], start["weight"].view(np.int32)[untouched])
    if start["color"] is not None:
        assert np.array_equal(_bits(vol.color)[:, untouched], start["color"].view(np.int32)[:, untouched])
