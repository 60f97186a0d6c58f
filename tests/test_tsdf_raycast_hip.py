"""GPU checks of TSDF ray casting (include/freesplat_ext_raycast.h, csrc/tsdf_raycast.hip, freesplat_amd/tsdf.py) against the fp32
restatement tests/tsdf_raycast_ref.py, bit for bit on every pixel of every case of tests/tsdf_raycast_cases.py (NaN compared as
"both NaN"): the same bits on a second run, on a side stream, with every array one float past a 16-byte boundary, for a view
alone and inside its batch, with and without each optional output; graph capture with device extrinsics; guard bands and
poisoned buffers; the normal convention against depth_normals; the integrate -> ray cast -> integrate round trip."""
import numpy as np
import pytest
import torch

import tsdf_raycast_cases as RC
import tsdf_raycast_ref as RR
from guarded_alloc import guarded

pytestmark = pytest.mark.gpu
EVERY = [(n, ()) for n in RC.NAMES] + RC.MORE
IDS = lambda x: x[0] + "".join(f" {k}={v}" for k, v in x[1])


def _same(got, want):
    """The same bits, a NaN in `want` matching any NaN."""
    g = got.detach().cpu().contiguous().numpy()
    w = np.ascontiguousarray(want, g.dtype)
    if g.shape != w.shape:
        return False
    if g.dtype == np.int32:
        return np.array_equal(g, w)
    nan = np.isnan(w)
    return np.array_equal(np.isnan(g), nan) and np.array_equal(g.view(np.int32)[~nan], w.view(np.int32)[~nan])


def _dev(a, dev, place=lambda t: t):
    return None if a is None else place(torch.from_numpy(np.array(a)).to(dev))


def _cast(c, dev, override=(), place=lambda t: t, views=slice(None), device_extrinsics=False, **outputs):
    from freesplat_amd.tsdf import raycast
    v = c["vol"]
    E = torch.from_numpy(c["c2w"][views])
    kw = dict(c["params"], return_steps=True)
    kw.update(dict(override), **outputs)
    return raycast(_dev(v["tsdf"], dev, place), _dev(v["weight"], dev, place), _dev(v["color"], dev, place), v["origin"], v["voxel_size"],
                   v["trunc"], _dev(c["intrinsics"][views], dev, place), E.to(dev) if device_extrinsics else E, c["hw"], **kw)


def _assert_result(got, want, what, views=slice(None)):
    assert _same(got.depth, want["depth"][views]), f"{what}: depth"
    if got.normals is not None:
        assert _same(got.normals, want["normals"][views]), f"{what}: normals"
    if got.color is not None:
        assert _same(got.color, want["color"][views]), f"{what}: color"
    if got.steps is not None:
        assert _same(got.steps, want["steps"][views]), f"{what}: steps"


def _shifted(t, device):
    """A copy of t that starts one float past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 5, dtype=t.dtype, device=device)
    off = 1 + (-(buf.data_ptr() // 4) % 4)
    assert (buf.data_ptr() + 4 * off) % 16 == 4
    v = buf[off: off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


# ---- 1. every case ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cs", EVERY, ids=IDS)
def test_raycast_matches_the_restatement_bit_for_bit(hip_device, cs):
    name, override = cs
    c, want = RC.case(name), RC.reference(name, np.float32, override)
    got = _cast(c, hip_device, override)
    assert (got.color is not None) == (c["vol"]["color"] is not None) and got.normals is not None and got.steps.dtype == torch.int32
    _assert_result(got, want, name)


# ---- 2. the same bits across conditions -----------------------------------------------------------------------------------------

VARIED = ["(5,3,2) 5x7 V=3 fusing/inside/away", "(70,17,9) 17x33 V=3 fusing/between/away", "holes 17x33 axis-parallel", "sphere 17x33"]


@pytest.mark.parametrize("name", VARIED)
def test_runs_streams_alignments_batches_and_outputs_give_the_same_bits(hip_device, name):
    from freesplat_amd import _lib
    c, want = RC.case(name), RC.reference(name)
    _assert_result(_cast(c, hip_device), want, "a second run")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = _cast(c, hip_device)
    torch.cuda.current_stream().wait_stream(side)
    _assert_result(got, want, "another stream")

    # every array of the library call, outputs included, one float past a 16-byte boundary
    v, (H, W), V = c["vol"], c["hw"], c["rows"].shape[0]
    shift = lambda a: None if a is None else _shifted(torch.from_numpy(np.array(a)).to(hip_device), hip_device)
    f, w, col, rows, k = shift(v["tsdf"]), shift(v["weight"]), shift(v["color"]), shift(c["rows"]), shift(c["intrinsics"])
    depth, nrm = _shifted(torch.empty(V, H, W, device=hip_device), hip_device), _shifted(torch.empty(V, 3, H, W, device=hip_device), hip_device)
    out_col = None if col is None else _shifted(torch.empty(V, 3, H, W, device=hip_device), hip_device)
    steps = _shifted(torch.empty(V, H, W, dtype=torch.int32, device=hip_device), hip_device)
    kw = dict(dict(min_depth=0.0, max_depth=float("inf"), min_weight=1.0, step_min=0.5, relax=0.8, refine=4, max_steps=4 * sum(v["dims"])),
              **c["params"])
    p = _lib.ptr
    _lib.launch("fs_tsdf_raycast", *v["dims"], *v["origin"], v["voxel_size"], v["trunc"], p(f), p(w), p(col), V, H, W, p(rows), p(k),
                kw["min_depth"], kw["max_depth"], kw["min_weight"], kw["step_min"], kw["relax"], kw["refine"], kw["max_steps"], p(depth),
                p(nrm), p(out_col), p(steps))
    from freesplat_amd.tsdf import RayCast
    _assert_result(RayCast(depth, nrm, out_col, steps), want, "every array one float past a 16-byte boundary")

    for i in range(V):                                                        # a view alone against the view inside its batch
        _assert_result(_cast(c, hip_device, views=slice(i, i + 1)), want, f"view {i} alone", slice(i, i + 1))

    has_color = v["color"] is not None
    for normals, color, steps_ in ((False, False, False), (True, False, False), (False, has_color, False), (False, False, True)):
        got = _cast(c, hip_device, normals=normals, color_out=color, return_steps=steps_)
        assert (got.normals is not None) == normals and (got.color is not None) == color and (got.steps is not None) == steps_
        _assert_result(got, want, f"normals={normals} color={color} steps={steps_}")


# ---- 3. graph capture ------------------------------------------------------------------------------------------------------------

def test_raycast_is_capturable_and_follows_the_camera_table(hip_device):
    """raycast with device extrinsics (no host synchronisation) captured in a graph; the camera table's contents are replaced and
    the graph replayed: the restatement's bits for the new cameras."""
    from freesplat_amd.tsdf import TSDFVolume
    first = RC.case("sphere 17x33")
    E2 = first["c2w"].copy()
    E2[0, :3, 3] += np.array([0.07, -0.05, 0.11])
    rows2 = np.ascontiguousarray(E2[:, :3]).astype(np.float32)
    want1 = RC.reference("sphere 17x33")
    want2 = RR.raycast(first["vol"], rows2, first["intrinsics"], first["hw"], **first["params"])
    assert not np.array_equal(want1["depth"], want2["depth"])

    v = first["vol"]
    vol = TSDFVolume(v["origin"], v["voxel_size"], v["dims"], v["trunc"], False, v["max_weight"], device=hip_device)
    vol.tsdf.copy_(torch.from_numpy(np.array(v["tsdf"])))
    vol.weight.copy_(torch.from_numpy(np.array(v["weight"])))
    E = torch.from_numpy(first["c2w"]).to(hip_device)
    k = torch.from_numpy(first["intrinsics"]).to(hip_device)
    run = lambda: vol.raycast(k, E, first["hw"], return_steps=True, **first["params"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _assert_result(got, want1, "eager, device extrinsics")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = run()
    E.copy_(torch.from_numpy(E2))
    graph.replay()
    torch.cuda.synchronize()
    _assert_result(got, want2, "replayed on new cameras")
    graph.replay()
    torch.cuda.synchronize()
    _assert_result(got, want2, "replayed again")


# ---- 4. guard bands --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fill", ["ff", "garbage"])
@pytest.mark.parametrize("name", ["one cell 1x1", "(5,3,2) 5x7 V=3 fusing/inside/away", "no cell (5,1,4) 5x7", "holes 17x33 axis-parallel",
                                  "(33,9,5) 17x33 V=3 refine=0"])
def test_nothing_is_written_outside_an_output_and_every_element_is_written(hip_device, fill, name):
    """Every output between guard bands and pre-filled with poison (0xFF bytes: NaN / -1; or garbage), every input between NaN
    guards: no guard byte changes, every output element holds the restatement's bits (so none kept its poison and no poison was
    read into a result), and the volume's bits are untouched."""
    c, want = RC.case(name), RC.reference(name)
    placed = []
    with guarded(fill) as arena:
        def place(t):
            placed.append((arena.place(t), t))
            return placed[-1][0]
        got = _cast(c, hip_device, place=place)
        torch.cuda.synchronize()
        arena.check("fs_tsdf_raycast")
        _assert_result(got, want, f"guarded, fill {fill}")
        for inside, original in placed:
            assert torch.equal(inside.view(torch.int32), original.view(torch.int32))
    assert len(arena.records) >= 6 and len(placed) >= 3


def test_the_python_layer_refuses_what_it_cannot_cast(hip_device):
    from freesplat_amd.tsdf import TSDFVolume
    vol = TSDFVolume((-0.5, -0.5, 1.0), 0.1, (11, 11, 6), color=True, device=hip_device)
    plain = TSDFVolume((-0.5, -0.5, 1.0), 0.1, (11, 11, 6), device=hip_device)
    k, E = (8.0, 8.0, 3.5, 2.5), torch.eye(4).repeat(2, 1, 1)
    out = vol.raycast(k, E, (6, 8))
    assert tuple(out.depth.shape) == (2, 6, 8) and tuple(out.normals.shape) == (2, 3, 6, 8) == tuple(out.color.shape) and out.steps is None
    assert not bool(out.depth.any()) and bool(out.normals.isnan().all()) and not bool(out.color.any())      # an empty volume: no hit
    assert plain.raycast(k, E, (6, 8), normals=False).normals is None and plain.raycast(k, E, (6, 8)).color is None
    for bad in (lambda: vol.raycast((8.0, 8.0, 3.5), E, (6, 8)), lambda: vol.raycast(torch.ones(3, 4), E, (6, 8)),
                lambda: vol.raycast(k, E[0], (6, 8)), lambda: vol.raycast(k, E, (6, 0)), lambda: plain.raycast(k, E, (6, 8), color=True),
                lambda: vol.raycast(k, E, (6, 8), refine=40), lambda: vol.raycast(k, E, (6, 8), step_min=0.0)):
        with pytest.raises(ValueError, match="freesplat_amd.tsdf"):
            bad()
    bad_E = E.clone()
    bad_E[0, 3, 3] = 2.0
    with pytest.raises(ValueError, match="last row"):
        vol.raycast(k, bad_E, (6, 8))
    with pytest.raises(RuntimeError, match="intrinsics gets no gradient"):
        vol.raycast(torch.tensor(k).requires_grad_(True), E, (6, 8))


# ---- 5. conventions --------------------------------------------------------------------------------------------------------------

def test_normals_follow_the_convention_of_depth_normals(hip_device):
    """The plane scene from the 25-degree camera: where a pixel's 3 x 3 neighbourhood is all hits, the ray cast's normals and
    depth_normals of the ray cast's depth agree within 1e-3 per component.  A sign and frame check: both sides are within 1e-5 of
    the analytic normal (tests/test_tsdf_raycast_host.py), so the margin is wide on purpose."""
    from freesplat_amd.normals_loss import depth_normals
    c = RC.case("plane 48x64 turned 25 degrees")
    got = _cast(c, hip_device, (("refine", 4),))
    k = torch.from_numpy(c["intrinsics"]).to(hip_device)
    from_depth = depth_normals(got.depth, k, smoothing=None)
    hit = (got.depth > 0).float()[:, None]
    all_hits = (-torch.nn.functional.max_pool2d(-hit, 3, stride=1, padding=1))[:, 0] == 1.0       # (a min-pool: the padding is -inf)
    all_hits[:, [0, -1]] = False
    all_hits[:, :, [0, -1]] = False
    assert int(all_hits.sum()) > 1500
    sel = all_hits[:, None].expand_as(got.normals)
    diff = (got.normals - from_depth)[sel]
    assert not bool(diff.isnan().any())
    print(f"normals against depth_normals on {int(all_hits.sum())} pixels: max |difference| = {float(diff.abs().max()):.2e}")
    assert float(diff.abs().max()) <= 1e-3
    assert float(got.normals[:, 2][all_hits].min()) > 0.5


def test_integrate_raycast_integrate_round_trip(hip_device):
    """Three views of a tilted plane fused, ray cast from the fusing cameras, the ray-cast depth fused into a fresh volume: where
    both volumes have weight and |tsdf| < 0.5 the values differ by less than voxel_size / trunc (one voxel).  The output is
    z-depth in integrate's convention, and (cx, cy) mean the same on both sides."""
    from freesplat_amd.tsdf import TSDFVolume
    v, c2w, intr, depth = RC.tilted_plane_scene()
    make = lambda: TSDFVolume(v["origin"], v["voxel_size"], v["dims"], v["trunc"], False, v["max_weight"], device=hip_device)
    E, k = torch.from_numpy(c2w), torch.from_numpy(intr).to(hip_device)
    one, two = make(), make()
    one.integrate(torch.from_numpy(depth).to(hip_device), k, E, near=0.05)
    cast = one.raycast(k, E, depth.shape[1:])
    assert float((cast.depth > 0).float().mean()) > 0.05
    two.integrate(cast.depth, k, E, near=0.05)
    both = (one.weight > 0) & (two.weight > 0) & (one.tsdf.abs() < 0.5)
    diff = float((one.tsdf - two.tsdf)[both].abs().max())
    print(f"round trip: {int(both.sum())} grid points compared, max |tsdf difference| = {diff:.3f} (bound {v['voxel_size'] / v['trunc']:.3f})")
    assert int(both.sum()) > 3000 and diff < v["voxel_size"] / v["trunc"]
