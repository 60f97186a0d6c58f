"""Forward blend, scan-first batches: a quadrant's wavefront scans the tile list 64 words at a time, queues the entries
that carry its quadrant bit (hits) and gathers / compacts / blends them in batches of 64 HITS.  Every case is compared
with the CPU oracle bit for bit (contract exp): colour, depth, alpha from the inference kernel and the tracking kernel,
final_T and n_contrib (the position in the tile's FULL list, where the backward starts) from the tracking kernel.
The constructed scenes place small isotropic Gaussians at chosen pixels of a 16x16 image (one tile), so that the number
of hits of one quadrant is known; it is checked on the CPU from the oracle's list and the saved list's masks first.
"""
import numpy as np
import pytest
import torch

from util_raster import hip_forward, oracle_forward, small_scene, view_inputs

pytestmark = pytest.mark.gpu


def _cull(monkeypatch, on):
    from freesplat_amd import rasterizer as R
    monkeypatch.setattr(R, "TILE_CULL", on)


def _compare(vi, device, lists=True):
    """Inference and tracking kernels against the oracle; returns (oracle state, debug state of the tracking run)."""
    from freesplat_amd.rasterizer import debug_state
    st = oracle_forward(vi)
    for grad in (False, True):
        (color, radii, depth, alpha), _ = hip_forward(vi, device, requires_grad=grad)
        np.testing.assert_array_equal(color.detach().cpu().numpy(), st["color"])
        np.testing.assert_array_equal(depth.detach().cpu().numpy(), st["depth"])
        np.testing.assert_array_equal(alpha.detach().cpu().numpy(), st["alpha"])
    dbg = debug_state(color.grad_fn.rs)
    np.testing.assert_array_equal(dbg["final_T"], st["final_T"])
    if lists:   # (culling off: the saved list is the oracle's, so are the positions in it)
        np.testing.assert_array_equal(dbg["point_list"], st["point_list"])
        np.testing.assert_array_equal(dbg["n_contrib"], st["n_contrib"])
    return st, dbg


def _placed(px, py, z, sigma, opacity, H=16, W=16, seed=0, bg=(0.1, 0.2, 0.3)):
    """Rasterizer inputs with one isotropic Gaussian per entry of (px, py, z): centre at pixel (px, py), depth z,
    screen-space standard deviation sigma pixels (the 0.3 px^2 low-pass included), degree-0 colours."""
    scene, cams = small_scene(N=8, H=H, W=W, seed=3)
    vi = view_inputs(scene, cams, 0, H, W, bg=bg)
    px, py, z = (np.asarray(a, np.float64) for a in (px, py, z))
    n = len(px)
    sigma, opacity = np.broadcast_to(sigma, n).astype(np.float64), np.broadcast_to(opacity, n).astype(np.float64)
    xv = ((2 * px + 1) / W - 1) * vi["tanfovx"] * z
    yv = ((2 * py + 1) / H - 1) * vi["tanfovy"] * z
    view = vi["viewmatrix"].double().numpy()           # row vectors: p_view = [p, 1] @ view
    world = np.stack([xv, yv, z, np.ones(n)], -1) @ np.linalg.inv(view)
    s2 = (z * np.sqrt(sigma ** 2 - 0.3) / (W / (2 * vi["tanfovx"]))) ** 2
    cov = np.zeros((n, 6))
    cov[:, 0] = cov[:, 3] = cov[:, 5] = s2
    rng = np.random.default_rng(seed)
    vi.update(means3D=torch.from_numpy(world[:, :3].astype(np.float32)), cov3D=torch.from_numpy(cov.astype(np.float32)),
              shs=torch.from_numpy(rng.uniform(-1.5, 1.5, (n, 1, 3)).astype(np.float32)), sh_degree=0,
              opacities=torch.from_numpy(opacity.astype(np.float32)))
    return vi


def _one_quadrant_scene(K, q, L=300, seed=0):
    """One tile whose list has L entries: K of them around the centre of quadrant q, the others around the centres of the
    three other quadrants, depths interleaved at random.  sigma 0.7 px at opacity 0.03 reaches alpha >= 1/255 within
    1.4 px of a centre, the centres stay >= 3 px from the next quadrant's pixels: every entry carries one quadrant bit."""
    rng = np.random.default_rng(1000 * K + q + seed)
    others = [o for o in range(4) if o != q]
    quad = np.concatenate([np.full(K, q), np.resize(others, L - K)]).astype(np.int64)
    px = 3.5 + 8 * (quad & 1) + rng.uniform(-1.5, 1.5, L)
    py = 3.5 + 8 * (quad >> 1) + rng.uniform(-1.5, 1.5, L)
    return _placed(px, py, rng.uniform(2.0, 4.0, L), 0.7, 0.03, seed=seed), quad


def _check_hit_count(st, dbg, quad, q, K, L):
    """The construction's promise, from the oracle's list and the saved list's masks (CPU)."""
    assert st["num_rendered"] == L and tuple(st["ranges"][0]) == (0, L)
    np.testing.assert_allclose(st["means2D"][:, 0] // 8 + 2 * (st["means2D"][:, 1] // 8), quad)   # centres where intended
    np.testing.assert_array_equal(dbg["quad"], 1 << quad[st["point_list"].astype(np.int64)])       # one bit each, its own
    assert int(((dbg["quad"] >> q) & 1).sum()) == K


# (a) partial tiles ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", [False, True])
def test_partial_tiles_bit_exact(hip_device, monkeypatch, cull):
    """40x56 is no multiple of the tile: quadrants wholly or partly outside the image."""
    _cull(monkeypatch, cull)
    H, W = 40, 56
    scene, cams = small_scene(N=3000, H=H, W=W, seed=23)
    st, dbg = _compare(view_inputs(scene, cams, 1, H, W, bg=(0.1, 0.2, 0.3)), hip_device, lists=not cull)
    n = dbg["offsets"].astype(np.int64)
    assert np.diff(n).max() > 64 and 0 < (dbg["quad"] & 1).mean() < 1     # several chunks, mixed masks


# (b) exact hit counts: empty chunks, one hit, a batch one short / exactly full / one over, two batches and one over -------
@pytest.mark.parametrize("K,q", [(0, 0), (1, 1), (63, 2), (64, 3), (65, 0), (129, 3)])
def test_quadrant_hit_counts(hip_device, monkeypatch, K, q):
    _cull(monkeypatch, False)
    L = 300
    vi, quad = _one_quadrant_scene(K, q, L)
    st, dbg = _compare(vi, hip_device)
    _check_hit_count(st, dbg, quad, q, K, L)
    if K:   # the quadrant's hits are blended to the end of the list (no saturation): its last hit contributes
        last = np.nonzero((dbg["quad"] >> q) & 1)[0][-1] + 1
        y0, x0 = 8 * (q >> 1), 8 * (q & 1)
        assert st["n_contrib"][y0:y0 + 8, x0:x0 + 8].max() == last and st["final_T"].min() > 1e-3


# (e) 1, 2 and 3 hits left over for the quadrant's last, partial step, alone and behind full steps ------------------------
@pytest.mark.parametrize("K", [2, 3, 69, 70, 71])
def test_partial_last_step(hip_device, monkeypatch, K):
    _cull(monkeypatch, False)
    L = 260
    vi, quad = _one_quadrant_scene(K, 1, L, seed=5)
    st, dbg = _compare(vi, hip_device)
    _check_hit_count(st, dbg, quad, 1, K, L)
    assert st["final_T"].min() > 1e-3


# (c) saturation in the middle of a hit batch, thousands of entries behind --------------------------------------------------
@pytest.mark.parametrize("behind", [1400, 3000])     # list blended from LDS | from the saved list in global memory
def test_saturation_inside_a_hit_batch(hip_device, monkeypatch, behind):
    """300 faint splats in front, 75 inside each quadrant (the first hit batch is full), then 12 opaque splats that cover
    the tile (every pixel saturates inside the second hit batch), then `behind` more entries nobody blends."""
    _cull(monkeypatch, False)
    rng = np.random.default_rng(behind)
    nf, no = 300, 12
    n = nf + no + behind
    px, py = rng.uniform(0, 16, n), rng.uniform(0, 16, n)
    qd = np.arange(nf) % 4
    px[:nf], py[:nf] = 3.5 + 8 * (qd & 1) + rng.uniform(-1.5, 1.5, nf), 3.5 + 8 * (qd >> 1) + rng.uniform(-1.5, 1.5, nf)
    px[nf:nf + no], py[nf:nf + no] = rng.uniform(6, 10, no), rng.uniform(6, 10, no)
    z = np.concatenate([rng.uniform(2.0, 2.4, nf), rng.uniform(2.6, 2.8, no), rng.uniform(3.0, 5.0, behind)])
    sigma = np.concatenate([np.full(nf, 0.7), np.full(no, 40.0), np.full(behind, 0.7)])
    opacity = np.concatenate([np.full(nf, 0.03), np.full(no, 1.0), np.full(behind, 0.5)])
    st, dbg = _compare(_placed(px, py, z, sigma, opacity, seed=2), hip_device)
    assert st["num_rendered"] == n and (n > 1792) == (behind == 3000)
    hits = np.stack([(dbg["quad"][:nf] >> q) & 1 for q in range(4)]).sum(1)
    np.testing.assert_array_equal(hits, 75)                                # saturation falls into the second hit batch
    assert st["n_contrib"].min() > nf and st["n_contrib"].max() <= nf + no  # every pixel ends on an opaque splat
    assert st["final_T"].max() < 2e-2


# (d) more than 1 792 entries per tile: the list is blended from global memory ----------------------------------------------
def test_global_list_mixed_masks(hip_device, monkeypatch):
    _cull(monkeypatch, False)
    H = W = 32
    rng = np.random.default_rng(9)
    n = 6500
    vi = _placed(rng.uniform(0, W, n), rng.uniform(0, H, n), rng.uniform(2.0, 5.0, n), 0.8, 0.012, H=H, W=W, seed=4)
    st, dbg = _compare(vi, hip_device)
    per_tile = (st["ranges"][:, 1] - st["ranges"][:, 0]).astype(np.int64)
    assert per_tile.min() > 1792, per_tile
    frac = np.mean([((dbg["quad"] >> q) & 1).mean() for q in range(4)])
    assert 0.15 < frac < 0.6, frac                                        # a quadrant owns a fraction of its tile's list
    assert st["n_contrib"].max() > 0.9 * per_tile.min()                   # ... and walks it to the end


# the opt-in hardware exp runs the same loop: the existing quantified bars (tests/test_raster_hip.py) on two of the scenes --
@pytest.mark.fast_exp
@pytest.mark.parametrize("case", ["partial_tiles", "hits_129"])
def test_fast_exp_same_loop(hip_device, monkeypatch, case):
    _cull(monkeypatch, False)
    from freesplat_amd import rasterizer as R
    from freesplat_amd.rasterizer import debug_state
    assert R.FAST_EXP
    if case == "partial_tiles":
        scene, cams = small_scene(N=3000, H=40, W=56, seed=23)
        vi = view_inputs(scene, cams, 1, 40, 56, bg=(0.1, 0.2, 0.3))
    else:
        vi, _ = _one_quadrant_scene(129, 3)
    st = oracle_forward(vi)
    (color, radii, depth, alpha), _ = hip_forward(vi, hip_device, requires_grad=True)
    d = np.abs(color.detach().cpu().numpy() - st["color"]).max(axis=0)
    assert int((d > 1e-4).sum()) <= 1 and d.max() <= 2e-4 and np.median(d) <= 1e-6, (d.max(), np.median(d))
    dbg = debug_state(color.grad_fn.rs)
    np.testing.assert_array_equal(dbg["point_list"], st["point_list"])
    assert float((dbg["n_contrib"] != st["n_contrib"]).mean()) < 1e-4     # termination flips only
