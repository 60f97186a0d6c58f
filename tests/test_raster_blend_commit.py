"""The forward blend's commit under the execution mask (raster_fwd.hip, FS_BLEND_ONE): a survivor's weight, its two
accumulations and the T / contributor updates run only for the lanes that take it, and are skipped when no lane does.

None of the older small scenes holds a survivor that no pixel takes (small_scene(600, 64, 80) and both edge_scene
opacities: 0 of them, every full step commits 4 of 4), so the skip is not reached by the rest of the suite.  The scenes
here are dense enough that quadrants saturate while their walks go on; `commit_cases` derives, from the oracle's state
alone, how often each case occurs, and every test first asserts that its scene still holds them (a condition on the scene,
not a tolerance).  Then the product is compared with the oracle bit for bit, in all instantiations of the kernel:
inference / tracking (TRACK), list in LDS / in global memory (LDS_LIST), contract exp / hardware exp (FAST_EXP).

Counted by `commit_cases` (a survivor = a list entry that reaches a pixel of the 8 x 8 quadrant, image or not, as the
kernel's quadrant masks do; a step that saturates its quadrant is evaluated to its end, as the kernel does):
N = 2 500: 8 756 evaluated, 972 dead, 22 saturate-only, steps with 0 - 4 commits 67 / 72 / 138 / 187 / 1 716, last steps
of 0 - 3 entries 5 / 9 / 9 / 3, 9 of 35 quadrants saturated, longest list 949; N = 6 000 without tile culling: 15 988
evaluated, 2 304 dead, 42 saturate-only, steps 43 / 172 / 382 / 852 / 2 548, all 35 quadrants saturated, longest list 2 248."""
import numpy as np
import pytest
import torch

from util_raster import hip_forward, oracle_forward, small_scene, view_inputs

pytestmark = pytest.mark.gpu

K_SORT_LDS = 1792   # raster_fwd.hip kSortLds: longer tile lists are blended from the list in global memory
H, W = 40, 56       # 3 x 4 tiles, partial on both edges: 5 x 7 quadrants hold pixels
FLOOR = 10          # each commit case occurs at least this often


# ------------------------------------------------------------------------------------------------ the cases, from the oracle
def _fma(a, b, c):
    """fp32 fma through float64: the product of two fp32 numbers is exact there, the sum is rounded twice (to 53, then to
    24 bits), which differs from one rounding in ~2^-29 of the cases: good for counting cases, and `commit_cases` checks
    its final transmittances against the oracle's."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _contract_exp(x):
    """raster_oracle.c fso_exp, vectorised (x <= 0)."""
    f = np.float32
    x = np.maximum(x.astype(np.float32), f(-100.0))
    t = _fma(x, f(1.44269504088896341), f(12582912.0))
    n = t - f(12582912.0)
    r = _fma(n, f(-0.693147182464599609375), x)
    p = _fma(r, f(0.008290314115583897), f(0.04189793020486832))
    for c in (0.1666763573884964, 0.4999915063381195, 0.9999997019767761, 1.0):
        p = _fma(r, p, f(c))
    return np.where(x < f(-80.0), f(0.0), np.ldexp(p, n.astype(np.int32)).astype(np.float32))


def tile_reach(st, tile, exp=_contract_exp):
    """(ids, alpha [n, 256], reach [n, 256], inside [256]) of one tile's list in the oracle's arithmetic: reach = the
    entry passes the pixel's power and alpha >= 1/255 tests (pixels row-major in the 16 x 16 tile)."""
    f = np.float32
    Hh, Ww = st["H"], st["W"]
    gx = (Ww + 15) // 16
    a, b = (int(v) for v in st["ranges"][tile])
    ids = st["point_list"][a:b].astype(np.int64)
    px = (tile % gx) * 16 + np.arange(256) % 16
    py = (tile // gx) * 16 + np.arange(256) // 16
    xy, co = st["means2D"][ids], st["conic_opacity"][ids]
    dx, dy = xy[:, 0:1] - px.astype(f)[None], xy[:, 1:2] - py.astype(f)[None]
    hA, hC, nB = f(-0.5) * co[:, 0:1], f(-0.5) * co[:, 2:3], -co[:, 1:2]
    power = _fma(hA * dx, dx, dy * _fma(hC, dy, nB * dx))
    alpha = np.minimum(f(0.99), co[:, 3:4] * exp(np.minimum(power, f(0.0))))
    reach = (power <= f(0.0)) & (alpha >= f(1.0 / 255.0))
    return ids, alpha, reach, (px < Ww) & (py < Hh)


def walk_quadrant(alpha, reach, inside, on_step=None):
    """The kernel's walk of one 8 x 8 quadrant (alpha, reach: [n, 64] of the tile's list; inside: [64]).  Its survivors are
    the list entries that reach a pixel of the quadrant; they are blended four per step, in list order, until every pixel
    is saturated or outside the image; a last step takes the 1 - 3 left over.
    Returns (lanes, vis_any, steps, tail, saturated, T): per evaluated survivor the number of committing lanes and whether
    an unsaturated pixel was reached at all; per FULL step the number of survivors with a committing lane; the length of
    the last, partial step (None: the quadrant saturated first); the final done state and transmittances.
    on_step(first, done): called before each step with the position (among the survivors) of its first entry."""
    f = np.float32
    hits = np.nonzero(reach.any(1))[0]
    T = np.ones(64, f)
    done = ~inside
    lanes, vis_any, steps, tail = [], [], [], None
    for s in range(0, len(hits), 4):
        if done.all():
            break
        group = hits[s:s + 4]
        if on_step is not None:
            on_step(s, done.copy())
        n = 0
        for e in group:
            test_T = T * (f(1.0) - alpha[e])
            vis = reach[e] & ~done
            ok = vis & (test_T >= f(0.0001))
            done = done | (vis & ~ok)
            T = np.where(ok, test_T, T)
            lanes.append(int(ok.sum()))
            vis_any.append(bool(vis.any()))
            n += bool(ok.any())
        if len(group) == 4:
            steps.append(n)
        else:
            tail = len(group)
    if tail is None and not done.all():
        tail = 0
    return np.array(lanes, np.int64), np.array(vis_any, bool), steps, tail, bool(done.all()), T, hits


QUAD_PIXELS = [np.array([(qy * 8 + y) * 16 + qx * 8 + x for y in range(8) for x in range(8)]) for qy in (0, 1) for qx in (0, 1)]


def commit_cases(st):
    """How often each commit case occurs in one view, from the oracle's forward state."""
    n = dict(evaluated=0, dead=0, saturate_only=0, steps=[0] * 5, tails=[0] * 4, saturated=0, unsaturated=0, longest=0)
    gx = (st["W"] + 15) // 16
    for tile in range(st["ranges"].shape[0]):
        ids, alpha, reach, inside = tile_reach(st, tile)
        n["longest"] = max(n["longest"], len(ids))
        for q, pix in enumerate(QUAD_PIXELS):
            if not inside[pix].any():
                continue
            lanes, vis_any, steps, tail, sat, T, _ = walk_quadrant(alpha[:, pix], reach[:, pix], inside[pix])
            n["evaluated"] += len(lanes)
            n["dead"] += int((lanes == 0).sum())
            n["saturate_only"] += int(((lanes == 0) & vis_any).sum())
            for k in steps:
                n["steps"][k] += 1
            if tail is not None:
                n["tails"][tail] += 1
            n["saturated" if sat else "unsaturated"] += 1
            # the helper's walk is the oracle's blend: same final transmittances
            ys, xs = (tile // gx) * 16 + pix // 16, (tile % gx) * 16 + pix % 16
            m = inside[pix]
            np.testing.assert_array_equal(T[m], st["final_T"][ys[m], xs[m]])
    return n


def assert_commit_cases_present(n, need_unsaturated=True):
    short = {k: n[k] for k in ("dead", "saturate_only") if n[k] < FLOOR}
    short.update({f"steps_{k}": v for k, v in enumerate(n["steps"]) if v < FLOOR})
    assert not short, f"the scene lost its commit cases (have, need {FLOOR}): {short}; all: {n}"
    assert n["saturated"] >= 1 and (n["unsaturated"] >= 1 or not need_unsaturated), n


# ------------------------------------------------------------------------------------------------ scenes, computed once
_cache = {}


def _scene(N):
    """(vi, oracle state, cases) of view 0 of small_scene(N, 40, 56, seed 3): shared by the tests, read-only."""
    if N not in _cache:
        scene, cams = small_scene(N=N, H=H, W=W, seed=3, n_views=1)
        vi = view_inputs(scene, cams, 0, H, W, bg=(0.1, 0.2, 0.3))
        st = oracle_forward(vi)
        _cache[N] = (vi, st, commit_cases(st))
    return _cache[N]


def _images(out):
    return [t.detach().cpu().numpy() for t in (out[0], out[2], out[3])]


def _last_contributor(offsets, point_list, n_contrib):
    """Per pixel the Gaussian that n_contrib points at in the pixel's tile list (-1: no contributor)."""
    Hh, Ww = n_contrib.shape
    gx = (Ww + 15) // 16
    ys, xs = np.mgrid[0:Hh, 0:Ww]
    start = np.asarray(offsets, np.int64)[(ys // 16) * gx + xs // 16]
    n = n_contrib.astype(np.int64)
    return np.where(n > 0, np.asarray(point_list, np.int64)[np.maximum(start + n - 1, 0)], -1)


def _assert_same_last_contributor(dbg, st):
    """n_contrib against the oracle's.  With tile culling the product's lists are order-preserving subsequences of the
    oracle's, so the positions differ while the Gaussian they name must not; without it the positions are equal too."""
    got = _last_contributor(dbg["offsets"][:-1], dbg["point_list"], dbg["n_contrib"])
    want = _last_contributor(st["ranges"][:, 0], st["point_list"], st["n_contrib"])
    np.testing.assert_array_equal(got, want, err_msg="last contributor")
    if dbg["num_rendered"] == st["num_rendered"]:
        np.testing.assert_array_equal(dbg["n_contrib"], st["n_contrib"])


def _check_bits(vi, st, device, longest_over=None):
    """Inference and tracking instantiations against the oracle, bit for bit: colour, depth, alpha, final_T; n_contrib
    in the tracking one."""
    from freesplat_amd import _lib, rasterizer as R
    with torch.no_grad():
        inf, _ = hip_forward(vi, device)
    assert inf[0].grad_fn is None
    trk, _ = hip_forward(vi, device, requires_grad=True)
    dbg = R.debug_state(trk[0].grad_fn.rs)
    assert not (trk[0].grad_fn.rs.dims.flags & _lib.RASTER_NO_BACKWARD_STATE)
    if longest_over is not None:
        assert np.diff(dbg["offsets"].astype(np.int64)).max() > longest_over
    # the inference forward once more, launched by hand: its state (final_T) is reachable
    d = lambda t: t.to(device)
    s = R.GaussianRasterizationSettings(vi["H"], vi["W"], vi["tanfovx"], vi["tanfovy"], d(vi["bg"]), 1.0, d(vi["viewmatrix"]),
                                        d(vi["projmatrix"]), vi["sh_degree"], d(vi["campos"]), False, False)
    dims = R.make_dims(vi["means3D"].shape[0], vi["shs"].shape[1], s, inference=True)
    assert dims.flags & _lib.RASTER_NO_BACKWARD_STATE
    rs, color, depth, alpha = R.rasterize_forward_checked(dims, d(vi["means3D"]), d(vi["cov3D"]), d(vi["shs"]), None,
                                                          d(vi["opacities"]), d(vi["bg"]), d(vi["viewmatrix"]),
                                                          d(vi["projmatrix"]), d(vi["campos"]))
    for name, out in (("inference", inf), ("inference by hand", (color, None, depth, alpha)), ("tracking", trk)):
        for what, got in zip(("color", "depth", "alpha"), _images(out)):
            np.testing.assert_array_equal(got.reshape(st[what].shape), st[what], err_msg=f"{name} {what}")
    np.testing.assert_array_equal(R.debug_state(rs)["final_T"], st["final_T"], err_msg="inference final_T")
    np.testing.assert_array_equal(dbg["final_T"], st["final_T"], err_msg="tracking final_T")
    _assert_same_last_contributor(dbg, st)
    return dbg


def test_scene_holds_every_commit_case_lds_list(hip_device):
    """N = 2 500: partial tiles on both edges, the longest list fits the LDS sort.  Dead survivors, survivors that only
    saturate, full steps with 0 - 4 committing survivors, last steps of 0 - 3 entries, saturated and unsaturated quadrants."""
    vi, st, n = _scene(2500)
    print("commit cases, N = 2500:", n)
    assert n["longest"] <= K_SORT_LDS
    assert_commit_cases_present(n)
    assert all(n["tails"]), n
    dbg = _check_bits(vi, st, hip_device)
    assert np.diff(dbg["offsets"].astype(np.int64)).max() <= K_SORT_LDS


def test_backward_after_masked_commit(hip_device):
    """One backward on the state the tracking kernel left (n_contrib, final_T): the suite's 2e-4 of max-abs."""
    from oracle import raster_oracle as ro
    vi, st, n = _scene(2500)
    assert_commit_cases_present(n)
    rng = np.random.default_rng(1)
    g_color = rng.normal(size=(3, H, W)).astype(np.float32)
    g_depth = rng.normal(size=(H, W)).astype(np.float32)
    ref = ro.backward(st, g_color, g_depth)
    (color, _, depth, _), leaves = hip_forward(vi, hip_device, requires_grad=True)
    ((color * torch.from_numpy(g_color).to(hip_device)).sum() + (depth * torch.from_numpy(g_depth).to(hip_device)).sum()).backward()
    for name in ("means3D", "cov3D", "shs", "opacities"):
        got = leaves[name].grad.cpu().numpy().reshape(ref[name].shape)
        err = np.abs(got - ref[name]).max() / (np.abs(ref[name]).max() + 1e-20)
        print(f"backward {name}: {err:.2e} of max-abs")
        assert err < 2e-4, f"{name}: {err}"
    m2 = leaves["means2D"].grad.cpu().numpy()
    assert np.abs(m2[:, :2] - ref["means2D"]).max() <= 2e-4 * (np.abs(ref["means2D"]).max() + 1e-20)


def test_scene_holds_every_commit_case_global_list(hip_device, monkeypatch):
    """N = 6 000 with tile culling off: the longest list exceeds the LDS sort's capacity, those tiles are blended from the
    list in global memory (LDS_LIST = false)."""
    from freesplat_amd import rasterizer as R
    monkeypatch.setattr(R, "TILE_CULL", False)
    vi, st, n = _scene(6000)
    print("commit cases, N = 6000:", n)
    assert n["longest"] > K_SORT_LDS
    assert_commit_cases_present(n, need_unsaturated=False)
    _check_bits(vi, st, hip_device, longest_over=K_SORT_LDS)


@pytest.mark.fast_exp
def test_fast_exp_inference_equals_tracking(hip_device):
    """Hardware exp: the inference and the tracking instantiation give the same image bits, and the contributor counts
    are those of the exact mode (this scene holds no termination flip between the two exps)."""
    from freesplat_amd import rasterizer as R
    from freesplat_amd.rasterizer import debug_state
    vi, st, n = _scene(2500)
    assert_commit_cases_present(n)
    assert R.FAST_EXP
    with torch.no_grad():
        inf, _ = hip_forward(vi, hip_device)
    trk, _ = hip_forward(vi, hip_device, requires_grad=True)
    for a, b in zip(_images(inf), _images(trk)):
        np.testing.assert_array_equal(a, b)
    assert np.abs(_images(inf)[0] - st["color"]).max() <= 1e-4
    fast = debug_state(trk[0].grad_fn.rs)["n_contrib"]
    R.FAST_EXP = False       # (the autouse fixture of conftest.py restores the mode)
    exact, _ = hip_forward(vi, hip_device, requires_grad=True)
    dbg = debug_state(exact[0].grad_fn.rs)
    np.testing.assert_array_equal(fast, dbg["n_contrib"])
    _assert_same_last_contributor(dbg, st)
