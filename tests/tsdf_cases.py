"""The cases the TSDF tests share (tests/test_tsdf_host.py, tests/test_tsdf_hip.py, smoke()): volumes placed by the kernels' brick
and run sizes, depth maps of 1 x 1, 7 x 5 and 40 x 30 pixels, 1, 3, MAX and MAX + 1 views, with and without colour and alpha.

kind "rand": cameras around the volume looking at its centre (view 1 of a case with three or more views looks AWAY: a view behind
the volume), focal lengths that make the volume overflow the map (the frustum's edge cuts bricks), depth maps of a noisy plane
through the centre with holes of all five kinds (NaN, +inf, -inf, 0, negative), alpha in (0.15, 1) with alpha_min = 0.3.
kind "exact": power-of-two geometry under three identity cameras -- grid points exactly on a pixel boundary in u (u = 1.5, 4.5,
7.5), a tsdf of exactly 0 on the plane z = 2, max_weight = 2 reached by the third view."""
import functools
import zlib

import numpy as np

import tsdf_ref as R

MAX_VIEWS = 64
BRICK = (32, 8, 4)
MESH_RUN = 256
SCAN_THREADS = 1024
HOLES = (np.nan, np.inf, -np.inf, 0.0, -1.5)
SCALARS = dict(near=0.05, min_depth=0.1, max_depth=50.0, alpha_min=0.3, alpha_floor=1e-3)

# (dims (X, Y, Z), (H, W), V, colour, alpha, kind)
CASES = [
    ((1, 1, 1), (1, 1), 1, False, False, "rand"),
    ((5, 3, 2), (5, 7), 3, True, False, "rand"),
    ((31, 7, 3), (5, 7), 1, True, True, "rand"),                 # one brick minus one in each dimension
    ((33, 9, 5), (30, 40), 3, False, True, "rand"),              # ... plus one
    ((70, 17, 9), (30, 40), 3, True, False, "rand"),             # three bricks in each dimension, X no multiple of 4
    ((70, 17, 9), (30, 40), MAX_VIEWS, True, True, "rand"),
    ((33, 9, 5), (5, 7), MAX_VIEWS + 1, False, False, "rand"),   # chunked by the Python layer
    ((9, 9, 9), (5, 7), 3, True, False, "exact"),
]
# the extraction's scan takes more than one block count per thread beyond SCAN_THREADS * MESH_RUN cubes
BIG = ((67, 66, 65), (30, 40), 3, False, False, "rand")
assert 66 * 65 * 64 > SCAN_THREADS * MESH_RUN and 67 % 4


def _look_at(pos, target, rng):
    z = target - pos
    z /= np.linalg.norm(z)
    up = rng.normal(size=3)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    E = np.eye(4)
    E[:3, 0], E[:3, 1], E[:3, 2], E[:3, 3] = x, y, z, pos
    return E


@functools.lru_cache(maxsize=None)
def case(dims, hw, V, color, alpha, kind):
    """dict: vol (an empty tsdf_ref volume), views (what tsdf_ref.integrate takes), c2w [V, 4, 4] float64 (camera-to-world, what
    the Python layer takes; views["world_to_cam"] is what the layer's host path makes of it)."""
    rng = np.random.default_rng(zlib.crc32(repr((dims, hw, V, color, alpha, kind)).encode()))
    H, W = hw
    if kind == "exact":
        vol = R.new_volume((-1.0, -1.0, 1.0), 0.25, dims, 0.5, 2.0, color)
        c2w = np.tile(np.eye(4), (V, 1, 1))
        intr = np.tile(np.array([6.0, 6.0, 3.0, 2.0], np.float32), (V, 1))
        depth = np.full((V, H, W), 2.0, np.float32)
        a = None
    else:
        vs = 0.05
        origin = np.array([-0.37, 0.21, 1.13])
        vol = R.new_volume(origin, vs, dims, 3 * vs, 3.0 if V > 3 else 64.0, color)
        ext = vs * (np.array(dims) - 1)
        centre = origin + ext / 2
        r = max(vs, 0.5 * float(np.linalg.norm(ext)))
        c2w, intr = np.zeros((V, 4, 4)), np.zeros((V, 4), np.float32)
        depth = np.zeros((V, H, W), np.float32)
        for v in range(V):
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            dist = 2.5 * r + 0.5
            pos = centre + d * dist
            target = centre + 0.1 * r * rng.uniform(-1, 1, 3)
            if V >= 3 and v == 1:
                target = 2 * pos - target                                    # looks away: every grid point is behind it
            c2w[v] = _look_at(pos, target, rng)
            f = 0.6 * max(H, W) * dist / r
            intr[v] = (f, 1.07 * f, (W - 1) / 2 + rng.uniform(-0.3, 0.3), (H - 1) / 2 + rng.uniform(-0.3, 0.3))
            depth[v] = dist + vs * rng.uniform(-2, 2, (H, W))
        holes = rng.random((V, H, W)) < 0.12
        depth[holes] = rng.choice(HOLES, int(holes.sum())).astype(np.float32)
        if H * W >= 12:
            depth[0].reshape(-1)[[1, W + 2, 2 * W + 3, 3 * W + 1, 4 * W + 4]] = HOLES
        elif H * W == 1:
            depth[0] = 2.5 * r + 0.5
        a = None
        if alpha:
            a = rng.uniform(0.15, 1.0, (V, H, W)).astype(np.float32)
            a.reshape(-1)[[0, H * W - 1]] = (np.nan, 0.0)
            with np.errstate(all="ignore"):
                depth = depth * np.where(np.isnan(a), np.float32(1.0), a)            # accumulated depth = expected depth * alpha
    image = rng.random((V, 3, H, W)).astype(np.float32) if color else None
    import torch
    from freesplat_amd.tsdf import world_to_cam
    w2c = world_to_cam(torch.from_numpy(c2w), "cpu").numpy()                 # (the package's host path: float64 inverse, fp32 rows)
    views = dict(world_to_cam=w2c, intrinsics=intr, depth=depth, alpha=a, image=image, **SCALARS)
    return dict(vol=vol, views=views, c2w=c2w, name=f"{dims} {hw} V={V} colour={color} alpha={alpha} {kind}")


def view_slice(views, lo, hi):
    out = dict(views)
    for k in ("world_to_cam", "intrinsics", "depth", "alpha", "image"):
        if out[k] is not None:
            out[k] = out[k][lo:hi]
    return out


@functools.lru_cache(maxsize=None)
def fused(cs):
    """The fp32 restatement's volume after all views of case `cs`, with the decisions: (vol, codes, pixels).  Shared, read-only."""
    c = case(*cs)
    vol = R.copy_volume(c["vol"])
    codes, pixels = R.integrate(vol, c["views"], np.float32, decisions=True)
    for k in ("tsdf", "weight", "color"):
        if vol[k] is not None:
            vol[k].setflags(write=False)
    return vol, codes, pixels
