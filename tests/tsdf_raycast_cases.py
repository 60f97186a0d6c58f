"""The cases the ray-casting tests share (tests/test_tsdf_raycast_host.py, tests/test_tsdf_raycast_hip.py, smoke()).

Volumes: the fused volumes of tests/tsdf_cases.py ((5, 3, 2), (33, 9, 5), (70, 17, 9): noisy planes seen from a few sides, with
unobserved regions), and a few of this module's own -- one cell (2, 2, 2), a volume without a cell (5, 1, 4), a pre-filled one
with NaN sprinkled into tsdf and weight and a block of weight 0 between the camera and the surface, a plane fused from
fronto-parallel cameras (the known answer) and a sphere fused from fourteen views (plausibility).
Images: 1 x 1, 5 x 7 (a partial tile), 17 x 33 (straddles the 16 x 16 workgroup and the 8 x 8 wavefront tiles), 48 x 64.
Cameras: a fusing one, one between two fusing ones, one INSIDE the volume, one looking away (no ray alive), an identity camera
with integer cx, cy (the centre ray has two direction components exactly 0); V = 3 with three different intrinsics.
max_steps = 3 on a scene that needs more; refine = 0, 1, 2 and 4; with and without colour.

The refinement's count per case: regula falsi on a trilinear cell reaches the zero to rounding level in two or three steps, and
on an exactly planar field in one; the sign of the value sampled THERE is rounding noise in fp32 and in float64 alike, so a
later step's branch differs between the two precisions although the depths agree to the last bits.  The cases keep `refine`
below that point (0 on the planar fields) so that the fp32 restatement and its float64 run take the same decisions on at
least 99 % of a case's pixels (tests/test_tsdf_raycast_host.py); MORE lists the same scenes at the default refine = 4, which the
GPU test checks bit for bit against the fp32 restatement like every case.

A case is a dict: name, vol (a tests/tsdf_ref.py volume, read-only), c2w [V, 4, 4] float64, rows [V, 3, 4] fp32 (what the Python
layer's host path hands the library), intrinsics [V, 4] fp32, hw, params (keywords of the ray cast)."""
import functools
import itertools
import math

import numpy as np

import tsdf_cases as TC
import tsdf_raycast_ref as RR
import tsdf_ref as R

TILE = 16


def _freeze(vol):
    for k in ("tsdf", "weight", "color"):
        if vol[k] is not None:
            vol[k].setflags(write=False)
    return vol


def look_at(pos, target, up=(0.1, -1.0, 0.2)):
    z = np.asarray(target, np.float64) - pos
    z /= np.linalg.norm(z)
    x = np.cross(np.asarray(up, np.float64), z)
    x /= np.linalg.norm(x)
    E = np.eye(4)
    E[:3, 0], E[:3, 1], E[:3, 2], E[:3, 3] = x, np.cross(z, x), z, pos
    return E


def _centre_radius(vol):
    ext = vol["voxel_size"] * (np.array(vol["dims"]) - 1)
    return np.array(vol["origin"]) + ext / 2, max(vol["voxel_size"], 0.5 * float(np.linalg.norm(ext)))


def _fused_cameras(cs, kinds, hw):
    """Cameras around the fused volume of tests/tsdf_cases.py case `cs`, one per entry of `kinds`, each with its own intrinsics."""
    c = TC.case(*cs)
    vol = TC.fused(cs)[0]
    centre, r = _centre_radius(vol)
    fusing = c["c2w"]
    H, W = hw
    c2w, intr = [], []
    for n, kind in enumerate(kinds):
        E = fusing[0].copy()
        dist = float(np.linalg.norm(E[:3, 3] - centre))
        if kind == "between":                                                # between the first and the last fusing camera
            p = 0.5 * (fusing[0][:3, 3] + fusing[-1][:3, 3]) - centre
            E = look_at(centre + p / np.linalg.norm(p) * dist, centre + 0.05 * r)
        elif kind == "inside":
            E[:3, 3] = centre - 0.3 * vol["voxel_size"] * E[:3, 2] + 0.11 * vol["voxel_size"]
            dist = r
        elif kind == "away":
            E[:3, 0], E[:3, 2] = -E[:3, 0], -E[:3, 2]
        else:
            assert kind == "fusing"
        f = (0.45 + 0.07 * n) * max(H, W) * dist / r
        c2w.append(E)
        intr.append((f, 1.05 * f, (W - 1) / 2 + 0.21 - 0.1 * n, (H - 1) / 2 - 0.17 + 0.1 * n))
    return vol, np.stack(c2w), np.array(intr, np.float32)


def _tiny():
    vol = R.new_volume((-0.5, -0.5, 1.0), 1.0, (2, 2, 2), 2.0, 64.0, True)
    vol["tsdf"][0], vol["tsdf"][1] = [[0.4, 0.5], [0.3, 0.45]], [[-0.5, -0.4], [-0.6, -0.35]]
    vol["weight"][...] = 2.0
    vol["color"] = np.random.default_rng(11).random((3, 2, 2, 2)).astype(np.float32)
    return vol


def _holes():
    """The plane z = 5.3 voxels in a (20, 12, 10) grid, observed everywhere; then NaN sprinkled into tsdf and weight and a block of
    weight 0 in front of the surface."""
    rng = np.random.default_rng(12)
    vol = R.new_volume((-1.0, -0.6, 1.0), 0.1, (20, 12, 10), 0.3, 64.0, True)
    vol["tsdf"][...] = np.clip((5.3 - np.arange(10, dtype=np.float64)[:, None, None]) / 3.0, -1, 1).astype(np.float32)
    vol["weight"][...] = rng.integers(1, 4, vol["weight"].shape).astype(np.float32)
    vol["color"] = rng.random(vol["color"].shape).astype(np.float32)
    vol["tsdf"][rng.random(vol["tsdf"].shape) < 0.02] = np.nan
    vol["weight"][rng.random(vol["weight"].shape) < 0.02] = np.nan
    vol["weight"][1:4, 3:8, 5:12] = 0.0
    return vol


PLANE_Z, PLANE_ANGLE = 2.5, math.radians(25.0)


def _plane():
    """40^3 grid points, voxel 0.05, trunc 4 voxels, the plane z = 2.5 fused from three identity-rotation cameras (the case where
    the projective value is the signed distance)."""
    vol = R.new_volume((-1.0, -1.0, 1.5), 0.05, (40, 40, 40), 0.2, 64.0, False)
    c2w = np.tile(np.eye(4), (3, 1, 1))
    c2w[:, :3, 3] = [(0.0, 0.0, 0.0), (0.3, -0.2, 0.4), (-0.25, 0.15, -0.5)]
    H, W = 120, 120
    intr = np.tile(np.array([50.0, 50.0, 59.5, 59.5], np.float32), (3, 1))
    depth = np.stack([np.full((H, W), PLANE_Z - c2w[v, 2, 3], np.float32) for v in range(3)])
    w2c = np.linalg.inv(c2w)[:, :3].astype(np.float32)
    R.integrate(vol, dict(world_to_cam=w2c, intrinsics=intr, depth=depth, alpha=None, image=None, near=0.05, min_depth=0.0,
                          max_depth=np.inf, alpha_min=0.0, alpha_floor=1e-3))
    return vol


def tilted_plane_scene(slope=0.3):
    """The round-trip scene: an empty 40^3 volume and three identity-rotation views (120 x 120) of the plane z = 2.5 + slope * x:
    (vol, c2w [3, 4, 4], intrinsics [3, 4], depth [3, 120, 120]).  Along a pixel's ray x = c_x + s * dx and z = c_z + s, so the
    z-depth of the plane is s = (2.5 + slope * c_x - c_z) / (1 - slope * dx)."""
    vol = R.new_volume((-1.0, -1.0, 1.5), 0.05, (40, 40, 40), 0.2, 64.0, False)
    c2w = np.tile(np.eye(4), (3, 1, 1))
    c2w[:, :3, 3] = [(0.0, 0.0, 0.0), (0.3, -0.2, 0.4), (-0.25, 0.15, -0.5)]
    H = W = 120
    intr = np.tile(np.array([50.0, 50.0, 59.5, 59.5], np.float32), (3, 1))
    dx = (np.arange(W, dtype=np.float64)[None, :] - 59.5) / 50.0
    depth = np.stack([np.broadcast_to((PLANE_Z + slope * c2w[v, 0, 3] - c2w[v, 2, 3]) / (1.0 - slope * dx), (H, W)) for v in range(3)])
    return vol, c2w, intr, depth.astype(np.float32)


def plane_camera():
    """A 48 x 64 camera turned 25 degrees about y that looks at the plane's centre: (c2w [1, 4, 4], intrinsics [1, 4], hw)."""
    c, s = math.cos(PLANE_ANGLE), math.sin(PLANE_ANGLE)
    E = np.eye(4)
    E[:3, :3] = [[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]
    E[:3, 3] = np.array([0.0, 0.0, PLANE_Z]) - 2.0 * E[:3, 2]
    return E[None], np.array([[60.0, 60.0, 31.5, 23.5]], np.float32), (48, 64)


SPHERE = dict(vs=0.1, n=34, trunc_vox=3.0, radius_vox=12.0, origin=(-1.63, -1.71, -1.67), centre_vox=(16.37, 16.62, 16.45))


def sphere_depth(c2w, k, H, W, centre, radius, grazing=0.0):
    """(analytic z-depth of the sphere through the pixel centres, NaN on a miss and where the cosine of the incidence angle is
    below `grazing`; that cosine)."""
    py, px = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.stack([(px - k[2]) / k[0], (py - k[3]) / k[1], np.ones_like(px)], -1) @ c2w[:3, :3].T
    oc = c2w[:3, 3] - centre
    a, b, cc = (ray * ray).sum(-1), (ray * oc).sum(-1), float(oc @ oc) - radius * radius
    disc = b * b - a * cc
    with np.errstate(invalid="ignore"):
        s = (-b - np.sqrt(disc)) / a
        cosine = -((oc + s[..., None] * ray) * ray).sum(-1) / (radius * np.sqrt(a))
        return np.where((disc > 0) & (cosine >= grazing), s, np.nan), cosine


def _sphere():
    """A sphere of radius 12 voxels in front of a far wall (depth 10 where a ray misses the sphere, so the free space around it is
    observed) fused from fourteen directions (the six axes and the eight diagonals), every hit kept: the scene of
    tests/test_tsdf_host.py's sphere at a larger radius, through the fp32 restatement."""
    S = SPHERE
    vs, n = S["vs"], S["n"]
    vol = R.new_volume(S["origin"], vs, (n, n, n), S["trunc_vox"] * vs, 64.0, False)
    centre = np.array(vol["origin"]) + vs * np.array(S["centre_vox"])
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)] + list(itertools.product((-1, 1), repeat=3))
    c2w = np.stack([look_at(centre + 4.0 * np.array(d, np.float64) / np.linalg.norm(d), centre, up=(0.3, 0.5 + 0.1 * i, -0.8))
                    for i, d in enumerate(dirs)])
    H = W = 128
    intr = np.tile(np.array([150.0, 150.0, 63.5, 63.5], np.float32), (len(dirs), 1))
    depth = np.stack([sphere_depth(c2w[v], intr[v], H, W, centre, S["radius_vox"] * vs, 0.0)[0] for v in range(len(dirs))])
    depth = np.where(np.isnan(depth), 10.0, depth).astype(np.float32)
    R.integrate(vol, dict(world_to_cam=np.linalg.inv(c2w)[:, :3].astype(np.float32), intrinsics=intr, depth=depth, alpha=None, image=None,
                          near=0.05, min_depth=0.0, max_depth=np.inf, alpha_min=0.0, alpha_floor=1e-3))
    return vol


def sphere_camera():
    """A new 96 x 128 camera off every fusing direction: (c2w [1, 4, 4], intrinsics [1, 4], hw, centre, radius)."""
    S = SPHERE
    centre = np.array([float(np.float32(o)) for o in S["origin"]]) + S["vs"] * np.array(S["centre_vox"])
    E = look_at(centre + 3.6 * np.array([0.48, -0.31, -0.82]) / np.linalg.norm([0.48, -0.31, -0.82]), centre)
    return E[None], np.array([[130.0, 130.0, 63.5, 47.5]], np.float32), (96, 128), centre, S["radius_vox"] * S["vs"]


@functools.lru_cache(maxsize=None)
def volume(key):
    if key[0] == "fused":
        return TC.fused(TC.CASES[key[1]])[0]
    return _freeze(dict(tiny=_tiny, holes=_holes, plane=_plane, sphere=_sphere,
                        flat=lambda: R.new_volume((0.0, 0.0, 1.0), 0.1, (5, 1, 4), 0.3, 64.0, True))[key[0]]())


def _identity(pos, k, hw):
    E = np.eye(4)
    E[:3, 3] = pos
    return E[None], np.array([k], np.float32), hw


# name -> (volume key, cameras, params)
@functools.lru_cache(maxsize=None)
def _specs():
    s = {}
    s["one cell 1x1"] = (("tiny",), _identity((0.1, -0.2, -1.0), (2.0, 2.0, 0.0, 0.0), (1, 1)), dict())
    s["(5,3,2) 5x7 V=3 fusing/inside/away"] = (("fused", 1), _fused_cameras(TC.CASES[1], ("fusing", "inside", "away"), (5, 7))[1:] + ((5, 7),), dict())
    s["(33,9,5) 17x33 V=3 refine=0"] = (("fused", 3), _fused_cameras(TC.CASES[3], ("fusing", "between", "inside"), (17, 33))[1:] + ((17, 33),),
                                       dict(refine=0))
    s["(70,17,9) 17x33 V=3 fusing/between/away"] = (("fused", 4), _fused_cameras(TC.CASES[4], ("fusing", "between", "away"), (17, 33))[1:]
                                                   + ((17, 33),), dict(refine=1))
    s["(70,17,9) 5x7 max_steps=3"] = (("fused", 4), _fused_cameras(TC.CASES[4], ("fusing",), (5, 7))[1:] + ((5, 7),),
                                     dict(max_steps=3, refine=2))
    s["no cell (5,1,4) 5x7"] = (("flat",), _identity((0.2, 0.0, 0.0), (6.0, 6.0, 3.0, 2.0), (5, 7)), dict())
    s["holes 17x33 axis-parallel"] = (("holes",), _identity((0.013, -0.021, 0.007), (18.0, 18.0, 16.0, 8.0), (17, 33)), dict(refine=0))
    s["plane 5x7 axis-parallel"] = (("plane",), _identity((0.0, 0.0, 0.0), (4.0, 4.0, 3.0, 2.0), (5, 7)), dict(relax=0.5, step_min=0.25))
    s["plane 48x64 turned 25 degrees"] = (("plane",), plane_camera(), dict(refine=0))
    E, k, _, _, _ = sphere_camera()
    s["sphere 17x33"] = (("sphere",), (E, k * np.float32(0.25), (17, 33)), dict(refine=1))
    return s


@functools.lru_cache(maxsize=None)
def case(name):
    key, (c2w, intr, hw), params = _specs()[name]
    vol = volume(key)
    return dict(name=name, vol=vol, c2w=c2w, rows=np.ascontiguousarray(c2w[:, :3, :]).astype(np.float32), intrinsics=intr, hw=hw,
                params=params)


NAMES = list(_specs())
# (case, overriding keywords as a tuple of pairs): the scenes whose cases refine less than the default, at the default
MORE = [(n, (("refine", 4),)) for n in NAMES if _specs()[n][2].get("refine", 4) != 4 and "refine=0" not in n]


@functools.lru_cache(maxsize=None)
def reference(name, dtype=np.float32, override=()):
    """The restatement's result for a case (shared by the tests, read-only)."""
    c = case(name)
    out = RR.raycast(c["vol"], c["rows"], c["intrinsics"], c["hw"], dtype, **dict(c["params"], **dict(override)))
    for a in out.values():
        if a is not None:
            a.setflags(write=False)
    return out
