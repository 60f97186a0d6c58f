"""Volumetric TSDF fusion of depth maps and triangle-mesh extraction on the device, through fs_tsdf_integrate and
fs_tsdf_mesh_plan / fs_tsdf_mesh_emit (libfreesplat_hip.so, include/freesplat_amd_tsdf.h, csrc/tsdf.hip).  The definitions are
those of DESIGN.md "TSDF fusion":

  volume   tsdf [Z, Y, X] = sdf / trunc in [-1, 1], weight [Z, Y, X] = observations capped at max_weight, color [3, Z, Y, X]
           (optional); grid point (i, j, k) lies at origin + voxel_size * (i, j, k) and is a corner of the cubes the mesh is cut from
  integrate  per grid point and view, in view order: camera point p = R x + t, skip unless p_z > near; pixel (rint(fx p_x / p_z
           + cx), rint(fy p_y / p_z + cy)), skip outside the map; d = depth there (depth / max(alpha, alpha_floor) with alpha,
           skipped where alpha < alpha_min), skip holes (NaN, +-inf, <= min_depth, >= max_depth); sdf = d - p_z (z-depth, what
           the rasterizer outputs), skip if sdf < -trunc; running means of min(1, sdf / trunc) and of the image's colour
  extract  marching tetrahedra over the cubes whose eight corners have weight >= min_weight: a triangle soup ordered by cube,
           tetrahedron, triangle, normals pointing into free space; an edge gives the same bits from every cube sharing it, so
           `weld` makes an indexed mesh from the bits alone

`intrinsics` = (fx, fy, cx, cy) in pixels, integer pixel coordinates being pixel centres (see normals_loss.py); the caller folds
its own convention into cx, cy.  `extrinsics` are camera-to-world [V, 4, 4], as render_views takes them.

  raycast  per view and pixel a ray marched through the volume in z-depth (include/freesplat_ext_raycast.h, csrc/tsdf_raycast.hip,
           DESIGN.md "TSDF ray casting"): depth [V, H, W] (0 = no hit, the rasterizer's hole), camera-space normals [V, 3, H, W] in
           depth_normals' convention (NaN = missing, what normals_loss(gt_normals=...) skips), colour, march samples per ray

Integration and ray casting are evaluation artefacts: no autograd, no backward.  Device tensors only: there is no CPU / eager
path.  integrate and raycast make no host synchronisation when `extrinsics` is a device tensor and are capturable in a graph;
extract_mesh reads one number (the triangle count) back.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple

import numpy as np
import torch
from torch import Tensor

from . import _args, _lib

MAX_VIEWS = _lib.TSDF_MAX_VIEWS
BRICK = _lib.TSDF_BRICK            # (x, y, z) grid points one workgroup of the integration owns; tests place shapes by it
MESH_RUN = _lib.TSDF_MESH_RUN      # consecutive cubes one workgroup of the extraction owns
SCAN_THREADS = 1024                # threads of the one workgroup that scans the extraction's block counts
_NAME = "freesplat_amd.tsdf"


def mt_table() -> np.ndarray:
    """The (tet, case) -> triangles table that ships with the library: uint8 [6, 16, 7] = (count, 6 edge codes)."""
    buf = (C.c_uint8 * (6 * 16 * 7))()
    _lib.call("fs_tsdf_mt_table", buf)
    return np.frombuffer(buf, np.uint8).reshape(6, 16, 7).copy()


def _pos_finite(x, what: str) -> float:
    x = float(x)
    if not (x > 0.0 and math.isfinite(x)):
        raise ValueError(f"{_NAME}: {what} must be a positive finite number, got {x!r}")
    return x


def world_to_cam(extrinsics, device) -> Tensor:
    """camera-to-world [V, 4, 4] -> the rows [R | t] of world-to-camera, [V, 3, 4] fp32 on `device`, inverted in float64.  A host
    matrix is validated (finite, last row (0, 0, 0, 1), invertible) and inverted on the host; a device matrix is inverted on the
    device by the closed form (adjugate / determinant), without a synchronisation."""
    if not isinstance(extrinsics, Tensor):
        extrinsics = torch.as_tensor(np.asarray(extrinsics))
    _args.no_grad_to(extrinsics, "extrinsics", _NAME)
    E = extrinsics.detach().to(torch.float64)
    if E.dim() != 3 or tuple(E.shape[1:]) != (4, 4) or E.shape[0] == 0:
        raise ValueError(f"{_NAME}: extrinsics must be camera-to-world [V, 4, 4], got {tuple(E.shape)}")
    A, t = E[:, :3, :3], E[:, :3, 3]
    c0 = torch.linalg.cross(A[:, :, 1], A[:, :, 2])
    c1 = torch.linalg.cross(A[:, :, 2], A[:, :, 0])
    c2 = torch.linalg.cross(A[:, :, 0], A[:, :, 1])
    det = (A[:, :, 0] * c0).sum(1)
    if E.device.type != "cuda":
        last = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64)
        if not bool(torch.isfinite(E).all()) or not bool((E[:, 3] == last).all()):
            raise ValueError(f"{_NAME}: extrinsics must be finite with a last row (0, 0, 0, 1)")
        if not bool((det.abs() > 1e-12 * A.abs().amax((1, 2)).clamp_min(1e-300) ** 3).all()):
            raise ValueError(f"{_NAME}: extrinsics are not invertible")
    R = torch.stack([c0, c1, c2], 1) / det[:, None, None]
    out = torch.cat([R, -(R @ t[:, :, None])], 2)
    return out.to(device=device, dtype=torch.float32).contiguous()


class TSDFVolume:
    """A dense TSDF volume on a HIP device.

    vol = TSDFVolume(origin, voxel_size, dims=(X, Y, Z), trunc=4 * voxel_size, color=True, max_weight=64.0, device="cuda")
    vol.integrate(depth, intrinsics, extrinsics, image=..., alpha=...); verts, cols = vol.extract_mesh()"""

    def __init__(self, origin, voxel_size: float, dims, trunc: float | None = None, color: bool = False, max_weight: float = 64.0,
                 device="cuda"):
        self.voxel_size = float(np.float32(_pos_finite(voxel_size, "voxel_size")))
        self.trunc = float(np.float32(_pos_finite(4.0 * self.voxel_size if trunc is None else trunc, "trunc")))
        self.max_weight = float(np.float32(_pos_finite(max_weight, "max_weight")))
        origin = tuple(float(np.float32(o)) for o in origin)
        if len(origin) != 3 or not all(math.isfinite(o) for o in origin):
            raise ValueError(f"{_NAME}: origin must be three finite numbers, got {origin!r}")
        self.origin = origin
        dims = tuple(int(d) for d in dims)
        if len(dims) != 3 or min(dims) <= 0:
            raise ValueError(f"{_NAME}: dims must be three positive sizes (X, Y, Z), got {dims!r}")
        if dims[0] * dims[1] * dims[2] > 2 ** 31 - 1:
            raise ValueError(f"{_NAME}: X * Y * Z = {dims[0] * dims[1] * dims[2]} grid points exceed 2^31 - 1")
        self.dims = dims
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"{_NAME}: the volume must live on a HIP device (got {self.device}); there is no CPU path")
        X, Y, Z = dims
        self.tsdf = torch.empty(Z, Y, X, device=self.device)
        self.weight = torch.empty(Z, Y, X, device=self.device)
        self.color = torch.empty(3, Z, Y, X, device=self.device) if color else None
        self.reset()

    @classmethod
    def from_bounds(cls, lo, hi, voxel_size: float, **kw):
        """The smallest grid with origin `lo` whose points cover the box [lo, hi]."""
        voxel_size = _pos_finite(voxel_size, "voxel_size")
        dims = tuple(int(math.ceil((float(h) - float(l)) / voxel_size - 1e-9)) + 1 for l, h in zip(lo, hi))
        return cls(lo, voxel_size, dims, **kw)

    def reset(self) -> None:
        """Free space everywhere, nothing observed."""
        self.tsdf.fill_(1.0)
        self.weight.zero_()
        if self.color is not None:
            self.color.zero_()

    def grid_points(self) -> Tensor:
        """[Z, Y, X, 3] fp32 coordinates of the grid points, as the kernels form them."""
        ax = [torch.tensor(o, device=self.device) + torch.tensor(self.voxel_size, device=self.device)
              * torch.arange(n, device=self.device, dtype=torch.float32) for o, n in zip(self.origin, self.dims)]
        z, y, x = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        return torch.stack([x, y, z], -1)

    # ---- integrate ------------------------------------------------------------------------------------------------------------

    def integrate(self, depth: Tensor, intrinsics, extrinsics, image: Tensor | None = None, alpha: Tensor | None = None, *,
                  near: float = 1e-3, min_depth: float = 0.0, max_depth: float = math.inf, alpha_min: float = 0.5,
                  alpha_floor: float = 1e-3, _flags: int = 0) -> None:
        """Fuses depth [V, H, W] (with image [V, 3, H, W] when the volume has colour, and the rasterizer's accumulated alpha
        [V, H, W] when `depth` is alpha-weighted) into the volume in place.  More than MAX_VIEWS views go in chunks, in order: the
        result is that of one call per view."""
        for t, what in ((depth, "depth"), (image, "image"), (alpha, "alpha"), (intrinsics, "intrinsics")):
            _args.no_grad_to(t, what, _NAME)
        d = _args.device_f32(depth, "depth", _NAME).detach()
        if d.dim() != 3 or d.numel() == 0:
            raise ValueError(f"{_NAME}: depth must be a non-empty [V, H, W], got {tuple(d.shape)}")
        V, H, W = d.shape
        if d.device != self.device:
            raise ValueError(f"{_NAME}: depth lives on {d.device}, the volume on {self.device}")
        if (image is None) != (self.color is None):
            raise ValueError(f"{_NAME}: a volume with colour planes needs `image` on every call, one without takes none")
        im = a = None
        if image is not None:
            im = _args.device_f32(image, "image", _NAME).detach()
            if tuple(im.shape) != (V, 3, H, W) or im.device != self.device:
                raise ValueError(f"{_NAME}: image must be [{V}, 3, {H}, {W}] on {self.device}, got {tuple(im.shape)} on {im.device}")
        if alpha is not None:
            a = _args.device_f32(alpha, "alpha", _NAME).detach()
            if a.shape != d.shape or a.device != self.device:
                raise ValueError(f"{_NAME}: alpha must be [{V}, {H}, {W}] on {self.device}, got {tuple(a.shape)} on {a.device}")
        min_depth, max_depth, alpha_floor = _args.depth_scalars(min_depth, max_depth, alpha_floor, _NAME)
        near, alpha_min = float(near), float(alpha_min)
        if math.isnan(near) or math.isnan(alpha_min):
            raise ValueError(f"{_NAME}: near / alpha_min must not be NaN")
        k = torch.as_tensor(intrinsics).detach().to(device=self.device, dtype=torch.float32)
        if k.shape == (4,):
            k = k.expand(V, 4)
        if tuple(k.shape) != (V, 4):
            raise ValueError(f"{_NAME}: intrinsics must be [4] or [{V}, 4] = (fx, fy, cx, cy), got {tuple(k.shape)}")
        k = k.contiguous()
        w2c = world_to_cam(extrinsics, self.device)
        if w2c.shape[0] != V:
            raise ValueError(f"{_NAME}: extrinsics must be [{V}, 4, 4], got {w2c.shape[0]} matrices")
        p = _lib.ptr
        X, Y, Z = self.dims
        for v0 in range(0, V, MAX_VIEWS):
            v1 = min(V, v0 + MAX_VIEWS)
            dv, kv, wv = d[v0:v1], k[v0:v1], w2c[v0:v1]               # (leading slices of contiguous tensors: contiguous)
            iv = None if im is None else im[v0:v1]
            av = None if a is None else a[v0:v1]
            _lib.launch("fs_tsdf_integrate", X, Y, Z, *self.origin, self.voxel_size, self.trunc, self.max_weight, p(self.tsdf),
                        p(self.weight), p(self.color), v1 - v0, H, W, p(wv), p(kv), p(dv), p(av), p(iv), near, min_depth,
                        max_depth, alpha_min, alpha_floor, int(_flags))

    # ---- extract --------------------------------------------------------------------------------------------------------------

    def extract_mesh(self, min_weight: float = 1.0):
        """The triangle soup (vertices [T, 3, 3], colors [T, 3, 3] | None) of the zero level set over the observed cubes."""
        return extract_mesh(self.tsdf, self.weight, self.color, self.origin, self.voxel_size, min_weight)

    # ---- ray cast -------------------------------------------------------------------------------------------------------------

    def raycast(self, intrinsics, extrinsics, hw, *, min_depth: float = 0.0, max_depth: float = math.inf, min_weight: float = 1.0,
                step_min: float = 0.5, relax: float = 0.8, refine: int = 4, max_steps: int | None = None, normals: bool = True,
                color: bool | None = None, return_steps: bool = False) -> "RayCast":
        """The volume seen from V cameras: RayCast(depth [V, H, W], normals [V, 3, H, W] | None, color [V, 3, H, W] | None,
        steps [V, H, W] int32 | None).  color = None: iff the volume has colour.  The keywords are those of the module-level
        raycast (whose colour switch is `color_out`, `color` being the volume's planes there)."""
        return raycast(self.tsdf, self.weight, self.color, self.origin, self.voxel_size, self.trunc, intrinsics, extrinsics, hw,
                       min_depth=min_depth, max_depth=max_depth, min_weight=min_weight, step_min=step_min, relax=relax,
                       refine=refine, max_steps=max_steps, normals=normals, color_out=color, return_steps=return_steps)


def extract_mesh(tsdf: Tensor, weight: Tensor, color: Tensor | None, origin, voxel_size: float, min_weight: float = 1.0):
    """Marching tetrahedra over tsdf / weight [Z, Y, X] (and color [3, Z, Y, X]): plan, one read of the triangle count, emit."""
    min_weight = float(min_weight)
    if not min_weight > 0.0:
        raise ValueError(f"{_NAME}: min_weight must be positive, got {min_weight!r}")
    voxel_size = _pos_finite(voxel_size, "voxel_size")
    f = _args.device_f32(tsdf, "tsdf", _NAME).detach()
    w = _args.device_f32(weight, "weight", _NAME).detach()
    if f.dim() != 3 or f.numel() == 0 or w.shape != f.shape or w.device != f.device:
        raise ValueError(f"{_NAME}: tsdf and weight must be non-empty [Z, Y, X] tensors of one shape on one device, got "
                         f"{tuple(f.shape)} and {tuple(w.shape)}")
    Z, Y, X = f.shape
    c = None
    if color is not None:
        c = _args.device_f32(color, "color", _NAME).detach()
        if tuple(c.shape) != (3, Z, Y, X) or c.device != f.device:
            raise ValueError(f"{_NAME}: color must be [3, {Z}, {Y}, {X}] on {f.device}, got {tuple(c.shape)} on {c.device}")
    origin = tuple(float(o) for o in origin)
    L, p = _lib.lib(), _lib.ptr
    nbytes = L.fs_tsdf_mesh_scratch_bytes(X, Y, Z)
    if nbytes == 0:
        raise ValueError(f"{_NAME}: a volume of {X} x {Y} x {Z} grid points is beyond 2^31 - 1")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=f.device)
    total = torch.empty(1, dtype=torch.int64, device=f.device)
    _lib.launch("fs_tsdf_mesh_plan", X, Y, Z, p(f), p(w), min_weight, p(total), p(scratch))
    T = int(total.item())                                           # the extraction's one host synchronisation
    vertices = torch.empty(T, 3, 3, device=f.device)
    colors = None if c is None else torch.empty(T, 3, 3, device=f.device)
    if T:
        _lib.launch("fs_tsdf_mesh_emit", X, Y, Z, *origin, voxel_size, p(f), p(w), p(c), min_weight, p(scratch), T, p(vertices),
                    p(colors))
    return vertices, colors


class RayCast(NamedTuple):
    depth: Tensor                # [V, H, W] z-depth, 0 where the ray hits nothing
    normals: Tensor | None       # [V, 3, H, W] camera space, NaN where there is none
    color: Tensor | None         # [V, 3, H, W], 0 where there is none
    steps: Tensor | None         # [V, H, W] int32 march samples per ray


def cam_rows(extrinsics, device) -> Tensor:
    """camera-to-world [V, 4, 4] -> its top three rows [V, 3, 4] fp32 on `device`, as given (no inverse).  A host matrix is
    validated (finite, last row (0, 0, 0, 1)); a device matrix is taken as it is, without a synchronisation."""
    if not isinstance(extrinsics, Tensor):
        extrinsics = torch.as_tensor(np.asarray(extrinsics))
    _args.no_grad_to(extrinsics, "extrinsics", _NAME)
    E = extrinsics.detach()
    if E.dim() != 3 or tuple(E.shape[1:]) != (4, 4) or E.shape[0] == 0:
        raise ValueError(f"{_NAME}: extrinsics must be camera-to-world [V, 4, 4], got {tuple(E.shape)}")
    if E.device.type != "cuda":
        E = E.to(torch.float64)
        last = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64)
        if not bool(torch.isfinite(E).all()) or not bool((E[:, 3] == last).all()):
            raise ValueError(f"{_NAME}: extrinsics must be finite with a last row (0, 0, 0, 1)")
    return E[:, :3, :].to(device=device, dtype=torch.float32).contiguous()


def raycast(tsdf: Tensor, weight: Tensor, color: Tensor | None, origin, voxel_size: float, trunc: float, intrinsics, extrinsics,
            hw, *, min_depth: float = 0.0, max_depth: float = math.inf, min_weight: float = 1.0, step_min: float = 0.5,
            relax: float = 0.8, refine: int = 4, max_steps: int | None = None, normals: bool = True, color_out: bool | None = None,
            return_steps: bool = False) -> RayCast:
    """Ray casts tsdf / weight [Z, Y, X] (and color [3, Z, Y, X]) from V cameras into maps of hw = (H, W) pixels, in one launch.
    color_out: whether the colour map is made (None: iff `color` is given).  step_min is in voxels, relax the share of the
    truncated distance a step takes, refine the number of regula-falsi steps on the bracket, max_steps the bound of the march
    (None: 4 (X + Y + Z))."""
    for t, what in ((tsdf, "tsdf"), (weight, "weight"), (color, "color"), (intrinsics, "intrinsics")):
        _args.no_grad_to(t, what, _NAME)
    try:
        H, W = (int(x) for x in hw)
    except (TypeError, ValueError):
        raise ValueError(f"{_NAME}: hw must be (H, W), got {hw!r}") from None
    if H <= 0 or W <= 0 or H * W > 2 ** 31 - 1:
        raise ValueError(f"{_NAME}: hw must be two positive sizes with H * W <= 2^31 - 1, got {(H, W)!r}")
    voxel_size, trunc = _pos_finite(voxel_size, "voxel_size"), _pos_finite(trunc, "trunc")
    step_min, relax = _pos_finite(step_min, "step_min"), _pos_finite(relax, "relax")
    min_depth, max_depth, min_weight = float(min_depth), float(max_depth), float(min_weight)
    if not min_depth >= 0.0 or math.isnan(max_depth):
        raise ValueError(f"{_NAME}: min_depth must be >= 0 and max_depth not NaN, got {min_depth!r} and {max_depth!r}")
    if not min_weight > 0.0:
        raise ValueError(f"{_NAME}: min_weight must be positive, got {min_weight!r}")
    origin = tuple(float(o) for o in origin)
    if len(origin) != 3 or not all(math.isfinite(o) for o in origin):
        raise ValueError(f"{_NAME}: origin must be three finite numbers, got {origin!r}")
    if not isinstance(tsdf, Tensor) or not isinstance(weight, Tensor) or tsdf.dim() != 3 or tsdf.numel() == 0 or weight.shape != tsdf.shape:
        raise ValueError(f"{_NAME}: tsdf and weight must be non-empty [Z, Y, X] tensors of one shape, got "
                         f"{tuple(getattr(tsdf, 'shape', ()))} and {tuple(getattr(weight, 'shape', ()))}")
    Z, Y, X = tsdf.shape
    if color is not None and (not isinstance(color, Tensor) or tuple(color.shape) != (3, Z, Y, X)):
        raise ValueError(f"{_NAME}: color must be [3, {Z}, {Y}, {X}], got {tuple(getattr(color, 'shape', ()))}")
    if color_out is None:
        color_out = color is not None
    if color_out and color is None:
        raise ValueError(f"{_NAME}: a colour map needs a volume with colour planes")
    refine = int(refine)
    if not 0 <= refine <= _lib.RAYCAST_MAX_REFINE:
        raise ValueError(f"{_NAME}: refine must be in 0 .. {_lib.RAYCAST_MAX_REFINE}, got {refine}")
    max_steps = 4 * (X + Y + Z) if max_steps is None else int(max_steps)
    if not 1 <= max_steps <= _lib.RAYCAST_MAX_STEPS:
        raise ValueError(f"{_NAME}: max_steps must be in 1 .. 2^20, got {max_steps}")
    f = _args.device_f32(tsdf, "tsdf", _NAME).detach()
    w = _args.device_f32(weight, "weight", _NAME).detach()
    c = None if color is None else _args.device_f32(color, "color", _NAME).detach()
    if w.device != f.device or (c is not None and c.device != f.device):
        raise ValueError(f"{_NAME}: tsdf, weight and color must live on one device")
    rows = cam_rows(extrinsics, f.device)
    V = rows.shape[0]
    k = torch.as_tensor(intrinsics).detach().to(device=f.device, dtype=torch.float32)
    if k.shape == (4,):
        k = k.expand(V, 4)
    if tuple(k.shape) != (V, 4):
        raise ValueError(f"{_NAME}: intrinsics must be [4] or [{V}, 4] = (fx, fy, cx, cy), got {tuple(k.shape)}")
    k = k.contiguous()
    depth = torch.empty(V, H, W, device=f.device)
    nrm = torch.empty(V, 3, H, W, device=f.device) if normals else None
    col = torch.empty(V, 3, H, W, device=f.device) if color_out else None
    steps = torch.empty(V, H, W, dtype=torch.int32, device=f.device) if return_steps else None
    p = _lib.ptr
    _lib.launch("fs_tsdf_raycast", X, Y, Z, *origin, voxel_size, trunc, p(f), p(w), p(c), V, H, W, p(rows), p(k), min_depth,
                max_depth, min_weight, step_min, relax, refine, max_steps, p(depth), p(nrm), p(col), p(steps))
    return RayCast(depth, nrm, col, steps)


def weld(vertices: Tensor, colors: Tensor | None = None, drop_degenerate: bool = True):
    """Triangle soup [T, 3, 3] -> (V [n, 3], F [m, 3] int64, C [n, 3] | None): vertices with the same bits become one
    (torch.unique on the bit patterns, where the soup lives).  drop_degenerate removes the faces that name a vertex twice."""
    if vertices.dim() != 3 or tuple(vertices.shape[1:]) != (3, 3) or vertices.dtype != torch.float32:
        raise ValueError(f"{_NAME}: vertices must be a float32 triangle soup [T, 3, 3], got {tuple(vertices.shape)} {vertices.dtype}")
    if colors is not None and colors.shape != vertices.shape:
        raise ValueError(f"{_NAME}: colors must have the vertices' shape, got {tuple(colors.shape)}")
    flat = vertices.reshape(-1, 3).contiguous()
    if flat.shape[0] == 0:
        return flat, torch.zeros(0, 3, dtype=torch.int64, device=flat.device), (None if colors is None else colors.reshape(-1, 3))
    bits = flat.view(torch.int32)
    uniq, inverse = torch.unique(bits, dim=0, return_inverse=True)
    first = torch.full((uniq.shape[0],), flat.shape[0], dtype=torch.int64, device=flat.device)
    first.scatter_reduce_(0, inverse, torch.arange(flat.shape[0], device=flat.device), "amin")
    F = inverse.view(-1, 3)
    if drop_degenerate:
        F = F[(F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 0] != F[:, 2])]
    return flat[first], F, (None if colors is None else colors.reshape(-1, 3)[first])


# ---- PLY ------------------------------------------------------------------------------------------------------------------------

def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, Tensor) else np.asarray(t)


def export_mesh_ply(path, vertices, faces, colors=None) -> None:
    """Binary little-endian PLY with a vertex element (x y z float, and red green blue uchar when `colors` [n, 3] in [0, 1] is
    given) and a face element (list uchar int vertex_indices)."""
    V = np.ascontiguousarray(_np(vertices), "<f4").reshape(-1, 3)
    F = np.ascontiguousarray(_np(faces), "<i4").reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {V.shape[0]}", "property float x", "property float y",
              "property float z"]
    if colors is not None:
        Cq = np.rint(np.clip(np.nan_to_num(_np(colors).astype(np.float64).reshape(-1, 3)), 0.0, 1.0) * 255.0).astype(np.uint8)
        if Cq.shape != V.shape:
            raise ValueError(f"{_NAME}: colors must be [{V.shape[0]}, 3], got {Cq.shape}")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    if F.size and (F.min() < 0 or F.max() >= V.shape[0]):
        raise ValueError(f"{_NAME}: a face names a vertex outside 0 .. {V.shape[0] - 1}")
    header += [f"element face {F.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    vert = np.empty(V.shape[0], fields)
    vert["x"], vert["y"], vert["z"] = V[:, 0], V[:, 1], V[:, 2]
    if colors is not None:
        vert["red"], vert["green"], vert["blue"] = Cq[:, 0], Cq[:, 1], Cq[:, 2]
    face = np.empty(F.shape[0], [("n", "u1"), ("v", "<i4", (3,))])
    face["n"], face["v"] = 3, F
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vert.tobytes())
        fh.write(face.tobytes())


def read_mesh_ply(path):
    """(vertices float32 [n, 3], faces int32 [m, 3], colors uint8 [n, 3] | None) of a PLY written by export_mesh_ply."""
    with open(path, "rb") as fh:
        lines = []
        while True:
            line = fh.readline()
            if not line:
                raise ValueError(f"{_NAME}: {path}: no end_header")
            line = line.decode("ascii").strip()
            lines.append(line)
            if line == "end_header":
                break
        body = fh.read()
    if lines[:2] != ["ply", "format binary_little_endian 1.0"]:
        raise ValueError(f"{_NAME}: {path}: not a binary little-endian PLY")
    n = m = None
    props = {"vertex": [], "face": []}
    cur = None
    for line in lines[2:-1]:
        tok = line.split()
        if tok[0] == "element":
            cur = tok[1]
            if cur == "vertex":
                n = int(tok[2])
            elif cur == "face":
                m = int(tok[2])
            else:
                raise ValueError(f"{_NAME}: {path}: unexpected element {cur!r}")
        elif tok[0] == "property":
            props[cur].append(tok[1:])
    has_color = props["vertex"] == [["float", "x"], ["float", "y"], ["float", "z"], ["uchar", "red"], ["uchar", "green"], ["uchar", "blue"]]
    if n is None or m is None or props["face"] != [["list", "uchar", "int", "vertex_indices"]] or \
            not (has_color or props["vertex"] == [["float", "x"], ["float", "y"], ["float", "z"]]):
        raise ValueError(f"{_NAME}: {path}: not the vertex / face layout export_mesh_ply writes")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if has_color else [])
    vdt, fdt = np.dtype(fields), np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    if len(body) != n * vdt.itemsize + m * fdt.itemsize:
        raise ValueError(f"{_NAME}: {path}: {len(body)} bytes of data, the header promises {n * vdt.itemsize + m * fdt.itemsize}")
    vert = np.frombuffer(body, vdt, n)
    face = np.frombuffer(body, fdt, m, n * vdt.itemsize)
    if m and not (face["n"] == 3).all():
        raise ValueError(f"{_NAME}: {path}: a face that is not a triangle")
    V = np.stack([vert["x"], vert["y"], vert["z"]], 1).astype(np.float32)
    Cq = np.stack([vert["red"], vert["green"], vert["blue"]], 1) if has_color else None
    return V, face["v"].astype(np.int32).reshape(-1, 3), Cq
