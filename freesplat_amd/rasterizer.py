"""Host side of the MI355X rasterizer behind the reference's operator API.

Mirrors the interface FreeSplat imports from the (un-vendored) CUDA extension
`diff_gaussian_rasterization_depth` at /root/reference/src/model/decoder/cuda_splatting.py:5-8
and calls at :100-127:

    settings   = GaussianRasterizationSettings(image_height, image_width, tanfovx, tanfovy, bg,
                     scale_modifier, viewmatrix, projmatrix, sh_degree, campos, prefiltered, debug)
    rasterizer = GaussianRasterizer(settings)
    color, radii, depth, alpha = rasterizer(means3D, means2D, shs=..., colors_precomp=...,
                                            opacities=..., cov3D_precomp=...)

Same names, argument meaning and error behaviour (Python exceptions).  The compute is
libfreesplat_hip.so (C ABI, include/freesplat_amd.h) on the current HIP stream; there is no CPU
or eager fallback -- a CPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple, Optional

import torch
from torch import Tensor, nn

from . import _lib


# Precise tile culling (include/freesplat_amd.h FS_RASTER_TILE_CULL): images unchanged bit for bit,
# tile lists shrink to the instances that can actually contribute.  FREESPLAT_TILE_CULL=0 keeps the
# reference's full 3-sigma-square lists.
TILE_CULL = os.environ.get("FREESPLAT_TILE_CULL", "1") != "0"
# Blend-loop exponential.  Default: the CPU-reproducible polynomial exp of the bit-exact contract (forward identical to
# the oracle bit for bit).  FREESPLAT_FAST_EXP=1 (or rasterizer.FAST_EXP = True) selects the hardware v_exp_f32
# (include/freesplat_amd.h FS_RASTER_FAST_EXP): +7 % views/s at config 3; lists / ordering / radii stay identical, the
# alpha >= 1/255 decisions are those of the exact mode (guard band: a step with an alpha within 16 ulp of the threshold
# is re-evaluated with the contract exp) and the image stays within ~1e-6 of the contract.  What is left is the
# T >= 1e-4 termination: a flipped one changes a pixel by less than its remaining transmittance, 1e-4 x colour (about one
# pixel per 2 M; counted in tests and in bench.py's `fast_exp` block).  Opt-in because it is not BIT-exact.
FAST_EXP = os.environ.get("FREESPLAT_FAST_EXP", "0") == "1"
# Deterministic backward (include/freesplat_amd.h FS_RASTER_DETERMINISTIC): the blend backward stores every quadrant's sums and
# adds them per Gaussian in a fixed order instead of with float atomics, so the gradients are the same bits on every run.  On
# when this is true (FREESPLAT_DETERMINISTIC=1) or torch.use_deterministic_algorithms(True) is in force; read when the
# backward is launched (the forward and its saved state are the same in both modes).  Costs scratch and time.
DETERMINISTIC = os.environ.get("FREESPLAT_DETERMINISTIC", "0") == "1"
# Views of one render_views call are spread round-robin over this many HIP streams so that the short
# latency-bound launches of one view (tile scan, kernel tails) overlap the VALU-bound blend of another.
NUM_STREAMS = max(1, int(os.environ.get("FREESPLAT_RASTER_STREAMS", "2")))  # views of one call round-robin over this many streams


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: Tensor
    scale_modifier: float
    viewmatrix: Tensor
    projmatrix: Tensor
    sh_degree: int
    campos: Tensor
    prefiltered: bool
    debug: bool


# ---------------------------------------------------------------------------------------------
# workspace management (plumbing): the C ABI never allocates, torch's caching allocator does.
# ---------------------------------------------------------------------------------------------
class _DeviceState:
    """Per-device scratch (reused across calls on the same stream) and capacity history."""

    def __init__(self):
        self.scratch: dict[int, Tensor] = {}   # one reusable scratch per HIP stream
        self.last_instances = 0
        # capacity a past overflow asked for (retry_capacity), per image size; decays on every call that fits (note_fit):
        # one close-up view must not inflate the scratch of every later call for good
        self.retry_caps: dict[tuple[int, int], int] = {}
        self.side_streams: list = []

    @property
    def retry_cap(self) -> int:                # (largest live value: bench / tests reset it through the setter)
        return max(self.retry_caps.values(), default=0)

    @retry_cap.setter
    def retry_cap(self, v: int) -> None:
        if v == 0:
            self.retry_caps.clear()
        else:
            raise ValueError("retry_cap can only be reset to 0; use note_overflow")

    def note_overflow(self, n_inst: int, max_tile: int, H: int, W: int) -> int:
        cap = max(self.retry_caps.get((H, W), 0), retry_capacity(n_inst, max_tile, H, W))
        self.retry_caps[(H, W)] = cap
        return cap

    def note_fit(self, H: int, W: int) -> None:
        """A call of this image size fitted its capacity: let the overflow-derived capacity decay (x0.9 per call; below the
        default capacity it no longer matters and is dropped)."""
        c = self.retry_caps.get((H, W))
        if c is not None:
            c = int(c * 0.9)
            if c < (1 << 20):
                del self.retry_caps[(H, W)]
            else:
                self.retry_caps[(H, W)] = c


_states: dict[int, _DeviceState] = {}


def _state(device: torch.device) -> _DeviceState:
    idx = device.index if device.index is not None else torch.cuda.current_device()
    st = _states.get(idx)
    if st is None:
        st = _states[idx] = _DeviceState()
    return st


def _buffer_sizes(N: int, H: int, W: int, cap: int):
    out = (C.c_size_t * 4)()
    _lib.call("fs_raster_buffer_sizes", N, H, W, cap, out)
    return [int(x) for x in out]


def default_capacity(N: int, st: _DeviceState, H: int = 0, W: int = 0) -> int:
    """Instance capacity: generous (HBM is 288 GB) so the overflow retry is the rare path."""
    return max(1 << 20, 8 * N, int(st.last_instances * 1.25) + 1024, st.retry_caps.get((H, W), 0))


def retry_capacity(n_inst: int, max_tile: int, H: int, W: int) -> int:
    """Capacity for the retry after an overflow: counters = {instances, largest tile list}.  The saved lists need
    `n_inst` entries; every tile owns a fixed key area of tile_capacity(cap, T) = pow2 >= 4*cap/T slots
    (csrc/fs_common.h), which must hold the largest tile list."""
    T = ((W + 15) // 16) * ((H + 15) // 16)
    return max(n_inst + 1024, (max_tile * T + 3) // 4 + 1)


class RasterState:
    """Everything one forward leaves behind for its backward (device buffers + dims)."""

    __slots__ = ("dims", "geom", "binning", "image", "radii", "counters", "cap", "bg", "view", "proj",
                 "campos", "tanfov", "scale", "num_rendered")

    def __init__(self, dims, geom, binning, image, radii, counters, cap, bg, view, proj, campos, tanfov, scale):
        self.dims, self.geom, self.binning, self.image = dims, geom, binning, image
        self.radii, self.counters, self.cap = radii, counters, cap
        self.bg, self.view, self.proj, self.campos, self.tanfov, self.scale = bg, view, proj, campos, tanfov, scale
        self.num_rendered = -1


def _u8(n: int, dev) -> Tensor:
    return torch.empty(n, dtype=torch.uint8, device=dev)


def _images(lead: tuple, H: int, W: int, dev) -> list:      # color [*lead,3,H,W], depth [*lead,H,W], alpha [*lead,H,W]
    return [torch.empty(*lead, *c, H, W, dtype=torch.float32, device=dev) for c in ((3,), (), ())]


def _launch_forward(dims: _lib.RasterDims, means3D, cov3D, shs, colors, opacities, bg, view, proj, campos, cap: int,
                    tanfov: Optional[Tensor] = None, scale: Optional[Tensor] = None, out: Optional[tuple] = None):
    """One stream-ordered forward launch (no host sync) -> (RasterState, color, depth, alpha).  `tanfov` [2] / `scale` [1]:
    optional device-resident settings; `out` = (color[3,H,W], depth[H,W], alpha[H,W]) views to write into."""
    dev, N, H, W = means3D.device, dims.N, dims.H, dims.W
    sz = _buffer_sizes(N, H, W, cap)
    st, skey = _state(dev), torch.cuda.current_stream().cuda_stream
    scratch = st.scratch.get(skey)
    if scratch is None or scratch.numel() < sz[3]:
        scratch = st.scratch[skey] = _u8(sz[3], dev)
    rs = RasterState(dims, _u8(sz[0], dev), _u8(sz[1], dev), _u8(sz[2], dev), torch.empty(N, dtype=torch.int32, device=dev),
                     torch.empty(2, dtype=torch.int32, device=dev), cap, bg, view, proj, campos, tanfov, scale)
    color, depth, alpha = out if out is not None else _images((), H, W, dev)
    p = _lib.ptr
    _lib.launch("fs_raster_forward", C.byref(dims), p(means3D), p(cov3D), p(shs), p(colors), p(opacities), p(bg), p(view),
                p(proj), p(campos), p(tanfov), p(scale), p(rs.geom), p(rs.binning), p(rs.image), p(scratch), cap, p(color),
                p(depth), p(alpha), p(rs.radii), p(rs.counters))
    return rs, color, depth, alpha


class ViewBuffers:
    """The strided buffers of one views call (fs_raster_forward_views / fs_raster_backward_views*): the opaque buffers of the v
    views lie sz[k] bytes apart in one allocation each, the cameras are the rows of [v, ...] tensors.  state(i) is view i as
    the RasterState of a single-view forward (slices, no copies)."""

    def __init__(self, dims: _lib.RasterDims, cap: int, bgs, views, fulls, campos, tanfov, scale):
        dev, v, N = views.device, views.shape[0], dims.N
        self.dims, self.v, self.cap = dims, v, cap
        self.sz = sz = _buffer_sizes(N, dims.H, dims.W, cap)
        self.geom, self.binning, self.image = _u8(v * sz[0], dev), _u8(v * sz[1], dev), _u8(v * sz[2], dev)
        self.radii = torch.empty(v, N, dtype=torch.int32, device=dev)
        self.counters = torch.empty(v, 2, dtype=torch.int32, device=dev)
        self.bgs, self.views, self.fulls, self.campos, self.tanfov, self.scale = bgs, views, fulls, campos, tanfov, scale

    def state(self, i: int) -> RasterState:
        a, b, c = self.sz[:3]
        return RasterState(self.dims, self.geom[i * a:(i + 1) * a], self.binning[i * b:(i + 1) * b], self.image[i * c:(i + 1) * c],
                           self.radii[i], self.counters[i], self.cap, self.bgs[i], self.views[i], self.fulls[i], self.campos[i],
                           None if self.tanfov is None else self.tanfov[i], None if self.scale is None else self.scale[i])


def _side_streams(dev, v: int, n_streams: Optional[int] = None):
    """(n_streams, streams) arguments of a views call: the views alternate over min(NUM_STREAMS, v) side streams of the device
    (created on first use and kept); one stream means none, the call then runs on the current stream alone."""
    st = _state(dev)
    n = min(NUM_STREAMS, v) if n_streams is None else n_streams
    while len(st.side_streams) < n:
        st.side_streams.append(torch.cuda.Stream(device=dev))
    handles = (C.c_void_p * max(n, 1))(*[s.cuda_stream for s in st.side_streams[:n]])
    return (n if n > 1 else 0), handles


def rasterize_forward_views(dims: _lib.RasterDims, means3D, cov3D, shs, colors, opacities, bgs, views, fulls, campos, tanfov,
                            scale, cap: int, n_streams: Optional[int] = None):
    """All v views of one Gaussian set in ONE library call (fs_raster_forward_views; no host sync): per-view host work is a few
    pointer offsets instead of seven allocations and a 23-argument ctypes call, the views alternate over the side streams
    inside the library and are joined back into the current stream before the call returns.  `cov3D` in the form `dims` names
    ([N,6], [N,3,3] or the (scales, rotation) rows [N,7]).  Returns (ViewBuffers, color [v,3,H,W], depth [v,H,W],
    alpha [v,H,W]); the capacity check is the caller's (capacity_verdict on buffers.counters)."""
    dev, v, H, W = means3D.device, views.shape[0], dims.H, dims.W
    buf = ViewBuffers(dims, cap, bgs, views, fulls, campos, tanfov, scale)
    color, depth, alpha = _images((v,), H, W, dev)
    ns, handles = _side_streams(dev, v, n_streams)
    # one key area per view in flight (the projection of a whole batch of views is ONE launch)
    scratch = _u8(max(_lib.lib().fs_raster_scratch_slots(v, ns), 1) * buf.sz[3], dev)
    p = _lib.ptr
    if v > 0:
        _lib.launch("fs_raster_forward_views", C.byref(dims), v, p(means3D), p(cov3D), p(shs), p(colors), p(opacities), p(bgs),
                    p(views), p(fulls), p(campos), p(tanfov), p(scale), p(buf.geom), p(buf.binning), p(buf.image), p(scratch),
                    (C.c_size_t * 4)(*buf.sz), cap, p(color), p(depth), p(alpha), p(buf.radii), p(buf.counters), ns, handles)
    return buf, color, depth, alpha


def _f32c(t: Tensor, name: str, allow_half: bool = False) -> Tensor:
    if t.device.type != "cuda":
        raise RuntimeError(f"freesplat_amd rasterizer: `{name}` must live on a HIP device "
                           f"(got {t.device}); there is no CPU path")
    if allow_half and t.dtype == torch.float16:
        return t.contiguous()
    if t.dtype != torch.float32:
        raise RuntimeError(f"freesplat_amd rasterizer: `{name}` must be float32 (got {t.dtype})")
    return t.contiguous()


def make_dims(N, M, settings: GaussianRasterizationSettings, sh_fp16: bool = False, native_layout: bool = False,
              inference: bool = False, scale_rot: bool = False) -> _lib.RasterDims:
    """`native_layout`: shs is the reference's harmonics [N,3,M] and cov3D its covariances [N,3,3]
    (FS_RASTER_SH_CHANNEL_MAJOR | FS_RASTER_COV_FULL) instead of the rasterizer API's [N,M,3] / [N,6].
    `inference`: no backward will follow (FS_RASTER_NO_BACKWARD_STATE: the blend skips the contributor count).
    `scale_rot`: cov3D holds (scales, rotation) rows [N,7] (FS_RASTER_SCALE_ROT; not with `native_layout`)."""
    d = _lib.RasterDims()
    d.N, d.M = int(N), int(M)
    d.H, d.W = int(settings.image_height), int(settings.image_width)
    d.sh_degree = int(settings.sh_degree)
    d.tanfovx, d.tanfovy = float(settings.tanfovx), float(settings.tanfovy)
    d.flags = ((_lib.RASTER_TILE_CULL if TILE_CULL else 0) | (_lib.RASTER_SH_FP16 if sh_fp16 else 0)
               | (_lib.RASTER_FAST_EXP if FAST_EXP else 0) | (_lib.RASTER_NO_BACKWARD_STATE if inference else 0)
               | (_lib.RASTER_SCALE_ROT if scale_rot else 0))
    if native_layout:
        d.flags |= _lib.RASTER_SH_CHANNEL_MAJOR | _lib.RASTER_COV_FULL
    return d


def deterministic() -> bool:
    """Whether a backward launched now runs in the deterministic mode (FS_RASTER_DETERMINISTIC)."""
    return DETERMINISTIC or torch.are_deterministic_algorithms_enabled()


def backward_dims(dims: _lib.RasterDims) -> _lib.RasterDims:
    """The dims a backward is launched with: the forward's, plus FS_RASTER_DETERMINISTIC when deterministic() holds."""
    if not deterministic():
        return dims
    d = _lib.RasterDims.from_buffer_copy(dims)
    d.flags |= _lib.RASTER_DETERMINISTIC
    return d


def backward_scratch_bytes(dims: _lib.RasterDims, v: int, n_streams: int, cap: int) -> int:
    """fs_raster_backward_scratch_bytes: v = 0 for the single-view backward."""
    n = int(_lib.lib().fs_raster_backward_scratch_bytes(C.byref(dims), v, n_streams, cap))
    if n == 0 and dims.N > 0:
        raise _lib.FreeSplatHipError("fs_raster_backward_scratch_bytes: invalid arguments")
    return n


def capacity_verdict(st: _DeviceState, pairs, H: int, W: int, lower: bool = True, may_fit: bool = True):
    """The one reading of the instance-capacity counters.  `pairs`: the host copies of one call's counters, per view (instances,
    0 | largest tile list of an overflowed view) as int32.  Returns (instances per view, {view: capacity to re-render it with})
    and updates the capacity history of `st`:
      * every overflowed view notes its overflow (note_overflow; what that returns is the view's retry capacity);
      * a call none of whose views overflowed notes a fit -- unless `may_fit` is false: the deferred check withholds it from
        every pending call after the first overflowed one;
      * last_instances becomes the largest count of the call (a single view: its count); with `lower` false (the deferred
        check, which runs after later calls were sized) it is only ever raised."""
    counts = [int(n) & 0xFFFFFFFF for n, _ in pairs]
    redo = {i: st.note_overflow(counts[i], int(o) & 0xFFFFFFFF, H, W) for i, (_, o) in enumerate(pairs) if o}
    if not redo and may_fit:
        st.note_fit(H, W)
    worst = max(counts, default=0)
    st.last_instances = worst if lower else max(st.last_instances, worst)
    return counts, redo


def relaunched_fit(states: dict) -> list:
    """The re-rendered views {view: RasterState} must have fitted (one host sync; returns their instance counts): a second overflow
    (capacity clamp, saturated count) would leave the blend unrun and the uninitialised colour buffer returned as the image."""
    pairs = torch.stack([rs.counters for rs in states.values()]).tolist()
    bad = [i for i, (_, o) in zip(states, pairs) if o]
    if bad:
        raise _lib.FreeSplatHipError("rasterizer instance list overflowed twice" + (f" (views {bad})" if bad != [None] else ""))
    return [int(n) & 0xFFFFFFFF for n, _ in pairs]


def rasterize_forward_checked(dims, means3D, cov3D, shs, colors, opacities, bg, view, proj, campos):
    """Forward + capacity check (one host sync on the 8-byte counter pair), retrying once with the
    exact capacity when the instance list overflowed."""
    st = _state(means3D.device)
    launch = lambda cap: _launch_forward(dims, means3D, cov3D, shs, colors, opacities, bg, view, proj, campos, cap)
    rs, color, depth, alpha = launch(default_capacity(dims.N, st, dims.H, dims.W))
    (n_inst,), redo = capacity_verdict(st, [rs.counters.tolist()], dims.H, dims.W)
    if redo:
        rs, color, depth, alpha = launch(redo[0])
        n_inst, = relaunched_fit({None: rs})
        st.last_instances = n_inst
    rs.num_rendered = n_inst
    return rs, color, depth, alpha


def _alloc_grads(N: int, cov3D, shs, colors, dev) -> dict:
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    return dict(means3D=f32(N, 3), means2D=f32(N, 3), cov3D=f32(cov3D.shape), shs=None if shs is None else f32(shs.shape),
                colors=None if colors is None else f32(N, 3), opacities=f32(N))


def _cotangents(g_color, g_depth, g_alpha, shape, dev):
    """Contiguous cotangents (the caller keeps them referenced over the launch); dL_dcolor is required by the library."""
    if g_color is None:
        g_color = torch.zeros(shape, dtype=torch.float32, device=dev)
    return tuple(None if g is None else g.contiguous() for g in (g_color, g_depth, g_alpha))


def rasterize_backward(rs: RasterState, means3D, cov3D, shs, colors, opacities, g_color, g_depth, out=None,
                       accumulate: bool = False, g_alpha=None):
    """Launch the backward of one view.  `out` = dict of preallocated gradient tensors (for the
    multi-view accumulate path) or None to allocate.  `g_alpha` [H,W] | None: cotangent of the accumulated alpha."""
    dev, d, N = means3D.device, backward_dims(rs.dims), rs.dims.N
    out = _alloc_grads(N, cov3D, shs, colors, dev) if out is None else out
    if d.flags & _lib.RASTER_DETERMINISTIC:
        scratch = torch.empty(max(backward_scratch_bytes(d, 0, 0, rs.cap), 1), dtype=torch.uint8, device=dev)
    else:
        scratch = torch.empty(max(N, 1) * 12, dtype=torch.float32, device=dev)
    g_color, g_depth, g_alpha = _cotangents(g_color, g_depth, g_alpha, (3, d.H, d.W), dev)
    p = _lib.ptr
    _lib.launch("fs_raster_backward_alpha", C.byref(d), p(means3D), p(cov3D), p(shs), p(colors), p(opacities), p(rs.bg),
                p(rs.view), p(rs.proj), p(rs.campos), p(rs.tanfov), p(rs.scale), p(rs.geom), p(rs.binning), p(rs.image),
                p(rs.counters), p(g_color), p(g_depth), p(g_alpha), p(scratch), p(out["means3D"]), p(out["means2D"]),
                p(out["cov3D"]), p(out["shs"]), p(out["colors"]), p(out["opacities"]), 1 if accumulate else 0)
    return out


def rasterize_backward_views(buf: ViewBuffers, means3D, cov3D, shs, colors, opacities, g_color, g_depth, g_alpha=None,
                             row_chunks=None, chunk_ready=None, n_streams: Optional[int] = None, dims=None) -> dict:
    """The backward of all views of a rasterize_forward_views call in one library call: the blend backward of the views
    alternates over the side streams, then ONE pass over the Gaussians sums the parameter gradients of all views
    (fs_raster_backward_views; with a `g_alpha` [v,H,W] its _alpha form).  `row_chunks` = [(row0, row1), ...]: the per-Gaussian
    pass runs chunk by chunk of the rows instead (fs_raster_backward_views_rows: the blend backward with the first chunk only)
    and `chunk_ready(row0, row1, grads)` is called after each chunk is queued.  `dims`: the dims to launch with (default
    backward_dims(buf.dims)).  Returns the gradient dict of rasterize_backward."""
    dev, v = means3D.device, buf.v
    d = backward_dims(buf.dims) if dims is None else dims           # (+ FS_RASTER_DETERMINISTIC: slabs sized by the forward's capacity)
    ns, handles = _side_streams(dev, v, n_streams)
    g_color, g_depth, g_alpha = _cotangents(g_color, g_depth, g_alpha, (v, 3, d.H, d.W), dev)
    out = _alloc_grads(d.N, cov3D, shs, colors, dev)
    scratch = torch.empty(backward_scratch_bytes(d, v, ns, buf.cap), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    args = [C.byref(d), v, p(means3D), p(cov3D), p(shs), p(colors), p(opacities), p(buf.bgs), p(buf.views), p(buf.fulls),
            p(buf.campos), p(buf.tanfov), p(buf.scale), p(buf.geom), p(buf.binning), p(buf.image), p(buf.counters),
            (C.c_size_t * 3)(*buf.sz[:3]), p(g_color), p(g_depth)] + ([] if g_alpha is None else [p(g_alpha)]) + [
            p(scratch), p(out["means3D"]), p(out["means2D"]), p(out["cov3D"]), p(out["shs"]), p(out["colors"]),
            p(out["opacities"]), 0, ns, handles, _lib.current_stream()]
    name = "fs_raster_backward_views" + ("" if row_chunks is None else "_rows") + ("" if g_alpha is None else "_alpha")
    if row_chunks is None:
        _lib.call(name, *args)
    for ci, (c0, c1) in enumerate(row_chunks or ()):
        _lib.call(name, *args, c0, c1 - c0, 1 if ci == 0 else 0)
        if chunk_ready is not None:
            chunk_ready(c0, c1, out)
    return out


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, shs, colors_precomp, opacities, cov3D, settings, scale_rot=False):
        # scale_rot: cov3D = (scales, rotation) rows [N,7] (FS_RASTER_SCALE_ROT), else the covariances [N,6]
        N = means3D.shape[0]
        M = 0 if shs is None else shs.shape[1]
        dims = make_dims(N, M, settings, sh_fp16=shs is not None and shs.dtype == torch.float16,
                         inference=not any(ctx.needs_input_grad[:6]), scale_rot=scale_rot)
        bg = _f32c(settings.bg, "bg")
        view = _f32c(settings.viewmatrix, "viewmatrix")
        proj = _f32c(settings.projmatrix, "projmatrix")
        campos = _f32c(settings.campos, "campos")
        rs, color, depth, alpha = rasterize_forward_checked(dims, means3D, cov3D, shs, colors_precomp,
                                                            opacities, bg, view, proj, campos)
        ctx.rs = rs
        ctx.opac_shape = None
        ctx.save_for_backward(means3D, cov3D, shs, colors_precomp, opacities)
        ctx.mark_non_differentiable(rs.radii)
        ctx.set_materialize_grads(False)
        return color, rs.radii, depth, alpha

    @staticmethod
    def backward(ctx, g_color, _g_radii, g_depth, g_alpha):
        means3D, cov3D, shs, colors, opacities = ctx.saved_tensors
        if g_color is None and g_depth is None and g_alpha is None:
            return (None,) * 8
        g = rasterize_backward(ctx.rs, means3D, cov3D, shs, colors, opacities, g_color, g_depth, g_alpha=g_alpha)
        g_shs = g["shs"] if (shs is None or shs.dtype == torch.float32) else g["shs"].to(shs.dtype)
        return g["means3D"], g["means2D"], g_shs, g["colors"], g["opacities"], g["cov3D"], None, None


def build_cov3d(scales: Tensor, rotations: Tensor, scale_modifier: float) -> Tensor:
    """cov3D 6-vector from scales [N,3] and rotations [N,4] (w,x,y,z) -- the (scales, rotations)
    input form of the original extension, as plain differentiable torch ops.  The definition the kernels follow
    (FS_RASTER_SCALE_ROT forms the same covariance in registers; GaussianRasterizer no longer calls this): kept as the
    eager yardstick of the tests and profiles/scale_rot_alpha_bench.py."""
    q = rotations / rotations.norm(dim=-1, keepdim=True)
    r, x, y, z = q.unbind(-1)
    R = torch.stack([
        1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    Mx = R * (scales * scale_modifier)[:, None, :]
    S = Mx @ Mx.transpose(1, 2)
    i, j = torch.triu_indices(3, 3)
    return S[:, i, j]


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None,
                rotations=None, cov3D_precomp=None):
        s = self.raster_settings
        if (shs is None) == (colors_precomp is None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        means3D = _f32c(means3D, "means3D")
        N = means3D.shape[0]
        scale_rot = cov3D_precomp is None
        if scale_rot:
            # (scales, rotations): one [N,7] row per Gaussian, the covariance is formed in the kernels (FS_RASTER_SCALE_ROT);
            # autograd of the cat splits the row gradients back into the two inputs
            scales = _f32c(scales, "scales").reshape(N, 3)
            rotations = _f32c(rotations, "rotations").reshape(N, 4)
            if float(s.scale_modifier) != 1.0:
                scales = scales * float(s.scale_modifier)
            cov3D = torch.cat([scales, rotations], 1)
        else:
            cov3D = _f32c(cov3D_precomp, "cov3D_precomp").reshape(N, 6)
        opac = _f32c(opacities, "opacities").reshape(N)
        if shs is not None:
            shs = _f32c(shs, "shs", allow_half=True)   # fp16 = storage-only SH (FS_RASTER_SH_FP16)
            if shs.dim() != 3 or shs.shape[0] != N or shs.shape[2] != 3:
                raise RuntimeError(f"shs must be [N, M, 3], got {tuple(shs.shape)}")
            if (int(s.sh_degree) + 1) ** 2 > shs.shape[1] or int(s.sh_degree) > 3:
                raise RuntimeError(f"sh_degree {s.sh_degree} unsupported for shs with {shs.shape[1]} coefficients "
                                   "(degree <= 3)")
        else:
            colors_precomp = _f32c(colors_precomp, "colors_precomp").reshape(N, 3)
        if means2D is None:
            means2D = torch.zeros(N, 3, dtype=torch.float32, device=means3D.device)
        return _RasterizeGaussians.apply(means3D, means2D, shs, colors_precomp, opac, cov3D, s, scale_rot)


# --- debug views into the opaque buffers (tests only) -------------------------------------------
def debug_state(rs: RasterState) -> dict:
    """Copy the forward's internal state to host numpy arrays (test helper)."""
    import numpy as np
    d = rs.dims
    L = _lib.lib()
    T = ((d.W + 15) // 16) * ((d.H + 15) // 16)
    # where the library keeps the parts of its buffers: its own accessors, as offsets from a buffer's first byte
    b0, i0 = rs.binning.data_ptr(), rs.image.data_ptr()
    off_ranges, off_bytes = L.fs_raster_tile_ranges(b0, d.H, d.W) - b0, L.fs_raster_point_list(b0, d.H, d.W) - b0
    binning = rs.binning.cpu().numpy()
    offsets = binning[off_ranges: off_ranges + (T + 1) * 4].view(np.uint32).copy()
    I = int(offsets[-1])
    words = binning[off_bytes: off_bytes + I * 4].view(np.uint32).copy()
    point_list, quad = words >> 4, words & 15
    geom = rs.geom.cpu().numpy()
    N = d.N
    rec = geom[: N * 48].view(np.float32).reshape(N, 12).copy()
    o1 = (N * 48 + 255) // 256 * 256
    rect = geom[o1: o1 + N * 8].view(np.uint16).reshape(N, 4).copy()
    o2 = o1 + (N * 8 + 255) // 256 * 256
    clamp = geom[o2: o2 + N].copy()
    P = d.H * d.W
    img = rs.image.cpu().numpy()
    oT, o3 = L.fs_raster_final_T(i0) - i0, L.fs_raster_n_contrib(i0, d.H, d.W) - i0
    final_T = img[oT: oT + P * 4].view(np.float32).reshape(d.H, d.W).copy()
    n_contrib = img[o3: o3 + P * 4].view(np.int32).reshape(d.H, d.W).copy()
    return dict(offsets=offsets, point_list=point_list, quad=quad, rec=rec, rect=rect, clamp=clamp,
                final_T=final_T, n_contrib=n_contrib, radii=rs.radii.cpu().numpy(),
                num_rendered=I)
