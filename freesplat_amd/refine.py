"""Per-scene refinement of fused Gaussians: the parameter update on the device, through fs_gaussian_adam_step
(libfreesplat_hip.so, include/freesplat_amd_optim.h, csrc/gaussian_adam.hip).

`GaussianAdam` owns the raw parameters of one scene (means, log-scales, rotations, opacity logits, SH), their Adam moments,
the six learning rates and the step counter, all on the device.  It exposes five leaves in the form
`GaussianRasterizer(...)(means3D, means2D, opacities, shs=, scales=, rotations=)` takes: `.means`, `.rotations` and `.shs` ARE
the raw arrays; `.scales` and `.opacities` hold exp(log-scales) and sigmoid(logits), rewritten by every step from the new raw
values.  `step()` is one library call: the chain rule through exp / sigmoid, Adam over the five arrays and the activation of
the result in one pass over the bytes (DESIGN.md "Gaussian Adam").  With `sparse=True` a step takes the rasterizer's `radii`
and skips every Gaussian the view did not see -- its gradients are not read, its parameters and moments are not written (the
sparse Adam of 3DGS trainers).  Nothing synchronises with the host; a step can be captured in a graph.  Device tensors only:
there is no CPU / eager path.

Adaptive density control (include/freesplat_amd_density.h, csrc/gaussian_density.hip, DESIGN.md "Gaussian density control"):
`.viewspace` goes in as the rasterizer's `means2D`, `accumulate(radii)` folds its gradient into per-Gaussian statistics,
`densify(extent, ...)` clones, splits and prunes in one compaction over parameters and moments and REPLACES the leaves with
tensors of the new size, `reset_opacity()` clamps the opacities.  densify() reads four counters back to size the new buffers:
the one host synchronisation of this module, once per densification.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import Tensor

from . import _args, _lib

ARRAYS = ("means", "scales", "rotations", "opacities", "shs")                       # FS_OPTIM_MEANS ... FS_OPTIM_SHS
GROUPS = ("means", "scales", "rotations", "opacity", "sh_dc", "sh_rest")            # FS_OPTIM_LR_*: the order of `lr`
DEFAULT_LR = dict(means=1.6e-4, sh_dc=2.5e-3, sh_rest=1.25e-4, opacity=5e-2, scales=5e-3, rotations=1e-3)   # the usual 3DGS rates
_RAW = ("means", "log_scales", "rotations", "logits", "shs")                        # state_dict names of the raw arrays
_STATS = ("grad_accum", "denom", "max_radii")                                       # density statistics, "density." + name in a state_dict


def _device_f32(t, what: str) -> Tensor:
    _args.device_tensor(t, what, "freesplat_amd.refine")
    if t.dtype != torch.float32:
        raise ValueError(f"freesplat_amd.refine: {what} must be float32, got {t.dtype}")
    return t.detach()


def _table(tensors) -> C.Array:
    return (C.c_void_p * len(ARRAYS))(*[None if t is None else t.data_ptr() for t in tensors])


class GaussianAdam:
    """Adam over the Gaussians of one scene.  means [N,3], scales [N,3] (> 0), rotations [N,4] (w, x, y, z; any norm),
    opacities [N] or [N,1] (inside (0, 1)), shs [N,M,3] with M in {1, 4, 9, 16}: float32 device tensors, copied.  `lr`: a dict
    over GROUPS that overrides DEFAULT_LR."""

    def __init__(self, means, scales, rotations, opacities, shs, lr=None, betas=(0.9, 0.999), eps=1e-15, sparse=False):
        means, scales, rotations = _device_f32(means, "means"), _device_f32(scales, "scales"), _device_f32(rotations, "rotations")
        opacities, shs = _device_f32(opacities, "opacities"), _device_f32(shs, "shs")
        dev = means.device
        if means.dim() != 2 or means.shape[1] != 3:
            raise ValueError(f"freesplat_amd.refine: means must be [N, 3], got {tuple(means.shape)}")
        N = means.shape[0]
        if shs.dim() != 3 or shs.shape[0] != N or shs.shape[2] != 3 or shs.shape[1] not in (1, 4, 9, 16):
            raise ValueError(f"freesplat_amd.refine: shs must be [N, M, 3] with M in (1, 4, 9, 16), got {tuple(shs.shape)}")
        if tuple(scales.shape) != (N, 3) or tuple(rotations.shape) != (N, 4) or opacities.numel() != N:
            raise ValueError(f"freesplat_amd.refine: expected scales [{N}, 3], rotations [{N}, 4], opacities [{N}], got "
                             f"{tuple(scales.shape)}, {tuple(rotations.shape)}, {tuple(opacities.shape)}")
        if any(t.device != dev for t in (scales, rotations, opacities, shs)):
            raise ValueError("freesplat_amd.refine: the five tensors must live on one device")
        if N == 0:
            raise ValueError("freesplat_amd.refine: no Gaussians")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0) or eps < 0.0:
            raise ValueError(f"freesplat_amd.refine: betas must lie in [0, 1) and eps must not be negative, got {betas}, {eps}")
        rates = dict(DEFAULT_LR)
        for k, v in (lr or {}).items():
            if k not in rates:
                raise ValueError(f"freesplat_amd.refine: learning-rate group must be one of {GROUPS}, got {k!r}")
            rates[k] = float(v)
        self.N, self.M, self.sparse = N, int(shs.shape[1]), bool(sparse)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        # the activations are inverted once, eagerly; from here on only the kernel's own exp / sigmoid touch the parameters
        opacities = opacities.reshape(N)
        values = (means, torch.log(scales), rotations, torch.log(opacities) - torch.log1p(-opacities), shs)
        if not all(bool(torch.isfinite(t).all()) for t in values):
            raise ValueError("freesplat_amd.refine: scales must be positive, opacities strictly inside (0, 1), and every value finite")
        self._raw = [torch.empty(t.shape, dtype=torch.float32, device=dev).copy_(t) for t in values]
        self.exp_avg = [torch.zeros(t.shape, dtype=torch.float32, device=dev) for t in values]
        self.exp_avg_sq = [torch.zeros(t.shape, dtype=torch.float32, device=dev) for t in values]
        self.lr = torch.empty(len(GROUPS), dtype=torch.float32, device=dev).copy_(torch.tensor([rates[k] for k in GROUPS]))
        self.step_count = torch.zeros(1, dtype=torch.int32, device=dev)
        self._scales = torch.empty(N, 3, dtype=torch.float32, device=dev)
        self._opacities = torch.empty(N, 1, dtype=torch.float32, device=dev)
        self._activate()
        self.densify_calls = 0
        self._bind()

    def _bind(self) -> None:
        """Leaves, pointer tables, density statistics and the view-space leaf for the buffers this object holds now."""
        dev = self.lr.device
        self.means, self.rotations, self.shs = (self._raw[i].requires_grad_(True) for i in (0, 2, 4))
        self.scales, self.opacities = self._scales.requires_grad_(True), self._opacities.requires_grad_(True)
        self._tables = tuple(_table(ts) for ts in (self._raw, self.exp_avg, self.exp_avg_sq))
        self.grad_accum, self.denom, self.max_radii = (torch.zeros(self.N, dtype=torch.float32, device=dev) for _ in _STATS)
        self.viewspace = torch.zeros(self.N, 3, dtype=torch.float32, device=dev).requires_grad_(True)

    @classmethod
    def from_gaussians(cls, gaussians, **kw) -> "GaussianAdam":
        """From the adapter's / encoder's `Gaussians` of ONE scene (means [g,3] or [1,g,3], covariances [.., g,3,3], harmonics
        [.., g,3,d_sh], opacities [.., g]).  The (scales, rotations) form is taken from the world-space covariances (their
        eigen-decomposition, once): the adapter's own scales / rotations describe the Gaussian in its camera's frame.
        harmonics are transposed to [N,M,3] once."""
        means = gaussians.means
        if means.dim() == 3 and means.shape[0] == 1:
            means = means[0]
        if means.dim() != 2:
            raise ValueError(f"freesplat_amd.refine: from_gaussians takes the Gaussians of one scene, got means {tuple(gaussians.means.shape)}")
        N = means.shape[0]
        cov = _device_f32(gaussians.covariances, "covariances").reshape(N, 3, 3)
        scales, rotations = scale_rot_from_covariances(cov)
        shs = _device_f32(gaussians.harmonics, "harmonics").reshape(N, 3, -1).transpose(1, 2).contiguous()
        return cls(_device_f32(means, "means").contiguous(), scales, rotations,
                   _device_f32(gaussians.opacities, "opacities").reshape(N), shs, **kw)

    def leaves(self):
        return [getattr(self, k) for k in ARRAYS]

    def _activate(self) -> None:
        p = _lib.ptr
        _lib.launch("fs_gaussian_activate", self.N, p(self._raw[1]), p(self._raw[3]), p(self._scales), p(self._opacities))

    def zero_grad(self) -> None:
        for t in self.leaves():
            t.grad = None

    def set_lr(self, name: str, value: float) -> None:
        """A stream-ordered write of one rate: steps queued before it keep the old value, steps after it see the new one (also
        between the replays of a captured graph)."""
        if name not in GROUPS:
            raise ValueError(f"freesplat_amd.refine: learning-rate group must be one of {GROUPS}, got {name!r}")
        k = GROUPS.index(name)
        self.lr[k:k + 1].fill_(float(value))

    def step(self, radii=None) -> None:
        """Consume the `.grad` of the leaves (a leaf without one is left untouched), update raw parameters and moments,
        rewrite `.scales` / `.opacities`, and clear the grads.  sparse=True: `radii` (int32 [N], the rasterizer's second
        output) is required, Gaussians with radii <= 0 are skipped whole.  A dense optimizer ignores `radii`."""
        visible = None
        if self.sparse:
            if radii is None:
                raise ValueError("freesplat_amd.refine: a sparse step needs the rasterizer's radii")
            if not isinstance(radii, Tensor) or radii.device != self.lr.device or radii.dtype != torch.int32 or radii.numel() != self.N:
                raise ValueError(f"freesplat_amd.refine: radii must be an int32 [{self.N}] tensor on {self.lr.device}")
            visible = radii.detach().contiguous()
        grads = []
        for name, leaf in zip(ARRAYS, self.leaves()):
            g = leaf.grad
            if g is not None:
                if g.shape != leaf.shape or g.device != leaf.device:
                    raise ValueError(f"freesplat_amd.refine: the gradient of {name} is {tuple(g.shape)} on {g.device}")
                if g.dtype != torch.float32 or not g.is_contiguous():
                    g = g.float().contiguous()
            grads.append(g)
        if all(g is None for g in grads):
            raise ValueError("freesplat_amd.refine: step() without any gradient (call backward() first)")
        p = _lib.ptr
        with torch.no_grad():
            _lib.launch("fs_gaussian_adam_step", self.N, self.M, self._tables[0], _table(grads), self._tables[1], self._tables[2],
                        p(visible), p(self.lr), p(self.step_count), self.betas[0], self.betas[1], self.eps, p(self._scales),
                        p(self._opacities))
        self.zero_grad()

    # ---- adaptive density control ----------------------------------------------------------------------------------------

    def _radii(self, radii) -> Tensor:
        if not isinstance(radii, Tensor) or radii.device != self.lr.device or radii.dtype != torch.int32 or tuple(radii.shape) != (self.N,):
            raise ValueError(f"freesplat_amd.refine: radii must be an int32 [{self.N}] tensor on {self.lr.device}")
        return radii.detach().contiguous()

    def accumulate(self, radii) -> None:
        """Fold the view-space gradient of the last backward into the density statistics: for every Gaussian the view saw
        (radii > 0) the norm of the (x, y) gradient of `.viewspace` (NDC units) is added to `grad_accum`, `denom` counts the
        view, `max_radii` keeps the largest screen radius.  Consumes and clears `viewspace.grad`; one library call, no host
        synchronisation.  Independent of step(): either order gives the same result (step() does not touch viewspace.grad)."""
        g = self.viewspace.grad
        if g is None:
            raise ValueError("freesplat_amd.refine: accumulate() without a view-space gradient (pass opt.viewspace as the "
                             "rasterizer's means2D and call backward() first)")
        radii = self._radii(radii)
        if tuple(g.shape) != (self.N, 3) or g.device != self.lr.device:
            raise ValueError(f"freesplat_amd.refine: the gradient of viewspace is {tuple(g.shape)} on {g.device}")
        if g.dtype != torch.float32 or not g.is_contiguous():
            g = g.float().contiguous()
        p = _lib.ptr
        _lib.launch("fs_density_accumulate", self.N, p(g), p(radii), p(self.grad_accum), p(self.denom), p(self.max_radii))
        self.viewspace.grad = None

    def _plan(self, thresholds):
        """fs_density_plan with six float thresholds -> (kind, offset, src, [n_out, n_cloned, n_split, n_dropped]); the list is
        read back to the host (a synchronisation)."""
        dev, N, p = self.lr.device, self.N, _lib.ptr
        L = _lib.lib()
        kind = torch.empty(N, dtype=torch.uint8, device=dev)
        offset = torch.empty(N, dtype=torch.int32, device=dev)               # uint32 in the library
        src = torch.empty(2 * N, dtype=torch.int32, device=dev)              # uint32 in the library
        totals = torch.empty(4, dtype=torch.int32, device=dev)
        scratch = torch.empty(int(L.fs_density_plan_scratch_bytes(N)), dtype=torch.uint8, device=dev)
        _lib.launch("fs_density_plan", N, p(self.grad_accum), p(self.denom), p(self.max_radii), p(self._scales),
                    p(self._opacities), *thresholds, p(kind), p(offset), p(src), p(totals), p(scratch))
        return kind, offset, src, [int(x) for x in totals.tolist()]

    def densify(self, extent, grad_threshold=2e-4, min_opacity=0.005, percent_dense=0.01, max_screen_size=None, prune_big=False,
                seed=None, max_gaussians=None) -> dict:
        """Clone, split and prune in one pass (the set 3DGS's clone -> split -> prune sequence leaves).  With avg = grad_accum /
        denom over the views accumulated since the last densify and s_max the largest scale of a Gaussian:
          avg >= grad_threshold and s_max <= percent_dense * extent   clone: the Gaussian keeps its moments, a copy starts with none
          avg >= grad_threshold and s_max >  percent_dense * extent   split: two children, scales / 1.6, means drawn from the parent
          opacity < min_opacity, screen radius > max_screen_size (if given), s_max > 0.1 * extent (if prune_big)   dropped
        (a split parent is dropped when its children would exceed 0.1 * extent; its screen radius is not tested).  `extent`: the
        scene's radius in world units.  `seed`: of the children's positions; None = the number of densify calls so far.
        `max_gaussians`: if the result would be larger, the plan is redone with cloning and splitting off (prune only).
        Returns {n_out, n_cloned, n_split, n_dropped}.

        The new size is known only on the device: the four counters are read back before the new buffers are allocated.  That
        read is the ONE host synchronisation of this module; it happens once per densification (twice when max_gaussians
        forces the prune-only plan), never per step.

        The raw arrays, both moments, the pointer tables and the leaves `.means`, `.scales`, `.rotations`, `.opacities`, `.shs`
        and `.viewspace` are REPLACED by tensors of the new size: re-read the leaves after a densify (tensors taken before it
        are stale), and capture a graph of step() again.  The density statistics start from zero; step_count, lr, betas and
        eps are kept.  A result of no Gaussians raises ValueError and leaves the optimizer untouched."""
        inf = float("inf")
        dense_scale = float(percent_dense) * float(extent)
        prune_scale = 0.1 * float(extent) if prune_big else 0.0
        screen = 0.0 if max_screen_size is None else float(max_screen_size)
        th = [float(grad_threshold), dense_scale, float(min_opacity), screen, prune_scale, 1.6 * prune_scale]
        if not all(t >= 0.0 for t in th):
            raise ValueError(f"freesplat_amd.refine: densify thresholds must not be negative or NaN, got grad_threshold={grad_threshold}, "
                             f"extent={extent}, percent_dense={percent_dense}, min_opacity={min_opacity}, max_screen_size={max_screen_size}")
        seed = self.densify_calls if seed is None else int(seed)
        kind, offset, src, totals = self._plan(th)
        if max_gaussians is not None and totals[0] > int(max_gaussians):
            kind, offset, src, totals = self._plan([inf] + th[1:])
        n_out = totals[0]
        if n_out == 0:
            raise ValueError("freesplat_amd.refine: densify() would drop every Gaussian; the optimizer is unchanged")
        dev, p = self.lr.device, _lib.ptr
        new = [[torch.empty((n_out,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev) for t in self._raw] for _ in range(3)]
        scales = torch.empty(n_out, 3, dtype=torch.float32, device=dev)
        opacities = torch.empty(n_out, 1, dtype=torch.float32, device=dev)
        with torch.no_grad():
            _lib.launch("fs_density_apply", self.N, self.M, n_out, p(src), *self._tables, *[_table(ts) for ts in new], p(scales),
                        p(opacities), seed & 0xFFFFFFFF)
        self.N = n_out
        self._raw, self.exp_avg, self.exp_avg_sq = new
        self._scales, self._opacities = scales, opacities
        self._bind()
        self.densify_calls += 1
        return dict(zip(("n_out", "n_cloned", "n_split", "n_dropped"), totals))

    def reset_opacity(self, max_opacity=0.01) -> None:
        """opacity = min(opacity, max_opacity) on the raw logits, both opacity moments set to zero, `.opacities` rewritten: one
        launch, no host synchronisation.  Everything else is left as it is."""
        if not 0.0 < float(max_opacity) < 1.0:
            raise ValueError(f"freesplat_amd.refine: max_opacity must lie inside (0, 1), got {max_opacity}")
        p = _lib.ptr
        with torch.no_grad():
            _lib.launch("fs_density_reset_opacity", self.N, float(max_opacity), p(self._raw[3]), p(self.exp_avg[3]),
                        p(self.exp_avg_sq[3]), p(self._opacities))

    def transform_(self, transform) -> None:
        """Move the scene by the similarity `transform` (a 4 x 4 [s R | t] or a tuple (s, R, t), as
        freesplat_amd.transform.transform_gaussians takes it) in place: means = s R means + t, log-scales + log s, rotations =
        q_R (x) rotations, every SH band rotated, opacity logits untouched; `.scales` / `.opacities` are rewritten.  The leaves
        stay the same tensors.  Both moments, the step counter, the density statistics and pending gradients are reset, as a
        fresh optimizer built from the transformed values would have them: moments of the old frame do not point anywhere
        in the new one.  lr, betas and eps are kept.  One table launch and two kernels; a host transform is validated
        (ValueError), a device transform is taken as given without synchronisation."""
        from . import transform as X
        xf, _ = X._xf(transform, self.lr.device)
        if xf.shape[0] != 1:
            raise ValueError(f"freesplat_amd.refine: transform_() takes one transform, got {xf.shape[0]}")
        table = X.prepare_table(xf)
        p = _lib.ptr
        means, rot, shs = self._raw[0], self._raw[2], self._raw[4]
        with torch.no_grad():
            _lib.launch("fs_gaussians_transform_forward", self.N, self.M, 1, 0, p(table), None, p(means), None, p(rot), None,
                        p(shs), p(means), None, p(rot), None, p(shs))
            self._raw[1].add_(torch.log(table[0, _lib.TRANSFORM_S]))
            for t in self.exp_avg + self.exp_avg_sq + [self.step_count, self.grad_accum, self.denom, self.max_radii]:
                t.zero_()
            self._activate()
        self.zero_grad()
        self.viewspace.grad = None

    def observed(self, extrinsics):
        """The five leaves for ONE rendered view whose camera is to receive a gradient: (means, scales, rotations, opacities,
        shs) with means, scales, rotations and shs routed through freesplat_amd.pose.observe(extrinsics, ...) -- the identity
        forward; backward, the leaves get their gradients bit for bit and `extrinsics` (a device [4, 4] camera-to-world matrix
        that requires grad) gets the camera's.  Opacities do not move with a pose and are the leaf itself."""
        from .pose import observe
        means, scales, rotations, _, shs = observe(extrinsics, means=self.means, scales=self.scales, rotations=self.rotations,
                                                   harmonics=self.shs, quat_order="wxyz", sh_layout="coeff_major")
        return means, scales, rotations, self.opacities, shs

    def state_dict(self) -> dict:
        """Copies of the raw parameters, both moments, the density statistics, the step counter and the rates (device tensors)
        and the scalars."""
        out = {k: t.detach().clone() for k, t in zip(_RAW, self._raw)}
        out.update({"exp_avg." + k: t.clone() for k, t in zip(_RAW, self.exp_avg)})
        out.update({"exp_avg_sq." + k: t.clone() for k, t in zip(_RAW, self.exp_avg_sq)})
        out.update({"density." + k: getattr(self, k).clone() for k in _STATS})
        out.update(step=self.step_count.clone(), lr=self.lr.clone(), betas=self.betas, eps=self.eps, sparse=self.sparse)
        return out

    def load_state_dict(self, state: dict) -> None:
        """Into the buffers this object already owns (the leaves stay the same tensors); `.scales` / `.opacities` are rewritten
        from the loaded raw values.  betas, eps and `sparse` are taken over as well; the density statistics are taken when the
        state has them and zeroed when it does not."""
        pairs = [(t, state[k]) for k, t in zip(_RAW, self._raw)]
        pairs += [(t, state["exp_avg." + k]) for k, t in zip(_RAW, self.exp_avg)]
        pairs += [(t, state["exp_avg_sq." + k]) for k, t in zip(_RAW, self.exp_avg_sq)]
        pairs += [(self.step_count, state["step"]), (self.lr, state["lr"])]
        pairs += [(getattr(self, k), state["density." + k]) for k in _STATS if "density." + k in state]
        for dst, src in pairs:
            if tuple(dst.shape) != tuple(src.shape) or dst.dtype != src.dtype:
                raise ValueError(f"freesplat_amd.refine: state of shape {tuple(src.shape)} {src.dtype} for a buffer "
                                 f"{tuple(dst.shape)} {dst.dtype}")
        with torch.no_grad():
            for k in _STATS:
                if "density." + k not in state:
                    getattr(self, k).zero_()
            for dst, src in pairs:
                dst.copy_(src)
            self._activate()
        self.betas, self.eps = (float(state["betas"][0]), float(state["betas"][1])), float(state["eps"])
        self.sparse = bool(state["sparse"])
        self.zero_grad()


def scale_rot_from_covariances(cov: Tensor):
    """World-space covariances [N,3,3] -> (scales [N,3], rotations [N,4] as (w, x, y, z)) with R diag(s^2) R^T = cov: the
    eigen-decomposition in float64, eigenvalues floored at 1e-12 of the largest of the scene, the eigenvector frame made right-handed."""
    dev = _device_f32(cov, "covariances").device
    cov = cov.detach().double().cpu()       # one-time set-up on the host: batched 3x3 eigh on the device is one solver call per matrix
    w, V = torch.linalg.eigh(0.5 * (cov + cov.transpose(1, 2)))
    V = V * torch.where(torch.linalg.det(V) < 0, -1.0, 1.0)[:, None, None]
    scales = w.clamp_min(1e-12 * float(w.max())).sqrt()
    m = lambda i, j: V[:, i, j]
    # four candidate quaternions, each exact where its own component is the largest; take that one
    q2 = torch.stack([1 + m(0, 0) + m(1, 1) + m(2, 2), 1 + m(0, 0) - m(1, 1) - m(2, 2),
                      1 - m(0, 0) + m(1, 1) - m(2, 2), 1 - m(0, 0) - m(1, 1) + m(2, 2)], 1)
    cand = torch.stack([
        torch.stack([q2[:, 0], m(2, 1) - m(1, 2), m(0, 2) - m(2, 0), m(1, 0) - m(0, 1)], 1),
        torch.stack([m(2, 1) - m(1, 2), q2[:, 1], m(1, 0) + m(0, 1), m(0, 2) + m(2, 0)], 1),
        torch.stack([m(0, 2) - m(2, 0), m(1, 0) + m(0, 1), q2[:, 2], m(2, 1) + m(1, 2)], 1),
        torch.stack([m(1, 0) - m(0, 1), m(0, 2) + m(2, 0), m(2, 1) + m(1, 2), q2[:, 3]], 1)], 1)
    q = cand[torch.arange(cov.shape[0]), q2.argmax(1)]
    q = q / q.norm(dim=1, keepdim=True)
    return scales.float().to(dev), q.float().to(dev)
