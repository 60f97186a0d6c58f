"""Restatement of TSDF ray casting (include/freesplat_ext_raycast.h) in vectorised numpy: the oracle of
tests/test_tsdf_raycast_host.py, tests/test_tsdf_raycast_hip.py and smoke().

Two modes, chosen by `dtype`, as in tests/tsdf_ref.py:
  np.float32   every operation of the header in the header's association order, each rounded on its own: the bits the kernel
               must give.
  np.float64   the same formulas in double from the same fp32 inputs: the value the fp32 result is bounded against.

A volume is the dict of tests/tsdf_ref.py.  Vectorised over the pixels of a view; Python loops run over views, march samples
and refinement steps only (each over the rays still alive)."""
import numpy as np

DEFAULTS = dict(min_depth=0.0, max_depth=np.inf, min_weight=1.0, step_min=0.5, relax=0.8, refine=4, max_steps=None)
# what the refinement did in one step: two bits per step of `branch`, step 0 lowest
UNOBSERVED, MOVED_B, MOVED_A = 0, 1, 2


def min2(a, b):
    return np.where((a < b) | np.isnan(b), a, b)


def max2(a, b):
    return np.where((a > b) | np.isnan(b), a, b)


def lerp(a, b, t):
    return a + t * (b - a)


def trilerp(c, t):
    c00, c01, c10, c11 = lerp(c[0], c[1], t[0]), lerp(c[2], c[3], t[0]), lerp(c[4], c[5], t[0]), lerp(c[6], c[7], t[0])
    return lerp(lerp(c00, c01, t[1]), lerp(c10, c11, t[1]), t[2])


def gradient(c, t):
    return (lerp(lerp(c[1] - c[0], c[3] - c[2], t[1]), lerp(c[5] - c[4], c[7] - c[6], t[1]), t[2]),
            lerp(lerp(c[2] - c[0], c[3] - c[1], t[0]), lerp(c[6] - c[4], c[7] - c[5], t[0]), t[2]),
            lerp(lerp(c[4] - c[0], c[5] - c[1], t[0]), lerp(c[6] - c[2], c[7] - c[3], t[0]), t[1]))


class _Field:
    def __init__(self, vol, f, min_weight):
        self.f = f
        self.dims = X, Y, Z = vol["dims"]
        self.offsets = [(q & 1) + ((q >> 1) & 1) * X + ((q >> 2) & 1) * X * Y for q in range(8)]
        self.tsdf = np.ascontiguousarray(vol["tsdf"]).reshape(-1).astype(f)
        self.weight = np.ascontiguousarray(vol["weight"], np.float32).reshape(-1)
        self.color = None if vol["color"] is None else np.ascontiguousarray(vol["color"]).reshape(3, -1).astype(f)
        self.min_weight = np.float32(min_weight)

    def cell(self, o, d, s):
        """Step 4's cell of the points o + s d: (linear index of corner 0, (t_x, t_y, t_z))."""
        f = self.f
        idx, t = [], []
        for c in range(3):
            g = o[c] + s * d[c]
            fl = np.floor(g)
            fi = np.where(fl > 0, fl, f(0))
            fi = np.where(fi < f(self.dims[c] - 2), fi, f(self.dims[c] - 2))
            idx.append(fi.astype(np.int64))
            t.append(g - fi)
        X, Y, _ = self.dims
        return (idx[2] * Y + idx[1]) * X + idx[0], t

    def sample(self, o, d, s):
        """(observed, value, cell, t, the eight corner values)."""
        cell, t = self.cell(o, d, s)
        obs = np.ones(cell.shape, bool)
        for off in self.offsets:
            obs &= self.weight[cell + off] >= self.min_weight
        c = [self.tsdf[cell + off] for off in self.offsets]
        return obs, trilerp(c, t), cell, t, c


def raycast(vol, cam_to_world, intrinsics, hw, dtype=np.float32, color=None, **kw):
    """vol: a tests/tsdf_ref.py volume; cam_to_world [V, 3, 4], intrinsics [V, 4] fp32; hw = (H, W); the scalars of DEFAULTS.
    color: None = iff the volume has colour.  Returns a dict: depth [V, H, W], normals [V, 3, H, W], color [V, 3, H, W] | None
    (arrays of `dtype`), steps [V, H, W] int32, and the decision record hit, valid [V, H, W] bool, branch [V, H, W] int64."""
    f = dtype
    p = dict(DEFAULTS, **kw)
    X, Y, Z = vol["dims"]
    max_steps = 4 * (X + Y + Z) if p["max_steps"] is None else int(p["max_steps"])
    refine = int(p["refine"])
    H, W = hw
    A = np.asarray(cam_to_world, np.float32).astype(f)
    K = np.asarray(intrinsics, np.float32).astype(f)
    V = A.shape[0]
    want_color = (vol["color"] is not None) if color is None else bool(color)
    assert not want_color or vol["color"] is not None
    field = _Field(vol, f, p["min_weight"])
    vs, trunc = f(np.float32(vol["voxel_size"])), f(np.float32(vol["trunc"]))
    step_min, relax = f(np.float32(p["step_min"])), f(np.float32(p["relax"]))
    tv = trunc / vs
    step_unobserved = relax * tv
    n = H * W
    out = dict(depth=np.zeros((V, n), f), normals=np.full((V, 3, n), np.nan, f), color=np.zeros((V, 3, n), f) if want_color else None,
               steps=np.zeros((V, n), np.int32), hit=np.zeros((V, n), bool), valid=np.zeros((V, n), bool),
               branch=np.zeros((V, n), np.int64))
    px = np.tile(np.arange(W), H).astype(f)
    py = np.repeat(np.arange(H), W).astype(f)
    with np.errstate(all="ignore"):
        for v in range(V):
            dx, dy = (px - K[v, 2]) / K[v, 0], (py - K[v, 3]) / K[v, 1]
            o = [(A[v, c, 3] - f(np.float32(vol["origin"][c]))) / vs for c in range(3)]
            d = [((A[v, c, 0] * dx + A[v, c, 1] * dy) + A[v, c, 2]) / vs for c in range(3)]
            s0, s1 = np.full(n, f(np.float32(p["min_depth"]))), np.full(n, f(np.float32(p["max_depth"])))
            for c in range(3):
                lo, hi = (f(0) - o[c]) / d[c], (f(vol["dims"][c] - 1) - o[c]) / d[c]
                s0 = max2(s0, min2(lo, hi))
                s1 = min2(s1, max2(lo, hi))
            L = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            active = (s0 <= s1) & (min(X, Y, Z) >= 2)
            s = s0.copy()
            sa, fa, sb, fb = (np.zeros(n, f) for _ in range(4))
            prev_obs, hit = np.zeros(n, bool), np.zeros(n, bool)
            steps = out["steps"][v]
            sub = lambda ids: [dc[ids] for dc in d]
            for _ in range(max_steps):
                ids = np.nonzero(active)[0]
                if ids.size == 0:
                    break
                obs, fv, _, _, _ = field.sample(o, sub(ids), s[ids])
                steps[ids] += 1
                cross = prev_obs[ids] & obs & ~(fa[ids] < 0) & (fv < 0)
                h = ids[cross]
                sb[h], fb[h], hit[h], active[h] = s[h], fv[cross], True, False
                r, fr, ob = ids[~cross], fv[~cross], obs[~cross]
                sa[r], fa[r], prev_obs[r] = s[r], fr, ob
                step = np.where(ob, np.fmax(step_min, relax * (np.abs(fr) * tv)), step_unobserved)
                s[r] = s[r] + step / L[r]
                active[r] = s[r] <= s1[r]
            ids = np.nonzero(hit)[0]
            if ids.size == 0:
                continue
            dh = sub(ids)
            a_s, a_f, b_s, b_f = sa[ids], fa[ids], sb[ids], fb[ids]
            branch = np.zeros(ids.size, np.int64)
            for it in range(refine):
                sm = a_s + (a_f / (a_f - b_f)) * (b_s - a_s)
                obs, fv, _, _, _ = field.sample(o, dh, sm)
                to_b, to_a = obs & (fv < 0), obs & ~(fv < 0)
                b_s, b_f = np.where(to_b, sm, b_s), np.where(to_b, fv, b_f)
                a_s, a_f = np.where(to_a, sm, a_s), np.where(to_a, fv, a_f)
                branch |= (to_b * MOVED_B + to_a * MOVED_A).astype(np.int64) << (2 * it)
            depth = a_s + (a_f / (a_f - b_f)) * (b_s - a_s)
            obs, _, cell, t, c = field.sample(o, dh, depth)
            G = gradient(c, t)
            m = [-((A[v, 0, j] * G[0] + A[v, 1, j] * G[1]) + A[v, 2, j] * G[2]) for j in range(3)]
            length = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
            valid = obs & (length > 0) & (length < np.inf)
            out["depth"][v, ids] = depth
            out["hit"][v, ids] = True
            out["valid"][v, ids] = valid
            out["branch"][v, ids] = branch
            for j in range(3):
                out["normals"][v, j, ids] = np.where(valid, m[j] / length, f(np.nan))
            if want_color:
                for ch in range(3):
                    cc = [field.color[ch][cell + off] for off in field.offsets]
                    out["color"][v, ch, ids] = np.where(valid, trilerp(cc, t), f(0))
    shape = dict(depth=(V, H, W), normals=(V, 3, H, W), color=(V, 3, H, W), steps=(V, H, W), hit=(V, H, W), valid=(V, H, W),
                 branch=(V, H, W))
    return {k: (None if a is None else a.reshape(shape[k])) for k, a in out.items()}


def decisions_agree(a, b):
    """[V, H, W] bool: the two runs took the same decisions on the ray (hit, march samples, every refinement branch, validity)."""
    return (a["hit"] == b["hit"]) & (a["steps"] == b["steps"]) & (a["branch"] == b["branch"]) & (a["valid"] == b["valid"])
