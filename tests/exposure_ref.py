"""Float64 restatement of freesplat_amd.exposure (DESIGN.md "Exposure compensation"): the per-view affine colour transform, its
gradients and the least-squares affine colour fit, with out-of-range ids, duplicate ids, masks and the identity fallbacks.
Plain torch on the CPU; a yardstick, not code under test.  Besides the values it returns the sums of absolute terms the
error bounds of tests/test_exposure_hip.py are built from.

  params [V, 3, 4]  row c of view v = (A[c,0], A[c,1], A[c,2], b[c])
  view_ids          None (entry b uses view b, B == V) or B integers; an id outside [0, V) passes its entry through
"""
import torch

U = 2.0 ** -24


def identity(V, dtype=torch.float64):
    return torch.cat([torch.eye(3, dtype=dtype), torch.zeros(3, 1, dtype=dtype)], 1).repeat(V, 1, 1)


def resolve_ids(view_ids, B, V):
    if view_ids is None:
        assert B == V, (B, V)
        return list(range(B))
    ids = [int(i) for i in (view_ids.tolist() if isinstance(view_ids, torch.Tensor) else view_ids)]
    assert len(ids) == B
    return ids


def apply(image, params, view_ids=None, absolute=False):
    """out [B, 3, H, W] float64.  absolute=True: sum_k |A[c,k] x_k| + |b[c]| instead (the out-of-range entries: |x|)."""
    x, q = image.double(), params.double()
    out = torch.empty_like(x)
    for b, v in enumerate(resolve_ids(view_ids, x.shape[0], q.shape[0])):
        if not 0 <= v < q.shape[0]:
            out[b] = x[b].abs() if absolute else x[b]
            continue
        A, off = q[v, :, :3], q[v, :, 3]
        if absolute:
            out[b] = torch.einsum("ck,khw->chw", A.abs(), x[b].abs()) + off.abs().view(3, 1, 1)
        else:
            out[b] = torch.einsum("ck,khw->chw", A, x[b]) + off.view(3, 1, 1)
    return out


def apply_grad(image, params, view_ids, g_out, absolute=False):
    """(g_image [B, 3, H, W], g_params [V, 3, 4], n [V]) float64; n = the number of products in each sum of g_params[v].
    absolute=True: the sums of the absolute values of the same terms."""
    x, q, g = image.double(), params.double(), g_out.double()
    V = q.shape[0]
    g_image, g_params, n = torch.empty_like(x), torch.zeros(V, 3, 4, dtype=torch.float64), torch.zeros(V, dtype=torch.int64)
    if absolute:
        x, q, g = x.abs(), q.abs(), g.abs()
    for b, v in enumerate(resolve_ids(view_ids, x.shape[0], V)):
        if not 0 <= v < V:
            g_image[b] = g[b]
            continue
        g_image[b] = torch.einsum("ck,chw->khw", q[v, :, :3], g[b])
        g_params[v, :, :3] += torch.einsum("chw,khw->ck", g[b], x[b])
        g_params[v, :, 3] += g[b].sum((1, 2))
        n[v] += x.shape[2] * x.shape[3]
    return g_image, g_params, n


def valid_pixels(pred, target, mask=None):
    ok = torch.isfinite(pred).all(1) & torch.isfinite(target).all(1)
    return ok if mask is None else ok & (mask != 0)


def normal_equations(pred, target, mask=None, view_ids=None, num_views=None):
    """(M [V, 4, 4], R [V, 4, 3]) float64 over the valid pixels of the entries of each view; cnt = M[:, 3, 3]."""
    x, y = pred.double(), target.double()
    B = x.shape[0]
    V = B if num_views is None else int(num_views)
    ok = valid_pixels(x, y, mask)
    M, R = torch.zeros(V, 4, 4, dtype=torch.float64), torch.zeros(V, 4, 3, dtype=torch.float64)
    for b, v in enumerate(resolve_ids(view_ids, B, V)):
        if not 0 <= v < V:
            continue
        X = torch.cat([x[b], torch.ones_like(x[b, :1])], 0)[:, ok[b]]          # [4, n]: an invalid pixel never enters
        M[v] += X @ X.T
        R[v] += X @ y[b][:, ok[b]].T
    return M, R


def cholesky_solve(M, rhs):
    """P with M P = rhs by Cholesky, in float64; ok = every pivot is positive and finite."""
    L = torch.zeros(4, 4, dtype=torch.float64)
    ok = True
    for j in range(4):
        d = float(M[j, j] - (L[j, :j] ** 2).sum())
        ok = ok and d > 0.0 and d < float("inf")
        if not ok:
            return None, False
        L[j, j] = d ** 0.5
        for i in range(j + 1, 4):
            L[i, j] = (M[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    z = torch.linalg.solve_triangular(L, rhs, upper=False)
    return torch.linalg.solve_triangular(L.T, z, upper=True), True


def fit(pred, target, mask=None, view_ids=None, num_views=None, ridge=1e-6):
    """(params [V, 3, 4] float64, count [V] int64, solved [V] bool, kappa [V] float64): kappa = the condition number of
    M + ridge cnt I (inf where the view has no valid pixel)."""
    M, R = normal_equations(pred, target, mask, view_ids, num_views)
    V = M.shape[0]
    params, count, solved = identity(V), M[:, 3, 3].round().long(), torch.zeros(V, dtype=torch.bool)
    kappa = torch.full((V,), float("inf"), dtype=torch.float64)
    for v in range(V):
        if count[v] == 0:
            continue
        lam = float(ridge) * float(count[v])
        Mr = M[v] + lam * torch.eye(4, dtype=torch.float64)
        rhs = R[v] + lam * torch.eye(4, 3, dtype=torch.float64)
        ev = torch.linalg.eigvalsh(Mr)
        kappa[v] = float(ev[-1] / ev[0]) if float(ev[0]) > 0 else float("inf")
        P, ok = cholesky_solve(Mr, rhs)
        if ok:
            params[v], solved[v] = P.T, True
    return params, count, solved, kappa


# ---- the eager fp32 forms a user writes today (the benchmark's yardstick; they run on any device) ----

def eager_apply(image, params, view_ids=None):
    q = params if view_ids is None else params[view_ids]
    return torch.einsum("bck,bkhw->bchw", q[:, :, :3], image) + q[:, :, 3, None, None]


def eager_fit(pred, target, mask=None, ridge=1e-6):
    """Masked float64 normal equations + torch.linalg.solve, one view per entry."""
    B = pred.shape[0]
    ok = torch.isfinite(pred).all(1) & torch.isfinite(target).all(1)
    if mask is not None:
        ok = ok & (mask != 0)
    w = ok[:, None].double()
    x = torch.where(ok[:, None], pred, torch.zeros_like(pred)).double()
    y = torch.where(ok[:, None], target, torch.zeros_like(target)).double()
    X = torch.cat([x, w], 1).flatten(2)                                        # [B, 4, P]
    M = X @ X.transpose(1, 2)
    R = X @ y.flatten(2).transpose(1, 2)
    lam = ridge * M[:, 3, 3]
    eye = torch.eye(4, dtype=torch.float64, device=pred.device)
    P = torch.linalg.solve(M + lam[:, None, None] * eye, R + lam[:, None, None] * eye[:, :3])
    return P.transpose(1, 2).float()
