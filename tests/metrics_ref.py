"""NumPy float64 restatements of the evaluation metrics (freesplat_amd/metrics.py), written from the algorithms:

ssim(gt, pred): skimage.metrics.structural_similarity(gt, pred, win_size=11, gaussian_weights=True, channel_axis=0,
    data_range=1.0) for one [C, H, W] view.  Per channel: u = G * x, y, x^2, y^2, xy with the separable 11-tap Gaussian
    (sigma 1.5, truncate 3.5, weights normalised in double), v = 121/120 (u_xx - u_x^2) etc. (sample covariance),
    C1 = (0.01 R)^2, C2 = (0.03 R)^2 with R = 1, S = (2 u_x u_y + C1)(2 v_xy + C2) / ((u_x^2 + u_y^2 + C1)(v_x + v_y + C2)),
    mean over [5, H-5) x [5, W-5), then over channels.  The filter is evaluated as a 'valid' correlation only, so no
    padding value is ever read: the 5-pixel crop discards every output whose window leaves the image.
psnr_mse(gt, pred): compute_psnr's mean of (clip(gt,0,1) - clip(pred,0,1))^2 per view.
depth(gt, pred): per-view abs_diff, abs_rel, delta_25, delta_10 of depth_render_metrics with torch's NaN rules.
"""
import numpy as np

SIGMA, RAD = 1.5, 5
C1, C2 = 0.01 ** 2, 0.03 ** 2
NP = (2 * RAD + 1) ** 2
COV_NORM = NP / (NP - 1.0)


def gauss_weights():
    k = np.arange(-RAD, RAD + 1, dtype=np.float64)
    e = np.exp(-0.5 * k * k / (SIGMA * SIGMA))
    return e / e.sum()


def _valid_filter(a):
    """Separable Gaussian correlation of a 2-D float64 array, 'valid' part only: [H-10, W-10]."""
    w = gauss_weights()
    H, W = a.shape
    t = sum(w[k] * a[k:H - 2 * RAD + k, :] for k in range(2 * RAD + 1))
    return sum(w[k] * t[:, k:W - 2 * RAD + k] for k in range(2 * RAD + 1))


def ssim_map(gt, pred):
    """S per interior pixel of one [C, H, W] view: [C, H-10, W-10] float64."""
    x = np.asarray(gt, np.float64)
    y = np.asarray(pred, np.float64)
    if x.shape[-1] < 2 * RAD + 1 or x.shape[-2] < 2 * RAD + 1:
        raise ValueError("win_size exceeds image extent")
    out = []
    for xc, yc in zip(x, y):
        ux, uy = _valid_filter(xc), _valid_filter(yc)
        uxx, uyy, uxy = _valid_filter(xc * xc), _valid_filter(yc * yc), _valid_filter(xc * yc)
        vx = COV_NORM * (uxx - ux * ux)
        vy = COV_NORM * (uyy - uy * uy)
        vxy = COV_NORM * (uxy - ux * uy)
        a1, a2 = 2 * ux * uy + C1, 2 * vxy + C2
        b1, b2 = ux * ux + uy * uy + C1, vx + vy + C2
        out.append((a1 * a2) / (b1 * b2))
    return np.stack(out)


def ssim(gt, pred):
    """skimage's value for one [C, H, W] view (mean over the interior of each channel, then over channels)."""
    return float(np.mean([m.mean() for m in ssim_map(gt, pred)]))


def ssim_batch(gt, pred):
    return np.array([ssim(a, b) for a, b in zip(gt, pred)])


def mse(gt, pred):
    """[B] mean of (clip(gt) - clip(pred))^2 over c, h, w (float64 of the fp32 inputs)."""
    d = np.clip(np.asarray(gt, np.float64), 0, 1) - np.clip(np.asarray(pred, np.float64), 0, 1)
    return (d * d).reshape(d.shape[0], -1).mean(axis=1)


def depth(gt, pred, threshold=0.5):
    """gt, pred [n_views, HW] float32 -> dict of per-view abs_diff, abs_rel, delta_25, delta_10 (float64 [n_views]).
    Valid pixels: gt > threshold (gt == threshold is invalid).  abs_* are nanmeans: NaN terms are dropped.  A ratio
    max(gt/pred, pred/gt) that is NaN counts as 'not within delta' and stays in the denominator; pred = 0 gives an
    infinite ratio; a negative pred passes.  A view with no valid pixel gives NaN throughout."""
    g = np.asarray(gt, np.float32)
    p = np.asarray(pred, np.float32)
    out = {k: [] for k in ("abs_diff", "abs_rel", "delta_25", "delta_10")}
    with np.errstate(divide="ignore", invalid="ignore"):
        for gv, pv in zip(g, p):
            m = gv > np.float32(threshold)
            gm, pm = gv[m], pv[m]
            d = np.abs(gm - pm)
            keep = ~np.isnan(d)
            n = keep.sum()
            out["abs_diff"].append(d[keep].astype(np.float64).sum() / n if n else np.nan)
            out["abs_rel"].append((d[keep] / gm[keep]).astype(np.float64).sum() / n if n else np.nan)
            r1, r2 = gm / pm, pm / gm
            nv = m.sum()
            for key, th in (("delta_25", np.float32(1.25)), ("delta_10", np.float32(1.1))):
                ok = (r1 < th) & (r2 < th)                       # False where either ratio is NaN
                out[key].append(ok.sum() / nv if nv else np.nan)
    return {k: np.array(v, np.float64) for k, v in out.items()}
