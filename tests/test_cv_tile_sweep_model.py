"""CPU model of the cost-volume backward's second pass (csrc/cost_volume.hip: cv_src_grad_kernel) -- the source-feature
gradient collected by TILES OF SOURCE TEXELS from per-(pixel, plane) records instead of scattered with global atomics --
checked against autograd of the reference-pinned oracle.  It pins, without a GPU, the two things the kernel's correctness
rests on: (i) the formula  d src_k[t] = sum w_tap (valid_k dfavg / cnt + [z_k > 0] ddot / cnt * cur), and (ii) that the
bounding box of a tile's corners under the inverse plane homography contains every pixel with a tap in the tile (tiles
behind the source skipped, horizon-straddling tiles walking the whole image)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

TW = TH = 16


def tile_sweep_model(aux, dfavg, ddot, cur, invK, h, w):
    """numpy restatement of cv_ginv_kernel + cv_src_grad_kernel (float64 positions, the kernel's box rule)."""
    P, planes = aux["P"].numpy(), aux["planes"].numpy()
    valid, front, cnt = aux["valid"].numpy(), aux["front"].numpy(), aux["cnt"].numpy()
    ix, iy = aux["ix"].numpy(), aux["iy"].numpy()
    B, K, D, N = ix.shape
    C = cur.shape[1]
    d_src = np.zeros((B, K, C, h, w))
    visited = useful = 0
    for b in range(B):
        cur_b = cur[b].reshape(C, N)
        for k in range(K):
            for d in range(D):
                G = planes[d] * P[b, k][:, :3] @ invK[b][:3, :3] + np.outer(P[b, k][:, 3], [0, 0, 1.0])
                Gi = np.linalg.inv(G)
                fx, fy = np.floor(ix[b, k, d]), np.floor(iy[b, k, d])
                txw, tyw = ix[b, k, d] - fx, iy[b, k, d] - fy
                dwv = (valid[b, k, d] * dfavg[b, :, d] + front[b, k, d] * ddot[b, 0, d] * cur_b) / cnt[b, 0, d]   # [C,N]
                for ty0 in range(0, h, TH):
                    for tx0 in range(0, w, TW):
                        tw_, th_ = min(TW, w - tx0), min(TH, h - ty0)
                        X0, X1, Y0, Y1 = tx0 - 0.55, tx0 + tw_ + 0.55, ty0 - 0.55, ty0 + th_ + 0.55
                        cs = np.array([[X0, Y0, 1], [X1, Y0, 1], [X0, Y1, 1], [X1, Y1, 1]]).T
                        pre = Gi @ cs
                        cc = pre[2]
                        amax = np.abs(cc).max()
                        bx0, bx1, by0, by1 = 0, w - 1, 0, h - 1
                        if cc.max() < -1e-3 * amax:
                            continue
                        if cc.min() > 1e-3 * amax:
                            u, v = pre[0] / cc - 0.5, pre[1] / cc - 0.5
                            bx0, bx1 = max(0, int(np.ceil(u.min() - 0.05))), min(w - 1, int(np.floor(u.max() + 0.05)))
                            by0, by1 = max(0, int(np.ceil(v.min() - 0.05))), min(h - 1, int(np.floor(v.max() + 0.05)))
                        if bx1 < bx0 or by1 < by0:
                            continue
                        vv, uu = np.meshgrid(np.arange(by0, by1 + 1), np.arange(bx0, bx1 + 1), indexing="ij")
                        pix = (vv * w + uu).ravel()
                        visited += pix.size
                        lx, ly = fx[pix] - tx0, fy[pix] - ty0
                        for ox in (0, 1):
                            for oy in (0, 1):
                                ok = front[b, k, d][pix] & (lx + ox >= 0) & (lx + ox <= tw_ - 1) & (ly + oy >= 0) & (ly + oy <= th_ - 1)
                                if not ok.any():
                                    continue
                                pp = pix[ok]
                                useful += pp.size
                                wt = (txw[pp] if ox else 1 - txw[pp]) * (tyw[pp] if oy else 1 - tyw[pp])
                                xs, ys = (fx[pp] + ox).astype(int), (fy[pp] + oy).astype(int)
                                np.add.at(d_src[b, k], (slice(None), ys, xs), wt * dwv[:, pp])
    return d_src, visited, useful


@pytest.mark.parametrize("V,K,h4,w4,D,behind", [(3, 2, 20, 36, 6, False), (3, 2, 15, 21, 5, True), (4, 3, 33, 18, 4, False)])
def test_tile_sweep_model_matches_oracle_autograd(V, K, h4, w4, D, behind):
    import inputs
    from oracle import cost_volume_oracle as cvo
    C = 8
    torch.manual_seed(1)
    kw = inputs.cv_inputs(V, K, h4, w4, C, seed=5 + V, behind=behind)
    mlp = dict(w1=torch.randn(32, C + 1).double() * 0.3, b1=torch.randn(32).double() * 0.1, w2=torch.randn(32, 32).double() * 0.2,
               b2=torch.randn(32).double() * 0.1, w3=torch.randn(1, 32).double() * 0.3, b3=torch.zeros(1).double())
    cur = kw["cur_feats"].double().requires_grad_(True)
    src = kw["src_feats"].double().requires_grad_(True)
    out, aux = cvo.cost_volume(cur, src, kw["src_extrinsics"].double(), kw["src_Ks"].double(), kw["cur_invK"].double(),
                               kw["min_depth"], kw["max_depth"], D, mlp, return_pre=True)
    aux["feat_mean"].retain_grad()
    aux["dot_mean"].retain_grad()
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(2)).double()
    (out * g).sum().backward()
    det = {k: v.detach() for k, v in aux.items()}
    d_src, visited, useful = tile_sweep_model(det, aux["feat_mean"].grad.numpy(), aux["dot_mean"].grad.numpy(),
                                              cur.detach().numpy(), kw["cur_invK"].double().numpy(), h4, w4)
    want = src.grad.numpy()
    assert np.abs(d_src - want).max() <= 1e-9 * (np.abs(want).max() + 1e-30) + 1e-12
    # the walk visits little more than the pixels it needs (and, with a source behind the planes, skips its tiles)
    assert visited <= 6 * max(useful, 1) + V * K * D * 64


def test_register_form_lists_blend_every_tap_exactly_once():
    """Model of round 6's pass 2 (cv_src_grad_kernel<C>): a batch's taps are appended to per-texel lists of 8 entries
    (slot = the value a ds_add_rtn_u32 returns; a tap whose slot is >= 8 stays pending), every texel blends min(count, 8)
    entries, the counters are cleared and the pending taps go round again.  Whatever the collisions, the result is the plain
    scatter-add."""
    import numpy as np
    rng = np.random.default_rng(7)
    CAP, TW, TH, C = 8, 8, 8, 6
    for trial in range(40):
        crowd = trial % 4 == 3                                   # every 4th trial: all pixels on a few texels (lists overflow)
        S = rng.normal(size=(64, C)).astype(np.float32)          # the staged records
        base_x = rng.integers(-1, 2 if crowd else TW, size=64)
        base_y = rng.integers(-1, 2 if crowd else TH, size=64)
        w = rng.random(size=(64, 4)).astype(np.float32)
        taps = []                                                # (lane, tap, texel)
        for lane in range(64):
            for tap in range(4):
                x, y = base_x[lane] + (tap & 1), base_y[lane] + (tap >> 1)
                if 0 <= x < TW and 0 <= y < TH:
                    taps.append((lane, tap, y * TW + x))
        want = np.zeros((TW * TH, C), np.float64)
        for lane, tap, t in taps:
            want[t] += np.float64(w[lane, tap]) * S[lane]
        got = np.zeros((TW * TH, C), np.float64)
        pending, rounds = list(taps), 0
        while pending:
            rounds += 1
            count = np.zeros(TW * TH, np.int64)
            lists = [[] for _ in range(TW * TH)]
            still = []
            for lane, tap, t in pending:                         # (any order: the adds are atomic)
                slot = count[t]
                count[t] += 1
                if slot < CAP:
                    lists[t].append((lane, w[lane, tap]))
                else:
                    still.append((lane, tap, t))
            for t in range(TW * TH):
                for lane, wt in lists[t][:min(count[t], CAP)]:
                    got[t] += np.float64(wt) * S[lane]
            pending = still
        assert np.allclose(got, want, rtol=0, atol=1e-12)
        assert rounds >= 1 and (crowd or rounds <= 3)
