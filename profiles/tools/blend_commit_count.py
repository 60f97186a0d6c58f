#!/usr/bin/env python
"""CPU count for the forward blend's commit (raster_fwd.hip, FS_BLEND_ONE): how many of the survivors a quadrant walk
evaluates are taken by no pixel at all (every pixel they reach is saturated already, or saturates at them), how they are
spread over pairs and steps, how many lanes commit, and what a filter that drops such survivors BEFORE the step -- at
compaction time, against the state the quadrant had when the survivor's hit batch was compacted -- could drop at best.

The oracle renders one config-3 view; sampled tiles are walked quadrant by quadrant as the kernel walks them
(tests/test_raster_blend_commit.py: walk_quadrant -- four survivors per step, in list order, until every pixel is
saturated), on the oracle's unculled lists and in its arithmetic (fp32 fma through float64: statistics, not bits; a
survivor = a list entry that reaches a pixel of the 8 x 8 quadrant, the product's conservative quadrant masks keep a few
more).  Filters, all judged on the pixels a survivor really reaches (an upper bound for a geometric test):
  rectangle  the bounding rectangle of the quadrant's undone pixels;
  4x4 / 2x2  the blocks that still hold an undone pixel;
  exact      the undone pixels themselves;
each on the snapshot taken before the first step that holds an entry of the survivor's batch of 64 hits.

  python profiles/tools/blend_commit_count.py [view] [tiles]     (one view of c3_968x1296_1M; ~1 minute on 8 threads)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from freesplat_amd import synthetic  # noqa: E402
from test_raster_blend_commit import QUAD_PIXELS, tile_reach, walk_quadrant  # noqa: E402
from util_raster import oracle_forward, view_inputs  # noqa: E402

# VALU of the step loop of sort_blend_kernel<false,false> per four survivors (gfx950 assembly): predicated commit, commit
# under the execution mask with all four taken, and what one survivor without a committing lane skips
VALU_SELECT, VALU_MASKED, VALU_SKIP = 82, 78, 4


def _blocks(mask, b):
    """[64] pixel mask -> the same mask spread over the b x b blocks of the 8 x 8 quadrant that hold a set pixel."""
    m = mask.reshape(8 // b, b, 8 // b, b).any(axis=(1, 3))
    return np.repeat(np.repeat(m, b, 0), b, 1).reshape(64)


def count_view(view=3, tiles=200, seed=0):
    H, W, N = synthetic.WORKLOADS["c3_968x1296_1M"]
    scene = synthetic.make_scene(N)
    cams = synthetic.target_cameras(16)
    st = oracle_forward(view_inputs(scene, cams, view, H, W))
    T = st["ranges"].shape[0]
    pick = np.sort(np.random.default_rng(seed).choice(T, min(tiles, T), replace=False))
    n = dict(walks=0, hits=0, evaluated=0, dead=0, saturate_only=0, lanes=0, pairs=0, dead_pairs=0, unreached_pairs=0,
             steps=[0] * 5, rect=0, b4=0, b2=0, exact=0)
    for tile in pick:
        ids, alpha, reach, inside = tile_reach(st, int(tile))
        for pix in QUAD_PIXELS:
            if not inside[pix].any():
                continue
            snaps = {}
            lanes, vis_any, steps, tail, sat, _, hits = walk_quadrant(
                alpha[:, pix], reach[:, pix], inside[pix], on_step=lambda s, done: snaps.setdefault(s // 64, done))
            ev = len(lanes)
            n["walks"] += 1
            n["hits"] += len(hits)
            n["evaluated"] += ev
            dead = lanes == 0
            n["dead"] += int(dead.sum())
            n["saturate_only"] += int((dead & vis_any).sum())
            n["lanes"] += int(lanes.sum())
            full = 4 * len(steps)
            d4, v4 = dead[:full].reshape(-1, 4), vis_any[:full].reshape(-1, 4)
            n["pairs"] += 2 * len(steps)
            n["dead_pairs"] += int((d4[:, :2].all(1)).sum() + (d4[:, 2:].all(1)).sum())
            n["unreached_pairs"] += int((~v4[:, :2].any(1)).sum() + (~v4[:, 2:].any(1)).sum())
            for k in steps:
                n["steps"][k] += 1
            r = reach[:, pix]
            for j in range(ev):
                k = j // 64
                while k not in snaps:      # the batch began inside a step: the snapshot of that step's batch
                    k -= 1
                und = ~snaps[k]
                re = r[hits[j]]
                ys, xs = np.nonzero(und.reshape(8, 8))
                box = np.zeros((8, 8), bool)
                if len(ys):
                    box[ys.min():ys.max() + 1, xs.min():xs.max() + 1] = True
                n["rect"] += not (re & box.reshape(64)).any()
                n["b4"] += not (re & _blocks(und, 4)).any()
                n["b2"] += not (re & _blocks(und, 2)).any()
                n["exact"] += not (re & und).any()
    return n, len(pick), T


def main(view=3, tiles=200):
    n, picked, T = count_view(view, tiles)
    ev, w = max(n["evaluated"], 1), max(n["walks"], 1)
    nsteps = max(sum(n["steps"]), 1)
    print(f"view {view}: {picked} of {T} tiles, {n['walks']} quadrant walks (oracle lists, no tile cull, contract exp)")
    print(f"  per walk: {n['hits'] / w:.1f} survivors in the list, {ev / w:.1f} evaluated ({ev / max(n['hits'], 1):.3f}); "
          f"whole view ~ {ev / picked * T / 1e6:.2f} M evaluated survivors")
    print(f"  dead survivors (no committing lane): {n['dead']} = {n['dead'] / ev:.4f} of the evaluated, {n['dead'] / w:.2f} per walk; "
          f"of them {n['saturate_only']} reach pixels that all saturate at them")
    print(f"  committing lanes per evaluated survivor: {n['lanes'] / ev:.1f} of 64")
    print(f"  pairs with both survivors dead: {n['dead_pairs']} = {n['dead_pairs'] / max(n['pairs'], 1):.4f} of the pairs; "
          f"with no unsaturated pixel reached by either: {n['unreached_pairs']} = {n['unreached_pairs'] / max(n['pairs'], 1):.4f}")
    print("  full steps by committing survivors 0/1/2/3/4: " + " / ".join(str(k) for k in n["steps"])
          + f"; all four dead: {n['steps'][0] / nsteps:.4f} of the steps")
    print(f"  dropped before the step, of the evaluated: rectangle {n['rect'] / ev:.4f}  4x4 blocks {n['b4'] / ev:.4f}  "
          f"2x2 blocks {n['b2'] / ev:.4f}  exact snapshot {n['exact'] / ev:.4f}")
    mean_skip = VALU_SKIP * sum(k * c for k, c in enumerate(n["steps"][::-1])) / nsteps   # dead survivors per full step x 4
    per_step = VALU_MASKED - mean_skip
    print(f"  step loop VALU per four survivors: {VALU_SELECT} predicated -> {per_step:.1f} under the execution mask "
          f"({VALU_MASKED} - {VALU_SKIP} x {mean_skip / VALU_SKIP:.3f} dead per step) = {per_step / VALU_SELECT - 1:+.1%}")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 3, int(sys.argv[2]) if len(sys.argv) > 2 else 200)
