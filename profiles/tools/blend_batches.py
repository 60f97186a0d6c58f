"""Forward blend: batches of 64 list entries a quadrant's wavefront SCANS against batches of 64 entries that carry its own
quadrant bit (hits), from the training instantiation's saved lists of a few config-3 views.

    python profiles/tools/blend_batches.py [--views 0,7,15] [--workload c3_968x1296_1M] [--pmc-dir DIR] [--out FILE.json]

The lists are read through fs_raster_tile_ranges / fs_raster_point_list (list word = id << 4 | quadrant mask).  Per view:
  scanned_batches       sum over tiles and quadrants of ceil(n / 64)           (the gather + compaction blocks issued today)
  hit_batches           sum of ceil(hits_q / 64)                               (... when a batch is filled with hits first)
  hit_fraction          sum hits_q / sum n over the quadrants of non-empty tiles
and the same three with every quadrant's walk cut at the 64-entry chunk of its last contributor (max n_contrib of its
pixels): a quadrant never walks less than that, and walks further only until its last pixel saturates, so the real
counts lie between the two rows.  saving_bound = 40 VALU x (scanned - hit batches).
--pmc-dir: a rocprofv3 --pmc SQ_INSTS_VALU output directory (counters only) of a bench.py run; the blend kernel's mean
count per launch is added and the bound is expressed as a share of it.
"""
import argparse
import collections
import csv
import ctypes
import glob
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

kGatherCompactValu = 40   # VALU per batch: record gather 18 + compaction writes 15 + part of the rank / carry bookkeeping


def view_batches(rs, L):
    d = rs.dims
    H, W = d.H, d.W
    gx, gy = (W + 15) // 16, (H + 15) // 16
    T = gx * gy
    base = rs.binning.data_ptr()
    o_rng = L.fs_raster_tile_ranges(ctypes.c_void_p(base), H, W) - base
    o_lst = L.fs_raster_point_list(ctypes.c_void_p(base), H, W) - base
    raw = rs.binning.cpu().numpy()
    off = raw[o_rng: o_rng + (T + 1) * 4].view(np.uint32).astype(np.int64)
    words = raw[o_lst: o_lst + int(off[-1]) * 4].view(np.uint32)
    n = np.diff(off)
    tile = np.repeat(np.arange(T), n)
    pos = np.arange(len(words)) - off[tile]                      # position in the tile's list
    img = rs.image.cpu().numpy()
    o_nc = L.fs_raster_n_contrib(ctypes.c_void_p(rs.image.data_ptr()), H, W) - rs.image.data_ptr()
    nc = img[o_nc: o_nc + H * W * 4].view(np.int32).reshape(H, W)
    pad = np.zeros((gy * 16, gx * 16), np.int32)
    pad[:H, :W] = nc
    last = pad.reshape(gy, 2, 8, gx, 2, 8).max(axis=(2, 5)).transpose(0, 2, 1, 3).reshape(T, 4)  # [tile, qy * 2 + qx]
    ceil64 = lambda a: (a + 63) // 64
    res = collections.OrderedDict()
    for tag in ("whole_list", "to_last_contributor"):
        scanned = hit_b = hits_sum = n_sum = 0
        for q in range(4):
            end = n if tag == "whole_list" else np.minimum(n, ceil64(last[:, q].astype(np.int64)) * 64)
            hit = ((words >> q) & 1).astype(bool) & (pos < end[tile])
            hq = np.bincount(tile[hit], minlength=T)
            scanned += int(ceil64(end).sum())
            hit_b += int(ceil64(hq).sum())
            hits_sum += int(hq.sum())
            n_sum += int(end.sum())
        res[tag] = dict(scanned_batches=scanned, hit_batches=hit_b, hit_fraction=round(hits_sum / max(n_sum, 1), 4),
                        saving_bound_valu=kGatherCompactValu * (scanned - hit_b))
    res["tiles"] = T
    res["instances"] = int(off[-1])
    res["mean_list"] = round(float(n.mean()), 1)
    return res


def pmc_blend_valu(pmc_dir):
    vals = collections.defaultdict(list)
    for f in sorted(glob.glob(pmc_dir + "/**/*counter_collection.csv", recursive=True)):
        for r in csv.DictReader(open(f)):
            k = r["Kernel_Name"].split("(")[0].replace("void ", "")
            if "sort_blend_kernel" in k and r["Counter_Name"] == "SQ_INSTS_VALU":
                vals[k].append(float(r["Counter_Value"]))
    return {k: dict(SQ_INSTS_VALU_per_launch=sum(v) / len(v), launches=len(v)) for k, v in vals.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", default="0,7,15")
    ap.add_argument("--workload", default="c3_968x1296_1M")
    ap.add_argument("--pmc-dir", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from freesplat_amd import _lib, synthetic
    from freesplat_amd.decoder import render_views
    dev = torch.device("cuda:0")
    H, W, N = synthetic.WORKLOADS[a.workload]
    sc, cams = synthetic.workload_scene(a.workload), synthetic.target_cameras(16)
    g = {k: sc[k].to(dev).requires_grad_(True) for k in ("means", "covariances", "harmonics", "opacities")}
    c = {k: v.to(dev) for k, v in cams.items()}
    col, _ = render_views(c["extrinsics"], c["intrinsics"], c["near"], c["far"], (H, W), torch.zeros(16, 3, device=dev),
                          g["means"], g["covariances"], g["harmonics"], g["opacities"])
    torch.cuda.synchronize()
    states = col.grad_fn.states
    out = collections.OrderedDict(workload=a.workload, gather_compact_valu_per_batch=kGatherCompactValu, views={})
    for i in (int(x) for x in a.views.split(",")):
        out["views"][str(i)] = view_batches(states[i], _lib.lib())
        print("view", i, json.dumps(out["views"][str(i)]), flush=True)
    for tag in ("whole_list", "to_last_contributor"):
        out["mean_saving_bound_valu_" + tag] = float(np.mean([v[tag]["saving_bound_valu"] for v in out["views"].values()]))
    if a.pmc_dir:
        out["pmc"] = pmc_blend_valu(a.pmc_dir)
        for k, v in out["pmc"].items():
            for tag in ("whole_list", "to_last_contributor"):
                v["saving_bound_share_" + tag] = round(out["mean_saving_bound_valu_" + tag] / v["SQ_INSTS_VALU_per_launch"], 4)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
