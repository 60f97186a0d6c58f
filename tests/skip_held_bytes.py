"""What the fused skip branch and the torch chain it replaces keep between forward and backward, measured in a process of its own
(run by tests/test_skip_latents_hip.py::test_no_skip_map_is_kept_for_the_backward):

    python tests/skip_held_bytes.py V h w    ->  one JSON line

torch.cuda.memory_allocated() accounts whole blocks of the caching allocator: a request served from a cached block left by earlier
work is charged that block's size (inside the whole suite: 1970176 B for the 1881792 B the op asks for).  In a fresh process every
tensor gets a block split to its own 512-byte-rounded size, so the counter shows what the op itself keeps.  Held = the bytes released
when the autograd graph goes while the outputs' storage stays; `requested` is the allocator's count of the bytes asked for."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch

import skip_ref as R


def held(fn):
    requested = lambda: torch.cuda.memory_stats()["requested_bytes.all.current"]
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    lat, dens = fn()
    torch.cuda.synchronize()
    with_graph = (torch.cuda.memory_allocated(), requested())
    keep = (lat.detach(), dens.detach())
    del lat, dens
    torch.cuda.synchronize()
    out = {"allocated": with_graph[0] - torch.cuda.memory_allocated(), "requested": with_graph[1] - requested()}
    del keep
    return out


def main():
    from freesplat_amd.gaussian_adapter import latents_pack, skip_latents
    V, h, w = (int(x) for x in sys.argv[1:4])
    dev = torch.device("cuda:0")
    a = R.make_inputs(V, h, w, seed=3)
    d = {k: a[k].to(dev) for k in ("head", "img", "weight", "bias")}
    for k in ("head", "weight", "bias"):
        d[k].requires_grad_(True)
    conv = lambda: torch.relu(torch.nn.functional.conv2d(d["img"], d["weight"], d["bias"], padding=3))
    out = {"fused": held(lambda: skip_latents(d["head"], d["img"], d["weight"], d["bias"])),
           "chain": held(lambda: latents_pack(d["head"], conv()))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
