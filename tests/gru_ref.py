"""The GRU of Pixel-wise Triplet Fusion (networks.py:201-214) restated on rows cat = [hid 64 | he 24 | x 64 | xe 24] with every
intermediate kept and an ANALYTIC backward, in float64 by default: what the kernels of csrc/ptf_gru.hip are judged against,
per row, in test_ptf_gru_edges_host.py (CPU) and test_ptf_gru_edges_hip.py (device).

`mutate=k` switches ONE deliberate mistake on (MUTATIONS), so that the host tests can show that the figures of gru_cases.py
see it; nothing broken ever runs on a device."""
import torch
import torch.nn.functional as F

KEYS = [f"{m}.{l}.{t}" for m in ("mlp_r", "mlp_z", "mlp_n") for l in ("0", "2") for t in ("weight", "bias")]   # ptf._gru_params order
U = 2.0 ** -24
SIDE_BLOCKS = ("dr1", "dz1", "dR", "dZ", "dn1", "dN", "a_r1", "a_z1", "a_n1", "rh")       # the kernel's documented order

MUTATIONS = {
    1: "ReLU mask >= 0 instead of > 0",
    2: "d hid loses the H * r term",
    3: "1 - q*q -> 1 - q",
    4: "dZ uses q for q - hid",
    5: "row t of dcat from row t ^ 1's cotangent in the last group of 16",
    6: "xe's sin / cos columns swapped in dcat",
    7: "sigmoid carrying 1e-5 absolute error",
    8: "last live row left out of the weight-gradient contraction",
    9: "sigmoid carrying 2e-7 absolute error (the kernel's stated contract: must pass)",
}


def pe64(a, b):
    """The positional encoding of the pair of scalars (a, b) per row (encoder_freesplat.py:62-77, six frequencies) in float64:
    [n] , [n] -> [n, 24]."""
    from oracle.ptf_oracle import positional_encoding
    return positional_encoding(torch.stack([a.double(), b.double()], -1), 6)


def as_dict(params, dtype=torch.float64):
    """The 12 parameters (ptf._gru_params order, or a dict with KEYS) as a dict of `dtype` CPU tensors."""
    if not isinstance(params, dict):
        params = dict(zip(KEYS, params))
    return {k: params[k].detach().cpu().to(dtype) for k in KEYS}


def _sigmoid(x, mutate):
    s = torch.sigmoid(x)
    if mutate == 7:
        s = s + 1e-5
    if mutate == 9:
        s = s + 2e-7
    return s


def forward(params, cat, dtype=torch.float64, mutate=None):
    """out [n,64], the pre-activations r1, z1, n1 (first layers), R, Z, N (second layers), the gates r, z, q and the magnitudes
    mag_r1 / mag_z1 / mag_n1 = |b| + |W| |x| of the three ReLU layers (what a rounding of the pre-activation scales with)."""
    p = as_dict(params, dtype)
    cat = cat.detach().cpu().to(dtype)
    hid, xx = cat[:, :64], cat[:, 88:]
    f = {}
    f["r1"] = F.linear(cat, p["mlp_r.0.weight"], p["mlp_r.0.bias"])
    f["z1"] = F.linear(cat, p["mlp_z.0.weight"], p["mlp_z.0.bias"])
    f["R"] = F.linear(F.relu(f["r1"]), p["mlp_r.2.weight"], p["mlp_r.2.bias"])
    f["Z"] = F.linear(F.relu(f["z1"]), p["mlp_z.2.weight"], p["mlp_z.2.bias"])
    f["r"], f["z"] = _sigmoid(f["R"], mutate), _sigmoid(f["Z"], mutate)
    f["rh"] = f["r"] * hid
    nin = torch.cat([f["rh"], xx], -1)
    f["n1"] = F.linear(nin, p["mlp_n.0.weight"], p["mlp_n.0.bias"])
    f["N"] = F.linear(F.relu(f["n1"]), p["mlp_n.2.weight"], p["mlp_n.2.bias"])
    f["q"] = torch.tanh(f["N"])
    f["out"] = (1 - f["z"]) * hid + f["z"] * f["q"]
    f["mag_r1"] = F.linear(cat.abs(), p["mlp_r.0.weight"].abs(), p["mlp_r.0.bias"].abs())
    f["mag_z1"] = F.linear(cat.abs(), p["mlp_z.0.weight"].abs(), p["mlp_z.0.bias"].abs())
    f["mag_n1"] = F.linear(nin.abs(), p["mlp_n.0.weight"].abs(), p["mlp_n.0.bias"].abs())
    return f


def near_kink(f):
    """bool [n]: rows where some first-layer ReLU unit has 0 < |pre| <= 64 u mag (f: forward() in float64).  fp32 may
    legitimately take the other slope there, so such rows are left out of the BACKWARD judgement.  A unit with pre == 0 and
    mag == 0 is exact in every summation order: not near-kink."""
    bad = torch.zeros(f["r1"].shape[0], dtype=torch.bool)
    for k in ("r1", "z1", "n1"):
        a = f[k].abs()
        bad |= ((a > 0) & (a <= 64 * U * f["mag_" + k])).any(1)
    return bad


def backward(params, cat, g, dtype=torch.float64, mutate=None, f=None):
    """Analytic backward for the cotangent g [n,64] of `out`: dcat [n,176] and side [n,640] = the ten 64-blocks
    [dr1 | dz1 | dR | dZ | dn1 | dN | relu(r1) | relu(z1) | relu(n1) | r*hid]; relu'(0) = 0 as torch has it."""
    p = as_dict(params, dtype)
    cat = cat.detach().cpu().to(dtype)
    g = g.detach().cpu().to(dtype)
    if f is None or mutate:
        f = forward(params, cat, dtype, mutate)
    hid, r, z, q = cat[:, :64], f["r"], f["z"], f["q"]
    mask = (lambda t: (t >= 0).to(dtype)) if mutate == 1 else (lambda t: (t > 0).to(dtype))

    def run(g):
        dN = g * z * ((1 - q) if mutate == 3 else (1 - q * q))
        dZ = g * (q if mutate == 4 else (q - hid)) * z * (1 - z)
        dh = g * (1 - z)
        dn1 = (dN @ p["mlp_n.2.weight"]) * mask(f["n1"])
        dnin = dn1 @ p["mlp_n.0.weight"]                       # [n,152]: d(r * hid) | dx | dxe
        H = dnin[:, :64]
        dR = H * hid * r * (1 - r)
        if mutate != 2:
            dh = dh + H * r
        dr1 = (dR @ p["mlp_r.2.weight"]) * mask(f["r1"])
        dz1 = (dZ @ p["mlp_z.2.weight"]) * mask(f["z1"])
        dcat = dr1 @ p["mlp_r.0.weight"] + dz1 @ p["mlp_z.0.weight"]
        dcat[:, :64] += dh
        dcat[:, 88:] += dnin[:, 64:]
        return dcat, (dr1, dz1, dR, dZ, dn1, dN)

    dcat, pre = run(g)
    n = cat.shape[0]
    if mutate == 5:
        t = torch.arange(n)
        last = t >= 16 * ((n - 1) // 16)
        src = torch.where(last & ((t ^ 1) < n), t ^ 1, t)
        dcat = torch.where(last[:, None], run(g[src])[0], dcat)
    if mutate == 6:
        xe = dcat[:, 152:].reshape(n, 12, 2).flip(-1).reshape(n, 24)
        dcat = torch.cat([dcat[:, :152], xe], -1)
    side = torch.cat(list(pre) + [F.relu(f["r1"]), F.relu(f["z1"]), F.relu(f["n1"]), f["rh"]], -1)
    return dict(dcat=dcat, side=side)


def weight_grad_terms(cat, side):
    """The 12 contractions of fs_ptf_gru_weight_grads as (dY [n,64], X [n,k] or None for a bias) in ptf._gru_params order, on
    the arrays given (any dtype)."""
    b = lambda k: side[:, 64 * k: 64 * k + 64]
    xn = torch.cat([b(9), cat[:, 88:]], -1)
    return [(b(0), cat), (b(0), None), (b(2), b(6)), (b(2), None), (b(1), cat), (b(1), None), (b(3), b(7)), (b(3), None),
            (b(4), xn), (b(4), None), (b(5), b(8)), (b(5), None)]


def weight_grads(cat, side, mutate=None):
    """float64 contraction of the arrays given: [(gradient, sum of |dY| |X|)] per parameter.  Any fp32 summation of the n
    products, in any order, is within (n + 2) u of the second of the first."""
    cat, side = cat.detach().cpu().double(), side.detach().cpu().double()
    if mutate == 8:
        cat, side = cat[:-1], side[:-1]
    out = []
    for dY, X in weight_grad_terms(cat, side):
        if X is None:
            out.append((dY.sum(0), dY.abs().sum(0)))
        else:
            out.append((dY.T @ X, dY.abs().T @ X.abs()))
    return out
