"""The edge rows of the PTF GRU kernels (csrc/ptf_gru.hip), in classes of ONE magnitude regime each, with the per-row figures
and the bounds of the tests on them (test_ptf_gru_edges_host.py on the CPU, test_ptf_gru_edges_hip.py on the device).

A case interleaves the classes that share a weight set row by row, so a row's neighbours in the 16-pair wavefront differ from
it, and every row is judged within its own class (tiny_lat / zero_lat: the tiny / zero_preact rows as a fold step can
build them, the latents scaled and the encodings left as they are):
    mixed   (base weights: GRU() under a fixed seed x 1.5)   plain, hid_x30, g_zero, g_1e4, tiny
    zero    (base weights, first-layer biases zeroed on ZERO_UNITS)   zero_preact, plain
    sat     (base weights, second-layer weights x 40)   tanh_sat
he / xe are sin / cos shaped as in test_ptf_hip.py.  Rows near a ReLU kink (gru_ref.near_kink) are left out of the backward
judgement only; they may be at most 2 % of a case (1 row below 50 rows), which the host test asserts for every case."""
import torch

import gru_ref as gr

CLASSES = ("plain", "hid_x30", "tiny", "tanh_sat", "zero_preact", "g_zero", "g_1e4", "tiny_lat", "zero_lat")
CASES = {"mixed": ("base", ("plain", "hid_x30", "g_zero", "g_1e4", "tiny")),
         "zero": ("zero_bias", ("zero_preact", "plain")),
         "sat": ("sat", ("tanh_sat",)),
         "plain": ("base", ("plain",)),
         "tail": ("base", ("plain",))}           # tail: the last 3 rows 1e3 x the rest (weight gradients only)
CLASS_WEIGHTS = dict(plain="base", hid_x30="base", tiny="base", g_zero="base", g_1e4="base", zero_preact="zero_bias", tanh_sat="sat",
                     tiny_lat="base", zero_lat="zero_fold")
SIZES = (1, 15, 16, 17, 63, 64, 65, 130, 1000)          # edges of a 16-pair wavefront, a 64-pair workgroup, a workgroup beyond n
DW_SIZES = (4097, 16411)                                # the full 256-workgroup grid of the weight gradients, ragged rows_per_wg
FWD_GROUPS = ("out",) + gr.SIDE_BLOCKS[6:]
BWD_GROUPS = ("dcat",) + gr.SIDE_BLOCKS[:6]             # judged on rows clear of a ReLU kink
GROUPS = ("out", "dcat") + gr.SIDE_BLOCKS
# units whose first-layer bias is zeroed: block 0 whole (a lane's four registers in every quarter) and one unit each of blocks
# 1 .. 3, in different quarters and registers (unit = 16 blk + 4 quarter + register)
ZERO_UNITS = tuple(range(16)) + (16 + 4 * 1 + 2, 32 + 4 * 2 + 3, 48 + 4 * 3 + 1)
NEAR_KINK_CAP = 0.02
SEED = 100000           # (chosen so that every case of the device test holds the near-kink cap: the host test asserts it)

_cache = {}


def weights(kind):
    """The 12 parameters (ptf._gru_params order) of weight set `kind`, fp32 on the CPU.  Shared: read-only."""
    if ("w", kind) in _cache:
        return _cache[("w", kind)]
    from freesplat_amd import ptf as P
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(20240607)
        gru = P.GRU()
    ps = dict(zip(gr.KEYS, (1.5 * q.detach().clone() for q in P._gru_params(gru))))
    if kind == "sat":
        for m in ("mlp_r", "mlp_z", "mlp_n"):
            ps[f"{m}.2.weight"] *= 40.0
    elif kind in ("zero_bias", "zero_fold"):
        for m in ("mlp_r", "mlp_z", "mlp_n"):
            ps[f"{m}.0.bias"][list(ZERO_UNITS)] = 0.0
            if kind == "zero_fold":     # rows of a fold step carry encodings that are never zero: their columns go too
                for lo in ((128,) if m == "mlp_n" else (64, 152)):
                    ps[f"{m}.0.weight"][list(ZERO_UNITS), lo:lo + 24] = 0.0
    else:
        assert kind == "base"
    _cache[("w", kind)] = out = [ps[k] for k in gr.KEYS]
    return out


def gru_module(kind, device):
    """A freesplat_amd GRU holding weight set `kind` on `device` (what ptf.gru_tables and the operand streams are built from)."""
    from freesplat_amd import ptf as P
    gru = P.GRU()
    with torch.no_grad():
        for q, v in zip(P._gru_params(gru), weights(kind)):
            q.copy_(v)
    return gru.to(device)


def class_rows(cls, n, seed):
    """n rows of one class: cat [n,176] and the cotangent g [n,64], fp32."""
    gen = torch.Generator().manual_seed(seed)
    cat = torch.randn(n, 176, generator=gen)
    cat[:, 64:88] = torch.sin(cat[:, 64:88] * 3.0)
    cat[:, 152:] = torch.cos(cat[:, 152:] * 3.0)
    g = torch.randn(n, 64, generator=gen)
    if cls == "hid_x30":
        cat[:, :64] *= 30.0
    elif cls == "tiny":
        cat *= 1e-3
    elif cls == "zero_preact":
        cat.zero_()
    elif cls in ("tiny_lat", "zero_lat"):       # what a fold step can build: the latents tiny / zero, the encodings as they are
        cat[:, :64] *= 1e-3 if cls == "tiny_lat" else 0.0
        cat[:, 88:152] *= 1e-3 if cls == "tiny_lat" else 0.0
    elif cls == "g_zero":
        g.zero_()
    elif cls == "g_1e4":
        g *= 1e4
    else:
        assert cls in ("plain", "tanh_sat")
    return cat, g


def build_case(name, n, nonfinite=False):
    """Case `name` at n rows: dict(cat, g, cls = the class of every row, kind = the weight set, skip = bool [n] rows that are
    not judged at all).  nonfinite: hid of one row mid-group holds inf and of another nan (the kernels promise no cross-lane
    traffic: every other row stays in its bound).  Computed once and shared: read-only."""
    key = (name, n, nonfinite)
    if key in _cache:
        return _cache[key]
    kind, order = CASES[name]
    cls = [order[t % len(order)] for t in range(n)]
    cat, g = torch.empty(n, 176), torch.empty(n, 64)
    for k, c in enumerate(order):
        rows = [t for t in range(n) if cls[t] == c]
        if rows:
            cat[rows], g[rows] = class_rows(c, len(rows), SEED + 1000 * list(CASES).index(name) + 17 * n + k)
    skip = torch.zeros(n, dtype=torch.bool)
    if name == "tail":
        g[-3:] *= 1e3                           # (every dY of those rows, hence every product with them, 1e3 x the rest)
    if nonfinite:
        assert n >= 15
        a, b = n - 10, n - 6                    # mid-group rows of the last (maybe ragged) group's neighbourhood
        cat[a, 3], cat[a, 40], cat[b, 17] = float("inf"), float("-inf"), float("nan")
        skip[a] = skip[b] = True
    case = dict(key=key, name=name, n=n, kind=kind, cls=cls, cat=cat, g=g, skip=skip)
    _cache[key] = case
    return case


def reference(case):
    """float64 forward and backward of a case and its near-kink rows: dict(out, dcat, side, kink, fwd).  Shared: read-only."""
    key = ("ref", case["key"])
    if key not in _cache:
        f = gr.forward(weights(case["kind"]), case["cat"])
        b = gr.backward(weights(case["kind"]), case["cat"], case["g"], f=f)
        _cache[key] = dict(out=f["out"], dcat=b["dcat"], side=b["side"], kink=gr.near_kink(f), fwd=f, case=case)
    return _cache[key]


# ------------------------------------------------------------------------------------------------- one fold step that fuses
FOLD_IMAGES = ((8, 12), (7, 9))          # 96 pixels: six whole groups of 16; 63: a ragged last group
FOLD_VARIANTS = {"mixed": ("base", ("plain", "hid_x30", "g_zero", "g_1e4", "tiny_lat")),
                 "sat": ("sat", ("tanh_sat",)),
                 "zero": ("zero_fold", ("zero_lat", "plain"))}
FOLD_FOCAL, FOLD_DEPTH = 16.0, 2.0       # a power of two: every pixel's ray and its projection are exact in fp32


def build_fold(variant, h, w):
    """A state that fuses with the view folded into it: the state IS the view's own unprojected pixels under the identity pose
    (focal length FOLD_FOCAL pixels, depth FOLD_DEPTH everywhere), so Gaussian p lands on pixel p and pair t of the step is
    (state row t, pixel t).  State latents G and view latents lat by the class of the row; state densities R up to 300 and
    weights O up to 40, the view's rho in [0, 1) and om up to 3 (the ranges of test_gru_inputs_rows_and_their_backward).
    cat = the rows the step should build, encodings in float64 rounded once.  Shared: read-only."""
    key = ("fold", variant, h, w)
    if key in _cache:
        return _cache[key]
    kind, order = FOLD_VARIANTS[variant]
    P = h * w
    gen = torch.Generator().manual_seed(31 * h + w + 7 * list(FOLD_VARIANTS).index(variant))
    cls = [order[t % len(order)] for t in range(P)]
    cat, g = torch.empty(P, 176), torch.empty(P, 64)
    for k, c in enumerate(order):
        rows = [t for t in range(P) if cls[t] == c]
        cat[rows], g[rows] = class_rows(c, len(rows), 9000 + 100 * list(FOLD_VARIANTS).index(variant) + 10 * h + k)
    R, O = 300.0 * torch.rand(P, generator=gen), 40.0 * torch.rand(P, generator=gen)
    rho, om = torch.rand(P, generator=gen), 3.0 * torch.rand(P, generator=gen)
    cat[:, 64:88], cat[:, 152:] = gr.pe64(rho, O).float(), gr.pe64(R, om).float()
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    kpix = torch.tensor([FOLD_FOCAL, FOLD_FOCAL, (w - 1) / 2.0, (h - 1) / 2.0])
    X = torch.stack([(xs - kpix[2]) / FOLD_FOCAL * FOLD_DEPTH, (ys - kpix[3]) / FOLD_FOCAL * FOLD_DEPTH,
                     torch.full((h, w), FOLD_DEPTH)], -1).reshape(P, 3)
    c = dict(key=key, name=f"fold_{variant}_{h}x{w}", n=P, kind=kind, cls=cls, cat=cat, g=g, skip=torch.zeros(P, dtype=torch.bool),
             G=cat[:, :64].contiguous(), lat=cat[:, 88:152].contiguous(), R=R, O=O, rho=rho, om=om, X=X, kpix=kpix, h=h, w=w,
             E=torch.eye(4).reshape(1, 16).repeat(P, 1), D=torch.full((P,), FOLD_DEPTH))
    _cache[key] = c
    return c


def gate_forms(case):
    """out, dZ and dN of a case with the float64 pre-activations Z, N pushed through the kernels' two gate forms in fp32 numpy,
    rcp(1 + exp2(-log2(e) x)) and 1 - 2 rcp(1 + exp2(2 log2(e) x)), every other block of side the float64 reference rounded
    once: what those forms alone cost, whatever the contractions do.  (numpy's exp2 and division are correctly rounded, the
    hardware's v_exp_f32 / v_rcp_f32 within 1 ulp: this reads low, if anything.)"""
    import numpy as np
    ref = reference(case)
    f, f32 = ref["fwd"], np.float32
    with np.errstate(all="ignore"):
        Z, N = f["Z"].numpy().astype(f32), f["N"].numpy().astype(f32)
        z = f32(1.0) / (f32(1.0) + np.exp2(f32(-1.44269504088896341) * Z))
        q = f32(1.0) - f32(2.0) * (f32(1.0) / (f32(1.0) + np.exp2(f32(2.88539008177792681) * N)))
        hid, g = case["cat"][:, :64].numpy(), case["g"].numpy()
        out = (f32(1.0) - z) * hid + z * q
        dZ = g * (q - hid) * z * (f32(1.0) - z)
        dN = g * z * (f32(1.0) - q * q)
    side = ref["side"].float()
    side[:, 192:256], side[:, 320:384] = torch.from_numpy(dZ), torch.from_numpy(dN)
    return dict(out=torch.from_numpy(out), side=side)


def bias_first(case):
    """side's blocks 6 .. 8 (relu of the three first layers) with each accumulator STARTING at the bias and taking the products
    in the kernels' order, four (one k-step of v_mfma_f32_16x16x4_f32, summed exactly here) per fp32 rounding: what that
    order alone costs where the bias dominates the sum -- every one of the 44 (38) steps rounds at the bias's magnitude, while
    torch adds the bias to the finished sum, once."""
    import numpy as np
    ref = reference(case)
    ps = dict(zip(gr.KEYS, weights(case["kind"])))
    cat = case["cat"].numpy().astype(np.float64)
    nin = np.concatenate([ref["fwd"]["rh"].numpy(), cat[:, 88:]], 1)
    steps1 = [[44 * g + s for g in range(4)] for s in range(44)]
    stepsn = [[16 * (s >> 2) + 4 * kk + (s & 3) for kk in range(4)] for s in range(16)] + [[64 + 22 * g + s for g in range(4)] for s in range(22)]
    side = ref["side"].float()
    for m, x, steps, blk in (("mlp_r", cat, steps1, 6), ("mlp_z", cat, steps1, 7), ("mlp_n", nin, stepsn, 8)):
        W, b = ps[f"{m}.0.weight"].numpy().astype(np.float64), ps[f"{m}.0.bias"].numpy()
        acc = np.broadcast_to(b, (x.shape[0], 64)).astype(np.float32)
        for ks in steps:
            acc = (acc.astype(np.float64) + x[:, ks] @ W[:, ks].T).astype(np.float32)
        side[:, 64 * blk: 64 * blk + 64] = torch.from_numpy(np.maximum(acc, 0.0))
    return dict(side_fwd=side)


# --------------------------------------------------------------------------------------------------------------- the figures
def _over(err, den):
    """err / den per row; a zero reference must be met exactly (0 where it is, inf where not); a non-finite result reads inf."""
    err = torch.nan_to_num(err.double(), nan=float("inf"), posinf=float("inf"))
    safe = torch.where(den > 0, den, torch.ones_like(den))
    return torch.where(den > 0, err / safe, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))


def row_figures(got, ref, cat):
    """{group: figure per row [n]} for the groups present in `got` (out [n,64], dcat [n,176], side [n,640], or side_fwd = a
    side whose blocks 6 .. 9 alone are filled):
      out        max_j |got - ref| / max(1, max_j |hid_j|)            (tanh has unit range, the gates' stated error is absolute)
      dcat       max_j |got - ref| / max_j |ref_j|
      side 0..5  per 64-block, over max(block max |ref|, 1e-3 x the row's largest |ref| over blocks 0 .. 5)
      side 6..9  per block, over max(block max |ref|, 1e-3 x max(1, max |hid|))"""
    hid = torch.nan_to_num(cat[:, :64].double().abs().amax(1), nan=1.0, posinf=1.0).clamp(min=1.0)
    fig = {}
    d = lambda a, b: (a.detach().cpu().double() - b).abs()
    if "out" in got:
        fig["out"] = _over(d(got["out"], ref["out"]).amax(1), hid)
    if "dcat" in got:
        fig["dcat"] = _over(d(got["dcat"], ref["dcat"]).amax(1), ref["dcat"].abs().amax(1))
    side = got.get("side", got.get("side_fwd"))
    if side is not None:
        n = side.shape[0]
        err = d(side, ref["side"]).reshape(n, 10, 64).amax(2)
        mx = ref["side"].abs().reshape(n, 10, 64).amax(2)
        row = mx[:, :6].amax(1)
        for k, name in enumerate(gr.SIDE_BLOCKS):
            if k < 6 and "side" in got:
                fig[name] = _over(err[:, k], torch.maximum(mx[:, k], 1e-3 * row))
            elif k >= 6:
                fig[name] = _over(err[:, k], torch.maximum(mx[:, k], 1e-3 * hid))
    return fig


def judge(got, ref):
    """{(class, group): (worst figure, row)} of a case's result against reference(case): every row within its class, the
    backward groups on rows clear of a ReLU kink, the skipped (non-finite) rows nowhere."""
    case = ref["case"]
    fig = row_figures(got, ref, case["cat"])
    out = {}
    for c in sorted(set(case["cls"])):
        rows = torch.tensor([x == c for x in case["cls"]]) & ~case["skip"]
        for name, f in fig.items():
            sel = (rows & ~ref["kink"]) if name in BWD_GROUPS else rows
            if bool(sel.any()):
                v = torch.where(sel, f, torch.full_like(f, -1.0))
                out[(c, name)] = (float(v.max()), int(v.argmax()))
    return out


def ratios(worst):
    """{(class, group): figure / TOL} (a zero bound: 0 where met, inf where not)."""
    out = {}
    for (c, name), (e, _) in worst.items():
        tol = GRU_TOL[c][name]
        out[(c, name)] = e / tol if tol > 0 else (0.0 if e == 0 else float("inf"))
    return out


def gate_allowance(case, pair):
    """The ceiling (in units of the bound) of an OVER_BOUND pair on THIS case: 1.5 x what the kernels' gate forms alone read on
    the case's own float64 pre-activations (gate_forms), if that is over the bound; else None -- the pair is held to its bound
    like every other, on every case where the forms do not explain a miss."""
    if pair not in OVER_BOUND:
        return None
    key = ("gates alone", case["key"])
    if key not in _cache:
        _cache[key] = ratios(judge(gate_forms(case), reference(case)))
    alone = _cache[key].get(pair, 0.0)
    return GATE_CEILING * alone if alone > 1.0 else None


def report(what, worst, case=None):
    """One line per class: worst figure / bound of every group; returns the (class, group) pairs over their bound.  A pair of
    OVER_BOUND is let over its bound only on a case on which the gate forms alone read over it, and then up to gate_allowance()
    and no further (its bound proper is asserted, as a strict expected failure, in a test of its own)."""
    r = ratios(worst)
    for c in sorted({k[0] for k in r}):
        print(f"{what}, {c}: figure / bound " + ", ".join(f"{g} {r[(c, g)]:.3f}" for g in GROUPS if (c, g) in r))
    bad = {}
    for k, v in r.items():
        limit = 1.0
        if v > 1.0 and case is not None and gate_allowance(case, k) is not None:
            limit = gate_allowance(case, k)
            print(f"{what}: {k} reads {v:.3f}, let up to {limit:.3f} = {GATE_CEILING} x the gate forms alone on this case")
        if not v <= limit:
            bad[k] = (v, worst[k])
    return bad


def dw_figure(got, want):
    """Worst |got - want| over the derived bound (n + 2) u sum_t |dY_ti| |X_tj| of the 12 gradients: valid for any order of
    summation (a zero bound must be met exactly).  want: gru_ref.weight_grads of the
    same arrays.  Returned in units of u sum |dY| |X|: to be held to n + 2."""
    worst = 0.0
    for a, (b, s) in zip(got, want):
        worst = max(worst, float(_over((a.detach().cpu().double() - b).abs().reshape(-1), s.reshape(-1)).max()))
    return worst


# ----------------------------------------------------------------------------------------------- fp32 against float64, on the CPU
def fp32_torch(case):
    """What fp32 CPU torch gives on a case: out and dcat from oracle.ptf_oracle.gru and autograd, the side blocks from the fp32
    run of the restatement (the oracle does not expose them)."""
    from oracle.ptf_oracle import gru
    ps = weights(case["kind"])
    cat = case["cat"].clone().requires_grad_(True)
    out = gru(dict(zip(gr.KEYS, ps)), cat[:, 88:152], cat[:, :64], cat[:, 152:], cat[:, 64:88])
    (dcat,) = torch.autograd.grad(out, cat, case["g"])
    side = gr.backward(ps, case["cat"], case["g"], dtype=torch.float32)["side"]
    return dict(out=out.detach(), dcat=dcat, side=side)


MEASURE_ROWS = 4096


def measure_case(cls):
    key = ("measure", cls)
    if key not in _cache:
        cat, g = class_rows(cls, MEASURE_ROWS, 50 + CLASSES.index(cls))
        _cache[key] = dict(key=key, name="measure_" + cls, n=MEASURE_ROWS, kind=CLASS_WEIGHTS[cls], cls=[cls] * MEASURE_ROWS, cat=cat, g=g,
                           skip=torch.zeros(MEASURE_ROWS, dtype=torch.bool))
    return _cache[key]


def measure_f32_vs_f64():
    """GRU_F32_VS_F64, measured: {class: {group: worst figure over MEASURE_ROWS rows}} and the share of near-kink rows."""
    out, kink = {}, {}
    for cls in CLASSES:
        case = measure_case(cls)
        ref = reference(case)
        w = judge(fp32_torch(case), ref)
        out[cls] = {g: w[(cls, g)][0] for g in GROUPS}
        kink[cls] = float(ref["kink"].double().mean())
    return out, kink


# What fp32 CPU torch reads against gru_ref in float64 over 4096 rows of each class (x86-64; `python gru_cases.py` prints this).
# The g_zero class's backward groups are exact zeros on both sides.
GRU_F32_VS_F64 = {
    "plain": dict(out=1.84e-07, dcat=3.78e-07, dr1=8.05e-07, dz1=6.70e-07, dR=7.78e-07, dZ=4.30e-07, dn1=6.32e-07, dN=4.57e-07, a_r1=9.58e-07, a_z1=1.06e-06, a_n1=8.18e-07, rh=3.84e-07),    # near-kink rows 0.44 %
    "hid_x30": dict(out=2.52e-06, dcat=5.76e-06, dr1=4.37e-05, dz1=6.57e-06, dR=6.42e-05, dZ=8.16e-06, dn1=2.37e-05, dN=2.51e-05, a_r1=1.24e-06, a_z1=1.35e-06, a_n1=1.62e-06, rh=3.62e-06),    # near-kink rows 0.39 %
    "tiny": dict(out=3.45e-08, dcat=2.42e-07, dr1=6.32e-08, dz1=7.02e-07, dR=1.00e-07, dZ=2.58e-07, dn1=7.38e-07, dN=2.00e-07, a_r1=5.06e-08, a_z1=4.58e-08, a_n1=4.01e-08, rh=1.56e-07),    # near-kink rows 0.02 %
    "tanh_sat": dict(out=8.87e-06, dcat=4.96e-05, dr1=2.43e-04, dz1=1.50e-05, dR=1.84e-04, dZ=1.82e-05, dn1=2.02e-04, dN=7.70e-05, a_r1=9.44e-07, a_z1=9.65e-07, a_n1=1.19e-06, rh=5.69e-06),    # near-kink rows 0.49 %
    "zero_preact": dict(out=1.05e-08, dcat=2.45e-07, dr1=0.00e+00, dz1=6.53e-07, dR=0.00e+00, dZ=2.24e-07, dn1=6.31e-07, dN=1.89e-07, a_r1=0.00e+00, a_z1=0.00e+00, a_n1=0.00e+00, rh=0.00e+00),    # near-kink rows 0.00 %
    "g_zero": dict(out=1.99e-07, dcat=0.00e+00, dr1=0.00e+00, dz1=0.00e+00, dR=0.00e+00, dZ=0.00e+00, dn1=0.00e+00, dN=0.00e+00, a_r1=1.19e-06, a_z1=9.10e-07, a_n1=8.86e-07, rh=3.46e-07),    # near-kink rows 0.37 %
    "g_1e4": dict(out=2.50e-07, dcat=3.78e-07, dr1=7.40e-07, dz1=6.49e-07, dR=9.86e-07, dZ=4.56e-07, dn1=5.79e-07, dN=4.25e-07, a_r1=1.03e-06, a_z1=8.93e-07, a_n1=7.71e-07, rh=2.92e-07),    # near-kink rows 0.63 %
    "tiny_lat": dict(out=1.06e-07, dcat=2.49e-07, dr1=5.34e-08, dz1=6.51e-07, dR=8.91e-08, dZ=5.81e-07, dn1=5.83e-07, dN=2.42e-07, a_r1=8.59e-07, a_z1=8.77e-07, a_n1=3.13e-07, rh=1.76e-07),    # near-kink rows 0.37 %
    "zero_lat": dict(out=6.95e-08, dcat=2.62e-07, dr1=0.00e+00, dz1=6.38e-07, dR=0.00e+00, dZ=5.35e-07, dn1=6.57e-07, dN=2.33e-07, a_r1=5.87e-07, a_z1=5.92e-07, a_n1=3.73e-07, rh=0.00e+00),    # near-kink rows 0.12 %
}
GRU_TOL = {c: {g: 4.0 * v for g, v in t.items()} for c, t in GRU_F32_VS_F64.items()}   # + the kernel's summation order and hardware exp2 / rcp gates
# What the MI355X kernels read, worst figure / GRU_TOL over every case and size of test_ptf_gru_edges_hip.py:
#   plain        out 0.29, dcat 0.64, dr1 0.34, dz1 0.25, dR 0.32, dZ 0.28, dn1 0.30, dN 0.35, a_r1 0.26, a_z1 0.26, a_n1 0.26, rh 0.23
#   hid_x30      out 0.13, dcat 0.13, dr1 0.20, dz1 0.16, dR 0.12, dZ 0.23, dn1 0.18, dN 0.18, a_r1 0.22, a_z1 0.15, a_n1 0.19, rh 0.12
#   tiny         out 0.71, dcat 0.77, dr1 0.21, dz1 0.34, dR 0.17, dZ 1.13, dn1 0.17, dN 0.26, a_r1 0.23, a_z1 0.23, a_n1 0.21, rh 0.24
#   tanh_sat     out 0.24, dcat 0.15, dr1 0.50, dz1 0.31, dR 0.18, dZ 0.28, dn1 0.68, dN 0.53, a_r1 0.26, a_z1 0.23, a_n1 0.31, rh 0.28
#   zero_preact  out 1.03, dcat 0.44, dr1 0, dz1 0.50, dR 0, dZ 1.25, dn1 0.22, dN 0.29, a_r1 0, a_z1 0, a_n1 0, rh 0
#   g_zero       out 0.23, a_r1 0.15, a_z1 0.21, a_n1 0.17, rh 0.17, every backward group 0
#   g_1e4        out 0.17, dcat 0.51, dr1 0.22, dz1 0.21, dR 0.19, dZ 0.17, dn1 0.22, dN 0.32, a_r1 0.17, a_z1 0.22, a_n1 0.24, rh 0.23
#   tiny_lat     out 0.25, dcat 0.63, dr1 0.14, dz1 0.28, dR 0.12, dZ 0.28, dn1 0.13, dN 0.16, a_r1 0.10, a_z1 0.12, a_n1 0.25, rh 0.23   (saved path)
#   zero_lat     out 0.40, dcat 0.44, dr1 0, dz1 0.25, dR 0, dZ 0.41, dn1 0.12, dN 0.17, a_r1 0.14, a_z1 0.18, a_n1 0.15, rh 0         (saved path)
#   weight gradients: 0.33 of (n + 2) u sum |dY| |X| at n = 1, 0.26 at 17, 0.09 at 64, 0.003 at 1000, under 0.001 at 4097 and 16411
#
# (tiny's a_r1 / a_z1 / a_n1 read 5.1 / 5.7 / 4.7 while the kernels started every first-layer accumulator at the bias -- each of
# the 44 k-steps then rounds at the bias's magnitude, and on tiny rows the products are 1e-3 of it; bias_first() reads 2.3 - 2.7
# from that order alone.  The kernels now add the bias to the finished sum, as torch does.)
#
# The three pairs that read over their bound through the exp2 / rcp gate forms: where hid is (next to) zero the row's whole output
# z q, and dZ = g q z (1 - z), carry the ABSOLUTE error of q = 1 - 2 rcp(1 + exp2(..)), 1e-7 on a q of 0.1, while libm's tanhf is
# good to an ulp OF q; the kernel states 2e-7 per gate, and a sigmoid off by exactly that reads 1.00 of zero_preact's out bound
# as well (mutation 9).  A more accurate form is VALU work inside the MFMA kernels: a performance decision.
# Per pair: the cases (name, n) on which the MI355X reads over the bound, with (device figure / bound, the gate forms ALONE in
# fp32 numpy on that case's float64 values: gate_forms).  On every one of them the forms alone are over too; on every other case
# and size the device is inside the bound, and is held to it.  Nothing is excused without a ceiling: on a case where the forms
# alone read a > 1 the pair may read up to GATE_CEILING x a (gate_allowance; numpy's exp2 and division are correctly rounded, the
# hardware's within an ulp, and the contractions add their own roundings -- the device reads 0.83 - 1.10 of a), anything above
# fails outright; test_pairs_read_over_their_bound asserts the bound proper on these cases as strict expected failures.
# zero_preact's forward is ONE row (cat = 0) whatever the size, hence the same out figure at every n.
GATE_CEILING = 1.5
OVER_BOUND = {
    ("zero_preact", "out"): {("zero", n): (1.03, 1.23) for n in SIZES},
    ("zero_preact", "dZ"): {("zero", 130): (1.25, 1.25), ("zero", 1000): (1.23, 1.23)},
    ("tiny", "dZ"): {("mixed", 1000): (1.13, 1.03)},
}


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # the package and the oracle
    table, kink = measure_f32_vs_f64()
    for cls, t in table.items():
        print(f'    "{cls}": dict(' + ", ".join(f"{g}={v:.2e}" for g, v in t.items()) + f"),    # near-kink rows {100 * kink[cls]:.2f} %")
