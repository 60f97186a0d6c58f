"""CPU side of the PTF GRU kernels' edge tests (gru_cases.py, gru_ref.py): the float64 restatement equals float64 autograd of the
reference-pinned oracle, fp32 torch is inside half of every bound the device is held to, the near-kink cap holds for every case
the device test runs, and the per-row figures see each plausible kernel mistake (gru_ref.MUTATIONS) -- most of which the
tensor-wide criteria of test_ptf_hip.py (1e-4 of a tensor's max-abs, 1e-5 absolute on the output) let through.  Nothing here
touches a device."""
import pytest
import torch

import gru_cases as gc
import gru_ref as gr


def _autograd64(case):
    from oracle.ptf_oracle import gru
    ps = [q.double().requires_grad_(True) for q in gc.weights(case["kind"])]
    cat = case["cat"].double().requires_grad_(True)
    out = gru(dict(zip(gr.KEYS, ps)), cat[:, 88:152], cat[:, :64], cat[:, 152:], cat[:, 64:88])
    grads = torch.autograd.grad(out, [cat] + ps, case["g"].double())
    return out.detach(), grads[0], grads[1:]


@pytest.mark.parametrize("cls", gc.CLASSES)
def test_restatement_equals_float64_autograd_of_the_oracle(cls):
    """out and dcat per row and the 12 parameter gradients (the float64 contraction of the restatement's `side` with its
    inputs) to 1e-12.  Where the 48 rows of a class have full rank, dW = dY^T X pins every entry of the six dY blocks and, through
    the second layers, of the activation blocks; the zero_preact rows are all the same zero row (rank 0), so there only the
    column sums of the dY blocks (the bias gradients) and dcat are pinned -- zero_lat, the same rows with their encodings left
    in, is the full-rank form of that class, and the exact-zero entries are asserted directly below."""
    cat, g = gc.class_rows(cls, 48, 5)
    case = dict(key=("host", cls), name=cls, n=48, kind=gc.CLASS_WEIGHTS[cls], cls=[cls] * 48, cat=cat, g=g,
                skip=torch.zeros(48, dtype=torch.bool))
    ref = gc.reference(case)
    out, dcat, pgrads = _autograd64(case)
    fig = gc.row_figures(dict(out=out, dcat=dcat), ref, cat)
    assert float(fig["out"].max()) <= 1e-12 and float(fig["dcat"].max()) <= 1e-12, {k: float(v.max()) for k, v in fig.items()}
    for k, ((got, _), want) in enumerate(zip(gr.weight_grads(cat.double(), ref["side"]), pgrads)):
        assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1e-300), (gr.KEYS[k], cls)
    if cls in ("zero_preact", "zero_lat"):       # relu'(0) = 0, as torch has it
        f, units = ref["fwd"], list(gc.ZERO_UNITS)
        for k, pre in enumerate(("r1", "z1")):
            assert bool((f[pre][:, units] == 0).all())
            assert bool((ref["side"][:, 64 * k: 64 * k + 64][:, units] == 0).all())
        assert bool((f["n1"][:, units] == 0).all()) and bool((ref["side"][:, 256:320][:, units] == 0).all())
        mut = gr.backward(gc.weights(case["kind"]), cat, g, mutate=1)
        assert bool((mut["side"][:, 256:320][:, units] != 0).any())


@pytest.mark.parametrize("cls", gc.CLASSES)
def test_fp32_torch_within_half_of_every_bound(cls):
    """Over the 4096 rows the table was measured on, fp32 CPU torch reads at most half of GRU_TOL (= 2 x what was recorded), so
    that BLAS threading or another libm cannot flip a bound; the kernels' two gate forms alone, in fp32 numpy on the float64
    pre-activations, are printed beside it."""
    case = gc.measure_case(cls)
    ref = gc.reference(case)
    worst = gc.judge(gc.fp32_torch(case), ref)
    r = gc.ratios(worst)
    print(f"{cls}: fp32 torch figure / bound " + ", ".join(f"{g} {r[(cls, g)]:.3f}" for g in gc.GROUPS))
    gate = gc.ratios(gc.judge(gc.gate_forms(case), ref))
    print(f"{cls}: the exp2 / rcp gate forms alone, figure / bound " + ", ".join(f"{g} {gate[(cls, g)]:.3f}" for g in ("out", "dZ", "dN")))
    assert max(r.values()) <= 0.5, {k: v for k, v in r.items() if v > 0.5}
    assert float(ref["kink"].double().mean()) <= gc.NEAR_KINK_CAP


def _device_cases():
    out = [gc.build_case(name, n) for name in ("mixed", "zero", "sat") for n in gc.SIZES]
    out += [gc.build_case(name, n, nonfinite=True) for name in ("mixed", "zero", "sat") for n in gc.SIZES if n >= 15]
    out += [gc.build_case(name, n) for name in ("plain", "tail") for n in gc.DW_SIZES]
    out += [gc.build_fold(v, h, w) for v in gc.FOLD_VARIANTS for h, w in gc.FOLD_IMAGES]
    return out


def near_kink_allowed(n):
    return 1 if n < 50 else int(gc.NEAR_KINK_CAP * n)


def test_every_device_case_holds_its_classes_and_the_near_kink_cap():
    """The exact inputs of test_ptf_gru_edges_hip.py: near-kink rows at most 2 % of a case (1 row below 50), fp32 torch inside
    half the bounds on them too, and each class shows what it is there for."""
    for case in _device_cases():
        ref = gc.reference(case)
        kink = int((ref["kink"] & ~case["skip"]).sum())
        assert kink <= near_kink_allowed(case["n"]), (case["name"], case["n"], kink)
        if case["name"] == "tail":
            continue                            # (weight gradients only: judged by the derived bound, not by class)
        r = gc.ratios(gc.judge(gc.fp32_torch(case), ref))
        assert max(r.values()) <= 0.5, (case["name"], case["n"], {k: v for k, v in r.items() if v > 0.5})
    f32 = lambda t: t.float()
    # hid_x30: gates that reach exactly 0 or 1 in fp32;  tanh_sat: pre-activations in the tens to hundreds (the kernels' exp2
    # overflows to inf from 128 / 1.4427 = 88.7 on), 1 - q q and z (1 - z) exactly 0 for many units
    f = gc.reference(gc.build_case("mixed", 1000))["fwd"]
    rows = torch.tensor([c == "hid_x30" for c in gc.build_case("mixed", 1000)["cls"]])
    r, z = f32(f["r"][rows]), f32(f["z"][rows])
    assert int(((r == 0) | (r == 1)).sum()) >= 10 and int(((z == 0) | (z == 1)).sum()) >= 10
    assert float(f["r1"][rows].abs().max()) >= 30.0
    f = gc.reference(gc.build_case("sat", 1000))["fwd"]
    for k in ("R", "Z", "N"):
        assert float(f[k].abs().max()) >= 80.0 and float(f[k].abs().median()) >= 10.0, k
    # (the sigmoid's exp2(-1.4427 x) is inf below -88.7, the tanh's exp2(2.885 x) above 44.4)
    assert float(torch.minimum(f["R"], f["Z"]).min()) <= -89.0 and int((f["N"] >= 45.0).sum()) >= 100
    q, z = f32(f["q"]), f32(f["z"])
    assert float(((1 - q * q) == 0).double().mean()) >= 0.3 and float(((z * (1 - z)) == 0).double().mean()) >= 0.1
    assert float(((1 - q * q) > 0).double().mean()) >= 0.02
    # zero_preact: pre-activations exactly 0 on the chosen units, in fp32 arithmetic of any order (zero row, zero bias)
    case = gc.build_case("zero", 130)
    f = gc.reference(case)["fwd"]
    rows = torch.tensor([c == "zero_preact" for c in case["cls"]])
    for k in ("r1", "z1", "n1"):
        assert bool((f[k][rows][:, list(gc.ZERO_UNITS)] == 0).all()) and bool((f["mag_" + k][rows][:, list(gc.ZERO_UNITS)] == 0).all())
    # g_zero rows sit beside g_1e4 rows
    cls = gc.build_case("mixed", 130)["cls"]
    assert any(a == "g_zero" and b == "g_1e4" for a, b in zip(cls, cls[1:]))


# ------------------------------------------------------------------------------------------------------------------ mutations
_MUT_CASES = (("mixed", 1000), ("zero", 130), ("sat", 130))
_NAMED = {1: "zero_preact", 4: "hid_x30", 5: "g_zero"}


def _run64(case, mutate=None):
    ps = gc.weights(case["kind"])
    f = gr.forward(ps, case["cat"], mutate=mutate)
    b = gr.backward(ps, case["cat"], case["g"], mutate=mutate, f=f)
    return dict(out=f["out"], dcat=b["dcat"], side=b["side"])


def _old_criteria(case, mut, ref):
    """What test_ptf_hip.py's tensor-wide criteria read: max |a - b| / max |b| of dcat and of the 12 parameter gradients
    (bar 1e-4), max |a - b| of the output (bar 1e-5)."""
    rel = lambda a, b: float((a - b).abs().max() / (b.abs().max() + 1e-20))
    cat = case["cat"].double()
    grads = max(rel(a, b) for (a, _), (b, _) in zip(gr.weight_grads(cat, mut["side"]), gr.weight_grads(cat, ref["side"])))
    return max(rel(mut["dcat"], ref["dcat"]), grads), float((mut["out"] - ref["out"]).abs().max())


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 9])
def test_figures_see_each_kernel_mistake(k):
    """With ONE mistake switched on in the float64 restatement, judged by the device test's own figures and bounds against the
    unmutated reference: at least 2 x a bound in the class named for it (1: zero_preact, 4: hid_x30, 5: g_zero, else any).
    Mutation 9, a sigmoid off by the 2e-7 the kernel states for its gates, must stay inside every bound (inside the ceiling
    gru_cases.gate_allowance, on a case where the gate forms themselves take a pair over its bound).
    Beside it the test prints what the older tensor-wide criteria of test_ptf_hip.py read on the same cases (DESIGN.md has the
    table): the whole-term mistakes 2 - 6 were within their reach on randn rows; 1 needs rows with an exactly zero
    pre-activation, 7 is invisible in every gradient, and so is any error confined to rows that are small beside the
    tensor's largest, which is why the figures here are per row."""
    best, named, over = (0.0, None), 0.0, {}
    for name, n in _MUT_CASES:
        case = gc.build_case(name, n)
        ref = gc.reference(case)
        mut = _run64(case, mutate=k)
        r = gc.ratios(gc.judge(mut, ref))
        top = max(r, key=r.get)
        old = _old_criteria(case, mut, ref)
        print(f"mutation {k} ({gr.MUTATIONS[k]}), {name} {n}: worst figure / bound {r[top]:.3g} {top}; tensor-wide: gradients "
              f"{old[0]:.1e} ({'seen' if old[0] >= 1e-4 else 'NOT seen'} at 1e-4), output {old[1]:.1e} "
              f"({'seen' if old[1] >= 1e-5 else 'NOT seen'} at 1e-5)")
        over.update({(name, n) + kk: v for kk, v in r.items() if not v <= (gc.gate_allowance(case, kk) or 1.0)})
        if r[top] > best[0]:
            best = (r[top], top)
        named = max([named] + [v for (c, _), v in r.items() if c == _NAMED.get(k, c)])
    if k == 9:      # (a pair the gate forms themselves take over its bound on a case is held to its ceiling there, as on the device)
        assert not over, f"a sigmoid within the kernel's stated 2e-7 reads {over}"
    else:
        assert named >= 2.0, f"mutation {k} is invisible: {best}"


@pytest.mark.parametrize("n", gc.DW_SIZES)
def test_weight_gradient_bound_sees_a_dropped_tail_row(n):
    """Mutation 8: the last live row left out of the contraction.  On the tail-heavy case it reads at least 2 x the derived
    bound; on the plain case 1 / n is of the bound's order and it may not (printed)."""
    u = gr.U
    for name in ("tail", "plain"):
        case = gc.build_case(name, n)
        f32 = gc.fp32_torch(case)
        want = gr.weight_grads(case["cat"], f32["side"])
        mut = [a for a, _ in gr.weight_grads(case["cat"], f32["side"], mutate=8)]
        fig = gc.dw_figure(mut, want) / ((n + 2) * u)
        rel = max(float((a - b).abs().max() / (b.abs().max() + 1e-20)) for a, (b, _) in zip(mut, want))
        print(f"mutation 8, {name} {n}: worst error / bound {fig:.3g}; tensor-wide {rel:.1e} ({'seen' if rel >= 1e-4 else 'NOT seen'} at 1e-4)")
        if name == "tail":
            assert fig >= 2.0
        # the float64 contraction itself is inside the bound of an fp32 one, by many orders
        assert gc.dw_figure([a.float() for a, _ in want], want) / ((n + 2) * u) <= 1.0


@pytest.mark.parametrize("cls,group", sorted(gc.OVER_BOUND))
def test_gate_forms_alone_read_each_excused_pair_over_its_bound(cls, group):
    """gru_cases.OVER_BOUND: on every case recorded for a pair, the kernels' two gate forms ALONE, in fp32 numpy on the float64
    pre-activations of that very case, read over the pair's bound (within 10 % of what is recorded for them), and leave every
    other group they touch inside its bound -- so the miss is the forms' and not a contraction's -- and the device's recorded
    figure is inside the ceiling the asserting tests hold it to."""
    for (name, n), (device, alone) in gc.OVER_BOUND[(cls, group)].items():
        case = gc.build_case(name, n)
        r = gc.ratios(gc.judge(gc.gate_forms(case), gc.reference(case)))
        print(f"{cls} {group}, {name} {n}: the gate forms alone read {r[(cls, group)]:.3f} of the bound")
        assert r[(cls, group)] > 1.0 and abs(r[(cls, group)] - alone) <= 0.1 * alone
        assert 1.0 < device <= gc.gate_allowance(case, (cls, group)) == gc.GATE_CEILING * r[(cls, group)]
        assert {k for k, v in r.items() if v > 1.0} <= set(gc.OVER_BOUND)
    assert gc.gate_allowance(gc.build_case("sat", 130), (cls, group)) is None       # no such rows, nothing excused


def test_an_accumulator_that_starts_at_the_bias_misses_the_tiny_class():
    """Why the kernels add the first layers' biases to the FINISHED sums: the other order alone (gru_cases.bias_first: fp32
    numpy, every k-step's four products summed exactly) reads 2.3 - 2.7 of the tiny class's bounds on relu(r1), relu(z1),
    relu(n1) -- 44 roundings at the bias's magnitude where the products are 1e-3 of it -- and stays inside every other class's."""
    case = gc.build_case("mixed", 1000)
    r = gc.ratios(gc.judge(gc.bias_first(case), gc.reference(case)))
    print({k: round(v, 2) for k, v in r.items() if k[0] == "tiny"})
    for g in ("a_r1", "a_z1", "a_n1"):
        assert r[("tiny", g)] > 2.0
    assert {k for k, v in r.items() if v > 1.0} == {("tiny", g) for g in ("a_r1", "a_z1", "a_n1")}
