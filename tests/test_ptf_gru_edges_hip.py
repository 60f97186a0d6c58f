"""The PTF GRU kernels (csrc/ptf_gru.hip: fs_ptf_gru_forward, fs_ptf_gru_backward, fs_ptf_gru_backward_saved,
fs_ptf_gru_weight_grads and the gathering, saving forward inside fs_ptf_fold_step_save) against the float64 restatement
gru_ref.py on the edge classes of gru_cases.py: every row judged within its class, at GRU_TOL = 4 x what fp32 CPU torch reads
against float64; the weight gradients in isolation, against the float64 contraction of the kernel's own fp32 `side` and `cat`
rows, within the bound (n + 2) u sum |dY| |X| that holds for any order of summation.  Every test prints worst figure / bound
per (class, group)."""
import ctypes as C

import pytest
import torch

import gru_cases as gc
import gru_ref as gr

pytestmark = pytest.mark.gpu
_ops = {}


def _operands(kind, dev):
    """(module, forward tables, backward operand stream, transposed-only stream) of a weight set, built once."""
    from freesplat_amd import ptf as P
    if kind not in _ops:
        gru = gc.gru_module(kind, dev)
        _ops[kind] = (gru, P.gru_tables(gru), P.gru_operand_stream(gru), P.gru_operand_stream_t(gru))
    return _ops[kind]


def _nan(*shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def _run(case, dev):
    """fs_ptf_gru_forward and fs_ptf_gru_backward (the re-run form) on a case's rows, into NaN-filled outputs."""
    from freesplat_amd import _lib
    p = _lib.ptr
    _, tab, stream, _ = _operands(case["kind"], dev)
    n = case["n"]
    cat, g = case["cat"].to(dev).contiguous(), case["g"].to(dev).contiguous()
    out, dcat, side = _nan(n, 64, dev=dev), _nan(n, 176, dev=dev), _nan(n, 640, dev=dev)
    _lib.launch("fs_ptf_gru_forward", n, p(cat), p(tab), p(out))
    _lib.launch("fs_ptf_gru_backward", n, p(cat), p(tab), p(stream), p(g), p(dcat), p(side))
    return dict(out=out, dcat=dcat, side=side), cat


def _weight_grads(n, cat, side, dev, twice=False):
    from freesplat_amd import _lib, ptf as P
    L, p = _lib.lib(), _lib.ptr
    flat = torch.zeros(L.fs_ptf_gru_grad_floats(), dtype=torch.float32, device=dev)
    ws = torch.empty(L.fs_ptf_gru_weight_grads_bytes(n), dtype=torch.uint8, device=dev)
    for _ in range(2 if twice else 1):
        _lib.launch("fs_ptf_gru_weight_grads", n, p(cat), p(side), p(flat), p(ws))
    return flat, P.gru_grad_views(flat)


def _exact_zero_checks(case, got, what):
    """zero_preact / zero_lat rows: the pre-activations of ZERO_UNITS are exactly 0, relu'(0) = 0: their dr1 / dz1 / dn1 entries
    are 0.0.  g_zero rows: dcat and side's blocks 0 .. 5 are zeros in every bit but the sign: with g = +0.0 the kernel's
    dZ = g (q - hid) z (1 - z) is 0 x a negative factor = -0.0 wherever q < hid, as IEEE 754 has it, and the
    transposed layers carry those signs on.  A sign bit on a zero is no leak (a leaked neighbour cotangent of
    1e4 would set magnitude bits), so |x| is what must be bitwise zero; DESIGN.md says the same."""
    units = list(gc.ZERO_UNITS)
    rows = [t for t, c in enumerate(case["cls"]) if c in ("zero_preact", "zero_lat") and not bool(case["skip"][t])]
    if rows:
        side = got["side"][rows].cpu()
        for blk in (0, 1, 4):
            assert bool((side[:, 64 * blk: 64 * blk + 64][:, units] == 0).all()), (what, "zero pre-activation, side block", blk)
    rows = [t for t, c in enumerate(case["cls"]) if c == "g_zero" and not bool(case["skip"][t])]
    if rows:
        bits = lambda t: t.abs().contiguous().view(torch.int32)
        assert bool((bits(got["dcat"][rows]) == 0).all()) and bool((bits(got["side"][rows][:, :384]) == 0).all()), (what, "zero cotangent")


@pytest.mark.parametrize("n", gc.SIZES)
@pytest.mark.parametrize("name", ["mixed", "zero", "sat"])
def test_forward_backward_and_weight_gradients_per_row(hip_device, name, n):
    """fs_ptf_gru_forward on materialised rows (out), fs_ptf_gru_backward (dcat and all ten side blocks) per row within the
    class bounds, the exact zeros of the zero_preact and g_zero rows, and fs_ptf_gru_weight_grads on the kernel's own side and
    cat just judged: all 12 gradients per element within (n + 2) u sum |dY| |X| of their float64 contraction; a second call
    into the same buffer doubles it."""
    dev = hip_device
    case = gc.build_case(name, n)
    ref = gc.reference(case)
    got, cat = _run(case, dev)
    bad = gc.report(f"{name} {n}", gc.judge(got, ref), case)
    _exact_zero_checks(case, got, (name, n))
    flat, grads = _weight_grads(n, cat, got["side"], dev)
    fig = gc.dw_figure(grads, gr.weight_grads(cat, got["side"]))
    print(f"{name} {n}: weight gradients, worst error / ((n + 2) u sum |dY| |X|) = {fig / ((n + 2) * gr.U):.3f}")
    assert torch.equal(_weight_grads(n, cat, got["side"], dev, twice=True)[0], 2 * flat)
    assert not bad, f"{name} {n}: (class, group): (figure / bound, (figure, row)) {bad}"
    assert fig <= (n + 2) * gr.U


class OverGateCeiling(Exception):
    """An excused pair reads more than the gate forms explain: a failure, never an expected one."""


def _over_bound_params():
    for (cls, group), cases in sorted(gc.OVER_BOUND.items()):
        for (name, n), (device, alone) in sorted(cases.items()):
            mark = pytest.mark.xfail(strict=True, raises=AssertionError,
                                     reason=f"the exp2 / rcp gate forms: {device:.2f} of the bound on the MI355X, {alone:.2f} from "
                                            "those two formulas alone in fp32 numpy on this case")
            yield pytest.param(cls, group, name, n, marks=mark, id=f"{cls}-{group}-{name}-{n}")


@pytest.mark.parametrize("cls,group,name,n", list(_over_bound_params()))
def test_pairs_read_over_their_bound(hip_device, cls, group, name, n):
    """The (class, group) pairs of gru_cases.OVER_BOUND on every case on which the MI355X reads them over their bound: the bound
    proper, as a strict expected failure (the issue's rule for a miss that the hardware exp2 / rcp gate forms alone produce; a more
    accurate form is VALU work inside the MFMA kernels, a performance decision).  Two-sided: the gate forms alone must read over
    the bound on this very case, and a figure above gate_allowance() = 1.5 x what they read raises OverGateCeiling, which is a
    plain failure -- as it is in the asserting tests above, which let these pairs up to that ceiling on such cases and hold
    them to their bound on every other.  MI355X (gate forms alone): zero_preact out 1.03 (1.23) at every size -- its forward is
    one row --, zero_preact dZ 1.25 (1.25) at 130 rows and 1.23 (1.23) at 1000, tiny dZ 1.13 (1.03) at 1000."""
    case = gc.build_case(name, n)
    limit = gc.gate_allowance(case, (cls, group))
    if limit is None:
        raise OverGateCeiling(f"the gate forms alone do not read {cls} {group} over its bound on {name} {n}")
    got, _ = _run(case, hip_device)
    worst = gc.judge(got, gc.reference(case))
    r = gc.ratios(worst)[(cls, group)]
    print(f"{name} {n}, {cls} {group}: figure {worst[(cls, group)][0]:.3e} = {r:.3f} of the bound, ceiling {limit:.3f}")
    if not r <= limit:
        raise OverGateCeiling(f"{cls} {group} on {name} {n}: {r:.3f} of the bound, the gate forms explain {limit:.3f}")
    assert r <= 1.0, (worst[(cls, group)], r)


@pytest.mark.parametrize("n", [n for n in gc.SIZES if n >= 15])
@pytest.mark.parametrize("name", ["mixed", "zero", "sat"])
def test_a_nonfinite_row_stays_in_its_lane(hip_device, name, n):
    """One row whose hid holds +-inf and one holding nan, mid-group: every OTHER row's out and dcat stay inside their class
    bounds (the kernels' header: no cross-lane traffic anywhere)."""
    case = gc.build_case(name, n, nonfinite=True)
    got, _ = _run(case, hip_device)
    bad = gc.report(f"{name} {n}, non-finite rows", gc.judge(dict(out=got["out"], dcat=got["dcat"]), gc.reference(case)), case)
    assert not bad, bad


@pytest.mark.parametrize("n", gc.DW_SIZES)
@pytest.mark.parametrize("name", ["plain", "tail"])
def test_weight_gradients_on_the_full_grid(hip_device, name, n):
    """fs_ptf_gru_weight_grads at the full 256-workgroup grid with ragged rows per workgroup, on plain rows and with the last 3
    rows 1e3 x the rest: a dropped or doubled tail row exceeds the bound there, although 1 / n is of the bound's order."""
    dev = hip_device
    case = gc.build_case(name, n)
    got, cat = _run(case, dev)
    if name == "plain":
        bad = gc.report(f"{name} {n}", gc.judge(got, gc.reference(case)), case)
        assert not bad, bad
    _, grads = _weight_grads(n, cat, got["side"], dev)
    fig = gc.dw_figure(grads, gr.weight_grads(cat, got["side"]))
    print(f"{name} {n}: weight gradients, worst error / ((n + 2) u sum |dY| |X|) = {fig / ((n + 2) * gr.U):.3f}")
    assert fig <= (n + 2) * gr.U


@pytest.mark.parametrize("h,w", gc.FOLD_IMAGES)
@pytest.mark.parametrize("variant", list(gc.FOLD_VARIANTS))
def test_saving_fold_step_and_saved_backward_at_kernel_level(hip_device, variant, h, w):
    """fs_ptf_fold_step_save for one step (i = 1, M_dev = NULL), queued as _PtfFold.forward queues it, on a state that fuses with
    the view (gru_cases.build_fold); everything below is built from the lists the step returned.  In order: the kept cat rows
    (hidden and latent columns bit-equal, encodings within 5e-6 of float64), the fused rows of oG against the restatement on
    those kept rows, side's blocks 6 .. 9 as the forward left them, then fs_ptf_gru_backward_saved: dcat and side's blocks
    0 .. 5 per row at the bounds of the re-run form, with the exact zeros (the masks here come from kept > 0).  The same step
    through fs_ptf_fold_step gives the same bits."""
    from freesplat_amd import _lib, ptf as P
    L, p, dev = _lib.lib(), _lib.ptr, hip_device
    c = gc.build_fold(variant, h, w)
    Pn = h * w
    _, tab, _, stream_t = _operands(c["kind"], dev)
    to = lambda t: t.to(dev).contiguous()
    G, X, R, O, E, D = (to(c[k]) for k in ("G", "X", "R", "O", "E", "D"))
    lat, rho, om, kpix = (to(c[k]) for k in ("lat", "rho", "om", "kpix"))
    eye = torch.eye(4, device=dev).reshape(16).contiguous()
    counts = torch.zeros(2, 4, dtype=torch.int32, device=dev)

    def step(save):
        out = [_nan(2 * Pn, k, dev=dev) for k in P.STATE_WIDTHS]
        scratch = torch.empty(L.fs_ptf_fold_scratch_bytes(Pn, h, w), dtype=torch.uint8, device=dev)
        args = (Pn, None, h, w, p(G), p(X), p(R), p(O), p(E), p(D), p(lat), p(X), p(rho), p(om), p(D), p(eye), p(eye), p(kpix),
                C.c_float(0.1), p(tab), p(scratch), *[p(t) for t in out], p(counts[int(save)]))
        if not save:
            _lib.launch("fs_ptf_fold_step", *args)
            return out, scratch, None
        kept = (_nan(Pn, L.fs_ptf_gru_side_cols(), dev=dev), _nan(-(-Pn // 16) * 16, L.fs_ptf_gru_act_cols(), dev=dev),
                _nan(Pn, 176, dev=dev))
        _lib.launch("fs_ptf_fold_step_save", *args, *[p(t) for t in kept])
        return out, scratch, kept

    out, scratch, (side, act, cat) = step(True)
    nk, nf, na, n_out = counts[1].tolist()
    assert nf >= 0.9 * Pn and nk + nf + na == n_out, (nk, nf, na, n_out)
    lists = (C.c_void_p * 4)()
    _lib.call("fs_ptf_fold_step_lists", Pn, h, w, p(scratch), lists)

    def read(k, n):
        off = lists[k] - scratch.data_ptr()
        return scratch[off: off + 8 * n].view(torch.int64).cpu()
    fuse, fpix = read(1, nf), read(2, nf)
    assert torch.equal(fuse, fpix), "a Gaussian of the scene does not land on its own pixel"
    # 1. the rows the step kept
    want = torch.cat([c["G"][fuse].double(), gr.pe64(c["rho"][fpix], c["O"][fuse]), c["lat"][fpix].double(),
                      gr.pe64(c["R"][fuse], c["om"][fpix])], -1)
    kept = cat[:nf].cpu()
    assert torch.equal(kept[:, :64], c["G"][fuse]) and torch.equal(kept[:, 88:152], c["lat"][fpix])
    assert float((kept.double() - want).abs().max()) < 5e-6
    # the case of those rows: classes by the state row, the reference on the KEPT rows
    g = c["g"][fuse].contiguous()
    case = dict(key=("fold on device", variant, h, w), name=c["name"], n=nf, kind=c["kind"], cls=[c["cls"][m] for m in fuse.tolist()],
                cat=kept, g=g, skip=torch.zeros(nf, dtype=torch.bool))
    gc._cache.pop(("ref", case["key"]), None)
    ref = gc.reference(case)
    assert int(ref["kink"].sum()) <= (1 if nf < 50 else int(gc.NEAR_KINK_CAP * nf))
    # 2., 3. the fused rows of the out state and the activations the forward left
    fwd = dict(out=out[0][nk: nk + nf], side_fwd=side[:nf].clone())
    bad = gc.report(f"{c['name']}: saving forward", gc.judge(fwd, ref))
    assert not bad, bad
    # 4. the backward that re-runs nothing
    gd, dcat = g.to(dev), _nan(nf, 176, dev=dev)
    _lib.launch("fs_ptf_gru_backward_saved", nf, p(cat), p(stream_t), p(act), p(gd), p(dcat), p(side))
    got = dict(dcat=dcat, side=side[:nf])
    bad = gc.report(f"{c['name']}: saved backward", gc.judge(got, ref))
    _exact_zero_checks(case, got, c["name"])
    assert not bad, bad
    # the step that saves nothing: the same bits
    out2, _, _ = step(False)
    assert counts[0].tolist() == [nk, nf, na, n_out]
    assert bool(torch.isfinite(out[0][:n_out]).all()) and torch.equal(out2[0][:n_out], out[0][:n_out])
