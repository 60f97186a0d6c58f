"""CPU checks of the evaluation metrics (freesplat_amd/metrics.py, fs_image_metrics / fs_depth_metrics): the float64
restatement (tests/metrics_ref.py) against known answers and the reference's outputs (tests/golden/depth_metrics.npz),
the C ABI's sizes and argument checks without a device, the opt-in drop-in wiring on a fake reference tree, and the
absence of host synchronisation in the product module."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "depth_metrics.npz")


def test_restatement_identical_images_give_one():
    x = np.random.default_rng(0).random((3, 20, 31))
    assert R.ssim(x, x) == pytest.approx(1.0, abs=1e-12)


@pytest.mark.parametrize("a,b", [(0.2, 0.7), (0.5, 0.5), (1.3, -0.4)])
def test_restatement_constant_images_closed_form(a, b):
    want = (2 * a * b + R.C1) / (a * a + b * b + R.C1)
    got = R.ssim(np.full((2, 15, 17), a), np.full((2, 15, 17), b))
    assert got == pytest.approx(want, abs=1e-12)


def test_restatement_never_reads_the_padding():
    """Against scipy's full-image Gaussian filter with three padding modes, cropped by 5: all three agree with the
    restatement, so the padding (skimage's 'reflect') cannot change the value."""
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(1)
    x, y = rng.random((2, 40, 53)), rng.random((2, 40, 53))
    for mode in ("reflect", "constant", "nearest"):
        f = lambda a: ndi.gaussian_filter(a, sigma=1.5, truncate=3.5, mode=mode)
        vals = []
        for xc, yc in zip(x, y):
            ux, uy, uxx, uyy, uxy = f(xc), f(yc), f(xc * xc), f(yc * yc), f(xc * yc)
            vx, vy, vxy = (R.COV_NORM * (uxx - ux * ux), R.COV_NORM * (uyy - uy * uy), R.COV_NORM * (uxy - ux * uy))
            S = ((2 * ux * uy + R.C1) * (2 * vxy + R.C2)) / ((ux * ux + uy * uy + R.C1) * (vx + vy + R.C2))
            vals.append(S[5:-5, 5:-5].mean())
        assert float(np.mean(vals)) == pytest.approx(R.ssim(x, y), abs=1e-12), mode


def test_restatement_matches_skimage():
    sk = pytest.importorskip("skimage.metrics")
    rng = np.random.default_rng(2)
    x = rng.random((3, 48, 64)).astype(np.float32)
    y = np.clip(x + 0.05 * rng.standard_normal(x.shape), 0, 1).astype(np.float32)
    want = sk.structural_similarity(x, y, win_size=11, gaussian_weights=True, channel_axis=0, data_range=1.0)
    assert R.ssim(x, y) == pytest.approx(want, abs=1e-6)


def test_restatement_rejects_small_images():
    with pytest.raises(ValueError):
        R.ssim(np.zeros((1, 10, 30)), np.zeros((1, 10, 30)))


def _close_with_nan(got, want, rel=1e-6):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    m = ~np.isnan(want)
    assert np.array_equal(np.isinf(got[m]), np.isinf(want[m])), (got, want)
    f = m & ~np.isinf(want)
    assert np.allclose(got[f], want[f], rtol=rel, atol=0), (got, want)


@pytest.mark.parametrize("case", ["mixed", "single", "empty", "inf_pred"])
def test_depth_restatement_matches_reference_outputs(case):
    z = np.load(GOLD)
    gt, pred = z[f"{case}__gt"], z[f"{case}__pred"]
    n = gt.shape[0] * gt.shape[1]
    r = R.depth(gt.reshape(n, -1), pred.reshape(n, -1))
    for k in ("abs_diff", "abs_rel", "delta_25", "delta_10"):
        _close_with_nan(r[k].mean(), z[f"{case}__{k}"])


def test_psnr_restatement_matches_reference_outputs():
    z = np.load(GOLD)
    with np.errstate(divide="ignore"):
        psnr = -10 * np.log10(R.mse(z["psnr__gt"], z["psnr__pred"]))
    _close_with_nan(psnr, z["psnr__out"], rel=1e-5)
    assert np.isinf(z["psnr__out"][3])


def test_metrics_abi_sizes_and_argument_checks():
    """Scratch sizes and FS_ERR_INVALID_ARG before any device is touched (NULL pointers: a device access would fault)."""
    from freesplat_amd import _lib
    L = _lib.lib()
    n16 = L.fs_image_metrics_scratch_bytes(16, 3, 968, 1296)
    n1 = L.fs_image_metrics_scratch_bytes(1, 3, 968, 1296)
    assert n1 >= 3 * 16 and n16 >= 16 * (n1 - 255) and n16 % 256 == 0
    assert L.fs_image_metrics_scratch_bytes(1, 1, 11, 11) > 0
    for bad in ((0, 3, 64, 64), (1, 0, 64, 64), (1, 3, 10, 64), (1, 3, 64, 10), (-1, 3, 64, 64)):
        assert L.fs_image_metrics_scratch_bytes(*bad) == 0, bad
    V = ctypes.c_void_p
    p = V(0x1000)       # never dereferenced: every call below fails its argument check
    assert L.fs_image_metrics(1, 3, 10, 64, p, p, p, p, None, p, None) == -1           # H = 10
    assert L.fs_image_metrics(1, 3, 64, 10, p, p, p, p, None, p, None) == -1           # W = 10
    assert L.fs_image_metrics(0, 3, 64, 64, p, p, p, p, None, p, None) == -1
    assert L.fs_image_metrics(1, 0, 64, 64, p, p, p, p, None, p, None) == -1
    for i in (4, 5, 6, 7, 9):                                                         # gt, pred, ssim, mse, scratch
        args = [1, 3, 64, 64, p, p, p, p, None, p, None]
        args[i] = None
        assert L.fs_image_metrics(*args) == -1, i
    assert L.fs_depth_metrics_scratch_bytes(6, 384 * 512) >= 6 * 6 * 8
    assert L.fs_depth_metrics_scratch_bytes(0, 100) == 0 and L.fs_depth_metrics_scratch_bytes(2, 0) == 0
    for i in (2, 3, 5, 6):
        args = [2, 100, p, p, 0.5, p, p, None]
        args[i] = None
        assert L.fs_depth_metrics(*args) == -1, i
    assert L.fs_depth_metrics(0, 100, p, p, 0.5, p, p, None) == -1


def test_metrics_module_queues_device_work_only():
    """No host synchronisation in the evaluation path: the results stay on the device until the caller reads them."""
    src = open(os.path.join(ROOT, "freesplat_amd", "metrics.py")).read()
    for pat in (r"\.item\(", r"\.cpu\(", r"\.tolist\(", r"synchronize"):
        assert not re.search(pat, src), pat


# ---- drop-in wiring on a fake reference tree ----

_FAKE = {
    "src/__init__.py": "",
    "src/evaluation/__init__.py": "",
    "src/evaluation/metrics.py": "def compute_psnr(a, b): return 'ref'\ndef compute_ssim(a, b): return 'ref'\n"
                                 "def compute_lpips(a, b): return 'ref'\n",
    "src/evaluation/metric_computer.py": "from .metrics import compute_lpips, compute_psnr, compute_ssim\n",
    "src/model/__init__.py": "",
    "src/model/model_wrapper.py": "from ..evaluation.metrics import compute_lpips, compute_psnr, compute_ssim\n"
                                  "def depth_render_metrics(prediction, batch): return 'ref'\n",
    "src/model/encoder/__init__.py": "",
    "src/model/encoder/modules/__init__.py": "",
    "src/model/encoder/modules/cost_volume.py": "class AVGFeatureVolumeManager: pass\n",
    "src/model/encoder/modules/networks.py": "class DepthDecoder:\n    def forward(self, x): return 'ref'\n",
    "src/model/encoder/encoder_freesplat.py": "class AVGFeatureVolumeManager: pass\nclass GaussianAdapter: pass\n"
                                              "class GRU: pass\nclass EncoderFreeSplat:\n"
                                              "    def forward(self): return 'ref'\n"
                                              "    def fuse_gaussians(self): return 'ref'\n",
}
_NAMES = [f"{m}.{n}" for m in ("src.evaluation.metrics", "src.model.model_wrapper", "src.evaluation.metric_computer")
          for n in ("compute_psnr", "compute_ssim")] + ["src.model.model_wrapper.depth_render_metrics"]


@pytest.fixture
def fake_src(tmp_path, monkeypatch):
    for rel, txt in _FAKE.items():
        f = tmp_path / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(txt)
    saved = {k: v for k, v in sys.modules.items() if k == "src" or k.startswith("src.")}
    for k in saved:
        del sys.modules[k]
    monkeypatch.syspath_prepend(str(tmp_path))
    yield tmp_path
    for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
        del sys.modules[k]
    sys.modules.update(saved)


def _lookup(dotted):
    import importlib
    mod, name = dotted.rsplit(".", 1)
    return getattr(importlib.import_module(mod), name)


def test_patch_metrics_rebinds_every_listed_name(fake_src):
    from freesplat_amd import compat, metrics
    done = compat.patch_metrics()
    assert sorted(done) == sorted(_NAMES)
    for name in _NAMES:
        got = _lookup(name)
        assert got is getattr(metrics, name.rsplit(".", 1)[1]), name
        assert done[name] is got
    assert _lookup("src.evaluation.metric_computer.compute_lpips")(0, 0) == "ref"


def test_patch_reference_leaves_metrics_alone_by_default(fake_src):
    from freesplat_amd import compat
    done = compat.patch_reference(decoder=False)
    assert not any(n in done for n in _NAMES)
    assert "src.model.model_wrapper" not in sys.modules and "src.evaluation.metrics" not in sys.modules
    done = compat.patch_reference(decoder=False, metrics=True)
    assert all(n in done for n in _NAMES)
    assert _lookup("src.model.model_wrapper.depth_render_metrics").__module__ == "freesplat_amd.metrics"


def test_run_strips_gpu_metrics_flag(fake_src, monkeypatch):
    from freesplat_amd import compat
    from freesplat_amd.compat import run
    seen = {}
    real = compat.patch_reference
    monkeypatch.setattr(compat, "patch_reference", lambda **k: seen.update(k) or real(decoder=False, **k))
    (fake_src / "fake_target.py").write_text("import sys\nARGV = list(sys.argv)\n")
    captured = {}
    monkeypatch.setattr(run.runpy, "run_module", lambda mod, **k: captured.update(argv=list(sys.argv), mod=mod))
    monkeypatch.setattr(sys, "argv", list(sys.argv))
    done = run.main(["fake_target", "a=1", "--gpu-metrics", "b=2"])
    assert seen == {"metrics": True}
    assert captured == {"argv": ["fake_target", "a=1", "b=2"], "mod": "fake_target"}
    assert all(n in done for n in _NAMES)
    seen.clear()
    run.main(["fake_target", "a=1"])
    assert seen == {"metrics": False} and captured["argv"] == ["fake_target", "a=1"]
