"""CPU checks of LPIPS (freesplat_amd/lpips.py, fs_lpips_*): the additive C ABI, size queries and argument checks without a
device, weight loading in both accepted key layouts, the refusal of CPU tensors, and the opt-in drop-in wiring on a fake
reference tree.  No fixture comes from the reference: it imports LPIPS from a package outside its tree."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fs_lpips_scratch_bytes", "fs_lpips_saved_bytes", "fs_lpips_layer_forward", "fs_lpips_layer_backward",
       "fs_lpips_prepare_forward", "fs_lpips_prepare_backward")


@pytest.fixture(autouse=True)
def _clean_defaults(monkeypatch):
    from freesplat_amd import lpips as L
    monkeypatch.delenv(L.ENV_WEIGHTS, raising=False)
    monkeypatch.delenv("FREESPLAT_LPIPS", raising=False)
    L.set_default_weights(None)
    yield
    L.set_default_weights(None)


def test_abi_is_additive_and_declared_on_both_sides():
    from freesplat_amd import _lib
    text = open(os.path.join(ROOT, "include", "freesplat_amd.h")).read()
    assert re.search(r"#define FS_ABI_VERSION 9\b", text) and _lib.ABI_VERSION == 9
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH) if os.path.exists(_lib.LIB_PATH) else ctypes.CDLL(_lib.build())
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} not declared in include/freesplat_amd.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(L, name), f"{name} not exported"
    assert _lib.lib().fs_abi_version() == 9


def test_size_queries_and_argument_checks():
    from freesplat_amd import _lib
    L = _lib.lib()
    shapes = [(1, 64, 3, 5), (1, 64, 37, 53), (3, 64, 37, 53), (4, 64, 968, 1296), (8, 64, 968, 1296), (4, 512, 60, 81)]
    for B, C, H, W in shapes:
        n = L.fs_lpips_scratch_bytes(B, C, H, W)
        assert n >= B * ((H * W + 63) // 64) * 4 and n % 256 == 0
        assert L.fs_lpips_saved_bytes(B, C, H, W) == 16 * B * H * W
        assert L.fs_lpips_scratch_bytes(B + 1, C, H, W) >= n and L.fs_lpips_scratch_bytes(B, C, H + 1, W) >= n
        assert L.fs_lpips_scratch_bytes(B, C, H, W + 64) > n - 256
    for bad in ((0, 64, 8, 8), (1, 0, 8, 8), (1, 64, 0, 8), (1, 64, 8, 0), (-1, 64, 8, 8), (1, 64, -8, 8)):
        assert L.fs_lpips_scratch_bytes(*bad) == 0 and L.fs_lpips_saved_bytes(*bad) == 0, bad
    p = ctypes.c_void_p(0x1000)        # never dereferenced: every call below fails its argument check
    for i in (0, 1, 2, 7, 8, 9):       # f0, f1, w, dist, saved, scratch
        args = [p, p, p, 1, 64, 8, 8, p, p, p, None]
        args[i] = None
        assert L.fs_lpips_layer_forward(*args) == -1, i
    assert L.fs_lpips_layer_forward(p, p, p, 1, 64, 0, 8, p, p, p, None) == -1
    assert L.fs_lpips_layer_forward(p, p, p, 1, 513, 8, 8, p, p, p, None) == -3      # FS_ERR_UNSUPPORTED: C > 512
    for i in (0, 1, 2, 3, 4):
        args = [p, p, p, p, p, 1, 64, 8, 8, p, p, None]
        args[i] = None
        assert L.fs_lpips_layer_backward(*args) == -1, i
    assert L.fs_lpips_layer_backward(p, p, p, p, p, 1, 64, 8, 8, None, None, None) == -1   # no gradient asked for
    assert L.fs_lpips_layer_backward(p, p, p, p, p, 0, 64, 8, 8, p, None, None) == -1
    for i in (0, 1, 2, 3, 9):
        args = [p, p, p, p, 1, 3, 8, 8, 0, p, None]
        args[i] = None
        assert L.fs_lpips_prepare_forward(*args) == -1, i
    assert L.fs_lpips_prepare_backward(p, p, 1, 3, 8, 8, 0, None, None, None) == -1
    assert L.fs_lpips_prepare_backward(None, p, 1, 3, 8, 8, 0, p, p, None) == -1
    assert L.fs_lpips_prepare_backward(p, p, 1, 3, 0, 8, 0, p, p, None) == -1


def _package_layout(state):
    """the `lpips` package's own state dict: canonical keys + the `lins` aliases + the scaling layer's buffers"""
    out = dict(state)
    for k in range(5):
        out[f"lins.{k}.model.1.weight"] = state[f"lin{k}.model.1.weight"].clone()
    out["scaling_layer.shift"] = torch.tensor([-0.030, -0.088, -0.188])[None, :, None, None]
    out["scaling_layer.scale"] = torch.tensor([0.458, 0.448, 0.450])[None, :, None, None]
    return out


def _torchvision_layout(state):
    """torchvision's VGG-16 state dict (features.N.*, classifier.*) and the linear-layer file, as two dicts"""
    vgg, lins = {}, {}
    for key, v in state.items():
        if key.startswith("net."):
            _, _, idx, leaf = key.split(".")
            vgg[f"features.{idx}.{leaf}"] = v
        else:
            lins[key] = v
    vgg["classifier.0.weight"] = torch.zeros(4, 4)
    vgg["classifier.0.bias"] = torch.zeros(4)
    return vgg, lins


def test_both_key_layouts_load_into_the_same_state(tmp_path):
    from freesplat_amd import lpips as L
    state = L.random_state(seed=3)
    assert len(state) == 2 * 13 + 5
    a = L.LPIPS(weights=_package_layout(state))
    vgg, lins = _torchvision_layout(state)
    b = L.LPIPS(weights=[vgg, lins])
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(lins, tmp_path / "lins.pth")
    c = L.LPIPS(net="vgg", weights=[str(tmp_path / "vgg16.pth"), tmp_path / "lins.pth"])
    r = L.LPIPS(weights="random", seed=3)
    sa = a.state_dict()
    assert set(state) <= set(sa) and {"scaling_layer.shift", "scaling_layer.scale"} <= set(sa)
    for m in (b, c, r):
        sm = m.state_dict()
        assert sorted(sm) == sorted(sa)
        for k in sa:
            assert torch.equal(sa[k], sm[k]), k
    for k, v in state.items():
        assert torch.equal(sa[k], v), k
    assert not list(a.parameters()), "everything in LPIPS is a buffer"
    assert not a.training
    assert [w.numel() for w in a.lin_weights()] == [64, 128, 256, 512, 512]
    assert torch.allclose(a.scaling_layer.shift.flatten(), torch.tensor(L.SHIFT))


def test_env_var_names_the_weights(tmp_path, monkeypatch):
    from freesplat_amd import lpips as L
    state = L.random_state(seed=1)
    vgg, lins = _torchvision_layout(state)
    torch.save(vgg, tmp_path / "v.pth")
    torch.save(lins, tmp_path / "l.pth")
    monkeypatch.setenv(L.ENV_WEIGHTS, os.pathsep.join([str(tmp_path / "v.pth"), str(tmp_path / "l.pth")]))
    m = L.LPIPS()
    assert torch.equal(m.state_dict()["net.slice3.12.weight"], state["net.slice3.12.weight"])
    monkeypatch.setenv(L.ENV_WEIGHTS, str(tmp_path / "absent.pth"))
    with pytest.raises(FileNotFoundError, match="never fetched"):
        L.LPIPS()


def test_missing_and_misspelt_keys_are_named():
    from freesplat_amd import lpips as L
    state = L.random_state(seed=0)
    short = dict(state)
    del short["net.slice4.19.bias"]
    with pytest.raises(KeyError, match=r"missing \['net\.slice4\.19\.bias'\]"):
        L.LPIPS(weights=short)
    typo = dict(state)
    typo["lin2.model.0.weight"] = typo.pop("lin2.model.1.weight")
    with pytest.raises(KeyError) as e:
        L.LPIPS(weights=typo)
    msg = str(e.value)
    assert "lin2.model.1.weight" in msg and "lin2.model.0.weight" in msg and "keys found" in msg
    vgg, lins = _torchvision_layout(state)
    with pytest.raises(KeyError, match="lin0.model.1.weight"):
        L.LPIPS(weights=vgg)                      # the convolutions without the linear layers
    vgg["features.30.weight"] = torch.zeros(1)
    with pytest.raises(KeyError, match="features.30.weight"):
        L.LPIPS(weights=[vgg, lins])
    bad = dict(state)
    bad["lin0.model.1.weight"] = torch.zeros(1, 63, 1, 1)
    with pytest.raises(ValueError, match="lin0.model.1.weight has shape"):
        L.LPIPS(weights=bad)


def test_no_weights_is_an_error_that_says_where_they_go():
    from freesplat_amd import lpips as L
    with pytest.raises(ValueError) as e:
        L.LPIPS(net="vgg")
    assert L.ENV_WEIGHTS in str(e.value) and "never downloaded" in str(e.value)
    with pytest.raises(NotImplementedError):
        L.LPIPS(net="alex", weights="random")
    with pytest.raises(NotImplementedError):
        L.LPIPS(net="vgg", weights="random", spatial=True)
    src = open(os.path.join(ROOT, "freesplat_amd", "lpips.py")).read()
    for pat in (r"torch\.hub", r"https?://", r"urllib", r"download_url"):
        assert not re.search(pat, src), pat


def test_cpu_tensors_are_refused():
    from freesplat_amd import lpips as L
    m = L.LPIPS(weights="random")
    x = torch.rand(1, 3, 32, 32)
    with pytest.raises(ValueError, match="must be a tensor on a HIP device .* there is no CPU path"):
        m(x, x)
    L.set_default_weights("random")
    with pytest.raises(ValueError, match="there is no CPU path"):
        L.compute_lpips(x, x)
    with pytest.raises(ValueError, match="there is no CPU path"):
        L.lpips_head([torch.rand(1, 64, 4, 4)], [torch.rand(1, 64, 4, 4)], [torch.rand(64)])
    with pytest.raises(ValueError, match="there is no CPU path"):
        L.lpips_loss(x[None], x[None], 0.05, 0, 10)


def test_loss_before_apply_after_step_is_a_zero_and_touches_nothing(monkeypatch):
    from freesplat_amd import _lib, lpips as L

    def boom(*a, **k):
        raise AssertionError("the library must not be touched before apply_after_step")

    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(L, "get_lpips", boom)
    x = torch.rand(1, 2, 3, 32, 32)
    out = L.lpips_loss(x, x, 0.05, apply_after_step=100, global_step=99)
    assert out.dtype == torch.float32 and out.shape == () and float(out) == 0.0 and out.device == x.device


# ---- the opt-in binding on a fake reference tree (the technique of tests/test_metrics_host.py) ----

_FAKE = {
    "src/__init__.py": "",
    "src/loss/__init__.py": "",
    "src/loss/loss_lpips.py": "from lpips import LPIPS\n",
    "src/evaluation/__init__.py": "",
    "src/evaluation/metrics.py": "from lpips import LPIPS\ndef compute_psnr(a, b): return 'ref'\ndef compute_ssim(a, b): return 'ref'\n"
                                 "def get_lpips(d): return 'ref'\ndef compute_lpips(a, b): return 'ref'\n",
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
    # stands for an installed third-party package
    "lpips/__init__.py": "class LPIPS:\n    origin = 'installed'\n",
}
_LPIPS_NAMES = ["src.loss.loss_lpips.LPIPS", "src.evaluation.metrics.LPIPS", "src.evaluation.metrics.get_lpips",
                "src.evaluation.metrics.compute_lpips", "src.model.model_wrapper.compute_lpips",
                "src.evaluation.metric_computer.compute_lpips"]


@pytest.fixture
def fake_src(tmp_path, monkeypatch):
    for rel, txt in _FAKE.items():
        f = tmp_path / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(txt)
    is_ours = lambda k: k in ("src", "lpips") or k.startswith("src.")
    saved = {k: v for k, v in sys.modules.items() if is_ours(k)}
    for k in saved:
        del sys.modules[k]
    monkeypatch.syspath_prepend(str(tmp_path))
    yield tmp_path
    for k in [k for k in sys.modules if is_ours(k)]:
        del sys.modules[k]
    sys.modules.update(saved)


def _lookup(dotted):
    import importlib
    mod, name = dotted.rsplit(".", 1)
    return getattr(importlib.import_module(mod), name)


def test_default_and_metrics_leave_every_lpips_name_alone(fake_src):
    from freesplat_amd import compat
    compat.install()
    assert "lpips" not in sys.modules, "install() as called today must not register the shim"
    done = compat.patch_reference(decoder=False)
    assert not any(n in done for n in _LPIPS_NAMES) and "src.loss.loss_lpips" not in sys.modules
    done = compat.patch_reference(decoder=False, metrics=True)
    assert not any(n in done for n in _LPIPS_NAMES)
    assert _lookup("src.evaluation.metrics.compute_lpips")(0, 0) == "ref"
    assert _lookup("src.model.model_wrapper.compute_lpips")(0, 0) == "ref"
    assert _lookup("src.evaluation.metrics.get_lpips")(0) == "ref"
    assert _lookup("src.evaluation.metrics.LPIPS").origin == "installed"
    assert _lookup("src.loss.loss_lpips.LPIPS").origin == "installed"


def test_lpips_opt_in_rebinds_every_name(fake_src):
    from freesplat_amd import compat, lpips as L
    done = compat.patch_reference(decoder=False, lpips=True, lpips_weights="random")
    assert sorted(n for n in done if "lpips" in n.lower()) == sorted(_LPIPS_NAMES)
    for name in _LPIPS_NAMES:
        leaf = name.rsplit(".", 1)[1]
        assert _lookup(name) is getattr(L, leaf) and done[name] is getattr(L, leaf), name
    assert _lookup("src.evaluation.metrics.compute_psnr")(0, 0) == "ref"      # metrics=False: the others stay
    # what LossLpips.__init__ does: LPIPS(net="vgg"), from the weights patch_lpips() was given
    m = _lookup("src.loss.loss_lpips.LPIPS")(net="vgg")
    assert isinstance(m, L.LPIPS) and torch.equal(m.lin0.model[1].weight, L.random_state(0)["lin0.model.1.weight"])


def test_shim_is_registered_only_on_request(fake_src, monkeypatch):
    import importlib
    from freesplat_amd import compat, lpips as L
    compat.install()
    assert importlib.import_module("lpips").LPIPS.origin == "installed"
    compat.install(lpips=True)
    assert sys.modules["lpips"].LPIPS is L.LPIPS and importlib.import_module("lpips").LPIPS is L.LPIPS
    del sys.modules["lpips"]
    monkeypatch.setenv("FREESPLAT_LPIPS", "hip")
    compat.install()
    assert sys.modules["lpips"].LPIPS is L.LPIPS
    shim_dir = os.path.join(ROOT, "freesplat_amd", "compat")
    assert not os.path.exists(os.path.join(shim_dir, "lpips")), "a directory named lpips beside the rasterizer shim would " \
        "shadow an installed package for anyone with freesplat_amd/compat on PYTHONPATH"


def test_run_flag_asks_for_the_shim_and_the_binding(fake_src, monkeypatch):
    from freesplat_amd import compat, lpips as L
    from freesplat_amd.compat import run
    (fake_src / "lpips" / "__init__.py").unlink()          # a machine without the package
    (fake_src / "lpips").rmdir()
    seen = {}
    real = compat.patch_reference
    monkeypatch.setattr(compat, "patch_reference", lambda **k: seen.update(k) or real(decoder=False, **k))
    captured = {}
    monkeypatch.setattr(run.runpy, "run_module", lambda mod, **k: captured.update(argv=list(sys.argv), mod=mod))
    monkeypatch.setattr(sys, "argv", list(sys.argv))
    (fake_src / "fake_target.py").write_text("")
    done = run.main(["fake_target", "a=1", "--hip-lpips", "b=2"])
    assert seen == {"metrics": False, "lpips": True}
    assert captured == {"argv": ["fake_target", "a=1", "b=2"], "mod": "fake_target"}
    assert all(n in done for n in _LPIPS_NAMES)
    assert _lookup("src.loss.loss_lpips.LPIPS") is L.LPIPS
