"""Import-compatibility for an unmodified FreeSplat tree.

    import freesplat_amd.compat as compat
    compat.install()            # before `import src.main`: provides `diff_gaussian_rasterization_depth`
                                # (install(lpips=True) also provides `lpips`, for machines without that package)
    compat.patch_reference()    # after `src` is importable: swaps the hot-path classes for the HIP ones

or, as ONE command from the root of the FreeSplat checkout (freesplat_amd on PYTHONPATH):

    python -m freesplat_amd.compat.run src.main +experiment=scannet/2views ...     (freesplat_amd/compat/run.py)
"""
import importlib
import os
import sys


def install(lpips: bool = False) -> None:
    """Register `diff_gaussian_rasterization_depth` (the module name FreeSplat imports at
    src/model/decoder/cuda_splatting.py:5) as an alias of freesplat_amd.rasterizer.
    With lpips=True (or FREESPLAT_LPIPS=hip in the environment) also register `lpips` (loss_lpips.py:6, metrics.py:6) as
    freesplat_amd/compat/lpips_shim, in front of an installed package of that name; by default `lpips` is left alone."""
    from . import diff_gaussian_rasterization_depth as m
    sys.modules.setdefault("diff_gaussian_rasterization_depth", m)
    if lpips or os.environ.get("FREESPLAT_LPIPS", "") == "hip":
        from . import lpips_shim
        sys.modules["lpips"] = lpips_shim


METRIC_MODULES = ("src.evaluation.metrics", "src.model.model_wrapper", "src.evaluation.metric_computer")


def patch_metrics() -> dict:
    """Rebind the evaluation metrics inside the importable reference package `src` to the device ones
    (freesplat_amd/metrics.py): compute_psnr and compute_ssim in each module that imported them by name
    (src.evaluation.metrics, src.model.model_wrapper, src.evaluation.metric_computer), and
    src.model.model_wrapper.depth_render_metrics.  compute_lpips stays the reference's.
    Returns {dotted name: replacement} like patch_reference()."""
    from .. import metrics
    done = {}
    for modname in METRIC_MODULES:
        mod = importlib.import_module(modname)
        for n in ("compute_psnr", "compute_ssim"):
            setattr(mod, n, getattr(metrics, n))
            done[f"{modname}.{n}"] = getattr(metrics, n)
    mw = importlib.import_module("src.model.model_wrapper")
    mw.depth_render_metrics = metrics.depth_render_metrics
    done["src.model.model_wrapper.depth_render_metrics"] = metrics.depth_render_metrics
    return done


LPIPS_MODULES = ("src.evaluation.metrics", "src.model.model_wrapper", "src.evaluation.metric_computer")


def patch_lpips(weights=None) -> dict:
    """Rebind LPIPS inside the importable reference package `src` to freesplat_amd/lpips.py (the VGG-16 convolutions on
    torch, the distance head in HIP): src.loss.loss_lpips.LPIPS, src.evaluation.metrics.{LPIPS, get_lpips, compute_lpips} and
    the copies of compute_lpips that src.model.model_wrapper and src.evaluation.metric_computer imported by name.
    `weights` (a path, a state dict or a list of those) becomes what LPIPS(net="vgg") loads; None keeps
    FREESPLAT_LPIPS_WEIGHTS.  Importing those modules needs an importable `lpips`: compat.install(lpips=True) provides one.
    Returns {dotted name: replacement} like patch_reference()."""
    from .. import lpips as L
    if weights is not None:
        L.set_default_weights(weights)
    done = {}
    loss = importlib.import_module("src.loss.loss_lpips")
    loss.LPIPS = L.LPIPS
    done["src.loss.loss_lpips.LPIPS"] = L.LPIPS
    ev = importlib.import_module("src.evaluation.metrics")
    ev.LPIPS = L.LPIPS
    ev.get_lpips = L.get_lpips
    done["src.evaluation.metrics.LPIPS"] = L.LPIPS
    done["src.evaluation.metrics.get_lpips"] = L.get_lpips
    for modname in LPIPS_MODULES:
        importlib.import_module(modname).compute_lpips = L.compute_lpips
        done[f"{modname}.compute_lpips"] = L.compute_lpips
    return done


def patch_reference(decoder: bool = True, metrics: bool = False, lpips: bool = False, lpips_weights=None) -> dict:
    """Rebind, inside the already importable reference package `src`, every name on the hot path to its
    MI355X implementation (same constructor / call signatures and state-dict keys, so configs and
    checkpoints are untouched):
      src.model.encoder.modules.cost_volume.AVGFeatureVolumeManager   (cost_volume.py:384)
      src.model.encoder.encoder_freesplat.{AVGFeatureVolumeManager, GaussianAdapter, GRU}
      src.model.encoder.encoder_freesplat.EncoderFreeSplat.fuse_gaussians       (:431)
      src.model.encoder.encoder_freesplat.EncoderFreeSplat.forward              (:190-429; encoder_forward.py: the
                                                                                 reference's sub-modules in the reference's
                                                                                 order, the repeat + gather glue of :216-288
                                                                                 replaced by direct indexing)
      src.model.encoder.modules.networks.DepthDecoder.forward                   (networks.py:108-154)
      src.model.decoder.DECODERS["splatting_cuda"]                              (decoder/__init__.py:5-13)
    and with metrics=True also the evaluation metrics (patch_metrics()); without it the evaluation modules are not
    imported.  metrics=True leaves compute_lpips alone; lpips=True rebinds LPIPS (patch_lpips(lpips_weights)).
    Returns {dotted name: replacement} for logging."""
    from .. import cost_volume, depth_tail, encoder_forward, gaussian_adapter, ptf
    from ..decoder import DecoderSplattingCUDA
    done = {}
    cvm = importlib.import_module("src.model.encoder.modules.cost_volume")
    cvm.AVGFeatureVolumeManager = cost_volume.AVGFeatureVolumeManager
    done["src.model.encoder.modules.cost_volume.AVGFeatureVolumeManager"] = cost_volume.AVGFeatureVolumeManager
    enc = importlib.import_module("src.model.encoder.encoder_freesplat")
    enc.AVGFeatureVolumeManager = cost_volume.AVGFeatureVolumeManager
    enc.GaussianAdapter = gaussian_adapter.GaussianAdapter
    enc.GRU = ptf.GRU
    enc.EncoderFreeSplat.fuse_gaussians = ptf.fuse_gaussians
    enc.EncoderFreeSplat.forward = encoder_forward.encoder_forward
    done["src.model.encoder.encoder_freesplat.EncoderFreeSplat.forward"] = encoder_forward.encoder_forward
    for n in ("AVGFeatureVolumeManager", "GaussianAdapter", "GRU"):
        done[f"src.model.encoder.encoder_freesplat.{n}"] = getattr(enc, n)
    done["src.model.encoder.encoder_freesplat.EncoderFreeSplat.fuse_gaussians"] = ptf.fuse_gaussians
    net = importlib.import_module("src.model.encoder.modules.networks")
    net.DepthDecoder.forward = depth_tail.depth_decoder_forward
    done["src.model.encoder.modules.networks.DepthDecoder.forward"] = depth_tail.depth_decoder_forward
    if decoder:
        # same constructor (cfg, dataset_cfg) as the class it replaces, so get_decoder() is untouched.  A failure to
        # import the reference's decoder package is an error of the caller's environment and propagates.
        dec = importlib.import_module("src.model.decoder")
        dec.DECODERS["splatting_cuda"] = DecoderSplattingCUDA
        dec.DecoderSplattingCUDA = DecoderSplattingCUDA
        done['src.model.decoder.DECODERS["splatting_cuda"]'] = DecoderSplattingCUDA
    if metrics:
        done.update(patch_metrics())
    if lpips:
        done.update(patch_lpips(lpips_weights))
    return done
