"""CPU checks of the drop-in boundary: libfreesplat_hip.so loads without a GPU, and every header under include/ agrees with
its record in _lib.HEADERS and with the built library (no compute calls here)."""
import ctypes
import itertools
import os
import re

import pytest

from freesplat_amd import _lib
from util_abi import INCLUDE, declared_names, header_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bare_library():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_the_registry_names_every_header_once_with_the_known_sizes_and_revisions():
    files = [h.file for h in _lib.HEADERS]
    assert sorted(files) == sorted(f for f in os.listdir(INCLUDE) if f.startswith("freesplat_amd") and f.endswith(".h"))
    assert len(set(files)) == len(files) == 11
    assert [len(h.signatures) for h in _lib.HEADERS] == [93, 5, 3, 6, 5, 6, 5, 6, 5, 4, 6]
    assert tuple(h.revision for h in _lib.HEADERS) == (9, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1)
    pairs = list(itertools.combinations(_lib.HEADERS, 2))
    assert len(pairs) == 55
    for a, b in pairs:
        assert not set(a.signatures) & set(b.signatures), (a.file, b.file)
    # the module attributes that tests, benchmarks and the integration notes read are the registry's own objects
    tables = ("SIGNATURES", "LOSS_SIGNATURES", "OPTIM_SIGNATURES", "DENSITY_SIGNATURES", "DEPTHLOSS_SIGNATURES", "NORMALS_SIGNATURES",
              "EXPOSURE_SIGNATURES", "MVDEPTH_SIGNATURES", "TRANSFORM_SIGNATURES", "POSE_SIGNATURES", "TSDF_SIGNATURES")
    versions = ("ABI_VERSION", "LOSS_API_VERSION", "OPTIM_API_VERSION", "DENSITY_API_VERSION", "DEPTHLOSS_API_VERSION",
                "NORMALS_API_VERSION", "EXPOSURE_API_VERSION", "MVDEPTH_API_VERSION", "TRANSFORM_API_VERSION", "POSE_API_VERSION",
                "TSDF_API_VERSION")
    for h, table, version in zip(_lib.HEADERS, tables, versions):
        assert h.signatures is getattr(_lib, table) and h.revision == getattr(_lib, version), h.file


@pytest.mark.parametrize("h", _lib.HEADERS, ids=lambda h: h.file)
def test_every_header_is_exported_bound_and_at_its_revision(h):
    """What each feature's host test asserts of its own header, for every header: the declared names are exported by the bare
    library and are exactly the table's; the header defines its revision macro, and the library answers that value through
    the bare handle and through the binding."""
    L = _bare_library()
    names = declared_names(h.file)
    assert names and h.version_fn in names
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/{h.file} but not exported"
    assert set(names) == set(h.signatures)
    assert re.search(rf"#define\s+{h.macro}\s+{h.revision}\b", header_text(h.file))
    assert getattr(L, h.version_fn)() == h.revision == getattr(_lib.lib(), h.version_fn)()


# lib()'s refusal of a library at another revision, as the binding worded it before the registry (here: the library is at
# `got`, the binding is made to expect one more)
MISMATCH = {
    "freesplat_amd.h": "{lib} has ABI revision 9, this binding expects 10 (include/freesplat_amd.h FS_ABI_VERSION): rebuild the library",
    "freesplat_amd_loss.h": "{lib} has loss API revision 1, this binding expects 2 (include/freesplat_amd_loss.h FS_LOSS_API_VERSION): rebuild the library",
    "freesplat_amd_optim.h": "{lib} has optimizer API revision 1, this binding expects 2 (include/freesplat_amd_optim.h FS_OPTIM_API_VERSION): rebuild the library",
    "freesplat_amd_density.h": "{lib} has density API revision 1, this binding expects 2 (include/freesplat_amd_density.h FS_DENSITY_API_VERSION): rebuild the library",
    "freesplat_amd_depthloss.h": "{lib} has depth-loss API revision 1, this binding expects 2 (include/freesplat_amd_depthloss.h FS_DEPTHLOSS_API_VERSION): rebuild the library",
    "freesplat_amd_normals.h": "{lib} has normals API revision 1, this binding expects 2 (include/freesplat_amd_normals.h FS_NORMALS_API_VERSION): rebuild the library",
    "freesplat_amd_exposure.h": "{lib} has exposure API revision 1, this binding expects 2 (include/freesplat_amd_exposure.h FS_EXPOSURE_API_VERSION): rebuild the library",
    "freesplat_amd_mvdepth.h": "{lib} has multi-view depth API revision 1, this binding expects 2 (include/freesplat_amd_mvdepth.h FS_MVDEPTH_API_VERSION): rebuild the library",
    "freesplat_amd_transform.h": "{lib} has transform API revision 1, this binding expects 2 (include/freesplat_amd_transform.h FS_TRANSFORM_API_VERSION): rebuild the library",
    "freesplat_amd_pose.h": "{lib} has pose API revision 1, this binding expects 2 (include/freesplat_amd_pose.h FS_POSE_API_VERSION): rebuild the library",
    "freesplat_amd_tsdf.h": "{lib} has TSDF API revision 1, this binding expects 2 (include/freesplat_amd_tsdf.h FS_TSDF_API_VERSION): rebuild the library",
}


@pytest.mark.parametrize("i", range(11), ids=lambda i: _lib.HEADERS[i].file)
def test_a_library_at_another_revision_is_refused_and_not_cached(i, monkeypatch):
    _bare_library()
    h = _lib.HEADERS[i]
    monkeypatch.setattr(_lib, "HEADERS", _lib.HEADERS[:i] + (h._replace(revision=h.revision + 1),) + _lib.HEADERS[i + 1:])
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.FreeSplatHipError) as e:
        _lib.lib()
    assert str(e.value) == MISMATCH[h.file].format(lib=_lib.LIB_PATH)
    assert _lib._lib is None


def test_header_symbols_exported_and_bound():
    L = _bare_library()
    names = declared_names("freesplat_amd.h")
    assert "fs_raster_forward" in names and "fs_raster_backward" in names
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/freesplat_amd.h but not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature in freesplat_amd/_lib.py"
    assert set(_lib.SIGNATURES) <= set(names)
    assert _lib.lib().fs_version().decode().endswith("gfx950")


def test_buffer_sizes_and_arg_validation():
    from freesplat_amd import _lib
    L = _lib.lib()
    out = (ctypes.c_size_t * 4)()
    assert L.fs_raster_buffer_sizes(1_000_000, 968, 1296, 8_000_000, out) == 0
    geom, binning, image, scratch = list(out)
    assert geom >= 1_000_000 * (48 + 8 + 1)
    assert binning >= 8_000_000 * 4 + (81 * 61 + 1) * 4
    assert image >= 968 * 1296 * 8
    assert scratch >= 8_000_000 * 8
    assert L.fs_raster_buffer_sizes(-1, 10, 10, 10, out) == -1
    assert L.fs_raster_buffer_sizes(10, 0, 10, 10, out) == -1
    # NULL dims -> FS_ERR_INVALID_ARG before anything touches a device
    args = [None] * 16 + [1] + [None] * 6
    assert L.fs_raster_forward(*args) == -1


def test_product_has_no_oracle_dependency():
    """The product package must never import/execute anything under oracle/."""
    pkg = os.path.join(ROOT, "freesplat_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")) or f == "Makefile":
                txt = open(os.path.join(dirpath, f), errors="replace").read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), f
                assert "raster_oracle" not in txt and "oracle/" not in txt, f


def test_key_area_sizing_and_retry_capacity():
    """Host logic of the single-pass binning (no GPU): fs_raster_buffer_sizes sizes the scratch as one fixed key area per
    tile -- tile_capacity(cap, T) = the power of two >= max(2048, 4 cap / T), bounded so that T * tile_capacity indexes
    in 32 bits -- and rasterizer.retry_capacity(instances, largest tile list, H, W) returns a capacity whose key areas
    hold that list and whose saved lists hold the instances."""
    import ctypes as C
    import random
    from freesplat_amd import _lib, rasterizer as R

    def tile_capacity(cap, T):
        want = (4 * max(cap, 1) + T - 1) // T
        c = 2048
        while c < want and c < (1 << 26):
            c <<= 1
        while c > 1 and c * T > 0xFFFFFFFF:
            c >>= 1
        return c

    L = _lib.lib()
    al = lambda x: (x + 255) // 256 * 256
    rng = random.Random(3)
    for _ in range(200):
        H, W = rng.randint(1, 3000), rng.randint(1, 3000)
        N = rng.randint(0, 2_000_000)
        cap = rng.choice([1, 64, 5000, 1 << 20, 8 * max(N, 1), rng.randint(1, 1 << 28)])
        T = ((W + 15) // 16) * ((H + 15) // 16)
        out = (C.c_size_t * 4)()
        assert L.fs_raster_buffer_sizes(N, H, W, cap, out) == 0
        tc = tile_capacity(cap, T)
        assert out[3] == al(T * 4) + al(T * tc * 8), (H, W, cap)
        assert out[1] == al((T + 1) * 4) + al(max(cap, 1) * 4)
        n_inst, max_tile = rng.randint(1, 1 << 24), rng.randint(1, 1 << 16)
        cap2 = R.retry_capacity(n_inst, max_tile, H, W)
        assert cap2 >= n_inst and (tile_capacity(cap2, T) >= max_tile or tile_capacity(cap2, T) * T * 2 > 0xFFFFFFFF)
    assert L.fs_abi_version() == _lib.ABI_VERSION


CV_FORWARDS = ("fs_cost_volume_forward", "fs_cost_volume_forward_layout", "fs_cost_volume_forward_train")
CV_BACKWARDS = ("fs_cost_volume_backward", "fs_cost_volume_backward_train", "fs_cost_volume_backward_det")


def _cv_call(name, B=1, K=1, C=48, h=8, w=8, D=8, strides=(0, 1, 0), null=None, saved=True, layout=0, det_scratch=True):
    """One cost-volume entry point with fake non-NULL pointers; `null`: index of the required pointer to pass as NULL (forwards:
    6 maps / cameras / planes, 6 MLP tensors, workspace, out; backwards: the same 6, 5 MLP tensors, grad_out, workspace, 8 gradients).
    EVERY call of this helper must carry a defect the library refuses before it launches anything."""
    import ctypes as C_
    from freesplat_amd import _lib
    p = C_.c_void_p(4096)
    opt = lambda present: p if present else None
    ptrs = [p] * (14 if name in CV_FORWARDS else 21)
    if null is not None:
        ptrs[null] = None
    args = [B, K, C, h, w, D] + ptrs[:6] + list(strides)
    if name in CV_FORWARDS:
        args += ptrs[6:] + {"fs_cost_volume_forward": [], "fs_cost_volume_forward_layout": [layout],
                            "fs_cost_volume_forward_train": [opt(saved)]}[name]
    else:
        args += ptrs[6:13] + ([] if name == "fs_cost_volume_backward" else [opt(saved)]) + ptrs[13:]
        args += [opt(det_scratch)] if name == "fs_cost_volume_backward_det" else []
    return getattr(_lib.lib(), name)(*args, None)


def _cv_status_codes(name):
    """Every FS_ERR_INVALID_ARG (-1) condition (a non-positive size, a NULL required pointer, a layout outside 0..3) is answered
    before any FS_ERR_UNSUPPORTED (-3) one (a matching dimension other than 48 / 16, a map of 4 GB or more, K > 16 or per-pixel
    planes for the deterministic backward)."""
    for bad in (dict(h=0), dict(B=0), dict(D=0)):
        assert _cv_call(name, **bad) == -1, bad
    for C in (48, 32):
        for i in range(14 if name in CV_FORWARDS else 21):
            assert _cv_call(name, C=C, null=i) == -1, (C, i)
    assert _cv_call(name, C=32) == -3
    assert _cv_call(name, h=4096, w=4096) == -3
    if name == "fs_cost_volume_forward_layout":
        for C in (48, 32):
            assert _cv_call(name, C=C, layout=4) == -1 and _cv_call(name, C=C, layout=-1) == -1
    if name in ("fs_cost_volume_forward_train", "fs_cost_volume_backward_train"):
        assert _cv_call(name, saved=False) == -1 and _cv_call(name, C=32, saved=False) == -1
    if name == "fs_cost_volume_backward_det":
        assert _cv_call(name, C=32, saved=False) == -3              # (`saved` is optional there)
        for C in (48, 32):
            assert _cv_call(name, C=C, det_scratch=False) == -1
            assert _cv_call(name, C=C, K=17) == -3
            assert _cv_call(name, C=C, strides=(512, 64, 1)) == -3
        assert _cv_call(name, K=17, det_scratch=False) == -1 and _cv_call(name, K=17, null=0) == -1


def test_cost_volume_rejects_maps_of_4GB_and_more(monkeypatch):
    """The sweeps address a tap as map base + 32-bit byte offset: a feature map of >= 4 GB is refused (FS_ERR_UNSUPPORTED, -3)
    before anything is launched -- so fake non-NULL pointers are enough here, no device involved.  All six entry points answer
    the same arguments alike (_cv_status_codes), and the backward's size queries follow the form that will run: the
    deterministic scratch is 0 for what that form refuses, the per-call workspace equals the upper bound for the two-pass form
    and leaves out the record / inverse-homography regions for per-pixel planes."""
    import ctypes as C
    from freesplat_amd import _lib
    L = _lib.lib()
    p = C.c_void_p(4096)
    h, w = 4096, 4096                      # 16.8 M texels x (48 + 32) floats x 4 B = 5.4 GB
    fwd = [1, 1, 48, h, w, 8] + [p] * 6 + [0, 0, 1] + [p] * 9
    assert L.fs_cost_volume_forward(*fwd) == -3
    bwd = [1, 1, 48, h, w, 8] + [p] * 6 + [0, 0, 1] + [p] * 16
    assert L.fs_cost_volume_backward(*bwd) == -3
    fwd[2] = 32                            # unsupported matching dimension
    assert L.fs_cost_volume_forward(*fwd) == -3
    fwd[2], fwd[3] = 48, 0
    assert L.fs_cost_volume_forward(*fwd) == -1
    for name in CV_FORWARDS + CV_BACKWARDS:
        _cv_status_codes(name)
    monkeypatch.delenv("FS_CV_BWD_ATOMIC", raising=False)
    assert L.fs_cost_volume_backward_det_bytes(1, 17, 48, 8, 8, 8) == 0 and L.fs_cost_volume_backward_det_bytes(1, 1, 32, 8, 8, 8) == 0
    assert L.fs_cost_volume_backward_workspace_bytes(2, 2, 48, 8, 8, 8) == 353792
    assert L.fs_cost_volume_backward_workspace_bytes_for(2, 2, 48, 8, 8, 8, 0) == 353792
    assert L.fs_cost_volume_backward_workspace_bytes_for(2, 2, 48, 8, 8, 8, 1) == 147712


# (entry point, {argument index: value}, pointer arguments set to NULL, expected status).  Every other int32 argument is 1, every
# other pointer a non-NULL dummy, the two `float* const*` arguments (A6) a host array of six dummies; A5 is such an array with
# its last entry NULL.  The third column is a tuple of argument indices, each NULLed IN TURN (one call per index), "all"
# (every pointer not named in the second column, at once) or None (one call).  Only combinations that return before the first
# launch are listed: a dummy pointer is never dereferenced.
A5, A6 = "five dummies + NULL", "six dummies"
PTF_STATUS_TABLE = [
    # M, h, w, xyz, w2c, kpix, depth_i, thres, scratch, keep, fuse, fpix, app, counts
    ("fs_ptf_match", {0: -1}, None, -1), ("fs_ptf_match", {1: 0}, None, -1), ("fs_ptf_match", {1: -1}, None, -1),
    ("fs_ptf_match", {2: 0}, None, -1), ("fs_ptf_match", {2: -1}, None, -1),
    ("fs_ptf_match", {}, (3, 4, 5, 6, 8, 9, 10, 11, 12, 13), -1),
    ("fs_ptf_match", {0: 0}, (4, 5, 6, 8, 12, 13), -1),              # (no state rows: xyz and the three state lists may be NULL)
    # n_fuse, fuse_idx, fuse_pix, G, R, O, g_i, rho_i, om_i, cat
    ("fs_ptf_gru_inputs", {0: -1}, None, -1), ("fs_ptf_gru_inputs", {0: 0}, None, 0), ("fs_ptf_gru_inputs", {0: 0}, "all", 0),
    ("fs_ptf_gru_inputs", {}, tuple(range(1, 10)), -1),
    # n_keep, n_fuse, n_app, keep, fuse, fpix, app, G X R O E D (7-12), g_i x_i rho_i om_i d_i E_i (13-18), fused, out (20-25)
    ("fs_ptf_write_state", {0: -1}, None, -1), ("fs_ptf_write_state", {1: -1}, None, -1), ("fs_ptf_write_state", {2: -1}, None, -1),
    ("fs_ptf_write_state", {0: 0, 1: 0, 2: 0}, None, 0), ("fs_ptf_write_state", {0: 0, 1: 0, 2: 0}, "all", 0),
    ("fs_ptf_write_state", {}, (4, 5) + tuple(range(7, 26)), -1),
    ("fs_ptf_write_state", {0: 0, 1: 0}, tuple(range(13, 19)) + tuple(range(20, 26)), -1),
    ("fs_ptf_write_state", {1: 0, 2: 0}, tuple(range(7, 13)), -1), ("fs_ptf_write_state", {0: 0, 2: 0}, tuple(range(7, 13)), -1),
    # M_max, M_dev, h, w, state (4-9), view (10-15), w2c, kpix, thres, tables, scratch, out (21-26), counts[, side, act, cat]
    ("fs_ptf_fold_step", {0: 0}, None, -1), ("fs_ptf_fold_step", {0: -1}, None, -1), ("fs_ptf_fold_step", {2: 0}, None, -1),
    ("fs_ptf_fold_step", {2: -1}, None, -1), ("fs_ptf_fold_step", {3: 0}, None, -1), ("fs_ptf_fold_step", {3: -1}, None, -1),
    ("fs_ptf_fold_step", {}, tuple(range(4, 18)) + tuple(range(19, 28)), -1),
    ("fs_ptf_fold_step_save", {0: 0}, None, -1), ("fs_ptf_fold_step_save", {0: -1}, None, -1), ("fs_ptf_fold_step_save", {2: 0}, None, -1),
    ("fs_ptf_fold_step_save", {2: -1}, None, -1), ("fs_ptf_fold_step_save", {3: 0}, None, -1), ("fs_ptf_fold_step_save", {3: -1}, None, -1),
    ("fs_ptf_fold_step_save", {}, tuple(range(4, 18)) + tuple(range(19, 31)), -1),
    ("fs_ptf_fold_step_save", {0: 0}, (28, 29, 30), -1),
    # V, h, w, lat, xs, rho, om, dep, Es, w2c (optional), Kn, thres, tables, scratch, bufA, bufB, counts
    ("fs_ptf_fold", {0: 1}, None, -1), ("fs_ptf_fold", {0: 0}, None, -1), ("fs_ptf_fold", {0: -1}, None, -1),
    ("fs_ptf_fold", {0: 2, 1: 0}, None, -1), ("fs_ptf_fold", {0: 2, 1: -1}, None, -1), ("fs_ptf_fold", {0: 2, 2: 0}, None, -1),
    ("fs_ptf_fold", {0: 2, 2: -1}, None, -1), ("fs_ptf_fold", {0: 2}, (3, 4, 5, 6, 7, 8, 10, 12, 13, 14, 15, 16), -1),
    ("fs_ptf_fold", {0: 1, 14: A5, 15: A5}, None, -1), ("fs_ptf_fold", {0: 2, 14: A5}, (3, 15), -1),
    # V, h, w, Es, Kn, kpix, E0
    ("fs_ptf_cameras", {0: 0}, None, -1), ("fs_ptf_cameras", {0: -1}, None, -1), ("fs_ptf_cameras", {1: 0}, None, -1),
    ("fs_ptf_cameras", {1: -1}, None, -1), ("fs_ptf_cameras", {2: 0}, None, -1), ("fs_ptf_cameras", {2: -1}, None, -1),
    ("fs_ptf_cameras", {}, (3, 4, 5, 6), -1),
    # M_max, h, w, scratch, lists: pointer arithmetic only, never a launch
    ("fs_ptf_fold_step_lists", {}, None, 0), ("fs_ptf_fold_step_lists", {0: 0}, None, -1), ("fs_ptf_fold_step_lists", {0: -1}, None, -1),
    ("fs_ptf_fold_step_lists", {1: 0}, None, -1), ("fs_ptf_fold_step_lists", {1: -1}, None, -1), ("fs_ptf_fold_step_lists", {2: 0}, None, -1),
    ("fs_ptf_fold_step_lists", {2: -1}, None, -1), ("fs_ptf_fold_step_lists", {}, (3, 4), -1),
]
# n_keep, n_fuse, n_app, keep, fuse, fpix, app, X R E D (7-10), x_i rho_i d_i E_i (11-14), g_out, g_in, g_lat_i .. g_d_i (17-21)
# [, P, scratch]: both forms answer these alike
for _name in ("fs_ptf_write_state_backward", "fs_ptf_write_state_backward_det"):
    PTF_STATUS_TABLE += [
        (_name, {0: -1}, None, -1), (_name, {1: -1}, None, -1), (_name, {2: -1}, None, -1), (_name, {}, (15, 16), -1),
        (_name, {0: 0, 1: 0, 2: 0}, (15, 16), -1),                       # (the two arrays are required even of an empty job)
        (_name, {0: 0, 1: 0, 2: 0}, None, 0), (_name, {0: 0, 1: 0, 2: 0, 15: A6, 16: A6}, "all", 0),
        (_name, {0: 0, 1: 0, 2: 0, 15: A5, 16: A5}, None, 0),
        (_name, {}, tuple(range(7, 15)) + tuple(range(17, 22)), -1),
        (_name, {0: 0, 1: 0}, tuple(range(11, 15)) + tuple(range(17, 22)), -1),
        (_name, {1: 0, 2: 0}, (7, 8, 9, 10), -1), (_name, {0: 0, 2: 0}, (7, 8, 9, 10), -1),
        (_name, {16: A5}, None, -1), (_name, {1: 0, 2: 0, 16: A5}, None, -1), (_name, {0: 0, 2: 0, 16: A5}, None, -1),
        (_name, {15: A5}, (11, 17), -1),                                 # (entries of g_out may be NULL; something else is wrong here)
    ]
# n_fuse, fuse_idx, fuse_pix, R, O, rho_i, om_i, dcat, g_G, g_R, g_O, g_lat_i, g_rho_i, g_om_i[, P, scratch]
for _name in ("fs_ptf_gru_inputs_backward", "fs_ptf_gru_inputs_backward_det"):
    PTF_STATUS_TABLE += [(_name, {0: -1}, None, -1), (_name, {0: 0}, None, 0), (_name, {0: 0}, "all", 0),
                         (_name, {}, tuple(range(1, 14)), -1)]
# the deterministic forms' own arguments: P (22 / 14) negative is refused before the empty job is answered, P = 0 and a NULL
# scratch (23 / 15) only where there are fused rows
PTF_STATUS_TABLE += [
    ("fs_ptf_write_state_backward_det", {0: 0, 1: 0, 2: 0, 22: -1}, None, -1), ("fs_ptf_write_state_backward_det", {22: -1}, None, -1),
    ("fs_ptf_write_state_backward_det", {1: 0, 22: -1}, None, -1),
    ("fs_ptf_write_state_backward_det", {0: 0, 1: 0, 2: 0, 22: 0}, None, 0), ("fs_ptf_write_state_backward_det", {22: 0}, None, -1),
    ("fs_ptf_write_state_backward_det", {0: 0, 2: 0, 22: 0}, None, -1),
    ("fs_ptf_write_state_backward_det", {0: 0, 1: 0, 2: 0}, (23,), 0), ("fs_ptf_write_state_backward_det", {}, (4, 5, 23), -1),
    ("fs_ptf_write_state_backward_det", {0: 0, 2: 0}, (4, 5, 23), -1),
    ("fs_ptf_gru_inputs_backward_det", {0: 0, 14: -1}, None, -1), ("fs_ptf_gru_inputs_backward_det", {14: -1}, None, -1),
    ("fs_ptf_gru_inputs_backward_det", {0: 0, 14: 0}, None, 0), ("fs_ptf_gru_inputs_backward_det", {14: 0}, None, -1),
    ("fs_ptf_gru_inputs_backward_det", {0: 0}, (15,), 0), ("fs_ptf_gru_inputs_backward_det", {}, (15,), -1),
    ("fs_ptf_gru_inputs_backward_det", {0: 0, 14: 0}, (15,), 0), ("fs_ptf_gru_inputs_backward_det", {0: 0, 14: -1}, "all", -1),
]


def test_ptf_entry_points_answer_the_recorded_statuses():
    """The PTF fold's twelve int-returning entry points over PTF_STATUS_TABLE: sizes negative / zero / positive, each required
    pointer NULL in turn, the empty jobs, and for the deterministic backwards P of -1 / 0 and a NULL scratch with and without
    fused rows.  The table was recorded from the revision before the host layer got one backward driver per pair and holds
    for both; no row reaches a launch, so no device is involved."""
    import ctypes as C
    from freesplat_amd import _lib
    L = _lib.lib()
    dummy = 4096
    arrays = {A6: [dummy] * 6, A5: [dummy] * 5 + [None]}
    n_calls = 0
    for name, over, nulls, want in PTF_STATUS_TABLE:
        _, at = _lib.SIGNATURES[name]
        is_ptr = [a is C.c_void_p or a is C.POINTER(C.c_void_p) for a in at]
        base = [A6 if a is C.POINTER(C.c_void_p) else dummy if a is C.c_void_p else 0.1 if a is C.c_float else 1 for a in at]
        if at[-1] is C.c_void_p:
            base[-1] = None                                              # the stream
        for i, v in over.items():
            base[i] = v
        if nulls == "all":
            variants = [[None if (is_ptr[i] and i not in over) else v for i, v in enumerate(base)]]
        else:
            variants = [base] if nulls is None else [base[:i] + [None] + base[i + 1:] for i in nulls]
            assert all(is_ptr[i] for i in (nulls or ()))
        for args in variants:
            keep = [(C.c_void_p * 6)(*arrays[v]) if isinstance(v, str) else v for v in args]     # (alive over the call)
            assert getattr(L, name)(*keep) == want, (name, over, nulls, args)
            n_calls += 1
    assert n_calls == 331


# ---------------------------------------------------------------------------------------------------- rasterizer statuses
_R_IN = ["means3D", "cov3D", "shs", "colors_precomp", "opacities", "bg", "viewmatrix", "projmatrix", "campos", "tanfov", "scale",
         "geom", "binning", "image"]
_R_OUT = ["out_color", "out_depth", "out_alpha", "radii", "counters"]
_R_GRADS = ["grad_scratch", "dL_dmeans3D", "dL_dmeans2D", "dL_dcov3D", "dL_dshs", "dL_dcolors", "dL_dopacities", "accumulate"]
RASTER_ARGS = {"fs_raster_forward": ["dims"] + _R_IN + ["scratch", "cap"] + _R_OUT + ["stream"],
               "fs_raster_forward_views": ["dims", "v"] + _R_IN + ["scratch", "strides", "cap"] + _R_OUT + ["n_streams", "streams", "stream"]}
for _a in ("", "_alpha"):
    _cot = ["dL_dcolor", "dL_ddepth"] + (["dL_dalpha"] if _a else [])
    _views = ["dims", "v"] + _R_IN + ["counters", "strides"] + _cot + _R_GRADS + ["n_streams", "streams", "stream"]
    RASTER_ARGS["fs_raster_backward" + _a] = ["dims"] + _R_IN + ["counters"] + _cot + _R_GRADS + ["stream"]
    RASTER_ARGS["fs_raster_backward_views" + _a] = _views
    RASTER_ARGS["fs_raster_backward_views_rows" + _a] = _views + ["row0", "nrows", "with_blend"]
FWD = ("fs_raster_forward", "fs_raster_forward_views")
BWD = tuple(n for n in RASTER_ARGS if "backward" in n)
VIEWS = tuple(n for n in RASTER_ARGS if "views" in n)
ROWS = tuple(n for n in RASTER_ARGS if "rows" in n)
WHOLE = tuple(n for n in BWD if n not in ROWS)       # (the backwards without a row range)
ALL = FWD + BWD
# what a call is made of unless a row says otherwise: the SH form (colors_precomp / dL_dcolors NULL), 4 Gaussians, 9 coefficients of
# degree 2, 40 x 56 pixels, 2 views, no side streams, rows [0, 2); every pointer a dummy that is never dereferenced
RASTER_DIMS = dict(N=4, M=9, H=40, W=56, sh_degree=2, tanfovx=0.5, tanfovy=0.5, flags=0)
RASTER_BASE = dict(colors_precomp=None, dL_dcolors=None, stream=None, streams=None, cap=1 << 20, v=2, n_streams=0, accumulate=0,
                   row0=0, nrows=2, with_blend=1)
RASTER_OPTIONAL = {"dims", "tanfov", "scale", "dL_ddepth", "dL_dalpha", "colors_precomp", "dL_dcolors", "stream", "streams", "strides"}
NBS, DET, SR, CF = 32, 64, 128, 8       # FS_RASTER_NO_BACKWARD_STATE, _DETERMINISTIC, _SCALE_ROT, _COV_FULL
P_ = "dummy"
EACH, EVERY = "each required pointer NULL in turn", "every pointer but dims and strides NULL at once"
# (entry points, dims fields, arguments, NULLed pointers, expected status).  Recorded from the library of the revision before the
# host layer got its one argument check and one backward driver; rows that the recording answered with FS_ERR_LAUNCH (-2: they
# reach a HIP call, which fails without a device) are not listed.
RASTER_STATUS_TABLE = [
    (ALL, {}, dict(dims=None), None, -1), (ALL, dict(N=-1), {}, None, -1), (WHOLE, dict(N=0), {}, None, 0), (WHOLE, dict(N=0), {}, EVERY, 0),
    (BWD, dict(N=0, flags=NBS), {}, None, -1), (BWD, dict(N=0, flags=SR | CF), {}, None, -1), (BWD, dict(flags=NBS), {}, None, -1),
    (BWD, dict(flags=NBS | DET), {}, EVERY, -1), (ALL, dict(flags=SR | CF), {}, None, -1), (ALL, dict(flags=SR | CF | NBS), {}, EVERY, -1),
    (FWD, dict(H=0), {}, None, -1), (FWD, dict(H=-1), {}, None, -1), (FWD, dict(W=0), {}, None, -1), (FWD, dict(W=-5), {}, None, -1),
    (FWD, {}, dict(cap=0), None, -1), (FWD, {}, dict(cap=-1), None, -1),
    # the limits: 32767 tiles along a side, 2^28 Gaussians, 2^32 - 1 instances
    (FWD, dict(W=16 * 32767 + 1), {}, None, -3), (FWD, dict(H=16 * 32767 + 1), {}, None, -3), (FWD, dict(N=(1 << 28) + 1), {}, None, -3),
    (FWD, {}, dict(cap=1 << 32), None, -3), (FWD, dict(N=(1 << 28) + 1, H=0), {}, None, -1), (FWD, dict(W=16 * 32767 + 1), {}, EACH, -1),
    # sh_degree against M (forward), M * 3 > 48 (backward); an invalid argument is answered before an unsupported one
    (FWD, dict(sh_degree=3), {}, None, -3), (FWD, dict(sh_degree=4, M=25), {}, None, -3), (FWD, dict(sh_degree=-1), {}, None, -3),
    (FWD, dict(sh_degree=3), {}, EACH, -1), (BWD, dict(M=17), {}, None, -3), (BWD, dict(M=17), {}, EACH, -1),
    (BWD, dict(M=17, flags=NBS), {}, None, -1), (BWD, dict(M=17), dict(colors_precomp=P_), None, -1),
    # shs and colors_precomp both / neither (EACH NULLs shs), a missing dL_dshs (EACH) / dL_dcolors
    (ALL, {}, dict(colors_precomp=P_), None, -1), (BWD, {}, dict(colors_precomp=P_, dL_dcolors=P_), None, -1),
    (BWD, {}, dict(shs=None, colors_precomp=P_), None, -1), (BWD, {}, dict(shs=None, colors_precomp=P_, dL_dshs=None), None, -1),
    (ALL, {}, {}, EACH, -1), (ALL, {}, {}, EVERY, -1), (ALL, dict(flags=DET), {}, EACH, -1),
    # the views forms: v, the side streams, the strides
    (VIEWS, {}, dict(v=-1), None, -1), (VIEWS, {}, dict(v=0), None, 0), (VIEWS, {}, dict(v=0), EVERY, 0),
    (VIEWS, {}, dict(v=0, strides=None), None, -1), (VIEWS, {}, dict(v=0, dims=None), None, -1), (VIEWS, {}, dict(strides=None), None, -1),
    (VIEWS, dict(flags=NBS), dict(v=0), None, 0), (tuple(n for n in VIEWS if n not in ROWS), dict(N=-1), dict(v=0), None, 0), (ROWS, dict(N=-1), dict(v=0, nrows=0), None, -1),
    (("fs_raster_forward_views",), dict(flags=SR | CF), dict(v=0), None, 0),
    (tuple(n for n in VIEWS if n in BWD), dict(flags=SR | CF), dict(v=0), None, -1),
    (VIEWS, {}, dict(n_streams=-1), None, -1), (VIEWS, {}, dict(n_streams=9, streams=P_), None, -1),
    (VIEWS, {}, dict(n_streams=2), None, -1), (VIEWS, {}, dict(n_streams=1), None, -1), (VIEWS, {}, dict(v=0, n_streams=2), None, -1),
    (VIEWS, {}, dict(n_streams=8, streams=P_), EACH, -1),
    # the row range of the chunked per-Gaussian pass
    (ROWS, {}, dict(row0=-1), None, -1), (ROWS, {}, dict(nrows=-1), None, -1), (ROWS, {}, dict(row0=3, nrows=2), None, -1),
    (ROWS, {}, dict(row0=0, nrows=5), None, -1), (ROWS, {}, dict(row0=5, nrows=0), None, -1), (ROWS, {}, dict(v=0, row0=3, nrows=2), None, -1),
    (ROWS, dict(N=0), dict(nrows=0), None, 0), (ROWS, dict(N=0), dict(nrows=0), EVERY, 0), (ROWS, dict(N=0), dict(nrows=1), None, -1), (ROWS, {}, dict(with_blend=0), EACH, -1),
]
# fs_raster_buffer_sizes (N, H, W, cap) -> status, out[4]; fs_raster_backward_scratch_bytes (N, H, W, flags, v, n_streams, cap);
# fs_raster_scratch_slots (v, n_streams): recorded the same way
RASTER_SIZE_TABLE = [
    ((0, 1, 1, 0), 0, [768, 512, 512, 16640]), ((4, 40, 56, 100), 0, [768, 768, 17920, 196864]),
    ((320, 40, 56, 1048576), 0, [18432, 4194560, 17920, 50331904]), ((1000, 17, 33, 64), 0, [57344, 512, 4608, 98560]),
    ((1000000, 968, 1296, 8000000), 0, [57000192, 32019968, 10036224, 323833344]),
    ((257, 3000, 2999, 268435456), 0, [15360, 1073883392, 71976448, 9265359104]), ((-1, 40, 56, 100), -1, None),
    ((4, 0, 56, 100), -1, None), ((4, 40, -1, 100), -1, None), ((4, 40, 56, -1), -1, None),
]
RASTER_BWD_SCRATCH_TABLE = [
    ((0, 40, 56, 0, 0, 0, 100), 0), ((0, 40, 56, 0, 3, 0, 100), 0), ((0, 40, 56, 0, 3, 2, 100), 0),
    ((0, 40, 56, 0, 20, 9, 100), 0), ((0, 40, 56, 64, 0, 0, 100), 27648), ((0, 40, 56, 64, 3, 0, 100), 27648),
    ((0, 40, 56, 64, 3, 2, 100), 55296), ((0, 40, 56, 64, 20, 9, 100), 221184), ((320, 40, 56, 0, 0, 0, 0), 15360),
    ((320, 40, 56, 0, 0, 0, 100), 15360), ((320, 40, 56, 0, 0, 0, 1048576), 15360), ((320, 40, 56, 0, 3, 0, 0), 46080),
    ((320, 40, 56, 0, 3, 0, 100), 46080), ((320, 40, 56, 0, 3, 0, 1048576), 46080), ((320, 40, 56, 0, 3, 2, 0), 46080),
    ((320, 40, 56, 0, 3, 2, 100), 46080), ((320, 40, 56, 0, 3, 2, 1048576), 46080), ((320, 40, 56, 0, 20, 9, 0), 307200),
    ((320, 40, 56, 0, 20, 9, 100), 307200), ((320, 40, 56, 0, 20, 9, 1048576), 307200), ((320, 40, 56, 64, 0, 0, 0), 30720),
    ((320, 40, 56, 64, 0, 0, 100), 44288), ((320, 40, 56, 64, 0, 0, 1048576), 220742656), ((320, 40, 56, 64, 3, 0, 0), 61440),
    ((320, 40, 56, 64, 3, 0, 100), 75008), ((320, 40, 56, 64, 3, 0, 1048576), 220773376), ((320, 40, 56, 64, 3, 2, 0), 76800),
    ((320, 40, 56, 64, 3, 2, 100), 103936), ((320, 40, 56, 64, 3, 2, 1048576), 441500672),
    ((320, 40, 56, 64, 20, 9, 0), 430080), ((320, 40, 56, 64, 20, 9, 100), 538624),
    ((320, 40, 56, 64, 20, 9, 1048576), 1766125568), ((1000, 17, 33, 0, 0, 0, 100), 48000),
    ((1000, 17, 33, 0, 0, 0, 1048576), 48000), ((1000, 17, 33, 0, 3, 0, 100), 144384),
    ((1000, 17, 33, 0, 3, 0, 1048576), 144384), ((1000, 17, 33, 0, 3, 2, 100), 144384),
    ((1000, 17, 33, 0, 3, 2, 1048576), 144384), ((1000, 17, 33, 0, 20, 9, 100), 962560),
    ((1000, 17, 33, 0, 20, 9, 1048576), 962560), ((1000, 17, 33, 64, 0, 0, 100), 79616),
    ((1000, 17, 33, 64, 0, 0, 1048576), 220777984), ((1000, 17, 33, 64, 3, 0, 100), 175872),
    ((1000, 17, 33, 64, 3, 0, 1048576), 220874240), ((1000, 17, 33, 64, 3, 2, 100), 207360),
    ((1000, 17, 33, 64, 3, 2, 1048576), 441604096), ((1000, 17, 33, 64, 20, 9, 100), 1214464),
    ((1000, 17, 33, 64, 20, 9, 1048576), 1766801408), ((-1, 40, 56, 0, 1, 0, 100), 0), ((4, 0, 56, 0, 1, 0, 100), 0),
    ((4, 40, 0, 64, 1, 0, 100), 0), ((4, 40, 56, 64, -1, 0, 100), 0), ((4, 40, 56, 64, 1, 0, -1), 0),
    ((4, 40, 56, 64, 1, -1, 100), 27904),
]
RASTER_SLOTS_TABLE = [((-1, 0), -1), ((0, -1), -1), ((0, 0), 1), ((1, 0), 1), ((3, 2), 3), ((16, 0), 16), ((17, 8), 16), ((40, 2), 16)]


def _raster_variants(name, dims_over, over, nulls):
    """The argument lists of one RASTER_STATUS_TABLE row for one entry point (None: the row names an argument it lacks)."""
    import ctypes as C
    from freesplat_amd import _lib
    names = RASTER_ARGS[name]
    assert len(names) == len(_lib.SIGNATURES[name][1])
    if any(k not in names for k in over):
        return None
    dims = _lib.RasterDims(**dict(RASTER_DIMS, **dims_over))
    n_strides = 4 if "forward" in name else 3
    base = dict(dims=C.byref(dims), strides=(C.c_size_t * n_strides)(*[1 << 20] * n_strides))
    at = dict(zip(names, _lib.SIGNATURES[name][1]))
    pointers = [k for k in names if at[k] in (C.c_void_p, C.POINTER(C.c_void_p))]
    base.update({k: C.c_void_p(4096) for k in pointers})
    base["streams"] = (C.c_void_p * 8)(*[4096] * 8)
    base.update(RASTER_BASE)
    for k, v in over.items():
        base[k] = v if v != P_ else (C.c_void_p * 8)(*[4096] * 8) if k == "streams" else C.c_void_p(4096)
    required = [k for k in pointers if k not in RASTER_OPTIONAL and k not in over and not (k == "counters" and name in BWD)]
    if nulls == EACH:
        sets = [[k] for k in required]
    else:
        sets = [[k for k in pointers if k not in over and k != "stream"]] if nulls == EVERY else [[]]
    return [([None if k in drop else base[k] for k in names], (dims, base)) for drop in sets]


def test_rasterizer_entry_points_answer_the_recorded_statuses():
    """The rasterizer's eight int-returning entry points over RASTER_STATUS_TABLE (dims NULL, N negative / 0 / positive, the flag
    combinations, the image / capacity / tile-grid / Gaussian-count limits, sh_degree against M, the colour pair, each required
    pointer NULL in turn, v, the side streams, the row range) and its three size queries over a few argument tuples.  Recorded
    from the revision before the host layer got one argument check and one backward driver and holds for both; no row reaches
    a launch, so no device is involved."""
    import ctypes as C
    from freesplat_amd import _lib
    L = _lib.lib()
    n_calls = 0
    for names, dims_over, over, nulls, want in RASTER_STATUS_TABLE:
        for name in names:
            for args, _alive in _raster_variants(name, dims_over, over, nulls) or ():
                assert getattr(L, name)(*args) == want, (name, dims_over, over, nulls, [i for i, a in enumerate(args) if a is None])
                n_calls += 1
    assert n_calls == 817
    out = (C.c_size_t * 4)()
    for args, status, sizes in RASTER_SIZE_TABLE:
        assert L.fs_raster_buffer_sizes(*args, out) == status and (status != 0 or list(out) == sizes), args
    assert L.fs_raster_buffer_sizes(4, 40, 56, 100, None) == -1
    for (N, H, W, flags, v, ns, cap), want in RASTER_BWD_SCRATCH_TABLE:
        d = _lib.RasterDims(**dict(RASTER_DIMS, N=N, H=H, W=W, flags=flags))
        assert L.fs_raster_backward_scratch_bytes(C.byref(d), v, ns, cap) == want, (N, H, W, flags, v, ns, cap)
    assert L.fs_raster_backward_scratch_bytes(None, 1, 0, 100) == 0
    for args, want in RASTER_SLOTS_TABLE:
        assert L.fs_raster_scratch_slots(*args) == want, args


def test_every_entry_point_validates_its_arguments_before_touching_a_device():
    """Error behaviour of the boundary, checked without a GPU: every int-returning entry point called with NULL pointers
    answers FS_ERR_INVALID_ARG (-1) when its sizes are positive, and -1 or FS_OK (an empty job) when they are zero --
    nothing dereferences or launches first."""
    import ctypes as C
    from freesplat_amd import _lib
    L = _lib.lib()
    getters = {"fs_abi_version", "fs_ptf_gru_table_rows", "fs_ptf_gru_table_t_rows", "fs_ptf_gru_stream_rows", "fs_ptf_gru_stream_layout", "fs_ptf_gru_table_layout", "fs_ptf_gru_stream_chunk_rows", "fs_ptf_gru_side_cols", "fs_ptf_gru_act_cols", "fs_ptf_gru_stream_t_rows",
               "fs_ptf_gru_grad_floats", "fs_raster_scratch_slots",
               "fs_profile_enable", "fs_profile_collect"}

    def call(name, size):
        _, at = _lib.SIGNATURES[name]
        args = [size if a in (C.c_int32, C.c_int64, C.c_int) else (0.0 if a is C.c_float else None) for a in at]
        return getattr(L, name)(*args)

    checked = 0
    for name, (rt, _) in _lib.SIGNATURES.items():
        if rt is not C.c_int or name in getters:
            continue
        assert call(name, 0) in (0, -1), name
        assert call(name, 1) == -1, name
        checked += 1
    assert checked >= 24


def test_workspace_size_queries():
    """The size queries a caller allocates from (host logic, no GPU): the cost volume's forward workspace holds the
    current view's [hw, C] copy, the sources' [hw, C + 32] records (features + the projected first-layer block of the
    K = 1 sweep) and the projection rows; the backward's holds the pixel-major copies and their gradients, the two-pass
    form's records (C + 2 floats per (view, plane, pixel)) and the inverse plane homographies; the training forward's
    saved buffer a header and C + 2 floats per point; the PTF sizes are monotone in their arguments; nonsense arguments
    give 0."""
    from freesplat_amd import _lib
    L = _lib.lib()
    al = lambda x: (x + 255) // 256 * 256
    for B, K, C, h, w in ((2, 1, 48, 96, 128), (3, 2, 48, 242, 324), (10, 8, 48, 96, 128), (3, 2, 16, 13, 19)):
        hw = h * w
        assert L.fs_cost_volume_workspace_bytes(B, K, C, h, w) == al((B * C + B * K * (C + 32)) * hw * 4) + al(B * K * 12 * 4)
        for D in (8, 128):
            bD = L.fs_cost_volume_backward_workspace_bytes(B, K, C, h, w, D)
            assert bD == (al(B * (1 + K) * C * hw * 2 * 4) + al(B * K * 12 * 4) + al(B * D * hw * C * 4) + al(B * D * hw * 2 * 4)
                          + al(B * K * D * 9 * 4))
            assert L.fs_cost_volume_saved_bytes(B, C, h, w, D) == 256 + al(B * D * hw * C * 4) + al(B * D * hw * 2 * 4)
    assert L.fs_cost_volume_saved_bytes(0, 48, 8, 8, 8) == 0
    assert L.fs_cost_volume_workspace_bytes(1, 1, 0, 8, 8) == 0 and L.fs_cost_volume_backward_workspace_bytes(0, 1, 48, 8, 8, 8) == 0
    prev = 0
    for V in (2, 3, 10, 30):
        n = L.fs_ptf_fold_bytes(V, 384, 512)
        assert n > prev
        prev = n
    assert L.fs_ptf_fold_bytes(1, 384, 512) == 0 and L.fs_ptf_fold_bytes(2, 0, 512) == 0
    assert L.fs_ptf_scratch_bytes(1000, 48, 64) <= L.fs_ptf_scratch_bytes(100000, 48, 64)
    assert L.fs_ptf_fold_scratch_bytes(1000, 48, 64) <= L.fs_ptf_fold_scratch_bytes(100000, 48, 64)
    assert L.fs_ptf_scratch_bytes(-1, 48, 64) == 0 and L.fs_ptf_fold_scratch_bytes(10, 48, 0) == 0


def test_overflow_capacity_is_per_image_size_and_decays():
    """Host logic of the rasterizer's capacity history: the capacity an overflow asked for is kept per image
    size, is what the next call of that size allocates, decays by 10 % with every call that fits, and is dropped once it
    falls below the default -- one close-up view does not inflate every later call for good."""
    from freesplat_amd import rasterizer as R
    st = R._DeviceState()
    N, H, W = 1000, 968, 1296
    base = R.default_capacity(N, st, H, W)
    cap = st.note_overflow(n_inst=5_000_000, max_tile=50_000, H=H, W=W)
    T = ((W + 15) // 16) * ((H + 15) // 16)
    assert cap == max(5_000_000 + 1024, (50_000 * T + 3) // 4 + 1) and R.default_capacity(N, st, H, W) == cap
    assert R.default_capacity(N, st, 480, 640) == base                     # another image size is unaffected
    assert st.note_overflow(10, 10, H, W) == cap                           # a smaller overflow never shrinks it
    seen = []
    for _ in range(200):
        st.note_fit(H, W)
        seen.append(R.default_capacity(N, st, H, W))
    assert seen[0] == max(base, int(cap * 0.9)) and all(a >= b for a, b in zip(seen, seen[1:])) and seen[-1] == base
    assert st.retry_cap == 0 and not st.retry_caps
    st.note_overflow(5_000_000, 50_000, H, W)
    st.retry_cap = 0                                                       # (bench / tests reset the history)
    assert R.default_capacity(N, st, H, W) == base


def test_capacity_verdict_keeps_the_three_update_rules():
    """Host logic of rasterizer.capacity_verdict, the one reading of the instance-capacity counters (no GPU: the counter pairs are
    lists).  Expected values follow the three code paths it replaced: a single view ASSIGNS last_instances its count,
    render_views assigns the MAXIMUM over its views, the deferred check never lowers it and withholds note_fit from every pending
    call after the first overflowed one; an overflowed view is to be re-rendered with retry_capacity of its own counters, never
    less than the history already asks for; counters are int32 bit patterns of unsigned values."""
    import torch
    from freesplat_amd import decoder as D, rasterizer as R
    H, W, T = 40, 56, 12
    key = (H, W)
    st = R._DeviceState()
    st.last_instances, st.retry_caps[key] = 9_000_000, 4_000_000
    # a single view that fits: assigned (here: lowered), and the overflow-derived capacity decays
    assert R.capacity_verdict(st, [[5000, 0]], H, W) == ([5000], {}) and st.last_instances == 5000 and st.retry_caps[key] == 3_600_000
    # three views that fit: the maximum, another decay step
    assert R.capacity_verdict(st, [[100, 0], [7000, 0], [300, 0]], H, W) == ([100, 7000, 300], {})
    assert st.last_instances == 7000 and st.retry_caps[key] == 3_240_000
    # views 1 and 2 overflowed: each gets the capacity the history asks for after its own overflow, nothing decays
    want1 = max(5_000_000 + 1024, (4000 * T + 3) // 4 + 1)
    want2 = max(300 + 1024, (3_000_000 * T + 3) // 4 + 1)
    assert want1 == R.retry_capacity(5_000_000, 4000, H, W) == 5_001_024 and want2 == R.retry_capacity(300, 3_000_000, H, W) == 9_000_001
    counts, redo = R.capacity_verdict(st, [[100, 0], [5_000_000, 4000], [300, 3_000_000]], H, W)
    assert counts == [100, 5_000_000, 300] and redo == {1: want1, 2: want2} and st.last_instances == 5_000_000 and st.retry_caps[key] == want2
    assert R.capacity_verdict(st, [[50, 7]], H, W) == ([50], {0: want2}) and st.last_instances == 50     # (a smaller overflow never shrinks it)
    # int32 bit patterns: -1 is 2^32 - 1 instances, a negative tile count an overflow
    st = R._DeviceState()
    counts, redo = R.capacity_verdict(st, [[-1, -2147483648]], H, W)
    assert counts == [0xFFFFFFFF] and redo == {0: (0x80000000 * T + 3) // 4 + 1} and st.last_instances == 0xFFFFFFFF
    assert R.capacity_verdict(R._DeviceState(), [], H, W) == ([], {})
    # the deferred rules: never lowered; a call after an overflowed one does not count as a fit
    st = R._DeviceState()
    st.last_instances, st.retry_caps[key] = 9_000_000, 4_000_000
    assert R.capacity_verdict(st, [[10, 0], [20, 0]], H, W, lower=False) == ([10, 20], {}) and st.last_instances == 9_000_000
    assert st.retry_caps[key] == 3_600_000
    assert R.capacity_verdict(st, [[9_500_000, 0]], H, W, lower=False, may_fit=False) == ([9_500_000], {})
    assert st.last_instances == 9_500_000 and st.retry_caps[key] == 3_600_000
    # ... and decoder.check_deferred over three pending calls (fits / one view overflows / fits), on host tensors
    dev = torch.device("cuda", 63)
    st = R._states[63] = R._DeviceState()
    try:
        st.last_instances, st.retry_caps[key] = 9_000_000, 4_000_000
        states = [R.RasterState(*[None] * 13) for _ in range(2)]
        i32 = lambda rows: torch.tensor(rows, dtype=torch.int32)
        D._pending_checks[:] = [(i32([[10, 0], [20, 0]]), states, dev, key), (i32([[3_000_000, 5000], [30, 0]]), None, dev, key),
                                (i32([[40, 0]]), None, dev, key)]
        with pytest.raises(R._lib.FreeSplatHipError, match="1 deferred view"):
            D.check_deferred()
        assert not D._pending_checks and [rs.num_rendered for rs in states] == [10, 20]
        assert st.last_instances == 9_000_000 and st.retry_caps == {key: 3_600_000}       # one decay (the first call), then withheld
    finally:
        del R._states[63]
        D._pending_checks.clear()


def test_traffic_lookup_refuses_kernels_the_library_no_longer_contains():
    """bench.py / bench_encoder.py read `roofline.traffic` through profiles/tools/fwd_traffic.lookup(); a committed traffic file
    that names a kernel the shipped library does not contain (round 3's K >= 2 rows named the deleted cost_volume_kernel<24>)
    must be skipped for that workload -- checked against the built library's embedded code object, no GPU needed."""
    import json
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "profiles", "tools"))
    import fwd_traffic
    assert fwd_traffic.kernel_shipped("fs::cost_volume16_kernel<48, false>") and fwd_traffic.kernel_shipped("fs::cv_src_grad_kernel<48>")
    assert fwd_traffic.kernel_shipped("fs::sort_blend_kernel<false, false>")
    assert not fwd_traffic.kernel_shipped("fs::cost_volume_kernel<24>") and not fwd_traffic.kernel_shipped("fs::cv_transpose_kernel")
    r3 = json.load(open(os.path.join(root, "profiles", "r3_traffic.json")))["workloads"]
    assert any("cost_volume_kernel<24>" in k for k in r3["cv_fvt10_K8"]["kernels"])          # the stale row is still in the old file
    val, src = fwd_traffic.lookup("cv_fvt10_K8")
    assert src is not None and "r3_traffic" not in src and val < 2e9                          # ... and is not what gets reported
    val, src = fwd_traffic.lookup("cvt_fvt10_K8")
    assert src is not None and val > 1e10                                                     # the training step's rows exist


def test_committed_bench_line_honours_the_contract():
    """The tracked copy of the bench output of the final code (profiles/r6_bench.json = the FULL sectioned line,
    profiles/r6_bench_headline.json = the compact LAST line the driver parses; both written by `python bench.py` on the GPU box):
    every key the bench contract names, the roofline / cpu_baseline objects, BASELINE.json's workload, the sub-objects the
    documentation cites, and the compact line's size."""
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = json.load(open(os.path.join(root, "profiles", "r6_bench.json")))
    raw = open(os.path.join(root, "profiles", "r6_bench_headline.json")).read().strip()
    hl = json.loads(raw)
    assert len(raw) <= 4096 and "\n" not in raw                              # the driver parsed nothing of 28 KB
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline", "parity"):
        assert k in d, k
        assert k in hl, k
    assert abs(hl["value"] - d["value"]) <= 1e-3 * d["value"] and hl["config"]["workload"] == d["config"]["workload"]
    assert hl["roofline"]["bound"] == "hbm" and hl["cpu_baseline"]["kind"] == "port" and hl["parity"]["bit_exact"] is True
    assert {"train", "c2", "c3_closeup", "c3_train_step_hotpath", "cost_volume.fvt10_96x128_K8", "ptf.fold_30_views"} <= set(hl["sections"])
    assert d["config"]["workload"] == "c3_968x1296_1M" and d["n_gpus"] == 1 and d["dtype"] == "f32" and d["vs_baseline"] is None
    assert d["unit"] == "views/s" and d["higher_is_better"] is True and d["scaling"] == "weak" and d["data"] == "synthetic"
    assert abs(d["value"] - 16 * d["steps"] / (d["ms_per_step"] * d["steps"] * 1e-3)) < 1e-6 * d["value"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "frac_overlapped", "frac_isolated", "pipeline_frac_wall"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["frac_isolated"] > r["frac_overlapped"] > 0 and r["traffic"] is not None
    # the VALU-issue roofline beside it: microbenchmark-priced issue cycles against the SIMD cycles of the launch
    for blk in (d["roofline_valu"], d["train"]["roofline_valu"]):
        assert blk["bound"] == "valu_issue" and 0.2 < blk["frac"] < 1.0 and 0.5 < blk["hw_valu_busy_frac"] <= 1.0
        assert abs(blk["frac"] - blk["issue_cycles_per_launch"] / (1024 * 2.4e9 * blk["isolated_launch_ms"] * 1e-3)) < 1e-6
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and "oracle/raster_oracle.c" in c["sample"]
    assert d["parity"]["bit_exact"] is True and d["parity"]["pixels_above_1e-4"] == 0
    # the sub-objects: training step, config 2, fp16 SH, the close-up workload, the three cost-volume shapes, four folds
    assert d["train"]["value"] > 1200 and d["value"] > 4200 and d["train"]["roofline"]["kernel"] == "render_bwd_kernel"
    assert d["c2"]["config"]["workload"].startswith("c2") and d["c3_fp16_sh"]["config"]["sh_storage"] == "fp16"
    assert d["c3_fp16_sh"]["parity"]["bit_exact"] is True
    cu = d["c3_closeup"]        # every tile list beyond the LDS sort; bit-exact; per list entry no slower than the headline
    assert cu["parity"]["bit_exact"] is True and cu["config"]["instances_per_gaussian"] >= 19 and cu["views_per_s_per_instance_vs_headline"] >= 0.6
    assert cu["raster_buffers"]["capacity_retries"] == 1 and cu["raster_buffers"]["scratch_bytes_per_stream"] > 1 << 30
    cv = d["cost_volume"]
    assert set(cv) == {"native_96x128_K1", "c3scale_242x324_K2", "fvt10_96x128_K8"}
    for name, v in cv.items():
        b = v["train_fwd_bwd"]["roofline"]
        assert v["roofline"]["bound"] == "mfma" and b["bound"] == "mfma" and b["global_float_atomics_on_source_maps"] == 0, name
        assert abs(b["algorithmic_flops_per_launch"] - 2 * v["roofline"]["algorithmic_flops_per_launch"]) < 1, name
        assert "cpu_baseline" in v and "parity" in v and v["roofline"]["traffic"] is not None and b["traffic"] is not None, name
    assert cv["fvt10_96x128_K8"]["train_fwd_bwd"]["ms"] <= 14.5 and cv["c3scale_242x324_K2"]["train_fwd_bwd"]["ms"] <= 13.2   # (round 5: 16.7 / 13.2)
    assert cv["native_96x128_K1"]["train_fwd_bwd"]["ms"] <= 1.25
    assert set(d["ptf"]) == {"fold_2_views", "fold_10_views", "fold_3_views_968x1296", "fold_30_views"}
    for name, v in d["ptf"].items():
        assert v["parity"]["same_count_and_order"] is True and v["roofline"]["bound"] == "hbm" and v["cpu_baseline"]["cores"] <= 16, name
        assert v["roofline"]["kernel_ms_per_fold"] <= v["ms_per_call"] + 1e-9, name          # 
        tr = v["train_fwd_bwd"]
        if tr["hip_ms"] is not None:
            assert tr["roofline"]["bound"] == "mfma" and 0 < tr["roofline"]["frac"] < 1, name
            assert tr["roofline"]["kernel_ms_per_step"] <= tr["hip_ms"], name
    assert d["ptf"]["fold_30_views"]["parity"]["views_compared"] >= 10                        # (item 8: was a 4-view prefix)
    assert d["ptf"]["fold_2_views"]["ms_per_call"] <= 0.23 and d["ptf"]["fold_2_views"]["train_fwd_bwd"]["hip_ms"] <= 1.6
    # round 6: 16-pair GRU kernels + kept activations (config 3's fold <= 8.2 ms, the native one <= 0.95 box to box)
    assert d["ptf"]["fold_3_views_968x1296"]["train_fwd_bwd"]["hip_ms"] <= 8.6 and d["ptf"]["fold_2_views"]["train_fwd_bwd"]["hip_ms"] <= 1.25   # (host-bound at this size: 0.82 - 1.10 run to run, kernels 0.58)
    assert d["train"]["value"] > 1280           # (>= 1 300 on the committed line's box)
    assert set(d["encoder_tail"]) == {"depth_tail", "gaussian_head"}
    # BASELINE config 3 as it is written, one composed step: stages sum to the library time, glue <= 10 %
    st = d["c3_train_step_hotpath"]
    assert st["config"]["image_hw"] == [968, 1296] and st["config"]["context_views"] == 3 and st["config"]["match_hw"] == [242, 324]
    assert abs(sum(st["library_kernel_ms_by_stage"].values()) - st["library_kernel_ms"]) < 1e-6
    assert set(st["library_kernel_ms_by_stage"]) >= {"cost_volume", "ptf", "encoder_tail", "render", "render_bwd", "preprocess", "preprocess_bwd"}
    assert st["library_kernel_ms"] < st["ms_per_step"] and st["glue_frac_of_gpu_time"] <= 0.10 and st["glue_source"].endswith("_c3_step_glue.json")
    c4 = d["c4_eval_step_hotpath"]          # config 4's per-GPU evaluation step: 10 views at the native size, K = 8, no backward stages
    assert c4["config"]["context_views"] == 10 and c4["config"]["sources_per_view"] == 8 and c4["config"]["image_hw"] == [384, 512]
    assert not {"render_bwd", "preprocess_bwd"} & set(c4["library_kernel_ms_by_stage"]) and c4["library_kernel_ms"] < c4["ms_per_step"]
    c5 = d["c5_eval_step_hotpath"]          # config 5: 30-view long-sequence fusion, fp16 SH storage, evaluation only
    assert c5["config"]["context_views"] == 30 and c5["config"]["sh_storage"] == "fp16" and c5["config"]["sources_per_view"] == 8
    assert c5["library_kernel_ms"] < c5["ms_per_step"] and not {"render_bwd", "preprocess_bwd"} & set(c5["library_kernel_ms_by_stage"])


def test_compact_headline_fits_the_driver_window():
    """bench.py prints the full sectioned object first and, as the LAST line, a compact object the driver can parse (round 4's
    single 28 KB line came back `parsed: null`): <= 4 KB with every contract key, `roofline`, `cpu_baseline`, `parity` and one
    digest per section -- checked on the largest committed full line; digests are dropped, never the contract keys, when a
    line would not fit."""
    import json
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    full = json.load(open(os.path.join(root, "profiles", "r6_bench.json")))
    h = bench.headline(full)
    line = json.dumps(h)
    assert len(line) <= bench.HEADLINE_MAX_BYTES <= 8192
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline", "parity", "sections"):
        assert k in h, k
    assert h["config"]["workload"] == "c3_968x1296_1M" and abs(h["value"] - full["value"]) < 1e-3 * full["value"]
    assert abs(h["roofline"]["frac"] - full["roofline"]["frac"]) < 1e-4 and h["cpu_baseline"]["kind"] == "port"
    assert {"train", "c2", "cost_volume.fvt10_96x128_K8", "ptf.fold_30_views", "encoder_tail.gaussian_head"} <= set(h["sections"])
    # a pathological full line (hundreds of sections) still yields a line inside the window, contract keys intact
    fat = dict(full, ptf={f"fold_{i}": full["ptf"]["fold_2_views"] for i in range(300)})
    h2 = bench.headline(fat)
    assert len(json.dumps(h2)) <= bench.HEADLINE_MAX_BYTES and h2["sections_truncated"] and "roofline" in h2 and "cpu_baseline" in h2
