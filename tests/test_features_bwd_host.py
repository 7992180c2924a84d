"""The feature pass's backward in the C-ABI, host side (no GPU): fdgs_render_features_bwd refuses every bad argument with FDGS_E_INVALID
and a message BEFORE anything is launched -- the library loads and validates without a device, as the feature pass's entry point does --,
and an empty frame (P == 0 or num_rendered == 0) succeeds without a launch and without touching dvalues."""
import importlib
import os
import re
import types

import numpy as np
import pytest

fdgs = importlib.import_module("4dgaussians_amd")
L = fdgs._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N, CH = 40, 36, 48, 5
SENTINEL = -7.0


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        importlib.import_module("4dgaussians_amd.build").build()
    return L.lib()


def test_header_declares_the_entry_point_and_lib_binds_it(lib):
    text = open(os.path.join(ROOT, "include", "fdgs.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+fdgs_render_features_bwd\s*\((.*?)\)\s*;", src, flags=re.S)
    assert decl and len(decl.group(1).split(",")) == 14
    assert "fdgs_render_features_bwd" in L.SYMBOLS and hasattr(lib, "fdgs_render_features_bwd")
    assert len(L.SYMBOLS["fdgs_render_features_bwd"][1]) == 14
    assert lib.fdgs_abi_version() == 6 and L.ABI_VERSION == 6                        # an addition to ABI 6
    flat = re.sub(r"[\s*]+", " ", text).lower()
    assert "of p only p, w, h and debug are read" in flat                            # (the `*` of `*p` goes with the comment's margin)
    assert "non-finite dl_dfeatures is out of contract" in flat


def _good():
    """A call that is valid up to the launch (never made here: there is no device), as keyword -> value; host arrays stand in for the buffers."""
    bufs = types.SimpleNamespace(geom=np.zeros(64, np.uint8), binning=np.zeros(64, np.uint8), img=np.zeros(64, np.uint8),
                                 row_map=np.arange(N, dtype=np.int32), grad=np.ones(CH * H * W + 1, np.float32),
                                 alpha=np.ones(H * W + 1, np.float32), dvalues=np.full((N, CH + 3), SENTINEL, np.float32))
    p = L.RasterParams()
    p.P, p.W, p.H = N, W, H
    good = dict(stream=None, p=p, geom=bufs.geom.ctypes.data, binning=bufs.binning.ctypes.data, img=bufs.img.ctypes.data, R=100, C=CH,
                grad=bufs.grad.ctypes.data, alpha=bufs.alpha.ctypes.data, min_alpha=1e-4, row_map=bufs.row_map.ctypes.data, rows=N,
                dvalues=bufs.dvalues.ctypes.data, dvalue_stride=CH + 3)
    return good, bufs


def _refused(lib, args, bufs, what):
    assert lib.fdgs_render_features_bwd(*args.values()) == -1, what                  # FDGS_E_INVALID
    msg = lib.fdgs_last_error()
    assert msg, what
    assert (bufs.dvalues == SENTINEL).all(), what
    return msg


def test_null_pointers_are_refused(lib):
    for name in ("p", "geom", "binning", "img", "grad", "dvalues"):
        good, bufs = _good()
        assert b"NULL" in _refused(lib, {**good, name: None}, bufs, name)


def test_a_normalised_backward_needs_the_alpha_image(lib):
    for min_alpha in (0.0, 1e-4, 0.5):
        good, bufs = _good()
        assert b"alpha_opt" in _refused(lib, {**good, "alpha": None, "min_alpha": min_alpha}, bufs, min_alpha)


@pytest.mark.parametrize("field,value", [("W", 0), ("H", 0), ("H", -3), ("W", -1)])
def test_bad_image_sizes_are_refused(lib, field, value):
    good, bufs = _good()
    setattr(good["p"], field, value)
    _refused(lib, good, bufs, (field, value))


@pytest.mark.parametrize("c", [0, -1, 8 * 65535 + 1])
def test_bad_channel_counts_are_refused(lib, c):
    good, bufs = _good()
    assert b"C" in _refused(lib, {**good, "C": c, "dvalue_stride": max(c, 1)}, bufs, c)


def test_a_stride_below_c_and_negative_rows_are_refused(lib):
    good, bufs = _good()
    assert b"dvalue_stride" in _refused(lib, {**good, "dvalue_stride": CH - 1}, bufs, "stride")
    assert b"dvalue_stride" in _refused(lib, {**good, "dvalue_stride": 0}, bufs, "stride")
    assert b"rows" in _refused(lib, {**good, "rows": -1}, bufs, "rows")


@pytest.mark.parametrize("which", ["grad", "alpha", "row_map", "dvalues"])
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_misaligned_arrays_are_refused(lib, which, shift):
    good, bufs = _good()
    good[which] += shift
    assert b"aligned" in _refused(lib, good, bufs, (which, shift))


def test_an_empty_frame_succeeds_without_a_launch_and_leaves_dvalues_alone(lib):
    """P == 0 or num_rendered == 0: FDGS_OK.  The buffers are host arrays and there is no device here: a launch could not succeed, and a
    write from the host side would show in the sentinels."""
    for change in ({"R": 0}, {"P": 0}, {"R": 0, "alpha": None, "min_alpha": -1.0}, {"P": 0, "row_map": None}):
        good, bufs = _good()
        if "P" in change:
            good["p"].P = change.pop("P")
        assert lib.fdgs_render_features_bwd(*{**good, **change}.values()) == 0, change
        assert (bufs.dvalues == SENTINEL).all(), change


def test_the_kernels_operand_layout_is_the_contraction():
    """The lane-level numpy model of the kernel's two park transposes and its 16 v_mfma_f32_16x16x4_f32 (tools/mfma_layout_model.py, as
    tests/test_mfma_layouts.py does for the deformation kernels) against plain matrix algebra, and the park's bank arithmetic."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("mfma_layout_model", os.path.join(ROOT, "tools", "mfma_layout_model.py"))
    model = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(model)
    assert model.check_features_bwd(np.random.default_rng(4))
    header = open(os.path.join(ROOT, "4dgaussians_amd", "csrc", "render_features_bwd.h")).read()
    assert re.search(r"constexpr int FBWD_PARK = (\d+);", header).group(1) == str(model.PARK)
