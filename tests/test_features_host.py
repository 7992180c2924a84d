"""The feature pass in the C-ABI and Composite.model_indicator, host side (no GPU): fdgs_render_features refuses every bad argument with
FDGS_E_INVALID and a message BEFORE anything is launched -- the library loads and validates without a device, as the pick entry point
does --, and the per-model indicator is checked on CPU tensors against a case worked out by hand."""
import importlib
import os
import re
import types

import numpy as np
import pytest
import torch

from test_pick_host import _stub_scene

fdgs = importlib.import_module("4dgaussians_amd")
P, C, L = fdgs.playback, fdgs.compose, fdgs._lib
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
    decl = re.search(r"\bint\s+fdgs_render_features\s*\((.*?)\)\s*;", src, flags=re.S)
    assert decl and len(decl.group(1).split(",")) == 14
    assert "fdgs_render_features" in L.SYMBOLS and hasattr(lib, "fdgs_render_features")
    assert len(L.SYMBOLS["fdgs_render_features"][1]) == 14
    assert lib.fdgs_abi_version() == 6 and L.ABI_VERSION == 6                        # an addition to ABI 6
    assert "writes nothing into the frame" in re.sub(r"[\s*]+", " ", text).lower()


def _good():
    """A call that is valid up to the launch (never made here: there is no device), as keyword -> value; host arrays stand in for the buffers."""
    bufs = types.SimpleNamespace(geom=np.zeros(64, np.uint8), binning=np.zeros(64, np.uint8), img=np.zeros(64, np.uint8),
                                 row_map=np.arange(N, dtype=np.int32), values=np.ones((N, CH + 3), np.float32),
                                 features=np.full(CH * H * W + 1, SENTINEL, np.float32), alpha=np.full(H * W + 1, SENTINEL, np.float32))
    p = L.RasterParams()
    p.P, p.W, p.H = N, W, H
    good = dict(stream=None, p=p, geom=bufs.geom.ctypes.data, binning=bufs.binning.ctypes.data, img=bufs.img.ctypes.data, R=100, C=CH,
                values=bufs.values.ctypes.data, value_stride=CH + 3, rows=N, row_map=bufs.row_map.ctypes.data, min_alpha=-1.0,
                features=bufs.features.ctypes.data, alpha=bufs.alpha.ctypes.data)
    return good, bufs


def _refused(lib, args, bufs, what):
    assert lib.fdgs_render_features(*args.values()) == -1, what                      # FDGS_E_INVALID
    msg = lib.fdgs_last_error()
    assert msg, what
    assert (bufs.features == SENTINEL).all() and (bufs.alpha == SENTINEL).all(), what
    return msg


def test_null_pointers_are_refused(lib):
    for name in ("p", "geom", "binning", "img", "values", "features"):
        good, bufs = _good()
        assert b"NULL" in _refused(lib, {**good, name: None}, bufs, name)


@pytest.mark.parametrize("field,value", [("W", 0), ("H", 0), ("H", -3), ("W", -1)])
def test_bad_image_sizes_are_refused(lib, field, value):
    good, bufs = _good()
    setattr(good["p"], field, value)
    _refused(lib, good, bufs, (field, value))


@pytest.mark.parametrize("c", [0, -1, 8 * 65535 + 1])
def test_bad_channel_counts_are_refused(lib, c):
    good, bufs = _good()
    assert b"C" in _refused(lib, {**good, "C": c, "value_stride": max(c, 1)}, bufs, c)


def test_a_stride_below_c_and_negative_rows_are_refused(lib):
    good, bufs = _good()
    assert b"value_stride" in _refused(lib, {**good, "value_stride": CH - 1}, bufs, "stride")
    assert b"value_stride" in _refused(lib, {**good, "value_stride": 0}, bufs, "stride")
    assert b"rows" in _refused(lib, {**good, "rows": -1}, bufs, "rows")


@pytest.mark.parametrize("which", ["values", "row_map", "features", "alpha"])
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_misaligned_arrays_are_refused(lib, which, shift):
    good, bufs = _good()
    good[which] += shift
    assert b"aligned" in _refused(lib, good, bufs, (which, shift))


# ---- Composite.model_indicator, on CPU tensors -------------------------------------------------------------------------------------------

def test_model_indicator_against_a_hand_worked_case():
    scene = _stub_scene([3, 0, 2, 1], [None] * 4)                                    # rows 0-2 | (none) | 3-4 | 5
    got = scene.model_indicator()
    assert got.dtype == torch.float32 and got.shape == (6, 4)
    assert got.tolist() == [[1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
    model, _ = scene.model_of_rows(torch.arange(6))                                  # the ranges model_of_rows splits ids by
    assert torch.equal(got.argmax(dim=1).to(torch.int32), model) and torch.equal(got.sum(dim=1), torch.ones(6))
    # a permutation inside a model changes which stored row a scene row is, not who owns it
    perm = torch.tensor([1, 0], dtype=torch.int32)
    assert torch.equal(_stub_scene([3, 0, 2, 1], [None, None, perm, None]).model_indicator(), got)
    assert _stub_scene([4], [None]).model_indicator().tolist() == [[1.0]] * 4
