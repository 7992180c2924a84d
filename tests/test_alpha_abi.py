"""CPU-side checks of the accumulated-alpha additions to the C-ABI: the three entry points are declared, exported and bound, they validate
their arguments on the host like their neighbours, and the ABI version did not move."""
import ctypes
import importlib
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fdgs_render_fwd_alpha", "fdgs_raster_fwd_capacity_alpha", "fdgs_raster_bwd_alpha")
OLD = ("fdgs_render_fwd", "fdgs_raster_fwd_capacity", "fdgs_raster_bwd")


@pytest.fixture(scope="module")
def L():
    _lib = importlib.import_module("4dgaussians_amd._lib")
    if not os.path.exists(_lib.LIB_PATH):
        importlib.import_module("4dgaussians_amd.build").build()
    return _lib


def test_the_three_alpha_entry_points_are_exported_and_the_abi_version_stays_6(L):
    lib = L.lib()
    for n in NEW + OLD:
        assert hasattr(lib, n), n
    assert lib.fdgs_abi_version() == 6 and L.ABI_VERSION == 6
    # each is its neighbour with ONE more pointer at the end: no existing signature changed
    for new, old in zip(NEW, OLD):
        assert L.SYMBOLS[new][0] is L.SYMBOLS[old][0]
        assert L.SYMBOLS[new][1] == L.SYMBOLS[old][1] + [ctypes.c_void_p], new


def test_the_header_declares_them_and_says_what_alpha_is():
    src = open(os.path.join(ROOT, "include", "fdgs.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in NEW:
        assert re.search(r"\bint %s\s*\(" % n, code), n
    assert re.search(r"float\* out_alpha\)", code) and re.search(r"const float\* dL_dalpha\)", code)
    assert "1 - T_final" in src and "T_final / (1 - alpha_i)" in src
    assert "does not\n * touch an alpha image" in src            # the note on a second fdgs_render_fwd over rewritten recC


def test_bad_arguments_are_refused_on_the_host(L):
    """Validation happens before anything is queued: the alpha calls refuse what their neighbours refuse (NULL params), and a misaligned
    alpha image."""
    lib = L.lib()
    p = L.RasterParams()
    assert lib.fdgs_render_fwd_alpha(None, None, None, None, None, 0, None, None, None) != 0
    assert lib.fdgs_raster_bwd_alpha(None, None, None, None, None, 0, None, None) != 0
    assert lib.fdgs_raster_fwd_capacity_alpha(None, ctypes.byref(p), None, None, None, 0, None, None, None, None, None) != 0
    assert b"capacity" in lib.fdgs_last_error()


def test_python_signatures_the_drop_in_pins_are_unchanged():
    fd = importlib.import_module("4dgaussians_amd")
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(fd.render) == ["viewpoint_camera", "pc", "pipe", "bg_color", "scaling_modifier", "override_color", "stage", "cam_type"]
    assert names(fd.rasterizer.GaussianRasterizer.forward) == ["self", "means3D", "means2D", "opacities", "shs", "colors_precomp", "scales",
                                                               "rotations", "cov3D_precomp"]
    init = inspect.signature(fd.rasterizer.GaussianRasterizer.__init__).parameters
    assert list(init) == ["self", "raster_settings", "render_alpha"] and init["render_alpha"].default is False
    assert inspect.signature(fd.rasterizer.rasterize_forward).parameters["want_alpha"].default is False
    assert inspect.signature(fd.rasterizer.rasterize_backward).parameters["grad_alpha"].default is None
