"""CPU-side checks of the absolute-gradient addition to the C-ABI: fdgs_raster_bwd_abs is declared, exported and bound, it validates its
arguments on the host like its siblings, the ABI version did not move, and the Python surface the drop-in pins is unchanged."""
import ctypes
import importlib
import inspect
import os
import re

import numpy as np
import pytest

import antialias_common as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "fdgs_raster_bwd_abs"


@pytest.fixture(scope="module")
def L():
    return AC.lib()[0]


def test_the_entry_point_is_exported_and_bound_and_the_abi_version_stays_6(L):
    lib = L.lib()
    assert hasattr(lib, NEW) and hasattr(lib, "fdgs_raster_bwd_alpha") and hasattr(lib, "fdgs_raster_bwd_aa")
    # the siblings' list, then the antialiasing case as an int and one more pointer: no existing signature changed
    assert L.SYMBOLS[NEW][0] is L.SYMBOLS["fdgs_raster_bwd_alpha"][0]
    assert L.SYMBOLS[NEW][1] == L.SYMBOLS["fdgs_raster_bwd_alpha"][1] + [ctypes.c_int, ctypes.c_void_p]
    assert L.SYMBOLS["fdgs_raster_bwd_aa"][1] == L.SYMBOLS["fdgs_raster_bwd_alpha"][1] == L.SYMBOLS["fdgs_raster_bwd"][1] + [ctypes.c_void_p]
    assert lib.fdgs_abi_version() == 6 and L.ABI_VERSION == 6


def test_the_header_declares_it_next_to_the_alpha_and_antialiasing_families_and_states_the_definition():
    src = open(os.path.join(ROOT, "include", "fdgs.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint %s\s*\(" % NEW, code)
    assert code.index("fdgs_raster_bwd_alpha") < code.index("fdgs_raster_bwd_aa") < code.index(NEW) < code.index("fdgs_mark_visible")
    assert re.search(r"const float\* dL_dalpha\s*,\s*int antialiased\s*,\s*float\* dL_dmeans2D_abs\s*\)", code)
    for phrase in ("sum_p |dL_p/dx_i| W/2", "sum_p |dL_p/dy_i| H/2", "slots 10", "dL_dmeans2D_abs = NULL IS the sibling call",
                   "the third column is exactly 0"):
        assert phrase in src, phrase
    api = open(os.path.join(ROOT, "4dgaussians_amd", "csrc", "api.hip")).read()
    assert re.search(r"fdgs_abi_version\(void\)\s*\{\s*return 6;", api)


def test_the_structs_and_the_pinned_signatures_are_unchanged(L):
    assert [k for k, _ in L.RasterGrads._fields_] == ["dL_dcolor", "dL_ddepth", "dL_dmeans2D", "dL_dmeans3D", "dL_dopacity", "dL_dcolors", "dL_dsh",
                                                     "dL_dscales", "dL_drotations", "dL_dcov3D", "scratch_acc", "deform_epilogue",
                                                     "scratch_acc_zeroed"]
    fd = importlib.import_module("4dgaussians_amd")
    assert list(fd.GaussianRasterizationSettings._fields) == ["image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix",
                                                             "projmatrix", "sh_degree", "campos", "prefiltered", "debug"]
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(fd.render) == ["viewpoint_camera", "pc", "pipe", "bg_color", "scaling_modifier", "override_color", "stage", "cam_type"]
    R = fd.rasterizer
    assert names(R.GaussianRasterizer.__init__) == ["self", "raster_settings", "render_alpha"]
    assert names(R.GaussianRasterizer.forward) == ["self", "means3D", "means2D", "opacities", "shs", "colors_precomp", "scales", "rotations",
                                                   "cov3D_precomp"]
    # the option is the LAST keyword of the two functions, a class attribute of the module and a slot of the state
    assert names(R.rasterize_forward)[-3:] == ["want_alpha", "antialiasing", "absgrad"]
    assert names(R.rasterize_gaussians)[-3:] == ["render_alpha", "antialiasing", "absgrad"]
    assert inspect.signature(R.rasterize_forward).parameters["absgrad"].default is False
    assert inspect.signature(R.rasterize_gaussians).parameters["absgrad"].default is False
    assert R.GaussianRasterizer.absgrad is False and R.GaussianRasterizer.antialiasing is False
    assert R.RasterState.__slots__[-3:] == ("with_alpha", "antialiasing", "absgrad")
    assert R.FrameOptions._fields == ("alpha", "antialiasing", "absgrad") and R.PLAIN == (False, False, False)
    assert R.FrameOptions(absgrad=True).keywords() == {"absgrad": True} and R.PLAIN.keywords() == {}
    pipe = type("Pipe", (), {"absgrad": 1})()
    assert R.FrameOptions.of(pipe) == (False, False, True) and R.FrameOptions.of(object()) == R.PLAIN


def test_null_and_misaligned_arguments_are_refused_on_the_host_with_a_message(L):
    lib = L.lib()
    assert lib.fdgs_raster_bwd_abs(None, None, None, None, None, 0, None, None, 0, None) != 0
    assert b"params is NULL" in lib.fdgs_last_error()
    pp, keep = AC.raster_params(AC.inputs(257, "sh16"), 1.0)
    buf = np.zeros(64, np.float32)
    g = L.RasterGrads()
    # NULL grads / geom / img, as the siblings refuse them
    assert lib.fdgs_raster_bwd_abs(None, pp, None, None, None, 0, ctypes.byref(g), None, 0, buf.ctypes.data) != 0
    assert b"NULL buffer" in lib.fdgs_last_error()
    assert lib.fdgs_raster_bwd_alpha(None, pp, None, None, None, 0, ctypes.byref(g), None) != 0 and b"NULL buffer" in lib.fdgs_last_error()
    # a misaligned output, and a misaligned alpha gradient: refused before any required buffer is looked at
    head = (None, pp, buf.ctypes.data, None, buf.ctypes.data, 0, ctypes.byref(g))
    assert lib.fdgs_raster_bwd_abs(*head, None, 0, buf.ctypes.data + 2) != 0
    assert b"dL_dmeans2D_abs must be 4-byte aligned" in lib.fdgs_last_error()
    assert lib.fdgs_raster_bwd_abs(*head, buf.ctypes.data + 1, 1, buf.ctypes.data) != 0
    assert b"dL_dalpha must be 4-byte aligned" in lib.fdgs_last_error()
    # aligned: the next refusal is the siblings' (the empty fdgs_raster_grads)
    assert lib.fdgs_raster_bwd_abs(*head, None, 0, buf.ctypes.data) != 0
    assert b"required gradient buffer is NULL" in lib.fdgs_last_error()
    # an empty set: accepted, nothing is written
    pp.P = 0
    buf[:] = 7.0
    assert lib.fdgs_raster_bwd_abs(*head, None, 0, buf.ctypes.data) == 0 and (buf == 7.0).all()
