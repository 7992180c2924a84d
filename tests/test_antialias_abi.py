"""CPU-side checks of the antialiasing additions to the C-ABI: the seven entry points are declared, exported and bound, they validate
their arguments on the host like their neighbours, the ABI version did not move, and the Python surface the drop-in pins is unchanged."""
import ctypes
import importlib
import inspect
import os
import re

import numpy as np
import pytest

import antialias_common as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (new entry point, the neighbour it extends, pointers added at the end of the neighbour's list -- for the twins: where they are added)
NEW = {"fdgs_preprocess_fwd_aa": ("fdgs_preprocess_fwd", 0), "fdgs_raster_fwd_capacity_aa": ("fdgs_raster_fwd_capacity_alpha", 0),
       "fdgs_raster_bwd_aa": ("fdgs_raster_bwd_alpha", 0), "fdgs_camera_grad_aa": ("fdgs_camera_grad", 0),
       "fdgs_preprocess_host_aa": ("fdgs_preprocess_host", 1), "fdgs_preprocess_bwd_host_aa": ("fdgs_preprocess_bwd_host", 2),
       "fdgs_camera_grad_host_aa": ("fdgs_camera_grad_host", 1)}


@pytest.fixture(scope="module")
def L():
    return AC.lib()[0]


def test_the_seven_entry_points_are_exported_and_the_abi_version_stays_6(L):
    lib = L.lib()
    for new, (old, extra) in NEW.items():
        assert hasattr(lib, new) and hasattr(lib, old), new
        assert L.SYMBOLS[new][0] is L.SYMBOLS[old][0]
        assert len(L.SYMBOLS[new][1]) == len(L.SYMBOLS[old][1]) + extra, new
        assert L.SYMBOLS[new][1][:4] == L.SYMBOLS[old][1][:4], new
    assert lib.fdgs_abi_version() == 6 and L.ABI_VERSION == 6


def test_the_header_declares_them_next_to_the_alpha_family_and_states_the_arithmetic():
    src = open(os.path.join(ROOT, "include", "fdgs.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in NEW:
        assert re.search(r"\bint %s\s*\(" % n, code), n
    assert code.index("fdgs_raster_bwd_alpha") < code.index("fdgs_preprocess_fwd_aa") < code.index("fdgs_mark_visible")
    for phrase in ("h = sqrt(max(2.5e-5, r))", "D0 = A C - b^2", "MUST take the case of the forward", "opacity_eff[P]", "dL_dopacity = h * g"):
        assert phrase in src, phrase
    api = open(os.path.join(ROOT, "4dgaussians_amd", "csrc", "api.hip")).read()
    assert re.search(r"fdgs_abi_version\(void\)\s*\{\s*return 6;", api)


def test_the_settings_tuple_and_the_pinned_signatures_are_unchanged():
    fd = importlib.import_module("4dgaussians_amd")
    assert list(fd.GaussianRasterizationSettings._fields) == ["image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix",
                                                             "projmatrix", "sh_degree", "campos", "prefiltered", "debug"]
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(fd.render) == ["viewpoint_camera", "pc", "pipe", "bg_color", "scaling_modifier", "override_color", "stage", "cam_type"]
    assert names(fd.rasterizer.GaussianRasterizer.__init__) == ["self", "raster_settings", "render_alpha"]
    R = fd.rasterizer
    assert inspect.signature(R.rasterize_forward).parameters["antialiasing"].default is False
    assert inspect.signature(R.rasterize_gaussians).parameters["antialiasing"].default is False
    assert R.GaussianRasterizer.antialiasing is False and "antialiasing" in R.RasterState.__slots__


def test_bad_arguments_are_refused_on_the_host(L):
    lib = L.lib()
    p = L.RasterParams()
    assert lib.fdgs_preprocess_fwd_aa(None, None, None, None) != 0
    assert lib.fdgs_raster_bwd_aa(None, None, None, None, None, 0, None, None) != 0
    assert lib.fdgs_camera_grad_aa(None, None, None, None, None, None) != 0
    assert lib.fdgs_raster_fwd_capacity_aa(None, ctypes.byref(p), None, None, None, 0, None, None, None, None, None) != 0
    assert b"capacity" in lib.fdgs_last_error()
    # the twins: what the plain twins refuse, and the arrays only they take
    sc = AC.inputs(257, "sh16")
    out, pp, keep = AC.twin_forward(sc, 1.0)
    args = [out[k].ctypes.data for k in AC.FWD_KEYS]
    assert lib.fdgs_preprocess_host_aa(pp, *args, None) != 0 and b"opacity_eff" in lib.fdgs_last_error()
    s = AC.sums_f32(AC.weights(sc, out["radii"]), np.ones(257))
    head = (pp, out["tiles"].ctypes.data, out["clamped"].ctypes.data, out["cov3D"].ctypes.data, s["xy"].ctypes.data, s["conic"].ctypes.data,
            s["rgb"].ctypes.data, s["depth"].ctypes.data)
    res = np.zeros(48)
    assert lib.fdgs_camera_grad_host_aa(*head, None, res.ctypes.data) != 0 and b"d_opacity" in lib.fdgs_last_error()
    assert lib.fdgs_camera_grad_host_aa(*head, s["opacity"].ctypes.data, None) != 0
    g = [np.zeros((257, k), np.float32) for k in (3, 3, 48, 3, 4, 6)]
    assert lib.fdgs_preprocess_bwd_host_aa(*head, s["opacity"].ctypes.data, *(a.ctypes.data for a in g), None) != 0
    assert b"dL_dopacity" in lib.fdgs_last_error()


def test_an_empty_set_is_accepted_by_the_twins(L):
    lib = L.lib()
    sc = AC.inputs(257, "sh16")
    pp, keep = AC.raster_params(sc, 1.0)
    pp.P = 0
    res = np.full(48, np.nan)
    assert lib.fdgs_preprocess_host_aa(pp, *([None] * 10)) == 0
    assert lib.fdgs_preprocess_bwd_host_aa(pp, *([None] * 15)) == 0
    assert lib.fdgs_camera_grad_host_aa(pp, *([None] * 8), res.ctypes.data) == 0 and not np.any(res)
