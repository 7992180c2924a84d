"""The pick pass in the C-ABI and its Python helpers, host side (no GPU): fdgs_render_pick refuses every bad argument with FDGS_E_INVALID and
a message BEFORE anything is launched -- the library loads and validates without a device, as the motion entry points do --, and
Composite.model_of_rows / playback.unproject are checked on CPU tensors against values worked out by hand."""
import ctypes
import importlib
import math
import os
import re
import types

import numpy as np
import pytest
import torch

fdgs = importlib.import_module("4dgaussians_amd")
P, C, L = fdgs.playback, fdgs.compose, fdgs._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 40, 36, 48


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        importlib.import_module("4dgaussians_amd.build").build()
    return L.lib()


def test_header_declares_the_entry_point_and_lib_binds_it(lib):
    text = open(os.path.join(ROOT, "include", "fdgs.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+fdgs_render_pick\s*\(", src)
    assert "fdgs_render_pick" in L.SYMBOLS and hasattr(lib, "fdgs_render_pick")
    assert lib.fdgs_abi_version() == 6 and L.ABI_VERSION == 6                        # an addition to ABI 6
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct fdgs_pick_out \{(.*?)\} fdgs_pick_out;", text, flags=re.S).group(1), flags=re.S)
    names = [re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in L.PickOut._fields_] == ["pick_id", "pick_weight", "surface_id", "surface_depth"]
    assert len(L.SYMBOLS["fdgs_render_pick"][1]) == 9


def _good():
    """A call that is valid up to the launch (never made here: there is no device), as keyword -> value; host arrays stand in for the buffers."""
    bufs = types.SimpleNamespace(geom=np.zeros(64, np.uint8), binning=np.zeros(64, np.uint8), img=np.zeros(64, np.uint8),
                                 row_map=np.arange(N, dtype=np.int32), planes=np.full((4, H * W + 1), -7, np.int32))
    p = L.RasterParams()
    p.P, p.W, p.H = N, W, H
    out = L.PickOut()
    out.pick_id, out.pick_weight, out.surface_id, out.surface_depth = (bufs.planes[k].ctypes.data for k in range(4))
    good = dict(stream=None, p=p, geom=bufs.geom.ctypes.data, binning=bufs.binning.ctypes.data, img=bufs.img.ctypes.data, R=100,
                alpha_cut=0.5, row_map=bufs.row_map.ctypes.data, out=out)
    return good, bufs


def _refused(lib, args, bufs, what):
    before = bufs.planes.copy()
    assert lib.fdgs_render_pick(*args.values()) == -1, what                          # FDGS_E_INVALID
    msg = lib.fdgs_last_error()
    assert msg, what
    assert np.array_equal(bufs.planes, before), what
    return msg


def test_null_pointers_are_refused(lib):
    for name in ("p", "geom", "binning", "img", "out"):
        good, bufs = _good()
        assert b"NULL" in _refused(lib, {**good, name: None}, bufs, name)
    good, bufs = _good()
    empty = L.PickOut()
    assert b"NULL" in _refused(lib, {**good, "out": empty}, bufs, "all four outputs NULL")


@pytest.mark.parametrize("field,value", [("W", 0), ("H", 0), ("H", -3), ("W", -1)])
def test_bad_image_sizes_are_refused(lib, field, value):
    good, bufs = _good()
    setattr(good["p"], field, value)
    _refused(lib, good, bufs, (field, value))


@pytest.mark.parametrize("cut", [0.0, -0.5, float(np.nextafter(np.float32(1.0), np.float32(2.0))), 2.0, math.inf, -math.inf, math.nan])
def test_bad_alpha_cuts_are_refused(lib, cut):
    good, bufs = _good()
    assert b"alpha_cut" in _refused(lib, {**good, "alpha_cut": cut}, bufs, cut)


@pytest.mark.parametrize("which", ["pick_id", "pick_weight", "surface_id", "surface_depth", "row_map"])
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_misaligned_arrays_are_refused(lib, which, shift):
    good, bufs = _good()
    if which == "row_map":
        good["row_map"] += shift
    else:
        setattr(good["out"], which, getattr(good["out"], which) + shift)
    assert b"aligned" in _refused(lib, good, bufs, (which, shift))


# ---- Composite.model_of_rows and the composite's row map, on CPU tensors -----------------------------------------------------------------

def _stub_scene(Ns, perms):
    scene = C.Composite.__new__(C.Composite)
    scene.models = tuple(types.SimpleNamespace(N=n, perm=p) for n, p in zip(Ns, perms))
    scene.offsets = tuple(int(v) for v in np.cumsum([0] + list(Ns))[:-1])
    scene.slices = tuple(slice(o, o + n) for o, n in zip(scene.offsets, Ns))
    scene._storage = torch.zeros(1)
    return scene


def test_model_of_rows_against_hand_computed_values():
    scene = _stub_scene([5, 0, 7, 1], [None] * 4)                                  # rows 0-4 | (none) | 5-11 | 12
    ids = torch.tensor([[0, 4, 5, -1], [11, 12, 6, -1]], dtype=torch.int32)
    model, row = scene.model_of_rows(ids)
    assert model.dtype == row.dtype == torch.int32 and model.shape == row.shape == ids.shape
    assert model.tolist() == [[0, 0, 2, -1], [2, 3, 2, -1]]
    assert row.tolist() == [[0, 4, 0, -1], [6, 0, 1, -1]]
    every = torch.arange(13, dtype=torch.int32)
    model, row = scene.model_of_rows(every)
    for m, sl in enumerate(scene.slices):
        assert bool((model[sl] == m).all()) and row[sl].tolist() == list(range(sl.stop - sl.start))
    one = _stub_scene([3], [None])
    assert [t.tolist() for t in one.model_of_rows(torch.tensor([-1, 2, 0]))] == [[-1, 0, 0], [-1, 2, 0]]


def test_row_maps_of_a_composite_and_of_a_bake():
    perm = torch.tensor([2, 0, 3, 1], dtype=torch.int32)
    assert _stub_scene([3, 4], [None, None])._make_pick_row_map() is None
    got = _stub_scene([3, 4, 2], [None, perm, None])._make_pick_row_map()
    assert got.dtype == torch.int32 and got.tolist() == [0, 1, 2, 3 + 2, 3 + 0, 3 + 3, 3 + 1, 7, 8]
    assert P._perm_row_map(None) is None
    assert P._perm_row_map(perm.to(torch.int64)).dtype == torch.int32 and torch.equal(P._perm_row_map(perm), perm)


# ---- playback.unproject ---------------------------------------------------------------------------------------------------------------------

def test_unproject_against_hand_computed_values():
    """A camera whose view matrix is a pure shift t (p_view = p_world + t) with tan(fov / 2) = 1 on a 4 x 2 image: pixel (0, 0) has
    ndc = (1/4 - 1, 1/2 - 1) = (-0.75, -0.5), so at depth 2 it is (-1.5, -1, 2) in view space; pixel (3, 1): ndc = (0.75, 0.5), at depth 4:
    (3, 2, 4).  Every value is a small dyadic rational; the only roundings are tan(pi / 4) (1 - 1.1e-16 in float64, 1 in float32) and the
    inverse of a unit-triangular matrix: 1e-6 absolute is loose."""
    view = torch.eye(4)
    view[3, :3] = torch.tensor([1.0, 2.0, 3.0])
    cam = types.SimpleNamespace(image_width=4, image_height=2, FoVx=math.pi / 2, FoVy=math.pi / 2, world_view_transform=view)
    got = P.unproject(cam, torch.tensor([[0.0, 0.0], [3.0, 1.0]]), torch.tensor([2.0, 4.0]))
    want = torch.tensor([[-1.5 - 1.0, -1.0 - 2.0, 2.0 - 3.0], [3.0 - 1.0, 2.0 - 2.0, 4.0 - 3.0]])
    assert got.shape == (2, 3) and got.dtype == torch.float32 and float((got - want).abs().max()) < 1e-6
    settings = types.SimpleNamespace(image_width=4, image_height=2, tanfovx=1.0, tanfovy=1.0, viewmatrix=view)
    again = P.unproject({"camera": settings, "time": 0.0}, torch.tensor([[0, 0], [3, 1]]), torch.tensor([2.0, 4.0]), cam_type="PanopticSports")
    assert torch.equal(again, got)
    with pytest.raises(ValueError):
        P.unproject(cam, torch.zeros(3, 2), torch.ones(2))


def test_unproject_inverts_the_projection_of_a_real_camera():
    """Float64 projection of random points through a synthetic camera, then unproject in float32.  Error: the pixel and the depth are
    rounded to float32 (relative 2**-24 each), the chain is ~10 float32 operations on values of the size of the view-space point (|p| <
    8 here), and the inverse view matrix is orthonormal up to rounding: 20 * 2**-24 * 8 ~ 1e-5 absolute; a wrong convention (a half-pixel
    shift) moves a point by z * tan / W ~ 1e-2."""
    cam = fdgs.synthetic.make_camera(96, 64, theta_deg=25.0, time=0.0)
    view = cam.world_view_transform.double()
    pts = torch.from_numpy(np.random.default_rng(3).uniform(-1.0, 1.0, (64, 3)))
    pv = torch.cat([pts, torch.ones(64, 1, dtype=torch.float64)], 1) @ view
    z = pv[:, 2]
    assert float(z.min()) > 0.2 and float(pv.abs().max()) < 8.0
    px = ((pv[:, 0] / (z * math.tan(cam.FoVx * 0.5)) + 1.0) * 96 - 1.0) * 0.5
    py = ((pv[:, 1] / (z * math.tan(cam.FoVy * 0.5)) + 1.0) * 64 - 1.0) * 0.5
    got = P.unproject(cam, torch.stack([px, py], 1).float(), z.float())
    err = float((got.double() - pts).abs().max())
    print(f"unproject vs float64: max |dp| = {err:.3e}")
    assert err < 1e-5
