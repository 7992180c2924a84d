"""The camera's gradient (fdgs_camera_grad_host, the host twin of fdgs_camera_grad) WITHOUT a GPU: the loop of fdgs_preprocess_bwd_host around
camera_terms of csrc/gs_math.h, summed in double, on the scene, weights and subsets of tests/test_preprocess_host.py.

Reference: float64 autograd of the same contraction through oracle/raster_torch.project with viewmatrix, projmatrix and campos as leaves.
Bound: the project's gradient bound, rel-L2 < 1e-3, per group -- view[:, :3], proj[:, (0, 1, 3)], campos -- over all visible rows and
separately over the "frustum", "colour" and "plain" subsets, for every SH_PAIRS x MODS case.  view[:, 3] and proj[:, 2] are exactly 0.

Three single-path contractions, because the full one can hide a wrong small path: colour weights alone (campos only: the view-direction
derivative of the SH colour), depth weights alone (view through dtz only), conic weights alone (view through J and Rv).  The pixel-position
weights reach projmatrix only: their float64 viewmatrix gradient is exactly 0 (asserted).

How much of the 1e-3 is the reference's own -- a float32 evaluation of raster_torch.project's autograd against the float64 one on this scene:
without rows 0..39 (no planted rows) view 2.9e-7, proj 2.5e-7, campos 3.0e-7; with the planted rows (minus above_near and scale_huge) view
2.3e-2 .. 4.5e-2 -- all of it from the conic path, the float32 evaluation's own loss on those rows --, proj <= 2.8e-7, campos <= 4.6e-7.
The twin holds the bound with every planted row.  Measured (maxima over the fourteen cases, printed by the test): all rows view 4.9e-07,
proj 6.9e-07, campos 2.1e-07; subsets view <= 8.5e-07, proj <= 6.8e-07, campos <= 1.9e-07; colour alone campos 2.1e-07; depth alone view
2.2e-08; conic alone view 5.1e-07; pixel position alone proj 6.9e-07.

The test was checked against deliberate faults in a scratch copy of gs_math.h, one at a time; each one fails it (largest figures seen):
the x clamp flag ignored (all fourteen cases: view 0.18 over all rows and conic alone, 0.22 frustum, 0.37 colour subset); the covariance
path of camera_terms dropped (all fourteen: view 0.63 .. 0.82); the colour mask ignored (the ten cases above degree 0: campos 1.2 over all
rows and colour alone, 3.2 on the colour subset); the sign of campos flipped (the same ten: campos 2.0); FDGS_W_EPS dropped from mw in
camera_terms (the fourteen cases do not see it -- on this scene w >= 0.2 and 1e-7 is below float32's resolution of it -- so
test_w_eps_is_in_mw places one Gaussian at w = 1e-6, where the term is 10 % of mw: it fails with 0.10 against the formula that has it).
"""
import importlib
import math

import numpy as np
import pytest
import torch

from oracle import raster_torch
from scenes import SH_PAIRS, rel_l2
from test_preprocess_host import GRAD_BOUND, H, MODS, N, W, _inputs, _L, _params, _subsets, _twin_forward

GROUPS = ("view", "proj", "campos")


def _split(v48):
    v48 = np.asarray(v48, np.float64)
    view, proj = v48[:16].reshape(4, 4), v48[16:32].reshape(4, 4)
    return dict(view=view[:, :3], proj=proj[:, (0, 1, 3)], campos=v48[32:35]), view[:, 3], proj[:, 2], v48[35:]


def _autograd(sc, mod, w, mask, dtype=torch.float64):
    """dL/d(viewmatrix, projmatrix, campos), [48] as the C call lays it out, of the contraction of test_preprocess_host._autograd."""
    t = {k: torch.tensor(sc[k], dtype=dtype) for k in ("means3D", "shs", "scales", "rotations")}
    cam = {k: torch.tensor(sc[k], dtype=dtype, requires_grad=True) for k in ("viewmatrix", "projmatrix", "campos")}
    g = raster_torch.project(**t, **cam, image_height=sc["image_height"], image_width=sc["image_width"], tanfovx=sc["tanfovx"], tanfovy=sc["tanfovy"],
                             sh_degree=sc["sh_degree"], scale_modifier=mod)
    T = lambda a: torch.tensor(a * mask.reshape((-1,) + (1,) * (a.ndim - 1)), dtype=dtype)
    loss = (T(w["xy"]) * torch.stack([g["px"], g["py"]], 1)).sum() + (T(w["conic"]) * torch.stack(g["conic"], 1)).sum() + \
           (T(w["rgb"]) * g["rgb"]).sum() + (T(w["depth"]) * g["tz"]).sum()
    loss.backward()
    out = np.zeros(48)
    for k, o in (("viewmatrix", 0), ("projmatrix", 16), ("campos", 32)):
        gr = cam[k].grad
        if gr is not None:
            out[o:o + gr.numel()] = gr.numpy().astype(np.float64).ravel()
    return out


def _twin(p, out, w, mask):
    """fdgs_camera_grad_host on the forward twin's state with the weights `w` (masked here) as the blending backward's sums."""
    f32 = lambda a: np.ascontiguousarray(a * mask.reshape((-1,) + (1,) * (a.ndim - 1)), np.float32)
    conic_half = w["conic"] * np.array([1.0, 0.5, 1.0])           # the kernel's convention: d/d(conic_xy) arrives at half weight
    d_xy, d_conic, d_rgb, d_depth = f32(w["xy"]), f32(conic_half), f32(w["rgb"]), f32(w["depth"])
    got = np.full(48, np.nan)
    _, L = _L()
    rc = L.fdgs_camera_grad_host(p, out["tiles"].ctypes.data, out["clamped"].ctypes.data, out["cov3D"].ctypes.data, d_xy.ctypes.data,
                                 d_conic.ctypes.data, d_rgb.ctypes.data, d_depth.ctypes.data, got.ctypes.data)
    assert rc == 0, L.fdgs_last_error()
    return got


def _weights(out):
    """The seeded weights of test_preprocess_host.test_host_twin_against_the_oracles (scaled as the blending backward scales its sums)."""
    rng = np.random.default_rng(9)
    r = np.clip(out["radii"], 1, math.hypot(W, H)).astype(np.float64)
    return dict(xy=rng.standard_normal((N, 2)) / r[:, None], conic=rng.standard_normal((N, 3)) * (r * r)[:, None], rgb=rng.standard_normal((N, 3)),
                depth=rng.standard_normal(N))


def _ref_vis(sc, mod):
    with torch.no_grad():
        return raster_torch.project(**{k: torch.tensor(sc[k], dtype=torch.float64) for k in ("means3D", "shs", "scales", "rotations", "viewmatrix",
                                                                                           "projmatrix", "campos")},
                                    image_height=H, image_width=W, tanfovx=sc["tanfovx"], tanfovy=sc["tanfovy"], sh_degree=sc["sh_degree"],
                                    scale_modifier=mod)["vis"].numpy()


def _compare(tag, got, ref, groups=GROUPS):
    g, gc3, gc2, gpad = _split(got)
    r, rc3, rc2, _ = _split(ref)
    assert np.isfinite(got).all(), tag
    assert not np.any(gc3) and not np.any(gc2) and not np.any(gpad), f"{tag}: view[:, 3], proj[:, 2] and the padding are exactly 0"
    assert not np.any(rc3) and not np.any(rc2), f"{tag}: the reference's view[:, 3] / proj[:, 2]"
    errs = {k: rel_l2(g[k], r[k]) for k in groups}
    print(f"   {tag}: " + ", ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    return errs, g, r


@pytest.mark.parametrize("mod", MODS)
@pytest.mark.parametrize("M,deg", SH_PAIRS)
def test_camera_twin_against_float64_autograd(M, deg, mod):
    sc = _inputs(M, deg)
    out, p, keep = _twin_forward(sc, mod)
    w = _weights(out)
    ref_vis = _ref_vis(sc, mod)
    mask = (ref_vis & (out["tiles"] > 0)).astype(np.float64)       # (rows only one side culls -- radii on a ceil boundary -- carry no weight)
    print(f"[M={M} deg={deg} mod={mod}] camera twin vs float64 autograd, rel-L2")
    failures = []

    def hold(tag, errs):
        for k, v in errs.items():
            if not v < GRAD_BOUND:
                failures.append((tag, k, v))

    errs, g, r = _compare("all rows", _twin(p, out, w, mask), _autograd(sc, mod, w, mask))
    hold("all rows", errs)
    assert np.linalg.norm(r["view"]) > 0 and np.linalg.norm(r["proj"]) > 0
    assert (np.linalg.norm(r["campos"]) > 0) == (deg > 0)
    bits = np.stack([(out["clamped"] >> c) & 1 for c in range(3)], 1).astype(np.uint8)
    for name, rows in _subsets(sc, bits).items():
        m = mask * rows
        assert int(m.sum()) >= 1000, (name, int(m.sum()))
        errs, _, _ = _compare(f"subset {name} ({int(m.sum())} rows)", _twin(p, out, w, m), _autograd(sc, mod, w, m))
        hold(name, errs)

    # ---- single paths: the full contraction can hide a wrong small one
    zero = {k: np.zeros_like(v) for k, v in w.items()}
    # colour weights alone: campos only, the view-direction derivative of the SH colour
    got_c, ref_c = _twin(p, out, zero | dict(rgb=w["rgb"]), mask), _autograd(sc, mod, zero | dict(rgb=w["rgb"]), mask)
    errs, g, r = _compare("colour alone", got_c, ref_c, ("campos",))
    hold("colour alone", errs)
    assert not np.any(g["view"]) and not np.any(g["proj"]) and not np.any(r["view"]) and not np.any(r["proj"]), "the colour reaches a matrix"
    if deg == 0:
        assert not np.any(g["campos"]) and not np.any(r["campos"])          # (degree 0 does not depend on the direction)
    # depth weights alone: view through dtz only
    got_d, ref_d = _twin(p, out, zero | dict(depth=w["depth"]), mask), _autograd(sc, mod, zero | dict(depth=w["depth"]), mask)
    errs, g, r = _compare("depth alone", got_d, ref_d, ("view",))
    hold("depth alone", errs)
    assert not np.any(g["proj"]) and not np.any(g["campos"]) and not np.any(r["proj"]) and not np.any(r["campos"])
    assert not np.any(g["view"][:, :2]), "the depth reaches column 2 of the view matrix only"
    # conic weights alone: view through J and Rv
    got_k, ref_k = _twin(p, out, zero | dict(conic=w["conic"]), mask), _autograd(sc, mod, zero | dict(conic=w["conic"]), mask)
    errs, g, r = _compare("conic alone", got_k, ref_k, ("view",))
    hold("conic alone", errs)
    assert not np.any(g["proj"]) and not np.any(g["campos"]) and not np.any(r["proj"]) and not np.any(r["campos"])
    # the pixel-position weights reach projmatrix only
    got_x, ref_x = _twin(p, out, zero | dict(xy=w["xy"]), mask), _autograd(sc, mod, zero | dict(xy=w["xy"]), mask)
    errs, g, r = _compare("xy alone", got_x, ref_x, ("proj",))
    hold("xy alone", errs)
    assert not np.any(g["view"]) and not np.any(r["view"]) and not np.any(g["campos"])
    assert not failures, failures


def test_w_eps_is_in_mw():
    """dhom goes through mw = 1 / (w + FDGS_W_EPS).  On the scene above w >= 0.2 and the 1e-7 is below float32's resolution of it, so one
    Gaussian is put where the projection's w is 1e-6 (a projection matrix whose fourth column is scaled down; the view matrix keeps the
    depth at 2): the term changes mw by 10 %.  Only the pixel-position weights are set."""
    sc = {k: (v[:1].copy() if isinstance(v, np.ndarray) and v.shape[:1] == (N,) else v) for k, v in _inputs(16, 0).items()}
    V = np.eye(4, dtype=np.float32)
    sc["means3D"] = np.array([[0.1, -0.05, 2.0]], np.float32)
    sc["scales"] = np.full((1, 3), 0.05, np.float32)
    PM = np.eye(4, dtype=np.float32)
    PM[:, 3] = 0.0
    PM[2, 3] = 5e-7                      # w = 2.0 * 5e-7 = 1e-6
    PM[0, 0] = PM[1, 1] = 1e-7           # keeps the NDC position inside the image: x / w = 0.01
    sc["viewmatrix"], sc["projmatrix"], sc["campos"] = V, PM, np.zeros(3, np.float32)
    _lib, L = _L()
    p, keep = _params(sc, 1.0)
    tiles, clamped = np.ones(1, np.uint32), np.zeros(1, np.uint32)
    cov3D = np.array([[0.0025, 0, 0, 0.0025, 0, 0.0025]], np.float32)
    d_xy, d_conic, d_rgb = np.array([[0.7, -0.3]], np.float32), np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32)
    got = np.full(48, np.nan)
    rc = L.fdgs_camera_grad_host(p, tiles.ctypes.data, clamped.ctypes.data, cov3D.ctypes.data, d_xy.ctypes.data, d_conic.ctypes.data,
                                 d_rgb.ctypes.data, None, got.ctypes.data)
    assert rc == 0, L.fdgs_last_error()
    pos, f = sc["means3D"][0].astype(np.float64), np.float64
    ph = np.array([pos[0], pos[1], pos[2], 1.0])
    PM64 = PM.astype(f)
    hom = ph @ PM64
    expected = {}
    for eps in (1e-7, 0.0):
        mw = 1.0 / (hom[3] + eps)
        gx, gy = 0.7 * 0.5 * W, -0.3 * 0.5 * H
        dhom = np.array([gx * mw, gy * mw, 0.0, -(hom[0] * gx + hom[1] * gy) * mw * mw])
        expected[eps] = np.outer(ph, dhom)
    proj = got[16:32].reshape(4, 4)
    with_eps, without = rel_l2(proj, expected[1e-7]), rel_l2(proj, expected[0.0])
    print(f"w = 1e-6: dL/dprojmatrix against the formula with FDGS_W_EPS {with_eps:.2e}, without {without:.2e}")
    assert with_eps < 1e-5 and without > 0.05


def test_argument_validation():
    _lib, L = _L()
    sc = _inputs(16, 2)
    out, p, keep = _twin_forward(sc, 1.0)
    n = _lib.c_size_t()
    assert L.fdgs_camera_grad_scratch_bytes(-1, n) != 0 and b"bad P" in L.fdgs_last_error()
    assert L.fdgs_camera_grad_scratch_bytes(10, None) != 0 and b"NULL" in L.fdgs_last_error()
    for P, rows in ((0, 1), (1, 1), (256, 1), (257, 2), (70001, 274)):
        assert L.fdgs_camera_grad_scratch_bytes(P, n) == 0 and n.value == rows * 128
    z2, z3, res = np.zeros((N, 2), np.float32), np.zeros((N, 3), np.float32), np.zeros(48)
    args = [p, out["tiles"].ctypes.data, out["clamped"].ctypes.data, out["cov3D"].ctypes.data, z2.ctypes.data, z3.ctypes.data, z3.ctypes.data, None,
            res.ctypes.data]
    assert L.fdgs_camera_grad_host(*args) == 0 and not np.any(res)          # d_depth may be NULL; zero sums give zeros
    for hole in (1, 3, 4, 5, 6, 8):
        bad = list(args)
        bad[hole] = None
        assert L.fdgs_camera_grad_host(*bad) != 0 and b"NULL" in L.fdgs_last_error(), hole
    bad = list(args)
    bad[2] = None                                                          # clamped is needed with SH inputs
    assert L.fdgs_camera_grad_host(*bad) != 0 and b"clamped" in L.fdgs_last_error()
    assert L.fdgs_camera_grad_host(None, *args[1:]) != 0
    # the device call refuses bad arguments before it touches the device (the library loads without a GPU)
    buf = np.zeros(64, np.float32)
    a16 = (buf.ctypes.data + 15) // 16 * 16
    dev = [None, p, a16, a16, a16, a16]
    assert L.fdgs_camera_grad(None, None, a16, a16, a16, a16) != 0
    for hole in (2, 3, 4, 5):
        bad = list(dev)
        bad[hole] = None
        assert L.fdgs_camera_grad(*bad) != 0 and b"NULL" in L.fdgs_last_error(), hole
    for hole in (3, 4, 5):
        bad = list(dev)
        bad[hole] = a16 + 4
        assert L.fdgs_camera_grad(*bad) != 0 and b"aligned" in L.fdgs_last_error(), hole
    old = p.P
    p.P = -1
    assert L.fdgs_camera_grad(*dev) != 0 and b"bad P" in L.fdgs_last_error()
    assert L.fdgs_camera_grad_host(*args) != 0 and b"bad P" in L.fdgs_last_error()
    p.P = old
    # P == 0 writes zeros whatever the arrays are
    p.P = 0
    res[:] = np.nan
    assert L.fdgs_camera_grad_host(p, None, None, None, None, None, None, None, res.ctypes.data) == 0 and not np.any(res)
    p.P = old
    assert L.fdgs_abi_version() == 6 and _lib.ABI_VERSION == 6            # additions to ABI 6
