"""The projection arithmetic of csrc/gs_math.h executed WITHOUT a GPU: fdgs_preprocess_host / fdgs_preprocess_bwd_host (csrc/preprocess.hip) loop
over the Gaussians on the CPU around the very functions the two projection kernels call.

Forward: against the float32 RasterOracle's per-Gaussian fields at the tolerances of tests/test_gpu_raster_settings.py.  Backward: against
float64 autograd through oracle/raster_torch.project, both contracted with the same seeded per-Gaussian weights, at the project's gradient
bound rel-L2 < 1e-3 -- over all rows and separately over the rows whose view-space centre is clamped ("frustum"), the rows with a colour
channel clamped at 0 ("colour") and the rest ("plain").

100 000 seeded Gaussians (extent 3.0) around a camera that sits at the origin, inside the cloud, with planted rows: behind the camera, view depth exactly 0.2 (culled) and
one float above it (visible), centres beyond the frustum clamp with large scales, scales of 0 and of 1e3, colour channels driven negative.

How much of the 1e-3 is the reference's own -- a FLOAT32 evaluation of raster_torch.project against the float64 one, same weights (printed
by the test; maxima over the fourteen cases): means2D 3.5e-08, means3D 4.7e-07, shs 8.7e-08, scales 6.1e-07, rotations 4.8e-07, cov3D 2.1e-07,
all without the planted row one float above the near plane.  WITH it the float32 evaluation is off by 7.4e-2 on means3D, 0.12 .. 0.14 on scales,
up to 8.0e-3 on rotations and 4.5e-2 on cov3D: its matrix product rounds that row's depth to 0.2 and culls the row, which carries a large
share of those gradients' norm (a splat 0.2 in front of the camera).  That is the float32 evaluation's fault, not the float64 reference's.
The twin keeps the row and measured, against float64 (maxima over the cases): means2D 3.5e-08, means3D 4.9e-07, shs 8.9e-08, scales 6.3e-07,
rotations 6.7e-07, cov3D 1.7e-07 over all rows; every subset figure <= 1.2e-06.  Each subset holds 1 232 .. 21 348 rows with a gradient.

A second contraction carries the colour weights alone: dL/dmeans3D is then the view-direction derivative of the SH colour (the second half of
sh_bwd), which in the full contraction is about 1e-3 of |dL/dmeans3D| and could be wrong without exceeding the bound.  Measured there:
means3D <= 1.4e-07, shs <= 9.0e-08.

The test was checked against seven deliberate faults in a scratch copy of gs_math.h: the modifier applied once in cov3d_bwd; the x, then the y
clamp flag of project_bwd ignored; the colour clamp mask of sh_bwd ignored; a wrong term in SH basis 6 -- each fails it by 0.2 and more --;
and, in the direction derivative of sh_bwd, 4 z for 2 z in the degree-2 term of ddz and the degree-1 term of ddz halved, which only the
colour-only contraction sees (0.12 .. 0.29 on means3D; the full contraction reads 3e-4 .. 5e-4 with them).
"""
import functools
import importlib
import math

import numpy as np
import pytest
import torch

from oracle import raster_torch
from oracle.raster_oracle import RasterOracle
from scenes import raster_scene, rel_l2
from test_gpu_raster import _radii_mismatches_sit_on_a_ceil_boundary
from scenes import SH_PAIRS

N, W, H = 100_000, 200, 152
MODS = (0.6, 1.7)
GRAD_BOUND = 1e-3
PLANTED = dict(behind=slice(0, 10), at_near=10, above_near=11, beyond_clamp=slice(12, 32), scale_zero=slice(32, 36), scale_huge=slice(36, 40))


def _L():
    _lib = importlib.import_module("4dgaussians_amd._lib")
    return _lib, _lib.lib()


def _depth_f32(V, p):
    """View depth as gs_math.h's view_xform and the oracle evaluate it in float32 without contraction: ((v2 x + v6 y) + v10 z) + v14."""
    f, V = np.float32, np.asarray(V).reshape(16)
    return ((f(V[2]) * p[..., 0].astype(f) + f(V[6]) * p[..., 1].astype(f)) + f(V[10]) * p[..., 2].astype(f)) + f(V[14])


@functools.lru_cache(maxsize=None)
def _scene():
    sc = raster_scene(N, W, H, seed=51, theta=25.0, extent=3.0, scale_boost=4.0)
    sc["bg"] = np.array([0.9, 0.1, 0.4], np.float32)
    rng = np.random.default_rng(52)
    # the synthetic camera's rotation and projection, moved to the origin: the camera sits INSIDE the cloud (rows behind it, rows beyond the
    # clamp on every side), and near the plane z = 0.2 the terms of the view depth are as small as the depth, so that a float32 depth of
    # exactly 0.2 can be met (4 away from the origin the last addition lands on multiples of 2^-22 only)
    V = sc["viewmatrix"].reshape(4, 4).astype(np.float64)
    proj_only = np.linalg.inv(V) @ sc["projmatrix"].reshape(4, 4).astype(np.float64)
    V[3, :3] = 0.0
    sc["viewmatrix"], sc["projmatrix"] = V.astype(np.float32), (V @ proj_only).astype(np.float32)
    sc["campos"] = np.zeros(3, np.float32)
    V = sc["viewmatrix"].astype(np.float64)
    inv = np.linalg.inv(V[:3, :3])
    world = lambda pv: ((np.asarray(pv, np.float64) - V[3, :3]) @ inv).astype(np.float32)       # p_view = p @ V[:3,:3] + V[3,:3]
    tx, ty = sc["tanfovx"], sc["tanfovy"]
    m, s = sc["means3D"], sc["scales"]
    # behind the camera
    m[PLANTED["behind"]] = world(np.c_[rng.uniform(-0.5, 0.5, (10, 2)), -rng.uniform(0.3, 4.0, 10)])
    # on the near plane: candidates with view depth 0.2 in exact arithmetic; keep one whose FLOAT32 depth is exactly 0.2f (culled: the test is
    # z <= 0.2) and one whose float32 depth is the next float above (visible)
    cand = world(np.c_[rng.uniform(-0.02, 0.02, (200000, 2)), np.full(200000, 0.2)])
    d = _depth_f32(sc["viewmatrix"], cand)
    near, above = np.float32(0.2), np.nextafter(np.float32(0.2), np.float32(1.0))
    m[PLANTED["at_near"]] = cand[np.nonzero(d == near)[0][0]]
    m[PLANTED["above_near"]] = cand[np.nonzero(d == above)[0][0]]
    s[[PLANTED["at_near"], PLANTED["above_near"]]] = 0.01
    # centres beyond the +-1.3 tanfov clamp, in x, in y and in both, with splats large enough to reach the image
    z = rng.uniform(1.0, 4.0, 20)
    fx = np.where(np.arange(20) % 3 != 1, rng.choice([-1, 1], 20) * rng.uniform(1.5, 3.0, 20), rng.uniform(-0.5, 0.5, 20))
    fy = np.where(np.arange(20) % 3 != 0, rng.choice([-1, 1], 20) * rng.uniform(1.5, 3.0, 20), rng.uniform(-0.5, 0.5, 20))
    m[PLANTED["beyond_clamp"]] = world(np.c_[fx * tx * z, fy * ty * z, z])
    s[PLANTED["beyond_clamp"]] = rng.uniform(1.0, 3.0, (20, 3)).astype(np.float32)
    # scales of 0 and of 1e3 in front of the camera
    for key, val in (("scale_zero", 0.0), ("scale_huge", 1e3)):
        m[PLANTED[key]] = world(np.c_[rng.uniform(-0.3, 0.3, (4, 2)), rng.uniform(1.0, 3.0, 4)])
        s[PLANTED[key]] = val
    # colour channels driven negative
    sc["shs"][::7, 0, :] -= np.float32(1.5)
    return sc


def _inputs(M, deg):
    sc = dict(_scene())
    sc["sh_degree"] = deg
    sc["shs"] = np.ascontiguousarray(sc["shs"][:, :M])
    return sc


def _params(sc, mod):
    _lib, _ = _L()
    P = len(sc["means3D"])
    p = _lib.RasterParams()
    p.P, p.sh_degree, p.sh_coeffs, p.W, p.H = P, sc["sh_degree"], sc["shs"].shape[1], sc["image_width"], sc["image_height"]
    p.tanfovx, p.tanfovy, p.scale_modifier = sc["tanfovx"], sc["tanfovy"], mod
    keep = {k: np.ascontiguousarray(sc[k], np.float32) for k in ("bg", "viewmatrix", "projmatrix", "campos", "means3D", "shs", "opacities", "scales",
                                                                 "rotations")}
    for k, a in keep.items():
        setattr(p, k, a.ctypes.data)
    return p, keep


def _twin_forward(sc, mod):
    _, L = _L()
    p, keep = _params(sc, mod)
    P = p.P
    out = dict(radii=np.full(P, -1, np.int32), xy=np.full((P, 2), np.nan, np.float32), conic=np.full((P, 3), np.nan, np.float32),
               depth=np.full(P, np.nan, np.float32), rgb=np.full((P, 3), np.nan, np.float32), clamped=np.full(P, 99, np.uint32),
               cov3D=np.full((P, 6), np.nan, np.float32), rect=np.full((P, 2), 99, np.uint32), tiles=np.full(P, 99, np.uint32))
    rc = L.fdgs_preprocess_host(p, *(out[k].ctypes.data for k in ("radii", "xy", "conic", "depth", "rgb", "clamped", "cov3D", "rect", "tiles")))
    assert rc == 0, L.fdgs_last_error()
    return out, p, keep


def _subsets(sc, clamped):
    V = sc["viewmatrix"].reshape(4, 4).astype(np.float64)
    pv = sc["means3D"].astype(np.float64) @ V[:3, :3] + V[3, :3]
    tz = np.where(pv[:, 2] == 0, 1e-30, pv[:, 2])
    frustum = (np.abs(pv[:, 0] / tz) > 1.3 * sc["tanfovx"]) | (np.abs(pv[:, 1] / tz) > 1.3 * sc["tanfovy"])
    colour = clamped.reshape(len(frustum), 3).any(axis=1)
    return {"frustum": frustum, "colour": colour, "plain": ~frustum & ~colour}


def _autograd(sc, mod, w, mask, dtype):
    """Gradients of sum_i mask_i (w_xy . (px, py) + w_conic . conic + w_rgb . rgb + w_depth tz)_i through raster_torch.project in `dtype`."""
    t = {k: torch.tensor(sc[k], dtype=dtype, requires_grad=True) for k in ("means3D", "shs", "scales", "rotations")}
    means2D = torch.zeros(len(sc["means3D"]), 3, dtype=dtype, requires_grad=True)
    cam = {k: torch.tensor(sc[k], dtype=dtype) for k in ("viewmatrix", "projmatrix", "campos")}
    g = raster_torch.project(**t, **cam, image_height=sc["image_height"], image_width=sc["image_width"], tanfovx=sc["tanfovx"], tanfovy=sc["tanfovy"],
                             sh_degree=sc["sh_degree"], scale_modifier=mod, means2D=means2D)
    g["Sigma"].retain_grad()
    T = lambda a: torch.tensor(a * mask.reshape((-1,) + (1,) * (a.ndim - 1)), dtype=dtype)
    loss = (T(w["xy"]) * torch.stack([g["px"], g["py"]], 1)).sum() + (T(w["conic"]) * torch.stack(g["conic"], 1)).sum() + \
           (T(w["rgb"]) * g["rgb"]).sum() + (T(w["depth"]) * g["tz"]).sum()
    loss.backward()
    S = g["Sigma"].grad if g["Sigma"].grad is not None else torch.zeros_like(g["Sigma"])      # (a contraction may not reach an input: zeros)
    cov = torch.stack([S[:, 0, 0], S[:, 0, 1] + S[:, 1, 0], S[:, 0, 2] + S[:, 2, 0], S[:, 1, 1], S[:, 1, 2] + S[:, 2, 1], S[:, 2, 2]], 1)
    out = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy().astype(np.float64) for k, v in t.items()}
    out["means2D"], out["cov3D"] = means2D.grad.numpy().astype(np.float64), cov.numpy().astype(np.float64)
    return out, g["vis"].numpy()


def _twin_backward(p, out, w, mask, M):
    """fdgs_preprocess_bwd_host on the forward twin's state with the weights `w` (float64, masked here) as the blending backward's sums."""
    f32 = lambda a: np.ascontiguousarray(a * mask.reshape((-1,) + (1,) * (a.ndim - 1)), np.float32)
    conic_half = w["conic"] * np.array([1.0, 0.5, 1.0])           # the kernel's convention: d/d(conic_xy) arrives at half weight
    d_xy, d_conic, d_rgb, d_depth = f32(w["xy"]), f32(conic_half), f32(w["rgb"]), f32(w["depth"])
    got = dict(means2D=np.full((N, 3), np.nan, np.float32), means3D=np.full((N, 3), np.nan, np.float32), shs=np.full((N, M, 3), np.nan, np.float32),
               scales=np.full((N, 3), np.nan, np.float32), rotations=np.full((N, 4), np.nan, np.float32), cov3D=np.full((N, 6), np.nan, np.float32))
    _, L = _L()
    rc = L.fdgs_preprocess_bwd_host(p, out["tiles"].ctypes.data, out["clamped"].ctypes.data, out["cov3D"].ctypes.data, d_xy.ctypes.data,
                                    d_conic.ctypes.data, d_rgb.ctypes.data, d_depth.ctypes.data,
                                    *(got[k].ctypes.data for k in ("means2D", "means3D", "shs", "scales", "rotations", "cov3D")))
    assert rc == 0, L.fdgs_last_error()
    return got


def test_planted_rows_are_what_they_claim():
    sc = _scene()
    d = _depth_f32(sc["viewmatrix"], sc["means3D"])
    assert np.all(d[PLANTED["behind"]] < 0)
    assert d[PLANTED["at_near"]] == np.float32(0.2) and d[PLANTED["above_near"]] == np.nextafter(np.float32(0.2), np.float32(1.0))
    out, _, _ = _twin_forward(_inputs(16, 2), 0.6)
    r = out["radii"]
    assert np.all(r[PLANTED["behind"]] == 0) and r[PLANTED["at_near"]] == 0
    assert r[PLANTED["above_near"]] > 0 and out["depth"][PLANTED["above_near"]] == np.nextafter(np.float32(0.2), np.float32(1.0))
    sub = _subsets(sc, np.zeros((N, 3), np.uint8))
    assert np.all(sub["frustum"][PLANTED["beyond_clamp"]]) and np.all(r[PLANTED["beyond_clamp"]] > 0)
    assert np.all(r[PLANTED["scale_zero"]] > 0) and np.all(r[PLANTED["scale_huge"]] > 0)
    assert np.all(out["cov3D"][PLANTED["scale_zero"]] == 0)


@pytest.mark.parametrize("mod", MODS)
@pytest.mark.parametrize("M,deg", SH_PAIRS)
def test_host_twin_against_the_oracles(M, deg, mod):
    sc = _inputs(M, deg)
    out, p, keep = _twin_forward(sc, mod)
    o = RasterOracle(**sc, scale_modifier=mod)

    # ---- forward against the float32 oracle's fields
    radii = out["radii"]
    _radii_mismatches_sit_on_a_ceil_boundary(sc | dict(scale_modifier=mod), radii, o)      # (covers culled-or-visible: a radius of 0 against r > 1 fails it)
    differ = radii != o.radii
    assert np.array_equal((radii > 0)[~differ], (o.radii > 0)[~differ]) and differ.mean() < 2e-4
    ok = ~differ & (o.radii > 0)
    assert ok.sum() > 10000
    culled = radii == 0
    for k in ("xy", "conic", "depth", "rgb", "cov3D", "clamped", "rect", "tiles"):
        assert not np.any(out[k][culled]), f"{k}: a culled row is not zero"
    np.testing.assert_allclose(out["xy"][ok], o.field("xy")[ok], rtol=0, atol=2e-3)
    co = o.field("conic_opacity")
    assert rel_l2(out["conic"][ok, :2], co[ok, :2]) < 1e-5 and rel_l2(out["conic"][ok, 2], co[ok, 2]) < 1e-5
    np.testing.assert_allclose(out["depth"][ok], o.field("depth")[ok], rtol=1e-6)
    np.testing.assert_allclose(out["rgb"][ok], o.field("rgb")[ok], rtol=0, atol=1e-5)
    ref_cov = o.field("cov3D")[ok]
    assert (np.abs(out["cov3D"][ok] - ref_cov) / np.maximum(np.abs(ref_cov).max(axis=1, keepdims=True), 1e-30)).max() < 1e-5
    assert np.array_equal(out["tiles"][ok].astype(np.int64), o.field("tiles_touched")[ok].astype(np.int64))
    rect = out["rect"][ok]
    assert np.array_equal(np.stack([rect[:, 0] & 0xFFFF, rect[:, 0] >> 16, rect[:, 1] & 0xFFFF, rect[:, 1] >> 16], 1), o.field("rect")[ok])
    bits = np.stack([(out["clamped"] >> c) & 1 for c in range(3)], 1).astype(np.uint8)
    rgb_ref = o.field("rgb")
    sure = ok[:, None] & ((rgb_ref > 1e-5) | o.field("clamped").astype(bool))          # (a channel within the colour tolerance of 0 may fall on either side)
    assert np.array_equal(bits[sure], o.field("clamped")[sure]) and (ok[:, None] & ~sure).mean() < 1e-3

    # ---- backward against float64 autograd through raster_torch.project, same weights
    # seeded per-Gaussian weights, scaled as the blending backward scales its sums for a splat of radius r pixels (d/d(xy) ~ conic * dx ~ 1/r,
    # d/d(conic) ~ dx^2 ~ r^2): with unscaled weights the position path outweighs the conic path in dL/dmeans3D by 1e4 and more, and the
    # frustum clamp flags of project_bwd, which act on the conic path alone, could be ignored without this test noticing
    rng = np.random.default_rng(9)
    # r stops at the image diagonal, as dx does.  (The planted splats of scale 1e3 have r ~ 3e5 and a cov2D determinant ~ 1e21: its square
    # overflows float32, k = 1 / (det^2 + 1e-7) is 0 and project_bwd gives their conic path exactly no gradient -- the float32 behaviour of the
    # reference's formula, Appendix B.5 (i) -- where float64 keeps ~ 1e-21; a weight of r^2 = 1e11 would make the test about that.)
    r = np.clip(out["radii"], 1, math.hypot(W, H)).astype(np.float64)
    w = dict(xy=rng.standard_normal((N, 2)) / r[:, None], conic=rng.standard_normal((N, 3)) * (r * r)[:, None], rgb=rng.standard_normal((N, 3)),
             depth=rng.standard_normal(N))
    with torch.no_grad():
        ref_vis = raster_torch.project(**{k: torch.tensor(sc[k], dtype=torch.float64) for k in ("means3D", "shs", "scales", "rotations", "viewmatrix",
                                                                                              "projmatrix", "campos")},
                                       image_height=H, image_width=W, tanfovx=sc["tanfovx"], tanfovy=sc["tanfovy"], sh_degree=deg,
                                       scale_modifier=mod)["vis"].numpy()
    mask = (ref_vis & (out["tiles"] > 0)).astype(np.float64)       # (rows only one side culls -- radii on a ceil boundary -- carry no weight)
    assert (ref_vis != (out["tiles"] > 0)).mean() < 2e-4
    ref, _ = _autograd(sc, mod, w, mask, torch.float64)
    got = _twin_backward(p, out, w, mask, M)
    for k, a in got.items():
        assert np.isfinite(a).all(), k
        assert not np.any(a[out["tiles"] == 0]), f"{k}: a row without tiles received a gradient"
    assert not np.any(got["shs"][:, (deg + 1) ** 2:]), "an inactive SH band received a gradient"
    errs = {k: rel_l2(got[k], ref[k].reshape(got[k].shape)) for k in got}
    print(f"[M={M} deg={deg} mod={mod}] twin vs float64 autograd, rel-L2: " + ", ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    subsets = _subsets(sc, o.field("clamped"))
    live = np.zeros(N, bool)
    for k, a in ref.items():
        live |= np.abs(a.reshape(N, -1)).sum(axis=1) > 0
    sub_errs = {}
    for name, rows in subsets.items():
        n = int((rows & live).sum())
        assert n >= 1000, (name, n)
        sub_errs[name] = {k: rel_l2(got[k][rows], ref[k].reshape(got[k].shape)[rows]) for k in got}
        print(f"   subset {name}: {n} rows with a gradient: " + ", ".join(f"{k}={v:.2e}" for k, v in sub_errs[name].items()))
    own, _ = _autograd(sc, mod, w, mask, torch.float32)
    print("   float32 autograd vs float64 autograd (the reference's own): " + ", ".join(f"{k}={rel_l2(own[k], ref[k]):.2e}" for k in ref))
    rest = np.ones(N, bool)
    rest[PLANTED["above_near"]] = False
    print("   ... without the row one float above the near plane: " + ", ".join(f"{k}={rel_l2(own[k][rest], ref[k][rest]):.2e}" for k in ref))
    for k, v in errs.items():
        assert v < GRAD_BOUND, (k, v)
    for name, e in sub_errs.items():
        for k, v in e.items():
            assert v < GRAD_BOUND, (name, k, v)


    # ---- the colour path alone: only w_rgb is non-zero, so dL/dmeans3D is the view-direction derivative of the SH colour (the second half of
    # sh_bwd) and nothing else.  In the full contraction above that path is about 1e-3 of |dL/dmeans3D|: a fault in it would pass the bound
    zero = {k: np.zeros_like(v) for k, v in w.items()}
    w_rgb = zero | dict(rgb=w["rgb"])
    ref_c, _ = _autograd(sc, mod, w_rgb, mask, torch.float64)
    got_c = _twin_backward(p, out, w_rgb, mask, M)
    for k in ("means2D", "scales", "rotations", "cov3D"):
        assert not np.any(got_c[k]) and not np.any(ref_c[k]), f"{k}: the colour reaches it"
    assert not np.any(got_c["shs"][:, (deg + 1) ** 2:])
    if deg == 0:
        assert not np.any(got_c["means3D"]) and not np.any(ref_c["means3D"])        # (degree 0 does not depend on the direction)
    else:
        assert int((np.abs(ref_c["means3D"]).sum(axis=1) > 0).sum()) > 10000
    errs_c = {k: rel_l2(got_c[k], ref_c[k].reshape(got_c[k].shape)) for k in ("means3D", "shs")}
    print(f"   colour path alone: " + ", ".join(f"{k}={v:.2e}" for k, v in errs_c.items()))
    for name, rows in subsets.items():
        e = {k: rel_l2(got_c[k][rows], ref_c[k].reshape(got_c[k].shape)[rows]) for k in ("means3D", "shs")}
        print(f"   colour path alone, subset {name}: " + ", ".join(f"{k}={v:.2e}" for k, v in e.items()))
        for k, v in e.items():
            assert v < GRAD_BOUND, ("colour path", name, k, v)
    for k, v in errs_c.items():
        assert v < GRAD_BOUND, ("colour path", k, v)
