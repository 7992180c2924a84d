"""Shared by the antialiasing tests (test_antialias_host.py, test_antialias_abi.py, test_gpu_antialias.py): the opacity compensation h of
csrc/gs_math.h restated in float64 torch, and the scenes.

    A, b, C = the projected covariance before the 0.3 dilation;  a = A + 0.3, c = C + 0.3
    D0 = A C - b^2,  D1 = a c - b^2,  r = D0 / D1,  h = sqrt(max(2.5e-5, r))

`project_abc` follows oracle/raster_torch.project's conventions: a clamped view-space x (y) is detached, and the floor is a clamp_min (no
gradient at or below it).  It is written from the formulas, not from gs_math.h.

Scenes (`scene(P, W, H)`): a seeded cloud in front of the synthetic camera whose scales are drawn per class so that, among the visible
rows, at least 20 % have h < 0.9, at least 10 % have h > 0.99, at least 8 sit at the floor (footprint below about 0.03 px) and at least 8
have a clamped view-space centre -- asserted here, on the CPU, for every scene of P >= 257 (`check_scene`).  P = 1 is one sub-pixel splat
in the middle of the image (h < 0.9): one row cannot hold a distribution.  The fifth property, one Gaussian covering more than 256 tiles
(no cull mask), needs more than 256 tiles: the 100 x 52 image has 28, so it is planted and asserted in the WIDE scene (320 x 272, 340
tiles) only, which the forward, host-twin and bit-identity tests run as well.
"""
import functools
import importlib
import math

import numpy as np
import torch

from oracle import raster_torch
from scenes import raster_scene

DILATION = 0.3
FLOOR = 2.5e-5
W, H = 100, 52                     # partial tiles on both edges: 7 x 4 tiles
WIDE = (257, 320, 272)             # (P, W, H) of the scene that holds the Gaussian of more than 256 tiles
SIZES = (1, 257, 1000)
MODS = (1.0, 0.25)
KINDS = ("sh16", "sh4", "colors", "cov3d")
GRAD_BOUND = 1e-3                  # the project's gradient bound (tests/test_preprocess_host.py)
N_FLOOR = N_CLAMPED = 12


def project_abc(means3D, viewmatrix, tanfovx, tanfovy, width, height, scales=None, rotations=None, cov3D=None, scale_modifier=1.0):
    """(A, b, C, clamped): the 2D covariance before the dilation, and whether the view-space centre was clamped, per Gaussian."""
    dt = means3D.dtype
    V = viewmatrix.reshape(4, 4).to(dt)
    pv = means3D @ V[:3, :3] + V[3, :3]
    if cov3D is None:
        R = raster_torch.quat_to_rot(rotations)
        L = R * (scale_modifier * scales)[:, None, :]
        Sigma = L @ L.transpose(1, 2)
    else:
        c = cov3D
        Sigma = torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], -1).reshape(-1, 3, 3)
    fx, fy = width / (2.0 * tanfovx), height / (2.0 * tanfovy)
    tz = pv[:, 2]
    tz = torch.where(tz > 0.2, tz, torch.ones_like(tz))
    limx, limy = 1.3 * tanfovx, 1.3 * tanfovy
    txtz, tytz = pv[:, 0] / tz, pv[:, 1] / tz
    xcl, ycl = (txtz < -limx) | (txtz > limx), (tytz < -limy) | (tytz > limy)
    tx = torch.where(xcl, (txtz.clamp(-limx, limx) * tz).detach(), pv[:, 0])
    ty = torch.where(ycl, (tytz.clamp(-limy, limy) * tz).detach(), pv[:, 1])
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -(fx * tx) / (tz * tz), zero, fy / tz, -(fy * ty) / (tz * tz)], -1).reshape(-1, 2, 3)
    M = J @ V[:3, :3].t()
    cov2 = M @ Sigma @ M.transpose(1, 2)
    return cov2[:, 0, 0], cov2[:, 0, 1], cov2[:, 1, 1], xcl | ycl


def h_of(A, b, C):
    """(h, r) of the formulas above."""
    a, c = A + DILATION, C + DILATION
    r = (A * C - b * b) / (a * c - b * b)
    return torch.sqrt(torch.clamp_min(r, FLOOR)), r


def cov3d_of(sc, mod, dtype=np.float64):
    """[P,6] of Sigma = (R S)(R S)^T with S = mod * scales, in `dtype`."""
    q, s = sc["rotations"].astype(dtype), sc["scales"].astype(dtype) * dtype(mod)
    r, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                  2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    L = R * s[:, None, :]
    S = L @ L.transpose(0, 2, 1)
    return np.ascontiguousarray(np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).astype(np.float32))


def _tensors(sc, dtype, grad=False, camera_grad=False):
    g = {k: torch.tensor(sc[k], dtype=dtype, requires_grad=grad) for k in ("means3D", "scales", "rotations", "cov3D_precomp", "shs",
                                                                           "colors_precomp") if sc.get(k) is not None}
    cam = {k: torch.tensor(sc[k], dtype=dtype, requires_grad=camera_grad) for k in ("viewmatrix", "projmatrix", "campos")}
    return g, cam


def h64(sc, mod=1.0):
    """(h, r, clamped, vis) as float64 / bool numpy arrays: the compensation of every row of the scene dict `sc`."""
    with torch.no_grad():
        t, cam = _tensors(sc, torch.float64)
        A, b, C, cl = project_abc(t["means3D"], cam["viewmatrix"], sc["tanfovx"], sc["tanfovy"], sc["image_width"], sc["image_height"],
                                  t.get("scales"), t.get("rotations"), t.get("cov3D_precomp"), mod)
        h, r = h_of(A, b, C)
        vis = _project(sc, mod, t, cam)["vis"]
    return h.numpy(), r.numpy(), cl.numpy(), vis.numpy()


def _project(sc, mod, t, cam, means2D=None):
    return raster_torch.project(means3D=t["means3D"], shs=t.get("shs"), colors_precomp=t.get("colors_precomp"), scales=t.get("scales"),
                                rotations=t.get("rotations"), cov3D_precomp=t.get("cov3D_precomp"), **cam, image_height=sc["image_height"],
                                image_width=sc["image_width"], tanfovx=sc["tanfovx"], tanfovy=sc["tanfovy"], sh_degree=sc["sh_degree"],
                                scale_modifier=mod, means2D=means2D)


def autograd(sc, mod, w, mask, dtype=torch.float64, parts=("geom", "h")):
    """Gradients of
        sum_i mask_i (w_xy . (px, py) + w_conic . conic + w_rgb . rgb + w_depth tz)_i                (part "geom": raster_torch.project)
      + sum_i mask_i w_opacity_i opacity_i h_i                                                     (part "h": the restatement above)
    with respect to the per-Gaussian inputs and the three camera tensors -> ({name: float64 array}, [48] camera gradient)."""
    t, cam = _tensors(sc, dtype, grad=True, camera_grad=True)
    op = torch.tensor(sc["opacities"].reshape(-1), dtype=dtype, requires_grad=True)
    P = len(sc["means3D"])
    means2D = torch.zeros(P, 3, dtype=dtype, requires_grad=True)
    T = lambda a: torch.tensor(np.asarray(a, np.float64) * mask.reshape((-1,) + (1,) * (np.ndim(a) - 1)), dtype=dtype)
    loss = torch.zeros((), dtype=dtype)
    Sigma = None
    if "geom" in parts:
        g = _project(sc, mod, t, cam, means2D)
        Sigma = g["Sigma"]
        Sigma.retain_grad()
        loss = loss + (T(w["xy"]) * torch.stack([g["px"], g["py"]], 1)).sum() + (T(w["conic"]) * torch.stack(g["conic"], 1)).sum() + \
            (T(w["rgb"]) * g["rgb"]).sum() + (T(w["depth"]) * g["tz"]).sum()
    c6 = None
    if "h" in parts:
        # the compensation reads the covariance through a [P,6] leaf of its own, so that dL/dcov3D of its path is read in the kernel's
        # convention (off-diagonal entries carry both symmetric halves)
        if "cov3D_precomp" in t:
            c6 = t["cov3D_precomp"]
            A, b, C, _ = project_abc(t["means3D"], cam["viewmatrix"], sc["tanfovx"], sc["tanfovy"], sc["image_width"], sc["image_height"],
                                     cov3D=c6)
        else:
            R = raster_torch.quat_to_rot(t["rotations"])
            L = R * (mod * t["scales"])[:, None, :]
            S = L @ L.transpose(1, 2)
            c6 = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)
            c6.retain_grad()
            A, b, C, _ = project_abc(t["means3D"], cam["viewmatrix"], sc["tanfovx"], sc["tanfovy"], sc["image_width"], sc["image_height"],
                                     cov3D=c6)
        h, _ = h_of(A, b, C)
        loss = loss + (T(w["opacity"]) * op * h).sum()
    loss.backward()
    z = lambda v: (v.grad if v.grad is not None else torch.zeros_like(v)).detach().numpy().astype(np.float64)
    out = {k: z(v) for k, v in t.items() if k in ("means3D", "scales", "rotations", "shs")}
    out["means2D"], out["opacities"] = z(means2D), z(op)
    cov = np.zeros((P, 6))
    if Sigma is not None and Sigma.grad is not None:
        S = Sigma.grad.numpy().astype(np.float64)
        cov += np.stack([S[:, 0, 0], S[:, 0, 1] + S[:, 1, 0], S[:, 0, 2] + S[:, 2, 0], S[:, 1, 1], S[:, 1, 2] + S[:, 2, 1], S[:, 2, 2]], 1)
    if c6 is not None and c6.grad is not None and "cov3D_precomp" not in t:
        cov += c6.grad.numpy().astype(np.float64)
    if "cov3D_precomp" in t:
        cov = z(t["cov3D_precomp"])          # (the leaf itself: both parts arrive in it; Sigma's share is the same sum)
    out["cov3D"] = cov
    cam48 = np.zeros(48)
    for k, o in (("viewmatrix", 0), ("projmatrix", 16), ("campos", 32)):
        if cam[k].grad is not None:
            cam48[o:o + cam[k].numel()] = cam[k].grad.numpy().astype(np.float64).ravel()
    return out, cam48


@functools.lru_cache(maxsize=None)
def scene(P, width=W, height=H, seed=71):
    """The scene dict (numpy float32, as tests/scenes.raster_scene) of P Gaussians; read-only."""
    sc = raster_scene(max(P, 2), width, height, seed=seed, theta=20.0, extent=1.0)
    if P == 1:
        sc = {k: (v[:1].copy() if isinstance(v, np.ndarray) and v.shape[:1] == (2,) else v) for k, v in sc.items()}
        sc["means3D"][:] = 0.0
        sc["scales"][:] = np.array([0.004, 0.006, 0.005], np.float32)       # about 0.2 px at depth 4: h ~ 0.1
        sc["opacities"][:] = 0.9
        return sc
    rng = np.random.default_rng(seed + 1)
    V = sc["viewmatrix"].reshape(4, 4).astype(np.float64)
    inv = np.linalg.inv(V[:3, :3])
    world = lambda pv: ((np.asarray(pv, np.float64) - V[3, :3]) @ inv).astype(np.float32)       # p_view = p @ V[:3,:3] + V[3,:3]
    s = sc["scales"]
    cls = rng.uniform(size=P)
    lo, hi = cls < 0.4, cls > 0.7
    base = np.where(lo, rng.uniform(0.005, 0.035, P), np.where(hi, rng.uniform(0.25, 0.4, P), rng.uniform(0.04, 0.2, P)))
    k_img = W / width                                                         # (the focal length grows with the image: the same footprints in pixels)
    s[:] = (k_img * base[:, None] * rng.uniform(0.8, 1.25, (P, 3))).astype(np.float32)
    s[:N_FLOOR] = 0.0004 * k_img                                              # 0.014 px at depth 4
    sc["means3D"][:N_FLOOR] = world(np.c_[rng.uniform(-0.6, 0.6, N_FLOOR), rng.uniform(-0.3, 0.3, N_FLOOR), rng.uniform(3.5, 4.5, N_FLOOR)])
    k = slice(N_FLOOR, N_FLOOR + N_CLAMPED)
    z = rng.uniform(2.0, 4.0, N_CLAMPED)
    i = np.arange(N_CLAMPED)
    fx = np.where(i % 3 != 1, rng.choice([-1, 1], N_CLAMPED) * rng.uniform(1.4, 2.0, N_CLAMPED), rng.uniform(-0.5, 0.5, N_CLAMPED))
    fy = np.where(i % 3 != 0, rng.choice([-1, 1], N_CLAMPED) * rng.uniform(1.4, 2.0, N_CLAMPED), rng.uniform(-0.5, 0.5, N_CLAMPED))
    sc["means3D"][k] = world(np.c_[fx * sc["tanfovx"] * z, fy * sc["tanfovy"] * z, z])
    s[k] = rng.uniform(0.5, 1.2, (N_CLAMPED, 3)).astype(np.float32)          # large enough to reach the image from outside it
    if (width + 15) // 16 * ((height + 15) // 16) > 256:
        sc["means3D"][N_FLOOR + N_CLAMPED] = world([0.0, 0.0, 4.0])
        s[N_FLOOR + N_CLAMPED] = 2.0                                          # sigma ~ 220 px at 320 x 272: its square is the whole grid
    sc["shs"][::5, 0, :] -= np.float32(0.6)                                   # colour channels driven below zero
    check_scene(sc)
    return sc


def check_scene(sc, mod=1.0):
    """The composition the docstring promises, from the float64 restatement, among the visible rows."""
    h, r, cl, vis = h64(sc, mod)
    n = int(vis.sum())
    assert n >= 200, n
    assert (h[vis] < 0.9).mean() >= 0.20, (h[vis] < 0.9).mean()
    assert (h[vis] > 0.99).mean() >= 0.10, (h[vis] > 0.99).mean()
    assert int((r[vis] <= FLOOR).sum()) >= 8, int((r[vis] <= FLOOR).sum())
    assert int(cl[vis].sum()) >= 8, int(cl[vis].sum())
    gx, gy = (sc["image_width"] + 15) // 16, (sc["image_height"] + 15) // 16
    if gx * gy > 256:
        with torch.no_grad():
            t, cam = _tensors(sc, torch.float64)
            rx0, ry0, rx1, ry1 = _project(sc, mod, t, cam)["rect"]
        assert int(((rx1 - rx0) * (ry1 - ry0)).max()) > 256


def inputs(P, kind, width=W, height=H):
    """The scene with the inputs of `kind`: SH with 16 or 4 coefficients per row, colors_precomp, or cov3D_precomp (unit modifier folded in
    by the caller: `with_cov3d`)."""
    sc = dict(scene(P, width, height))
    if kind == "sh16":
        sc["sh_degree"] = 3
    elif kind == "sh4":
        sc["sh_degree"], sc["shs"] = 1, np.ascontiguousarray(sc["shs"][:, :4])
    elif kind == "colors":
        rng = np.random.default_rng(5)
        sc["colors_precomp"], sc["shs"] = rng.uniform(0.0, 1.0, (len(sc["means3D"]), 3)).astype(np.float32), None
    elif kind == "cov3d":
        sc["sh_degree"] = 3
    else:
        raise ValueError(kind)
    return sc


def with_cov3d(sc, mod):
    """`sc` with scales and rotations replaced by the covariance they give under the modifier (the rasterizer ignores the modifier then)."""
    out = dict(sc)
    out["cov3D_precomp"], out["scales"], out["rotations"] = cov3d_of(sc, mod), None, None
    return out


def weights(sc, radii, seed=9):
    """Seeded per-Gaussian sums, scaled as the blending backward scales them for a splat of radius r pixels (tests/test_preprocess_host.py):
    d/d(xy) ~ 1 / r, d/d(conic) ~ r^2; the opacity sum grows with the pixels a splat covers, ~ r^2."""
    P = len(sc["means3D"])
    rng = np.random.default_rng(seed)
    r = np.clip(radii, 1, math.hypot(sc["image_width"], sc["image_height"])).astype(np.float64)
    return dict(xy=rng.standard_normal((P, 2)) / r[:, None], conic=rng.standard_normal((P, 3)) * (r * r)[:, None],
                rgb=rng.standard_normal((P, 3)), depth=rng.standard_normal(P), opacity=rng.standard_normal(P) * r * r)


def assert_h_path_is_material(sc, mod, w, mask):
    """The compensation's share of the scales gradient (of the covariance gradient where the covariance is an input) must be above 1e-2 of
    the whole, or the 1e-3 bound could pass with the path missing."""
    whole, _ = autograd(sc, mod, w, mask)
    part, _ = autograd(sc, mod, w, mask, parts=("h",))
    k = "scales" if sc.get("scales") is not None else "cov3D"
    share = np.linalg.norm(part[k]) / np.linalg.norm(whole[k])
    assert share > 1e-2, share
    return share


def lib():
    _lib = importlib.import_module("4dgaussians_amd._lib")
    if not __import__("os").path.exists(_lib.LIB_PATH):
        importlib.import_module("4dgaussians_amd.build").build()
    return _lib, _lib.lib()


def raster_params(sc, mod):
    """(fdgs_raster_params with HOST pointers, the arrays it points at) of the scene dict."""
    _lib, _ = lib()
    P = len(sc["means3D"])
    p = _lib.RasterParams()
    p.P, p.sh_degree, p.W, p.H = P, sc["sh_degree"], sc["image_width"], sc["image_height"]
    p.sh_coeffs = 0 if sc.get("shs") is None else sc["shs"].shape[1]
    p.tanfovx, p.tanfovy, p.scale_modifier = sc["tanfovx"], sc["tanfovy"], mod
    keep = {k: np.ascontiguousarray(sc[k], np.float32) for k in ("bg", "viewmatrix", "projmatrix", "campos", "means3D", "shs", "colors_precomp",
                                                                 "opacities", "scales", "rotations", "cov3D_precomp") if sc.get(k) is not None}
    for k, a in keep.items():
        setattr(p, k, a.ctypes.data)
    return p, keep


FWD_KEYS = ("radii", "xy", "conic", "depth", "rgb", "clamped", "cov3D", "rect", "tiles")


def twin_forward(sc, mod, aa=True):
    """fdgs_preprocess_host_aa (aa) or fdgs_preprocess_host -> (outputs, params, kept arrays)."""
    _, L = lib()
    p, keep = raster_params(sc, mod)
    P = p.P
    out = dict(radii=np.full(P, -1, np.int32), xy=np.full((P, 2), np.nan, np.float32), conic=np.full((P, 3), np.nan, np.float32),
               depth=np.full(P, np.nan, np.float32), rgb=np.full((P, 3), np.nan, np.float32), clamped=np.full(P, 99, np.uint32),
               cov3D=np.full((P, 6), np.nan, np.float32), rect=np.full((P, 2), 99, np.uint32), tiles=np.full(P, 99, np.uint32))
    args = [out[k].ctypes.data for k in FWD_KEYS]
    if aa:
        out["opacity_eff"] = np.full(P, np.nan, np.float32)
        rc = L.fdgs_preprocess_host_aa(p, *args, out["opacity_eff"].ctypes.data)
    else:
        rc = L.fdgs_preprocess_host(p, *args)
    assert rc == 0, L.fdgs_last_error()
    return out, p, keep


def sums_f32(w, mask):
    """The weights as the float32 arrays the twins and the kernels take (the conic's xy entry at half weight)."""
    f32 = lambda a: np.ascontiguousarray(a * mask.reshape((-1,) + (1,) * (a.ndim - 1)), np.float32)
    return dict(xy=f32(w["xy"]), conic=f32(w["conic"] * np.array([1.0, 0.5, 1.0])), rgb=f32(w["rgb"]), depth=f32(w["depth"]),
                opacity=f32(w["opacity"]))


BWD_KEYS = ("means2D", "means3D", "shs", "scales", "rotations", "cov3D")


def twin_backward(p, out, s, M, aa=True):
    """fdgs_preprocess_bwd_host_aa (aa) or fdgs_preprocess_bwd_host on the forward twin's state with the float32 sums `s`."""
    _, L = lib()
    P = p.P
    got = dict(means2D=np.full((P, 3), np.nan, np.float32), means3D=np.full((P, 3), np.nan, np.float32),
               shs=np.full((P, max(M, 1), 3), np.nan, np.float32), scales=np.full((P, 3), np.nan, np.float32),
               rotations=np.full((P, 4), np.nan, np.float32), cov3D=np.full((P, 6), np.nan, np.float32))
    head = (p, out["tiles"].ctypes.data, out["clamped"].ctypes.data, out["cov3D"].ctypes.data, s["xy"].ctypes.data, s["conic"].ctypes.data,
            s["rgb"].ctypes.data, s["depth"].ctypes.data)
    outs = [got[k].ctypes.data for k in BWD_KEYS]
    if aa:
        got["opacities"] = np.full(P, np.nan, np.float32)
        rc = L.fdgs_preprocess_bwd_host_aa(*head, s["opacity"].ctypes.data, *outs, got["opacities"].ctypes.data)
    else:
        rc = L.fdgs_preprocess_bwd_host(*head, *outs)
    assert rc == 0, L.fdgs_last_error()
    return got


def twin_camera(p, out, s, aa=True):
    _, L = lib()
    got = np.full(48, np.nan)
    head = (p, out["tiles"].ctypes.data, out["clamped"].ctypes.data, out["cov3D"].ctypes.data, s["xy"].ctypes.data, s["conic"].ctypes.data,
            s["rgb"].ctypes.data, s["depth"].ctypes.data)
    rc = L.fdgs_camera_grad_host_aa(*head, s["opacity"].ctypes.data, got.ctypes.data) if aa else L.fdgs_camera_grad_host(*head, got.ctypes.data)
    assert rc == 0, L.fdgs_last_error()
    return got


def ulps(a, b):
    """|a - b| in units of the float32 spacing at b (b float64: the reference)."""
    b32 = np.asarray(b, np.float64).astype(np.float32)
    sp = np.spacing(np.abs(b32)).astype(np.float64)
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / sp
