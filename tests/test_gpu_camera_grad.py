"""The camera's gradient on the device: fdgs_camera_grad (csrc/preprocess.hip), its autograd wiring in GaussianRasterizer and render(), and
a pose fitted through it.  Run with -m gpu on MI355X.

1. The kernel against float64 autograd through raster_torch.project and against its host twin, on the 100 000-row scene of
   tests/test_preprocess_host.py with a synthetic accumulator written in the packed layout of render.hip, at P = 100 000, 70 001, 257, 63, 1
   (more partial rows than the second launch has threads; a ragged last wave) and P = 0; two runs are bit-equal.
2. The whole backward through GaussianRasterizer against float64 autograd through the dense raster_torch.rasterize, small scene.
3. The translation identity from device outputs alone.  Moving the camera and every Gaussian by the same delta changes nothing, so for
   r = 0..2:  sum_i dL/dmeans3D_i[r] + dcampos[r] - sum_c V[r,c] dV[3,c] - sum_c PM[r,c] dPM[3,c] = 0.  The residual is reported relative
   to sum_i |dL/dmeans3D_i[r]|.  Its bound is 8 x the same ratio of a FLOAT32 run of raster_torch.project's autograd on the same plain
   raster_scene (CPU, _identity_float32_figure below; its float64 value is rounding of double): measured 2.0e-09 in float32 (9.0e-17 in
   float64), so the bound is 1.6e-08; the factor 8 covers the device's contraction and its different summation order.
   The device measured, largest axis, six runs (the accumulator's atomic order differs from run to run, and the rounding with it):
   2.0e-09, 4.6e-09, 2.0e-09, 6.3e-09, 5.1e-09, 4.5e-09.  With the second launch adding its rows in float the same test read 2.0e-09 in one run
   and 1.6e-08 (over the bound) in the next: the launch adds in double since.
4. render(): the fused node against the two-node form, both with camera leaves, and the model's gradients against a run without them.
5. Pose recovery: a PoseDelta 2 degrees and 0.05 units off is fitted with Adam through GaussianRasterizer, all Gaussians frozen, against
   the same fit through raster_torch.rasterize in float64 on the CPU: reference 0.0350 degrees / 0.00175 after 200 steps, device the same
   to the digits printed.

Measured rel-L2 (bound 1e-3): kernel against float64 autograd <= 6.4e-07 over the five sizes, against its twin <= 9.7e-07; whole backward view
1.0e-04, proj 1.7e-04, campos 1.9e-05; render() camera gradients fused against two-node 4.5e-07, model gradients with against without
camera leaves 6.2e-07 (bound 2e-5).
"""
import ctypes
import functools
import importlib
import math

import numpy as np
import pytest
import torch

from oracle import raster_torch
from scenes import raster_scene, rel_l2
import test_camera_grad_host as TH
import test_preprocess_host as TP
from test_gpu_raster import _dev_field

pytestmark = pytest.mark.gpu
GRAD_BOUND = 1e-3            # the project's gradient bound
CAM_KEYS = ("viewmatrix", "projmatrix", "campos")


def _mod():
    return importlib.import_module("4dgaussians_amd")


def _settings(sc, dev, leaves=False, scale_modifier=1.0, dtype=torch.float32):
    R = _mod().rasterizer
    cam = {k: torch.tensor(np.asarray(sc[k]), device=dev, dtype=dtype).requires_grad_(leaves) for k in CAM_KEYS}
    return R.GaussianRasterizationSettings(image_height=sc["image_height"], image_width=sc["image_width"], tanfovx=sc["tanfovx"], tanfovy=sc["tanfovy"],
                                           bg=torch.tensor(sc["bg"], device=dev), scale_modifier=scale_modifier, sh_degree=sc["sh_degree"],
                                           prefiltered=False, debug=False, **cam)


def _groups(view, proj, campos):
    view, proj = np.asarray(view, np.float64).reshape(4, 4), np.asarray(proj, np.float64).reshape(4, 4)
    return dict(view=view[:, :3], proj=proj[:, (0, 1, 3)], campos=np.asarray(campos, np.float64).reshape(3)), view[:, 3], proj[:, 2]


# ---- 1. the kernel on a synthetic accumulator -----------------------------------------------------------------------------------------

M_DEG, MOD = (16, 2), 0.6


def _slice_scene(start, P):
    sc = dict(TP._inputs(*M_DEG))
    for k in ("means3D", "shs", "opacities", "scales", "rotations"):
        sc[k] = np.ascontiguousarray(sc[k][start:start + P])
    return sc


@functools.lru_cache(maxsize=None)
def _full_forward():
    return TP._twin_forward(TP._inputs(*M_DEG), MOD)[0]


@functools.lru_cache(maxsize=None)
def _full_weights():
    """The seeded per-row weights of the host tests for all 100 000 rows; a slice of the scene takes the rows' own."""
    return TH._weights(_full_forward())


def _first_visible_row():
    """Where the small slices start: the first row behind the planted ones whose centre lies in the image with a radius of 2 pixels and more
    (its centre pixel passes the alpha test, so the exact tile culling keeps a tile and the row takes a gradient)."""
    o = _full_forward()
    ok = (o["tiles"] > 0) & (o["radii"] >= 2) & (o["xy"][:, 0] > 1) & (o["xy"][:, 0] < TP.W - 2) & (o["xy"][:, 1] > 1) & (o["xy"][:, 1] < TP.H - 2)
    return int(np.nonzero(ok[40:])[0][0]) + 40


def _device_camera_grad(sc, acc_np, dev):
    """fdgs_preprocess_fwd on `sc`, then fdgs_camera_grad on the accumulator `acc_np` [P,16] -> ([48] twice, tiles != 0 [P], radii > 0 [P])."""
    fd = _mod()
    R, L = fd.rasterizer, fd._lib.lib()
    t = {k: torch.tensor(sc[k], device=dev) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    p, keep = R._frame_params(_settings(sc, dev, scale_modifier=MOD), t["means3D"], t["shs"], None, t["opacities"], t["scales"], t["rotations"], None)
    P = p.P
    geom = torch.empty(R._bytes(L, "geom", P), dtype=torch.uint8, device=dev)
    radii = torch.empty(P, dtype=torch.int32, device=dev)
    st = fd._lib.stream_ptr()
    fd._lib.check(L.fdgs_preprocess_fwd(st, p, fd._lib.ptr(geom), fd._lib.ptr(radii)))
    acc = torch.tensor(acc_np, device=dev)
    nbytes = fd._lib.c_size_t()
    fd._lib.check(L.fdgs_camera_grad_scratch_bytes(P, nbytes))
    assert nbytes.value == max(1, (P + 255) // 256) * 128
    outs = []
    for _ in range(2):
        scratch = torch.full((nbytes.value // 4,), float("nan"), device=dev)
        out = torch.full((48,), float("nan"), device=dev)
        fd._lib.check(L.fdgs_camera_grad(st, p, fd._lib.ptr(geom), fd._lib.ptr(acc), fd._lib.ptr(scratch), fd._lib.ptr(out)))
        outs.append(out)
    torch.cuda.synchronize()
    q = ctypes.c_void_p()
    fd._lib.check(L.fdgs_geom_field(fd._lib.ptr(geom), P, 5, ctypes.byref(q)))          # tiles_touched u32[P]: what the kernel's activity test reads
    tiles = _dev_field(lambda: q.value, (P,), torch.int32, dev)
    return outs, tiles != 0, radii.cpu().numpy() > 0


@pytest.mark.parametrize("P", [100_000, 70_001, 257, 63, 1])
def test_kernel_against_twin_and_float64_autograd(P):
    dev = torch.device("cuda:0")
    start = 0 if P > 1000 else _first_visible_row()
    sc = _slice_scene(start, P)
    out, p_host, keep = TP._twin_forward(sc, MOD)
    w = {k: v[start:start + P] for k, v in _full_weights().items()}
    with torch.no_grad():
        ref_vis = raster_torch.project(**{k: torch.tensor(sc[k], dtype=torch.float64) for k in ("means3D", "shs", "scales", "rotations", "viewmatrix",
                                                                                              "projmatrix", "campos")},
                                       image_height=TP.H, image_width=TP.W, tanfovx=sc["tanfovx"], tanfovy=sc["tanfovy"], sh_degree=M_DEG[1],
                                       scale_modifier=MOD)["vis"].numpy()
    # a first device pass only to learn which rows the device's activity test lets through: tiles != 0, where the device's count is that of
    # the exact tile culling (csrc/gs_math.h) -- a visible row whose ellipse reaches no tile has none and takes no gradient in a real frame
    zeros = np.zeros((P, 16), np.float32)
    _, dev_tiles, dev_vis = _device_camera_grad(sc, zeros, dev)
    mask = (ref_vis & (out["tiles"] > 0) & dev_tiles).astype(np.float64)
    assert not np.any(dev_tiles & ~dev_vis) and (ref_vis != dev_vis).sum() <= max(1, 2e-4 * P)     # (radii on a ceil boundary may cull on one side only)
    assert mask.sum() >= max(1, 0.05 * P if P > 1000 else 1), mask.sum()
    m = lambda a: (a * mask.reshape((-1,) + (1,) * (a.ndim - 1))).astype(np.float32)
    acc = np.zeros((P, 16), np.float32)        # render.hip: 0,1 mean2D (pixels) | 2,3,4 conic xx, xy(half), yy | 5 opacity | 6,7,8 rgb | 9 depth
    acc[:, 0:2], acc[:, 2:5], acc[:, 6:9], acc[:, 9] = m(w["xy"]), m(w["conic"] * np.array([1.0, 0.5, 1.0])), m(w["rgb"]), m(w["depth"])
    (a, b), _, _ = _device_camera_grad(sc, acc, dev)
    assert torch.equal(a, b), "two runs on one accumulator differ"
    got = a.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all() and not np.any(got[35:])
    # (the twin takes the arrays of its own forward: the mask keeps the rows both sides let through)
    twin = TH._twin(p_host, out, w, mask)
    ref = TH._autograd(sc, MOD, w, mask)
    g, c3, c2 = _groups(got[:16], got[16:32], got[32:35])
    r, _, _ = _groups(ref[:16], ref[16:32], ref[32:35])
    tw, _, _ = _groups(twin[:16], twin[16:32], twin[32:35])
    assert not np.any(c3) and not np.any(c2), "view[:, 3] and proj[:, 2] are exactly 0"
    errs = {k: rel_l2(g[k], r[k]) for k in g}
    print(f"[P={P}] device vs float64 autograd: " + ", ".join(f"{k}={v:.2e}" for k, v in errs.items()) +
          " | device vs twin: " + ", ".join(f"{k}={rel_l2(g[k], tw[k]):.2e}" for k in g))
    for k, v in errs.items():
        assert v < GRAD_BOUND, (k, v)


def test_kernel_without_gaussians_writes_zeros():
    fd = _mod()
    dev = torch.device("cuda:0")
    L = fd._lib.lib()
    sc = _slice_scene(0, 1)
    t = {k: torch.tensor(sc[k][:0], device=dev) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    p, keep = fd.rasterizer._frame_params(_settings(sc, dev), t["means3D"], None, None, t["opacities"], None, None, None)
    assert p.P == 0
    out = torch.full((48,), float("nan"), device=dev)
    fd._lib.check(L.fdgs_camera_grad(fd._lib.stream_ptr(), p, None, None, None, fd._lib.ptr(out)))
    torch.cuda.synchronize()
    assert not out.any()


# ---- 2. the whole backward, small ---------------------------------------------------------------------------------------------------

SMALL = dict(n=2000, width=128, height=96, seed=7, theta=20.0, scale_boost=3.0)
SMALL_CASES = {"deg3": dict(sh_degree=3), "deg0": dict(sh_degree=0), "precomp": dict(sh_degree=3, precomp=True)}


@functools.lru_cache(maxsize=None)
def _small(case):
    kw = dict(SMALL_CASES[case])
    precomp = kw.pop("precomp", False)
    sc = raster_scene(**SMALL, **kw)
    sc["bg"] = np.array([0.2, 0.5, 0.1], np.float32)
    rng = np.random.default_rng(5)
    if precomp:
        sc["colors_precomp"], sc["shs"] = rng.uniform(0, 1, (SMALL["n"], 3)).astype(np.float32), None
    wc, wd = rng.standard_normal((3, SMALL["height"], SMALL["width"])), rng.standard_normal((1, SMALL["height"], SMALL["width"]))
    return sc, wc, wd


@functools.lru_cache(maxsize=None)
def _small_reference(case):
    """float64 autograd through the dense raster_torch.rasterize with the three camera tensors as leaves (computed once per case)."""
    sc, wc, wd = _small(case)
    f64 = lambda a: None if a is None else torch.tensor(a, dtype=torch.float64)
    cam = {k: f64(sc[k]).requires_grad_(True) for k in CAM_KEYS}
    color, depth, _ = raster_torch.rasterize(means3D=f64(sc["means3D"]), opacities=f64(sc["opacities"]), shs=f64(sc.get("shs")),
                                             colors_precomp=f64(sc.get("colors_precomp")), scales=f64(sc["scales"]), rotations=f64(sc["rotations"]),
                                             bg=f64(sc["bg"]), image_height=sc["image_height"], image_width=sc["image_width"], tanfovx=sc["tanfovx"],
                                             tanfovy=sc["tanfovy"], sh_degree=sc["sh_degree"], **cam)
    ((color * f64(wc)).sum() + (depth * f64(wd)).sum()).backward()
    z = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()
    return {k: z(v) for k, v in cam.items()}


@pytest.mark.parametrize("case", list(SMALL_CASES))
def test_whole_backward_against_dense_float64_autograd(case):
    fd = _mod()
    R = fd.rasterizer
    dev = torch.device("cuda:0")
    sc, wc, wd = _small(case)
    wc_d, wd_d = torch.tensor(wc, device=dev, dtype=torch.float32), torch.tensor(wd, device=dev, dtype=torch.float32)
    names = ("means3D", "opacities", "scales", "rotations") + (("shs",) if sc.get("shs") is not None else ("colors_precomp",))

    def run(leaves):
        t = {k: torch.tensor(sc[k], device=dev).requires_grad_(True) for k in names}
        t["means2D"] = torch.zeros(len(sc["means3D"]), 3, device=dev, requires_grad=True)
        s = _settings(sc, dev, leaves=leaves)
        color, radii, depth = R.GaussianRasterizer(s)(**t)
        ((color * wc_d).sum() + (depth * wd_d).sum()).backward()
        return color, radii, depth, t, s

    color, radii, depth, t, s = run(True)
    color0, radii0, depth0, t0, s0 = run(False)
    assert type(color.grad_fn).__name__ == "_RasterizeGaussiansCameraBackward" and type(color0.grad_fn).__name__ == "_RasterizeGaussiansBackward"
    assert all(getattr(s0, k).grad is None for k in CAM_KEYS)
    # the image does not know about the leaves: bit-equal; the per-Gaussian gradients come from atomically summed accumulators of two
    # runs: equal at tests/test_gpu_raster.py's tolerance for them
    assert torch.equal(color, color0) and torch.equal(depth, depth0) and torch.equal(radii, radii0)
    for k in t:
        assert rel_l2(t[k].grad.cpu().numpy(), t0[k].grad.cpu().numpy()) < 1e-3, k
    ref = _small_reference(case)
    g, c3, c2 = _groups(*(getattr(s, k).grad.cpu().numpy() for k in CAM_KEYS))
    r, _, _ = _groups(*(ref[k] for k in CAM_KEYS))
    assert not np.any(c3) and not np.any(c2)
    errs = {k: rel_l2(g[k], r[k]) for k in g}
    print(f"[{case}] GaussianRasterizer camera gradients vs dense float64 autograd: " + ", ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    if case == "precomp":
        assert not np.any(g["campos"]) and not np.any(r["campos"])
    for k, v in errs.items():
        assert v < GRAD_BOUND, (k, v)
    # one accumulator, both sets: the keyword of rasterize_backward returns the camera's gradient next to the others, which are the
    # same call's -- and the camera's is what a second fdgs_camera_grad on that accumulator gives, bit for bit
    tt = {k: torch.tensor(sc[k], device=dev) for k in names}
    _, _, _, state = R.rasterize_forward(s0, tt["means3D"], tt.get("shs"), tt.get("colors_precomp"), tt["opacities"], tt["scales"], tt["rotations"],
                                         None, expect_backward=True)
    acc = state.acc
    both = R.rasterize_backward(state, wc_d, wd_d, camera=True)
    again = R.camera_gradients(state, acc)
    assert torch.equal(both["camera"], again)
    assert rel_l2(both["means3D"].cpu().numpy(), t0["means3D"].grad.cpu().numpy()) < 1e-3


# ---- 3. the translation identity ------------------------------------------------------------------------------------------------------

IDENTITY_SCENE = dict(n=100_000, width=800, height=800, seed=11, theta=100.0, scale_boost=2.0)       # BASELINE config 2's frame
IDENTITY_FLOAT32 = 2.0e-09       # _identity_float32_figure(torch.float32), measured on the CPU (float64: 9.0e-17)
IDENTITY_FACTOR = 8.0


def _identity_ratio(dmeans, V, PM, dV, dPM, dcampos):
    V, PM, dV, dPM = (np.asarray(a, np.float64).reshape(4, 4) for a in (V, PM, dV, dPM))
    dmeans, dcampos = np.asarray(dmeans, np.float64), np.asarray(dcampos, np.float64).reshape(3)
    res = dmeans.sum(axis=0) + dcampos - V[:3, :] @ dV[3, :] - PM[:3, :] @ dPM[3, :]
    return np.abs(res) / np.abs(dmeans).sum(axis=0)


def _identity_float32_figure(dtype=torch.float32):
    """The identity's residual ratio from raster_torch.project's autograd in `dtype` on the plain scene, with the seeded weights of
    tests/test_preprocess_host.py as the contraction (run on the CPU; what IDENTITY_FLOAT32 records)."""
    sc = raster_scene(**IDENTITY_SCENE)
    n = IDENTITY_SCENE["n"]
    t = {k: torch.tensor(sc[k], dtype=dtype) for k in ("shs", "scales", "rotations")}
    means = torch.tensor(sc["means3D"], dtype=dtype, requires_grad=True)
    cam = {k: torch.tensor(sc[k], dtype=dtype, requires_grad=True) for k in CAM_KEYS}
    g = raster_torch.project(means3D=means, **t, **cam, image_height=sc["image_height"], image_width=sc["image_width"], tanfovx=sc["tanfovx"],
                             tanfovy=sc["tanfovy"], sh_degree=sc["sh_degree"])
    rng = np.random.default_rng(9)
    r = np.clip(g["radii"].numpy(), 1, math.hypot(sc["image_width"], sc["image_height"])).astype(np.float64)
    vis = g["vis"].numpy().astype(np.float64)
    T = lambda a: torch.tensor(a * vis.reshape((-1,) + (1,) * (a.ndim - 1)), dtype=dtype)
    loss = (T(rng.standard_normal((n, 2)) / r[:, None]) * torch.stack([g["px"], g["py"]], 1)).sum() + \
           (T(rng.standard_normal((n, 3)) * (r * r)[:, None]) * torch.stack(g["conic"], 1)).sum() + \
           (T(rng.standard_normal((n, 3))) * g["rgb"]).sum() + (T(rng.standard_normal(n)) * g["tz"]).sum()
    loss.backward()
    return float(_identity_ratio(means.grad.numpy(), sc["viewmatrix"], sc["projmatrix"], cam["viewmatrix"].grad.numpy(),
                                 cam["projmatrix"].grad.numpy(), cam["campos"].grad.numpy()).max())


def test_translation_identity_from_device_outputs():
    fd = _mod()
    dev = torch.device("cuda:0")
    sc = raster_scene(**IDENTITY_SCENE)
    sc["bg"] = np.zeros(3, np.float32)
    t = {k: torch.tensor(sc[k], device=dev).requires_grad_(k == "means3D") for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    t["means2D"] = torch.zeros(IDENTITY_SCENE["n"], 3, device=dev)
    s = _settings(sc, dev, leaves=True)
    color, radii, depth = fd.rasterizer.GaussianRasterizer(s)(**t)
    gen = torch.Generator().manual_seed(12)
    wc, wd = torch.randn(color.shape, generator=gen).to(dev), torch.randn(depth.shape, generator=gen).to(dev)
    ((color * wc).sum() + (depth * wd).sum()).backward()
    ratio = _identity_ratio(t["means3D"].grad.cpu().numpy(), sc["viewmatrix"], sc["projmatrix"], s.viewmatrix.grad.cpu().numpy(),
                            s.projmatrix.grad.cpu().numpy(), s.campos.grad.cpu().numpy())
    print(f"translation identity, residual / sum|dL/dmeans3D| per axis: {ratio[0]:.2e} {ratio[1]:.2e} {ratio[2]:.2e}; float32 autograd figure "
          f"{IDENTITY_FLOAT32:.2e}, bound {IDENTITY_FACTOR * IDENTITY_FLOAT32:.2e}")
    assert np.all(ratio < IDENTITY_FACTOR * IDENTITY_FLOAT32), ratio


# ---- 4. render(): fused against two-node -------------------------------------------------------------------------------------------------

class _Pipe:
    convert_SHs_python = compute_cov3D_python = debug = False


@pytest.mark.parametrize("cfg", ["dynerf_default", "dnerf_bouncingballs"])      # a five-head and a three-head configuration
def test_render_fused_against_two_node_with_camera_leaves(cfg, monkeypatch):
    fd = _mod()
    syn = fd.synthetic
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(4)
    w, wd = torch.randn(3, 180, 240, generator=gen).to(dev), torch.randn(1, 180, 240, generator=gen).to(dev)

    def run(fused, leaves):
        monkeypatch.setattr(fd.renderer, "FUSED_BACKWARD", fused)
        pc = syn.SynthModel(7001, cfg, seed=23)
        with torch.no_grad():
            pc._scaling.add_(1.0)
        pc = pc.to(dev)
        cam = syn.make_camera(240, 180, theta_deg=-35.0, time=0.45).to(dev)
        if leaves:
            for k in ("world_view_transform", "full_proj_transform", "camera_center"):
                setattr(cam, k, getattr(cam, k).clone().requires_grad_(True))
        res = fd.render(cam, pc, _Pipe(), torch.zeros(3, device=dev), stage="fine")
        ((res["render"] * w).sum() + (res["depth"] * wd).sum()).backward()
        cg = {k: getattr(cam, k).grad for k in ("world_view_transform", "full_proj_transform", "camera_center")}
        return res, {k: p.grad.clone() for k, p in pc.named_parameters() if p.grad is not None}, cg

    ra, ga, ca = run(True, True)
    rb, gb, cb = run(False, True)
    r0, g0, c0 = run(True, False)
    assert type(ra["render"].grad_fn).__name__ == "_FusedRenderCameraFunctionBackward" and all(v is None for v in c0.values())
    assert torch.equal(ra["render"], rb["render"]) and torch.equal(ra["render"], r0["render"]) and torch.equal(ra["depth"], r0["depth"])
    assert all(ca[k].shape == cb[k].shape and ca[k].abs().sum() > 0 for k in ca)
    worst_cam = max((rel_l2(ca[k].cpu().numpy(), cb[k].cpu().numpy()), k) for k in ca)
    worst_model = max((rel_l2(ga[k].cpu().numpy(), g0[k].cpu().numpy()), k) for k in ga)
    worst_two = max((rel_l2(gb[k].cpu().numpy(), g0[k].cpu().numpy()), k) for k in gb)
    print(f"[{cfg}] camera gradients fused vs two-node: worst rel-L2 {worst_cam[0]:.1e} ({worst_cam[1]}); model gradients with vs without camera "
          f"leaves: fused {worst_model[0]:.1e} ({worst_model[1]}), two-node {worst_two[0]:.1e} ({worst_two[1]})")
    assert set(ga) == set(g0) == set(gb)
    assert worst_cam[0] < 2e-5 and worst_model[0] < 2e-5 and worst_two[0] < 2e-5


# ---- 5. pose recovery ---------------------------------------------------------------------------------------------------------------

# (chosen on the CPU reference before any device run: at lr 5e-3 the float64 fit ends at 0.017 of the start in rotation and 0.035 in
# translation after 200 steps -- still the optimiser's distance, not float64's resolution, so a float32 device can be held to 2 x;
# with splats three times larger the same fit does not converge at any of the rates tried)
POSE_SCENE = dict(n=300, width=64, height=48, seed=21, theta=15.0, scale_boost=1.0)
POSE_LR, POSE_STEPS = 5e-3, 200
POSE_START = (np.deg2rad(2.0) * np.array([0.6, -0.64, 0.48]), 0.05 * np.array([0.48, 0.6, -0.64]))      # unit axes: 2 degrees, 0.05 units


def _fit_pose(sc, render, dev, dtype):
    """Adam on a PoseDelta that starts POSE_START off, against the image `render` gives at the true pose -> (|omega|, |tau|) at the end.
    `render(view, proj, campos) -> color`."""
    fd = _mod()
    base = {k: torch.tensor(np.asarray(sc[k]), device=dev, dtype=dtype) for k in CAM_KEYS}
    with torch.no_grad():
        target = render(base["viewmatrix"].reshape(4, 4), base["projmatrix"].reshape(4, 4), base["campos"])
    delta = fd.camera.PoseDelta(dtype=dtype).to(dev)
    with torch.no_grad():
        delta.omega.copy_(torch.tensor(POSE_START[0], dtype=dtype))
        delta.tau.copy_(torch.tensor(POSE_START[1], dtype=dtype))
    opt = torch.optim.Adam(delta.parameters(), lr=POSE_LR)
    for _ in range(POSE_STEPS):
        opt.zero_grad(set_to_none=True)
        V, F, c = delta.transforms(base["viewmatrix"], base["projmatrix"])
        ((render(V, F, c) - target) ** 2).mean().backward()
        opt.step()
    return float(delta.omega.detach().norm()), float(delta.tau.detach().norm())


def _pose_scene():
    sc = raster_scene(**POSE_SCENE)
    sc["bg"] = np.zeros(3, np.float32)
    return sc


def _fit_pose_reference():
    """The fit through raster_torch.rasterize in float64 on the CPU."""
    sc = _pose_scene()
    f64 = lambda a: torch.tensor(a, dtype=torch.float64)
    fixed = dict(means3D=f64(sc["means3D"]), opacities=f64(sc["opacities"]), shs=f64(sc["shs"]), scales=f64(sc["scales"]), rotations=f64(sc["rotations"]),
                 bg=f64(sc["bg"]), image_height=sc["image_height"], image_width=sc["image_width"], tanfovx=sc["tanfovx"], tanfovy=sc["tanfovy"],
                 sh_degree=sc["sh_degree"])
    return _fit_pose(sc, lambda V, F, c: raster_torch.rasterize(viewmatrix=V, projmatrix=F, campos=c, **fixed)[0], torch.device("cpu"), torch.float64)


def test_pose_recovery_against_the_float64_fit():
    fd = _mod()
    R = fd.rasterizer
    dev = torch.device("cuda:0")
    sc = _pose_scene()
    start = (float(np.linalg.norm(POSE_START[0])), float(np.linalg.norm(POSE_START[1])))
    ref = _fit_pose_reference()
    assert ref[0] < 0.1 * start[0] and ref[1] < 0.1 * start[1], ("the reference fit itself", ref, start)
    t = {k: torch.tensor(sc[k], device=dev) for k in ("means3D", "opacities", "shs", "scales", "rotations")}      # frozen
    means2D = torch.zeros(POSE_SCENE["n"], 3, device=dev)
    s0 = _settings(sc, dev)

    def render(V, F, c):
        return R.GaussianRasterizer(s0._replace(viewmatrix=V, projmatrix=F, campos=c))(means2D=means2D, **t)[0]

    got = _fit_pose(sc, render, dev, torch.float32)
    print(f"pose recovery after {POSE_STEPS} Adam steps (lr {POSE_LR}): start {math.degrees(start[0]):.2f} deg / {start[1]:.3f}; float64 reference "
          f"{math.degrees(ref[0]):.4f} deg / {ref[1]:.5f}; device {math.degrees(got[0]):.4f} deg / {got[1]:.5f}")
    assert got[0] <= 2 * ref[0] and got[1] <= 2 * ref[1], (got, ref)
    assert got[0] < 0.1 * start[0] and got[1] < 0.1 * start[1], (got, start)
