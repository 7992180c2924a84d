"""The opacity compensation on the device (fdgs_preprocess_fwd_aa / fdgs_raster_fwd_capacity_aa / fdgs_raster_bwd_aa / fdgs_camera_grad_aa,
pipe.antialiasing): scenes and the float64 restatement of h from tests/antialias_common.py.

  forward    the geom fields of an antialiased frame are the plain frame's bits except recB.y, which is the host twin's opacity * h within
             4 ulp; image, depth and alpha against the float64 C oracle given opacity * h (float64 h) as its opacities, at the bounds
             tests/test_gpu_raster.py puts on the plain frame.
  backward   reference = the oracle's gradients at those opacities (its opacity gradient G is dL/d(opacity * h)) plus float64 autograd of
             sum_i G_i opacity_i h_i -- the loss is linear in that path; every group below 1e-3 over all rows and over the clamped rows.
  identity   an antialiased frame is the same bits under tile_cull, bin_form and bin_count, and when it overflowed its capacity.
             (n_contrib is a position in the pair list: it is compared among the settings that keep the lists, not across tile_cull.)
  plumbing   render() / render_views / playback with pipe.antialiasing against the rasterizer with the switch; behaviour by ordering only.
"""
import functools
import importlib
import math

import numpy as np
import pytest
import torch

import antialias_common as AC
from conftest import set_knob
from oracle.raster_oracle import RasterOracle
from scenes import rel_l2
from test_gpu_raster import _geom, _img, _settings

pytestmark = pytest.mark.gpu
synthetic = importlib.import_module("4dgaussians_amd.synthetic")
GEOM_GROUPS = ("means2D", "means3D", "opacities", "scales", "rotations")


def _fd():
    return importlib.import_module("4dgaussians_amd")


def _dev():
    return torch.device("cuda:0")


def _t(sc, grad=False):
    keys = [k for k in ("means3D", "shs", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp") if sc.get(k) is not None]
    return {k: torch.tensor(sc[k], device=_dev(), requires_grad=grad) for k in keys}


def _forward(sc, mod=1.0, aa=True, **kw):
    R = _fd().rasterizer
    t = _t(sc)
    return R.rasterize_forward(_settings(sc, _dev(), debug=False, scale_modifier=mod), t["means3D"], t.get("shs"), t.get("colors_precomp"),
                               t["opacities"], t.get("scales"), t.get("rotations"), t.get("cov3D_precomp"),
                               **({"antialiasing": True} if aa else {}), **kw)


def _case(P, kind, mod, size=(AC.W, AC.H)):
    sc = AC.inputs(P, kind, *size)
    return AC.with_cov3d(sc, mod) if kind == "cov3d" else sc


def _oracle_scene(sc, mod):
    """The scene as the oracle takes it, with opacity * h (float64) as its opacities."""
    h, r, cl, vis = AC.h64(sc, mod)
    o = {k: (np.asarray(v, np.float64) if isinstance(v, np.ndarray) else v) for k, v in sc.items() if v is not None}
    o["opacities"] = (sc["opacities"].reshape(-1).astype(np.float64) * h).reshape(sc["opacities"].shape)
    return o, h, r, cl, vis


FWD_CASES = [(1, "sh16", 1.0), (257, "sh16", 1.0), (257, "sh4", 0.25), (257, "colors", 1.0), (257, "cov3d", 0.25), (1000, "sh16", 1.0),
             (1000, "sh16", 0.25), (AC.WIDE[0], "sh16", 1.0, AC.WIDE[1:])]


def _id(c):
    return "-".join(str(x) for x in c)


# ---- 6. / 7. forward ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", FWD_CASES, ids=_id)
def test_forward_fields_and_images(case):
    dev = _dev()
    P, kind, mod = case[:3]
    sc = _case(P, kind, mod, *case[3:])
    W, H = sc["image_width"], sc["image_height"]
    c0, r0, d0, st0 = _forward(sc, mod, aa=False)
    c1, r1, d1, a1, st1 = _forward(sc, mod, want_alpha=True)
    torch.cuda.synchronize()
    assert st1.antialiasing and not st0.antialiasing
    # radii and rect are the plain frame's, and so is every other field but recB.y
    assert torch.equal(r0, r1)
    shapes = {0: ((P,), torch.float32), 1: ((P, 4), torch.float32), 2: ((P, 4), torch.float32), 3: ((P, 4), torch.float32), 4: ((P, 6), torch.float32),
              6: ((P,), torch.int32), 7: ((P, 2), torch.int32)}
    vis = r1.cpu().numpy() > 0
    f0 = {k: _geom(st0, k, *v, dev)[vis] for k, v in shapes.items()}
    f1 = {k: _geom(st1, k, *v, dev)[vis] for k, v in shapes.items()}
    assert np.array_equal(f0[7], f1[7]) and np.array_equal(f0[6], f1[6])          # rect, colour clamp bits
    # (the float fields come from another instantiation of the kernel, whose compiler may contract a * b + c elsewhere: they are held to
    # the host twin below, at the plain fields' tolerances, and reported here)
    differ = {k: int((f0[k].view(np.uint32) != f1[k].view(np.uint32))[:, (0, 2, 3)].sum() if k == 2 else (f0[k].view(np.uint32) != f1[k].view(np.uint32)).sum())
              for k in (0, 1, 2, 3, 4)}
    print(f"[{_id(case)}] float words that differ from the plain frame's (depth, recA, recB.xzw, recC, cov3D): {differ}")
    # ... against the host twin, at the tolerances of the plain fields; recB.y within 4 ulp
    tw, _, _ = AC.twin_forward(sc, mod)
    both = vis & (tw["tiles"] > 0)
    assert (vis != (tw["tiles"] > 0)).mean() < 2e-3
    sel = both[vis]
    np.testing.assert_allclose(f1[1][sel, :2], tw["xy"][both], rtol=0, atol=2e-3)
    conic = np.c_[f1[1][sel, 2:], f1[2][sel, 0]]
    assert rel_l2(conic, tw["conic"][both]) < 1e-5
    np.testing.assert_allclose(f1[2][sel, 2], tw["depth"][both], rtol=1e-6)
    np.testing.assert_allclose(f1[3][sel, :3], tw["rgb"][both], rtol=0, atol=1e-5)
    u = AC.ulps(f1[2][sel, 1], tw["opacity_eff"][both].astype(np.float64))
    print(f"[{_id(case)}] recB.y vs the host twin: max {u.max():.2f} ulp over {int(both.sum())} rows; pairs {st0.num_rendered} -> {st1.num_rendered}")
    assert u.max() <= 4.0
    assert st1.num_rendered <= st0.num_rendered                      # h <= 1 can only tighten the cull
    # image, depth and alpha against the float64 oracle at opacity * h
    osc, h, r, cl, _ = _oracle_scene(sc, mod)
    o = RasterOracle(**osc, scale_modifier=mod, dtype=np.float64)
    d = np.abs(c1.cpu().numpy() - o.color)
    dd = np.abs(d1.cpu().numpy() - o.depth)
    fT, _ = o.image_state()
    da = np.abs(a1.cpu().numpy()[0] - (1.0 - fT))
    print(f"   colour mean {d.mean():.2e} q {np.quantile(d, 0.9999):.2e}; depth mean {dd.mean():.2e} q {np.quantile(dd, 0.9999):.2e}; "
          f"alpha mean {da.mean():.2e} q {np.quantile(da, 0.9999):.2e}")
    assert d.mean() < 2e-6 and np.quantile(d, 0.9999) < 5e-5
    assert dd.mean() < 2e-5 and np.quantile(dd, 0.9999) < 5e-4
    assert da.mean() < 2e-6 and np.quantile(da, 0.9999) < 5e-5
    if P >= 257:      # the switch is visible: the plain frame is not this image
        assert float((c0 - c1).abs().max()) > 1e-3


# ---- 8. backward ------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _bwd_reference(P, kind, mod, with_depth, with_alpha):
    """(scene, image gradients, reference gradients, clamped rows): computed once per case, read-only."""
    sc = _case(P, kind, mod)
    W, H = sc["image_width"], sc["image_height"]
    osc, h, r, cl, vis = _oracle_scene(sc, mod)
    o = RasterOracle(**osc, scale_modifier=mod, dtype=np.float64)
    rng = np.random.default_rng(12)
    dc = rng.standard_normal((3, H, W)).astype(np.float32)
    dd = rng.standard_normal((1, H, W)).astype(np.float32) if with_depth else None
    ga = rng.standard_normal((1, H, W)).astype(np.float32) if with_alpha else None
    g = {k: np.asarray(v, np.float64).copy() for k, v in o.backward(dc, dd).items() if v is not None}
    if with_alpha:      # alpha is the red channel of the same geometry with unit red colours over black
        tw = {k: v for k, v in osc.items() if k not in ("shs", "colors_precomp")}
        tw["colors_precomp"], tw["bg"] = np.tile(np.array([1.0, 0.0, 0.0]), (P, 1)), np.zeros(3)
        gt = RasterOracle(**tw, scale_modifier=mod, dtype=np.float64).backward(np.concatenate([ga, np.zeros((2, H, W), np.float32)]))
        for k in g:
            if k not in ("shs", "colors") and gt.get(k) is not None and g[k] is not None:
                g[k] = g[k] + np.asarray(gt[k], np.float64).reshape(g[k].shape)
    G = g["opacities"].reshape(-1)                   # dL/d(opacity * h)
    zero = {k: np.zeros((P,) + s) for k, s in (("xy", (2,)), ("conic", (3,)), ("rgb", (3,)), ("depth", ()))}
    part, _ = AC.autograd(sc, mod, dict(zero, opacity=G), np.ones(P), parts=("h",))
    ref = dict(g)
    ref["opacities"] = part["opacities"]
    for k in ("means3D", "scales", "rotations", "cov3D"):
        if ref.get(k) is not None and k in part:
            ref[k] = np.asarray(ref[k], np.float64).reshape(part[k].shape) + part[k]
    k = "cov3D" if ref.get("cov3D") is not None else "scales"
    share = np.linalg.norm(part[k]) / np.linalg.norm(ref[k])
    assert share > 1e-2, share                       # the compensation's path is material at the oracle's own sums as well
    return sc, (dc, dd, ga), ref, cl


def _device_grads(sc, mod, grads, ppl=None, aa=True):
    R = _fd().rasterizer
    if ppl is not None:
        set_knob("rbwd_ppl", ppl)
    dc, dd, ga = grads
    t = _t(sc, grad=True)
    means2D = torch.zeros(len(sc["means3D"]), 3, device=_dev(), requires_grad=True)
    rast = R.GaussianRasterizer(_settings(sc, _dev(), scale_modifier=mod), render_alpha=ga is not None)
    rast.antialiasing = aa
    color, radii, depth, *alpha = rast(means3D=t["means3D"], means2D=means2D, shs=t.get("shs"), colors_precomp=t.get("colors_precomp"),
                                       opacities=t["opacities"], scales=t.get("scales"), rotations=t.get("rotations"),
                                       cov3D_precomp=t.get("cov3D_precomp"))
    loss = (color * torch.tensor(dc, device=_dev())).sum()
    if dd is not None:
        loss = loss + (depth * torch.tensor(dd, device=_dev())).sum()
    if ga is not None:
        loss = loss + (alpha[0] * torch.tensor(ga, device=_dev())).sum()
    loss.backward()
    torch.cuda.synchronize()
    g = {k: v.grad.cpu().numpy() for k, v in t.items()}
    g["means2D"] = means2D.grad.cpu().numpy()
    return g, (color.detach(), depth.detach())


_NAMES = dict(means2D="means2D", means3D="means3D", opacities="opacities", scales="scales", rotations="rotations", shs="shs",
              colors_precomp="colors", cov3D_precomp="cov3D")


def _hold(tag, g, ref, cl):
    failures = []
    for k, a in g.items():
        r = np.asarray(ref[_NAMES[k]], np.float64).reshape(a.shape)
        e_all = rel_l2(a, r)
        e_cl = rel_l2(a[cl], r[cl]) if cl.sum() and np.linalg.norm(r[cl]) > 0 else 0.0
        print(f"   [{tag}] {k:14s} all rows {e_all:.2e}   clamped rows {e_cl:.2e}")
        if not (e_all < AC.GRAD_BOUND and e_cl < AC.GRAD_BOUND):
            failures.append((k, e_all, e_cl))
    assert not failures, (tag, failures)


@pytest.mark.parametrize("with_alpha", [False, True])
@pytest.mark.parametrize("with_depth", [False, True])
@pytest.mark.parametrize("ppl", [4, 2, 0])
def test_backward_against_the_oracle_plus_the_compensations_autograd(ppl, with_depth, with_alpha):
    sc, grads, ref, cl = _bwd_reference(1000, "sh16", 1.0, with_depth, with_alpha)
    g, _ = _device_grads(sc, 1.0, grads, ppl)
    _hold(f"P=1000 sh16 ppl={ppl} depth={with_depth} alpha={with_alpha}", g, ref, cl)


@pytest.mark.parametrize("case", [(1, "sh16", 1.0), (257, "sh4", 0.25), (257, "colors", 1.0), (257, "cov3d", 1.0), (257, "cov3d", 0.25),
                                  (1000, "sh16", 0.25)], ids=_id)
def test_backward_at_the_other_sizes_and_input_kinds(case):
    sc, grads, ref, cl = _bwd_reference(*case, True, False)
    g, _ = _device_grads(sc, case[2], grads)
    _hold(_id(case), g, ref, cl)


# ---- 9. one frame whatever the binning does ---------------------------------------------------------------------------------------------

def _frame_bits(sc, **kw):
    out = _forward(sc, **kw)
    st = out[-1]
    torch.cuda.synchronize()
    H, W = sc["image_height"], sc["image_width"]
    return dict(color=out[0].cpu().numpy(), depth=out[2].cpu().numpy(), final_T=_img(st, 0, (H, W), torch.float32, _dev()),
                n_contrib=_img(st, 1, (H, W), torch.int32, _dev())), st


@pytest.mark.parametrize("size", [(1000, AC.W, AC.H), AC.WIDE], ids=_id)
def test_an_antialiased_frame_is_the_same_bits_under_every_binning_setting(size, monkeypatch):
    R = _fd().rasterizer
    monkeypatch.setattr(R, "BINNING", "exact")
    sc = AC.inputs(size[0], "sh16", size[1], size[2])
    frames = {}
    for cull in (0, 1):
        for form in (0, 1):
            for count in (0, 1, 2):
                set_knob("tile_cull", cull)
                set_knob("bin_form", form)
                set_knob("bin_count", count)
                frames[cull, form, count] = _frame_bits(sc)[0]
                if count and (cull, form, count) == (1, 1, 1):          # the one-call path counts in the projection: run it too
                    monkeypatch.setattr(R, "BINNING", "auto")
                    frames["auto"] = _frame_bits(sc)[0]
                    monkeypatch.setattr(R, "BINNING", "exact")
    base = frames[0, 0, 0]
    for key, f in frames.items():
        for k in ("color", "depth", "final_T"):
            assert np.array_equal(f[k].view(np.uint32), base[k].view(np.uint32)), (key, k)
        same_lists = frames[(key[0], 0, 0)] if key != "auto" else frames[1, 0, 0]
        assert np.array_equal(f["n_contrib"], same_lists["n_contrib"]), key


def test_an_antialiased_frame_that_overflowed_its_capacity_is_the_exact_frame(monkeypatch):
    from scenes import raster_scene
    R = _fd().rasterizer
    sc = raster_scene(20000, 416, 304, seed=22, scale_boost=2.0)      # (the scene of tests/test_gpu_raster.py's overflow test)
    key = (_dev().index, sc["image_width"], sc["image_height"], 20000)
    monkeypatch.setattr(R, "BINNING", "exact")
    want, st0 = _frame_bits(sc)
    n = st0.num_rendered
    assert n > 40000
    monkeypatch.setattr(R, "BINNING", "auto")
    R._seen[key] = [1, 20000]
    before = R.capacity_reruns
    got, st1 = _frame_bits(sc)
    assert R.capacity_reruns == before + 1 and st1.capacity == n
    assert st1.num_rendered == n and st1.antialiasing
    for k in want:
        assert np.array_equal(want[k], got[k]), k


# ---- 10. the switch given as False ---------------------------------------------------------------------------------------------------------

def test_antialiasing_false_is_the_default_frame():
    sc, grads, _, _ = _bwd_reference(1000, "sh16", 1.0, True, False)
    a = _forward(sc, aa=False)
    b = _forward(sc, aa=False, antialiasing=False)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and b[-1].antialiasing is False
    R = _fd().rasterizer
    dc, dd = torch.tensor(grads[0], device=_dev()), torch.tensor(grads[1], device=_dev())
    set_knob("rbwd_ppl", 0)
    outs = []
    for kw in ({}, {"antialiasing": False}):
        t = _t(sc)
        *_, st = R.rasterize_forward(_settings(sc, _dev(), debug=False), t["means3D"], t["shs"], None, t["opacities"], t["scales"], t["rotations"],
                                     None, expect_backward=True, **kw)
        outs.append(R.rasterize_backward(st, dc, dd))
    torch.cuda.synchronize()
    worst = max(rel_l2(outs[1][k].cpu().numpy(), outs[0][k].cpu().numpy()) for k in outs[0] if outs[0][k] is not None)
    print(f"explicit False vs default, gradients: worst rel-L2 {worst:.1e} (the blending backward's sums are atomic: the same call twice)")
    # the same entry points run on the same inputs: the per-Gaussian chain rule is bit for bit the same function of the accumulator
    assert worst < 5e-6


# ---- 11. render() ------------------------------------------------------------------------------------------------------------------------------

class _Pipe:
    convert_SHs_python = compute_cov3D_python = debug = False

    def __init__(self, aa=True):
        self.antialiasing = aa


def _model(cfg="dynerf_default", n=1000, shrink=3.0):
    pc = synthetic.SynthModel(n, cfg, seed=23)
    with torch.no_grad():
        pc._scaling.add_(-shrink)                 # footprints around and below a pixel: h well under 1 for most rows
    return pc.to(_dev())


def _cam(W=96, H=80, radius=4.0):
    return synthetic.make_camera(W, H, theta_deg=15.0, time=0.3, radius=radius).to(_dev())


def _weights(H=80, W=96, seed=4):
    return torch.randn(3, H, W, generator=torch.Generator().manual_seed(seed)).to(_dev())


def _param_grads(pc):
    return {k: p.grad.clone() for k, p in pc.named_parameters() if p.grad is not None}


def test_render_fused_node_against_deform_plus_the_antialiased_rasterizer(monkeypatch):
    """The bounds tests/test_gpu_alpha.py puts on the same comparison: images bit for bit, parameter gradients within 2e-5 rel-L2,
    viewspace_points.grad within 1e-6."""
    fd = _fd()
    cam, bg, w = _cam(), torch.zeros(3, device=_dev()), _weights()
    out = []
    for fused in (True, False):
        monkeypatch.setattr(fd.renderer, "FUSED_BACKWARD", fused)
        pc = _model()
        res = fd.render(cam, pc, _Pipe(), bg, stage="fine")
        (res["render"] * w).sum().backward()
        out.append((res, _param_grads(pc), res["viewspace_points"].grad.clone()))
    (ra, ga, va), (rb, gb, vb) = out
    for k in ("render", "depth", "radii"):
        assert torch.equal(ra[k], rb[k]), k
    worst = max((rel_l2(ga[k].cpu().numpy(), gb[k].cpu().numpy()), k) for k in ga)
    print(f"fused vs two-node, antialiased: worst gradient rel-L2 {worst[0]:.1e} ({worst[1]})")
    assert set(ga) == set(gb) and worst[0] < 2e-5 and rel_l2(va.cpu().numpy(), vb.cpu().numpy()) < 1e-6
    # the two-node form IS deform() + the rasterizer with the switch: the same frame from those two calls
    pc = _model()
    with torch.no_grad():
        m, s, r, o, sh = fd.deformation.deform(pc._deformation, pc.get_xyz, pc._scaling, pc._rotation, pc._opacity, shs_dc=pc._features_dc,
                                               shs_rest=pc._features_rest, time=0.3, activate=True)
        rs = fd.GaussianRasterizationSettings(80, 96, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), bg, 1.0, cam.world_view_transform,
                                              cam.full_proj_transform, pc.active_sh_degree, cam.camera_center, False, False)
        rast = fd.GaussianRasterizer(rs)
        rast.antialiasing = True
        img, radii, depth = rast(means3D=m, means2D=torch.zeros_like(m), opacities=o, shs=sh, scales=s, rotations=r)
    assert torch.equal(img, ra["render"]) and torch.equal(radii, ra["radii"])
    # the switch reaches the gradients: the opacity gradient of the plain frame is another one
    pc = _model()
    res = fd.render(cam, pc, _Pipe(False), bg, stage="fine")
    (res["render"] * w).sum().backward()
    diff = rel_l2(_param_grads(pc)["_opacity"].cpu().numpy(), ga["_opacity"].cpu().numpy())
    print(f"_opacity gradient, plain vs antialiased: rel-L2 {diff:.2f}")
    assert diff > 1e-2 and torch.equal(res["radii"], ra["radii"]) and not torch.equal(res["render"], ra["render"])


def test_render_through_the_implicit_permutation_and_render_views(monkeypatch):
    fd = _fd()
    cam, bg, w = _cam(), torch.zeros(3, device=_dev()), _weights()
    outs = {}
    for implicit in (False, True):
        monkeypatch.setattr(fd.renderer, "IMPLICIT_ORDER_MIN_N", 0 if implicit else 1 << 30)
        pc = _model()
        res = fd.render(cam, pc, _Pipe(), bg, stage="fine")
        (res["render"] * w).sum().backward()
        outs[implicit] = (res, _param_grads(pc))
    (ra, ga), (rb, gb) = outs[False], outs[True]
    assert torch.equal(ra["render"], rb["render"]) and torch.equal(ra["radii"], rb["radii"])
    for k in ga:
        assert rel_l2(gb[k].cpu().numpy(), ga[k].cpu().numpy()) < 2e-5, k
    monkeypatch.setattr(fd.renderer, "IMPLICIT_ORDER_MIN_N", 1 << 30)
    cams = [synthetic.make_camera(96, 80, theta_deg=-40.0 + 50.0 * v, time=0.2 + 0.3 * v).to(_dev()) for v in range(3)]
    ws = [_weights(seed=40 + v) for v in range(3)]
    pc = _model()
    res_a = fd.render_views(cams, pc, _Pipe(), bg, stage="fine")
    sum((r["render"] * x).sum() for r, x in zip(res_a, ws)).backward()
    g_a = _param_grads(pc)
    for p in pc.parameters():
        p.grad = None
    res_b = [fd.render(c, pc, _Pipe(), bg, stage="fine") for c in cams]
    sum((r["render"] * x).sum() for r, x in zip(res_b, ws)).backward()
    g_b = _param_grads(pc)
    for a, b in zip(res_a, res_b):
        assert torch.equal(a["render"], b["render"]) and torch.equal(a["radii"], b["radii"])
    assert max(rel_l2(g_a[k].cpu().numpy(), g_b[k].cpu().numpy()) for k in g_a) < 2e-5
    plain = fd.render_views(cams, pc, _Pipe(False), bg, stage="fine")
    assert not torch.equal(plain[0]["render"], res_a[0]["render"])


# ---- 12. the camera's gradient ---------------------------------------------------------------------------------------------------------------

def test_camera_gradient_against_float64_autograd_and_the_host_twin():
    """The kernel on a seeded accumulator (the layout of csrc/render.hip: xy, conic, opacity, rgb, depth), against the host twin on the same
    sums and against float64 autograd, at the bound of tests/test_gpu_camera_grad.py (1e-3 per group)."""
    fd = _fd()
    L, lib = fd._lib, fd._lib.lib()
    dev = _dev()
    sc = AC.inputs(1000, "sh16")
    P = 1000
    *_, st = _forward(sc)
    torch.cuda.synchronize()
    tw, p, keep = AC.twin_forward(sc, 1.0)
    h, r, cl, vis = AC.h64(sc, 1.0)
    seen = _geom(st, 5, (P,), torch.int32, dev) > 0
    mask = (vis & (tw["tiles"] > 0) & seen).astype(np.float64)
    w = AC.weights(sc, tw["radii"])
    s = AC.sums_f32(w, mask)
    acc = np.zeros((P, 16), np.float32)
    acc[:, 0:2], acc[:, 2:5], acc[:, 5], acc[:, 6:9], acc[:, 9] = s["xy"], s["conic"], s["opacity"], s["rgb"], s["depth"]
    acc_d = torch.tensor(acc, device=dev)
    got = fd.rasterizer.camera_gradients(st, acc_d).cpu().numpy().astype(np.float64)
    twin = AC.twin_camera(p, tw, s)
    _, ref = AC.autograd(sc, 1.0, w, mask)
    view = lambda v: v[:16].reshape(4, 4)[:, :3]
    proj = lambda v: v[16:32].reshape(4, 4)[:, (0, 1, 3)]
    for k, f in (("view", view), ("proj", proj), ("campos", lambda v: v[32:35])):
        e_ref, e_twin = rel_l2(f(got), f(ref)), rel_l2(f(got), f(twin))
        print(f"   {k:6s} device vs float64 {e_ref:.2e}   device vs host twin {e_twin:.2e}")
        assert e_ref < AC.GRAD_BOUND and e_twin < AC.GRAD_BOUND, (k, e_ref, e_twin)
    # the plain call on the same accumulator gives another view gradient: the compensation's share is in the antialiased one
    st.antialiasing = False
    plain = fd.rasterizer.camera_gradients(st, acc_d).cpu().numpy().astype(np.float64)
    assert rel_l2(view(plain), view(got)) > 1e-2 and np.array_equal(proj(plain), proj(got))


# ---- 13. playback -------------------------------------------------------------------------------------------------------------------------------

def test_playback_renders_the_antialiased_frame_of_render():
    fd = _fd()
    P_, C_ = fd.playback, fd.compose
    cam, bg = _cam(), torch.zeros(3, device=_dev())
    pc = _model()
    with torch.no_grad():
        live = fd.render(cam, pc, _Pipe(), bg, stage="fine")
        plain = fd.render(cam, pc, _Pipe(False), bg, stage="fine")
    assert not torch.equal(live["render"], plain["render"])
    baked = P_.bake(pc, [0.3])
    objs = {"Baked": baked, "SparseBaked": P_.bake_sparse(pc, [0.3], tol=-1.0), "Composite": C_.compose([baked])}
    for name, obj in objs.items():
        out = obj.render(cam, _Pipe(), bg)
        assert torch.equal(out["render"], live["render"]) and torch.equal(out["depth"], live["depth"]), name
        assert torch.equal(out["radii"], live["radii"]), name
        assert torch.equal(obj.render(cam, _Pipe(False), bg)["render"], plain["render"]), name
    # a unit channel blended over the antialiased frame's lists is its alpha
    with torch.no_grad():
        pipe = _Pipe()
        pipe.render_alpha = True
        alpha = fd.render(cam, pc, pipe, bg, stage="fine")["alpha"]
    ones = torch.ones(pc._xyz.shape[0], device=_dev())
    f = baked.render_features(cam, _Pipe(), bg, ones)
    # (the pass's alpha IS the blend of a channel of ones, bit for bit -- tests/test_gpu_features.py; the frame's own alpha image is
    # 1 - final_T, the same sum in another association)
    assert torch.equal(f["features"], f["alpha"]) and torch.equal(f["render"], live["render"])
    assert float((f["alpha"] - alpha).abs().max()) < 1e-6
    g = baked.render_features(cam, _Pipe(False), bg, ones)
    assert float((g["alpha"] - f["alpha"]).abs().max()) > 1e-3


# ---- 14. behaviour, by ordering only -----------------------------------------------------------------------------------------------------------

def test_a_distant_frame_is_nearer_to_the_box_filtered_truth_with_the_switch_on():
    """Sub-pixel splats at a quarter of the resolution: the mean alpha of the small frame is compared with the mean alpha of the full
    frame (what a box filter of it keeps).  No threshold: only which of the two is nearer."""
    fd = _fd()
    bg = torch.zeros(3, device=_dev())
    pc = _model(n=4000, shrink=2.0)
    means = {}
    for name, (W, H), aa in (("full", (384, 320), False), ("small off", (96, 80), False), ("small on", (96, 80), True)):
        pipe = _Pipe(aa)
        pipe.render_alpha = True
        with torch.no_grad():
            means[name] = float(fd.render(_cam(W, H), pc, pipe, bg, stage="fine")["alpha"].mean())
    print("mean alpha: " + ", ".join(f"{k} {v:.4f}" for k, v in means.items()))
    assert abs(means["small on"] - means["full"]) < abs(means["small off"] - means["full"])
    assert means["small on"] < means["small off"]


def test_large_splats_are_left_alone():
    """Splats far larger than the dilation (every h above 0.99; here 1 - h is a few 1e-7): on and off differ by less than the bound the
    forward is held to against the oracle."""
    sc = dict(AC.inputs(257, "sh16"))
    sc["scales"] = np.full_like(sc["scales"], 30.0)
    sc["opacities"] = (0.2 * sc["opacities"]).astype(np.float32)
    h, r, cl, vis = AC.h64(sc, 1.0)
    assert vis.sum() > 200 and h[vis].min() > 0.99
    c0, _, d0, _ = _forward(sc, aa=False)
    c1, _, d1, _ = _forward(sc, aa=True)
    d = (c0 - c1).abs().cpu().numpy()
    print(f"all h > 0.99: colour on vs off mean {d.mean():.2e}, 0.9999-quantile {np.quantile(d, 0.9999):.2e}, max {d.max():.2e}; "
          f"1 - min h {1.0 - h[vis].min():.1e}")
    assert d.mean() < 2e-6 and np.quantile(d, 0.9999) < 5e-5


# ---- 15. nothing to draw ----------------------------------------------------------------------------------------------------------------------

def test_empty_and_all_culled_sets():
    fd = _fd()
    R = fd.rasterizer
    dev = _dev()
    sc = AC.inputs(257, "sh16")
    rs = _settings(sc, dev)
    z = lambda *s: torch.zeros(*s, device=dev, requires_grad=True)
    t = dict(means3D=z(0, 3), means2D=z(0, 3), shs=z(0, 16, 3), opacities=z(0, 1), scales=z(0, 3), rotations=z(0, 4))
    rast = R.GaussianRasterizer(rs, render_alpha=True)
    rast.antialiasing = True
    color, radii, depth, alpha = rast(**t)
    assert not alpha.any() and torch.equal(color, torch.ones_like(color)) and not depth.any()
    (alpha.sum() + color.sum()).backward()
    assert all(t[k].grad is not None and t[k].grad.shape == t[k].shape for k in ("means3D", "opacities"))
    far = (torch.tensor(sc["means3D"], device=dev) * 0 + 50.0).requires_grad_(True)
    op = torch.tensor(sc["opacities"], device=dev, requires_grad=True)
    s = _settings(sc, dev)
    s = s._replace(viewmatrix=s.viewmatrix.clone().requires_grad_(True))
    rast = R.GaussianRasterizer(s, render_alpha=True)
    rast.antialiasing = True
    color, radii, depth, alpha = rast(means3D=far, means2D=torch.zeros(257, 3, device=dev), shs=torch.tensor(sc["shs"], device=dev), opacities=op,
                                      scales=torch.tensor(sc["scales"], device=dev), rotations=torch.tensor(sc["rotations"], device=dev))
    assert (radii == 0).all() and not alpha.any() and torch.equal(color, torch.ones_like(color))
    (alpha * torch.randn_like(alpha) + color.sum(0, keepdim=True)).sum().backward()
    assert not far.grad.any() and not op.grad.any() and not s.viewmatrix.grad.any()
