"""The accumulated-opacity image (alpha = 1 - final transmittance) of the HIP rasterizer and of render(), forward and backward, on the GPU.

The reference needs no oracle change: alpha does not depend on colour, so for a scene S the TWIN S' -- same geometry, colors_precomp = (1, 0, 0)
per row, bg = 0, no SH -- has color[0] = sum of the blend weights = alpha, and RasterOracle(S').backward((G_A, 0, 0)) is the gradient of
sum(G_A * alpha).  By linearity a loss on colour, depth and alpha together is the sum of the oracle's run on S and its run on S'.  All
gradient references are float64 (the project's one gradient reference).

The scenes are ones where alpha MOVES (the suite's usual scenes are opaque: a wrong alpha path would pass any mixed-loss test there); each
test asserts its scene's condition from the oracle before it compares, so a change of the generator cannot hollow the test."""
import functools
import importlib
import math

import numpy as np
import pytest

from conftest import set_knob
import torch

from oracle.raster_oracle import RasterOracle
from scenes import raster_scene, rel_l2
from test_gpu_raster import _img, _settings

pytestmark = pytest.mark.gpu
synthetic = importlib.import_module("4dgaussians_amd.synthetic")

GRAD_BOUND = 1e-3          # rel-L2 of a gradient group against the float64 oracle (tests/test_gpu_raster.py::test_backward_parity)
GROUPS = ("means2D", "means3D", "opacities", "scales", "rotations")
SCENES = {
    "A": dict(n=150, width=72, height=56, seed=5, theta=20.0),                          # 72 x 56: partial tiles on both edges
    "B": dict(n=700, width=201, height=77, seed=1, theta=-100.0, scale_boost=0.6),      # a ragged wide image
    "C": dict(n=400, width=72, height=56, seed=5, theta=20.0),                          # lists longer than one 128-entry round, saturated pixels
}


def _fd():
    return importlib.import_module("4dgaussians_amd")


def _dev():
    return torch.device("cuda:0")


def _twin(sc):
    """S': the geometry of S with unit red colours over black -- its red channel is alpha."""
    tw = {k: v for k, v in sc.items() if k != "shs"}
    tw["colors_precomp"] = np.tile(np.array([1.0, 0.0, 0.0], np.float32), (sc["means3D"].shape[0], 1))
    tw["bg"] = np.zeros(3, np.float32)
    return tw


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(scene, float64 oracle of S, float64 oracle of S', alpha of the oracle [H,W], n_contrib): computed once, read-only."""
    sc = raster_scene(**SCENES[name])
    o = RasterOracle(**sc, dtype=np.float64)
    ot = RasterOracle(**_twin(sc), dtype=np.float64)
    fT, nc = o.image_state()
    alpha = 1.0 - fT
    assert np.abs(ot.color[0] - alpha).max() < 1e-12 and np.abs(ot.color[1:]).max() == 0.0      # the twin's red channel IS alpha
    return sc, o, ot, alpha, nc


def _scene_condition(name):
    """What makes the scene a test of alpha, asserted from the oracle."""
    _, _, _, alpha, nc = _reference(name)
    mid = float(((alpha >= 0.05) & (alpha <= 0.95)).mean())
    sat = float((alpha > 0.999).mean())
    print(f"scene {name}: share of pixels with alpha in [0.05, 0.95] {mid:.2f}, with alpha > 0.999 {sat:.2f}, max n_contrib {int(nc.max())}")
    if name == "A":
        assert mid >= 0.25
    elif name == "B":
        assert mid >= 0.30
    else:
        assert sat >= 0.40 and int(nc.max()) > 128


def _inputs(sc, grad=False):
    t = {k: torch.tensor(sc[k], device=_dev(), requires_grad=grad) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    return t


def _forward(sc, want_alpha, settings=None, **kw):
    R = _fd().rasterizer
    t = _inputs(sc)
    extra = {"want_alpha": True} if want_alpha else {}
    return R.rasterize_forward(settings or _settings(sc, _dev(), debug=False), t["means3D"], t["shs"], None, t["opacities"], t["scales"],
                               t["rotations"], None, **extra, **kw)


def _final_T(state):
    return torch.tensor(_img(state, 0, (1, state.params.H, state.params.W), torch.float32, _dev()))


def _alpha_against_the_oracle(alpha, ref, tag):
    d = np.abs(alpha.cpu().numpy()[0].astype(np.float64) - ref)
    print(f"[{tag}] alpha vs float64 oracle: mean {d.mean():.2e}, 0.9999-quantile {np.quantile(d, 0.9999):.2e}, max {d.max():.2e}")
    assert d.mean() < 2e-6 and np.quantile(d, 0.9999) < 5e-5      # the bounds test_stagewise_forward_parity puts on colour: the same sum, unit colours


# ---- 1. forward ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_forward_alpha_is_one_minus_final_T_and_changes_nothing_else(name, form, monkeypatch):
    """Both inner loops of the blending forward, the blocking exact path and the speculative one-call path: colour, depth and radii of a frame
    with alpha are the bits of a frame without, alpha is bit for bit 1 - final_T of the frame's own state, and it is the oracle's alpha."""
    R = _fd().rasterizer
    _scene_condition(name)
    sc, _, _, ref, _ = _reference(name)
    set_knob("blend_fwd_form", form)
    for path in ("exact", "auto"):
        monkeypatch.setattr(R, "BINNING", path)
        if path == "auto":       # the exact frames above fed the predictor: these are queued by the one call
            assert (_dev().index, sc["image_width"], sc["image_height"], sc["means3D"].shape[0]) in R._seen
        c0, r0, d0, st0 = _forward(sc, False)
        c1, r1, d1, a1, st1 = _forward(sc, True)
        torch.cuda.synchronize()
        if path == "auto":
            assert st1.capacity % 4096 == 0 and st1.capacity >= st1.num_rendered > 0
        else:
            assert st1.capacity == st1.num_rendered
        assert st1.with_alpha and not st0.with_alpha
        assert torch.equal(c0, c1) and torch.equal(d0, d1) and torch.equal(r0, r1), (name, form, path)
        assert a1.shape == (1, sc["image_height"], sc["image_width"]) and a1.dtype == torch.float32
        assert torch.equal(a1.cpu(), 1.0 - _final_T(st1)), (name, form, path)
        _alpha_against_the_oracle(a1, ref, f"{name} form {form} {path}")


def test_forward_alpha_of_a_frame_that_overflowed_its_capacity_is_the_exact_alpha(monkeypatch):
    """A speculative frame that lists more pairs than its binning buffer holds is finished exactly before rasterize_forward returns
    (tests/test_gpu_raster.py::test_capacity_overflow_in_the_default_mode_returns_the_exact_frame): the alpha image too."""
    R = _fd().rasterizer
    sc = raster_scene(20000, 416, 304, seed=22, scale_boost=2.0)      # (that test's scene: more pairs than the smallest capacity holds)
    key = (_dev().index, sc["image_width"], sc["image_height"], sc["means3D"].shape[0])
    monkeypatch.setattr(R, "BINNING", "exact")
    c0, r0, d0, a0, st0 = _forward(sc, True)
    torch.cuda.synchronize()
    n = st0.num_rendered
    assert n > 40000
    monkeypatch.setattr(R, "BINNING", "auto")
    R._seen[key] = [1, sc["means3D"].shape[0]]
    before = R.capacity_reruns
    out = (torch.full_like(c0, float("nan")), torch.zeros_like(r0), torch.full_like(d0, float("nan")), torch.full_like(a0, float("nan")))
    c1, r1, d1, a1, st1 = _forward(sc, True, out=out)
    torch.cuda.synchronize()
    assert R.capacity_reruns == before + 1 and st1.capacity == n == st1.num_rendered and a1 is out[3]
    assert torch.equal(a1, a0) and torch.equal(c1, c0) and torch.equal(d1, d0) and torch.equal(r1, r0)
    assert torch.equal(a1.cpu(), 1.0 - _final_T(st1))


# ---- 2. / 3. backward against the twin oracle --------------------------------------------------------------------------------------------

def _device_grads(sc, loss_of, bg=None, ppl=None):
    """Gradients of loss_of(color, depth, alpha) through GaussianRasterizer(render_alpha=True) -> ({group: array}, alpha)."""
    R = _fd().rasterizer
    if ppl is not None:
        set_knob("rbwd_ppl", ppl)
    s = dict(sc)
    if bg is not None:
        s["bg"] = np.asarray(bg, np.float32)
    t = _inputs(sc, grad=True)
    means2D = torch.zeros_like(t["means3D"], requires_grad=True)
    color, radii, depth, alpha = R.GaussianRasterizer(_settings(s, _dev()), render_alpha=True)(
        means3D=t["means3D"], means2D=means2D, shs=t["shs"], colors_precomp=None, opacities=t["opacities"], scales=t["scales"],
        rotations=t["rotations"], cov3D_precomp=None)
    loss_of(color, depth, alpha).backward()
    torch.cuda.synchronize()
    g = {k: t[k].grad.cpu().numpy() for k in t}
    g["means2D"] = means2D.grad.cpu().numpy()
    return g, alpha.detach()


def _worst(g, ref, groups, tag):
    errs = {k: rel_l2(g[k], np.asarray(ref[k]).reshape(g[k].shape)) for k in groups}
    print(f"[{tag}] grad rel-L2 vs float64 oracle: " + ", ".join(f"{k}={v:.2e}" for k, v in errs.items()) + f"; worst {max(errs.values()):.2e}")
    for k, v in errs.items():
        assert v < GRAD_BOUND, (tag, k, v)


@pytest.mark.parametrize("ppl", [4, 2, 0])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_backward_of_a_loss_on_alpha_alone(name, ppl):
    """sum(G_A * alpha), seeded normal G_A, through both strip widths and the whole-tile form of the blending backward, against the float64
    oracle of the twin; the SH coefficients get exactly nothing."""
    _scene_condition(name)
    sc, _, ot, _, _ = _reference(name)
    H, W = sc["image_height"], sc["image_width"]
    ga = np.random.default_rng(11).standard_normal((1, H, W)).astype(np.float32)
    ref = ot.backward(np.concatenate([ga, np.zeros((2, H, W), np.float32)]))
    assert np.linalg.norm(ref["opacities"]) > 0 and np.linalg.norm(ref["means3D"]) > 0
    g, _ = _device_grads(sc, lambda c, d, a: (a * torch.tensor(ga, device=_dev())).sum(), ppl=ppl)
    _worst(g, ref, GROUPS, f"{name} rbwd_ppl={ppl} alpha alone")
    assert not g["shs"].any()


@pytest.mark.parametrize("ppl", [4, 2, 0])
@pytest.mark.parametrize("with_depth", [False, True])
def test_backward_of_a_mixed_loss_is_the_sum_of_the_two_oracle_runs(with_depth, ppl):
    """Colour + alpha and colour + depth + alpha on scene A over a WHITE background, where the background term and the alpha term of
    dL/dalpha_i meet in one factor: the reference is the oracle's run on S (colour, depth) plus its run on the twin (alpha)."""
    _scene_condition("A")
    sc, _, ot, _, _ = _reference("A")
    assert tuple(sc["bg"]) == (1.0, 1.0, 1.0)
    o = _reference("A")[1]
    H, W = sc["image_height"], sc["image_width"]
    rng = np.random.default_rng(12)
    dc = rng.standard_normal((3, H, W)).astype(np.float32)
    dd = rng.standard_normal((1, H, W)).astype(np.float32) if with_depth else None
    ga = rng.standard_normal((1, H, W)).astype(np.float32)
    r_s = o.backward(dc, dd)
    r_t = ot.backward(np.concatenate([ga, np.zeros((2, H, W), np.float32)]))
    ratio = np.linalg.norm(r_t["opacities"]) / np.linalg.norm(r_s["opacities"])
    print(f"alpha / colour gradient norm (opacities): {ratio:.2f}")
    assert ratio > 0.05                                          # alpha's share is no rounding error of the sum
    ref = {k: np.asarray(r_s[k], np.float64) + np.asarray(r_t[k], np.float64) for k in GROUPS}
    ref["shs"] = r_s["shs"]
    dev = _dev()

    def loss(c, d, a):
        v = (c * torch.tensor(dc, device=dev)).sum() + (a * torch.tensor(ga, device=dev)).sum()
        return v + (d * torch.tensor(dd, device=dev)).sum() if with_depth else v

    g, _ = _device_grads(sc, loss, ppl=ppl)
    _worst(g, ref, GROUPS + ("shs",), f"A rbwd_ppl={ppl} colour{' + depth' if with_depth else ''} + alpha")


# ---- 4. edges ---------------------------------------------------------------------------------------------------------------------------------

def test_empty_and_all_culled_sets_give_a_zero_alpha_and_zero_gradients():
    R = _fd().rasterizer
    dev = _dev()
    sc = raster_scene(64, 50, 34, seed=5)
    rs = _settings(sc, dev)
    z = lambda *s: torch.zeros(*s, device=dev, requires_grad=True)
    t = dict(means3D=z(0, 3), means2D=z(0, 3), shs=z(0, 16, 3), opacities=z(0, 1), scales=z(0, 3), rotations=z(0, 4))
    color, radii, depth, alpha = R.GaussianRasterizer(rs, render_alpha=True)(**t)
    assert alpha.shape == (1, 34, 50) and not alpha.any() and torch.equal(color, torch.ones_like(color))
    (alpha.sum() + color.sum()).backward()
    assert all(t[k].grad is not None and t[k].grad.shape == t[k].shape for k in ("means3D", "opacities"))      # zero rows
    far = (torch.tensor(sc["means3D"], device=dev) * 0 + 50.0).requires_grad_(True)
    op = torch.tensor(sc["opacities"], device=dev, requires_grad=True)
    color, radii, depth, alpha = R.GaussianRasterizer(rs, render_alpha=True)(
        means3D=far, means2D=torch.zeros(64, 3, device=dev), shs=torch.tensor(sc["shs"], device=dev), opacities=op,
        scales=torch.tensor(sc["scales"], device=dev), rotations=torch.tensor(sc["rotations"], device=dev))
    assert (radii == 0).all() and not alpha.any()
    (alpha * torch.randn(1, 34, 50, device=dev)).sum().backward()
    assert far.grad.shape == (64, 3) and not far.grad.any() and not op.grad.any()


def test_one_gaussian_alpha_is_zero_off_the_splat_and_empty_pixels_pass_no_gradient():
    R = _fd().rasterizer
    dev = _dev()
    sc = raster_scene(1, 40, 24, seed=3)
    sc["means3D"][:] = 0.0                       # at the point the camera looks at
    sc["scales"][:] = 0.12
    sc["opacities"][:] = 0.8
    o = RasterOracle(**sc, dtype=np.float64)
    fT, nc = o.image_state()
    on = nc > 0
    assert 8 < on.sum() < 0.5 * on.size          # a splat, and an empty rest
    near = np.zeros_like(on)                     # the splat and the pixels next to it (where rounding may move the 1/255 cut)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            near |= np.roll(np.roll(on, dy, 0), dx, 1)
    off = torch.tensor(~near, device=dev)[None]
    inner = on.copy()                            # the splat without its rim
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            inner &= np.roll(np.roll(on, dy, 0), dx, 1)
    assert inner.sum() > 4
    t = _inputs(sc, grad=True)
    means2D = torch.zeros(1, 3, device=dev, requires_grad=True)
    color, radii, depth, alpha = R.GaussianRasterizer(_settings(sc, dev), render_alpha=True)(
        means3D=t["means3D"], means2D=means2D, shs=t["shs"], opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"])
    got = alpha.detach()
    assert int(radii[0]) > 0 and float(got.max()) > 0.5
    assert not got[off].any()                    # exactly 0 off the splat
    assert np.abs(got.cpu().numpy()[0] - (1.0 - fT))[inner | ~near].max() < 5e-5
    ga = torch.randn(1, 24, 40, generator=torch.Generator().manual_seed(1)).to(dev) * off
    assert float(ga.abs().sum()) > 0
    (alpha * ga).sum().backward()
    torch.cuda.synchronize()
    for k, v in t.items():
        assert v.grad is not None and not v.grad.any(), k
    assert not means2D.grad.any()


def test_alpha_rendered_but_not_in_the_loss_takes_the_null_path():
    """render_alpha = True with a loss on colour alone: dL_dalpha arrives as None and goes down as NULL; the gradients are those of a frame
    rendered without alpha (to the association of the atomics)."""
    R = _fd().rasterizer
    sc, _, _, _, _ = _reference("A")
    dev = _dev()
    w = torch.randn(3, sc["image_height"], sc["image_width"], generator=torch.Generator().manual_seed(2)).to(dev)
    g1, _ = _device_grads(sc, lambda c, d, a: (c * w).sum())
    t = _inputs(sc, grad=True)
    means2D = torch.zeros_like(t["means3D"], requires_grad=True)
    color, radii, depth = R.GaussianRasterizer(_settings(sc, dev))(means3D=t["means3D"], means2D=means2D, shs=t["shs"], opacities=t["opacities"],
                                                                  scales=t["scales"], rotations=t["rotations"])
    (color * w).sum().backward()
    g0 = {k: v.grad.cpu().numpy() for k, v in t.items()} | {"means2D": means2D.grad.cpu().numpy()}
    for k in g0:
        assert rel_l2(g1[k], g0[k]) < 2e-5, (k, rel_l2(g1[k], g0[k]))


# ---- 5. render() ------------------------------------------------------------------------------------------------------------------------------

class _Pipe:
    def __init__(self, alpha=True, sh=False, cov=False):
        self.convert_SHs_python, self.compute_cov3D_python, self.debug = sh, cov, False
        if alpha:
            self.render_alpha = True


def _model(cfg="dynerf_default", n=1000):
    pc = synthetic.SynthModel(n, cfg, seed=23)
    with torch.no_grad():
        pc._scaling.add_(-1.0)                   # small splats: a translucent frame
    return pc.to(_dev())


def _cam():
    return synthetic.make_camera(96, 80, theta_deg=15.0, time=0.3).to(_dev())


def _mid_share(alpha):
    return float(((alpha >= 0.05) & (alpha <= 0.95)).float().mean())


def _weights(H=80, W=96, seed=4):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(3, H, W, generator=gen).to(_dev()), torch.randn(1, H, W, generator=gen).to(_dev())


def _param_grads(pc):
    return {k: p.grad.clone() for k, p in pc.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("cfg", ["dynerf_default", "dnerf_bouncingballs"])
def test_render_with_alpha_fused_node_equals_two_node_form(cfg, monkeypatch):
    """pipe.render_alpha through the fused fine stage and through the two-node form, loss on render + alpha: images and alpha bit for bit,
    every parameter gradient within 2e-5 rel-L2 and viewspace_points.grad within 1e-6 (the bounds of
    test_fused_backward_node_equals_two_node_form); under no_grad the same bits without a graph."""
    fd = _fd()
    dev = _dev()
    cam, bg = _cam(), torch.zeros(3, device=dev)
    w, wa = _weights()
    out = []
    for fused in (True, False):
        monkeypatch.setattr(fd.renderer, "FUSED_BACKWARD", fused)
        pc = _model(cfg)
        res = fd.render(cam, pc, _Pipe(), bg, stage="fine")
        assert set(res) == {"render", "viewspace_points", "visibility_filter", "radii", "depth", "alpha"} and res["alpha"].shape == (1, 80, 96)
        ((res["render"] * w).sum() + (res["alpha"] * wa).sum()).backward()
        out.append((res, _param_grads(pc), res["viewspace_points"].grad.clone()))
        with torch.no_grad():
            r2 = fd.render(cam, pc, _Pipe(), bg, stage="fine")
        assert torch.equal(r2["alpha"], res["alpha"]) and r2["alpha"].grad_fn is None and not r2["alpha"].requires_grad
        assert torch.equal(r2["render"], res["render"])
        plain = fd.render(cam, pc, _Pipe(alpha=False), bg, stage="fine")
        assert "alpha" not in plain and torch.equal(plain["render"], res["render"]) and torch.equal(plain["depth"], res["depth"])
    (ra, ga, va), (rb, gb, vb) = out
    mid = _mid_share(ra["alpha"])
    print(f"[{cfg}] share of pixels with alpha in [0.05, 0.95]: {mid:.2f}")
    assert mid >= 0.5
    for k in ("render", "depth", "radii", "alpha"):
        assert torch.equal(ra[k], rb[k]), k
    assert set(ga) == set(gb)
    worst = max((rel_l2(ga[k].cpu().numpy(), gb[k].cpu().numpy()), k) for k in ga)
    print(f"[{cfg}] fused vs two-node with alpha in the loss: worst gradient rel-L2 {worst[0]:.1e} ({worst[1]})")
    assert worst[0] < 2e-5
    assert rel_l2(va.cpu().numpy(), vb.cpu().numpy()) < 1e-6
    # alpha's share reached the parameters: the gradients differ from those of the colour loss alone
    pc = _model(cfg)
    res = fd.render(cam, pc, _Pipe(), bg, stage="fine")
    (res["render"] * w).sum().backward()
    assert rel_l2(_param_grads(pc)["_opacity"].cpu().numpy(), ga["_opacity"].cpu().numpy()) > 1e-2


def test_coarse_stage_and_override_color_return_the_rasterizers_alpha():
    fd = _fd()
    dev = _dev()
    pc, cam, bg = _model(), _cam(), torch.zeros(3, device=dev)
    rs = fd.GaussianRasterizationSettings(80, 96, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), bg, 1.0, cam.world_view_transform,
                                          cam.full_proj_transform, pc.active_sh_degree, cam.camera_center, False, False)
    geometry = dict(means3D=pc._xyz, means2D=torch.zeros_like(pc._xyz), opacities=torch.sigmoid(pc._opacity), scales=torch.exp(pc._scaling),
                    rotations=torch.nn.functional.normalize(pc._rotation))
    cols = torch.rand(1000, 3, generator=torch.Generator().manual_seed(0)).to(dev)
    with torch.no_grad():
        img, radii, depth, alpha = fd.GaussianRasterizer(rs, render_alpha=True)(shs=pc.get_features, **geometry)
        img_c, _, _, alpha_c = fd.GaussianRasterizer(rs, render_alpha=True)(colors_precomp=cols, **geometry)
    assert torch.equal(alpha, alpha_c) and _mid_share(alpha) >= 0.5          # (alpha does not depend on colour)
    a = fd.render(cam, pc, _Pipe(), bg, stage="coarse")
    assert torch.equal(a["alpha"], alpha) and torch.equal(a["render"], img) and a["alpha"].requires_grad
    b = fd.render(cam, pc, _Pipe(), bg, stage="coarse", override_color=cols)
    assert torch.equal(b["alpha"], alpha) and torch.equal(b["render"], img_c)
    (a["alpha"].sum() + b["alpha"].sum()).backward()
    assert float(pc._opacity.grad.abs().sum()) > 0 and (pc._features_dc.grad is None or not pc._features_dc.grad.any())
    # the python formulations of SH and covariance hand precomputed arrays to the same rasterizer call
    c = fd.render(cam, pc, _Pipe(sh=True, cov=True), bg, stage="coarse")
    assert c["alpha"].shape == (1, 80, 96) and float((c["alpha"].detach() - alpha).abs().max()) < 1.0 / 255 + 1e-5
    # a PanopticSports dict camera and a foreign deformation module (the non-fused fine stage)
    fine = fd.render(cam, pc, _Pipe(), bg, stage="fine")
    pan = fd.render({"camera": rs, "time": 0.3}, pc, _Pipe(), bg, stage="fine", cam_type="PanopticSports")
    assert torch.equal(pan["alpha"], fine["alpha"])
    from test_gpu_render_branches import _Foreign
    inner = pc._deformation
    pc._deformation = _Foreign(inner)
    foreign = fd.render(cam, pc, _Pipe(), bg, stage="fine")
    pc._deformation = inner
    d = (foreign["alpha"] - fine["alpha"]).detach().abs()    # (torch activations against the kernel's: rounding, single 1/255 crossings)
    assert float(d.mean()) < 1e-6 and float(d.max()) <= 1.05 / 255.0
    foreign["alpha"].sum().backward()


def test_render_with_alpha_through_the_implicit_hilbert_permutation(monkeypatch):
    """A model read through the cached Hilbert permutation of its rows: the frame is the same frame -- alpha is an image, nothing of it is
    permuted -- and the gradients come back in the model's own order.  Alpha is unchanged to the bit: the forward is deterministic and the
    permutation could only reorder list entries of EQUAL depth, of which this seeded scene has none in front of a pixel's stop; gradients within
    2e-5 (the association of the atomics)."""
    fd = _fd()
    dev = _dev()
    cam, bg = _cam(), torch.zeros(3, device=dev)
    w, wa = _weights()
    outs = {}
    for implicit in (False, True):
        monkeypatch.setattr(fd.renderer, "IMPLICIT_ORDER_MIN_N", 0 if implicit else 1 << 30)
        pc = _model()
        assert fd.deformation.spatial_order_hint(pc._xyz) is False
        res = fd.render(cam, pc, _Pipe(), bg, stage="fine")
        ((res["render"] * w).sum() + (res["alpha"] * wa).sum()).backward()
        e = fd.deformation._perm_cache.get(id(pc._xyz))
        assert (e is not None and e[0]() is pc._xyz) == implicit
        outs[implicit] = (res, _param_grads(pc), res["viewspace_points"].grad.clone())
    (ra, ga, va), (rb, gb, vb) = outs[False], outs[True]
    print(f"alpha with vs without the permutation: max difference {float((ra['alpha'] - rb['alpha']).detach().abs().max()):.1e}")
    assert torch.equal(ra["alpha"], rb["alpha"]) and torch.equal(ra["render"], rb["render"])
    assert torch.equal(ra["radii"], rb["radii"])
    for k in ga:
        assert rel_l2(gb[k].cpu().numpy(), ga[k].cpu().numpy()) < 2e-5, k
    assert rel_l2(vb.cpu().numpy(), va.cpu().numpy()) < 2e-5


# ---- 6. render_views ----------------------------------------------------------------------------------------------------------------------------

def test_render_views_with_alpha_equals_per_view_render_with_summed_loss():
    """Three views behind one node with an alpha slice each, against per-view render() with the losses summed: the bounds of
    test_render_views_equals_per_view_render_with_summed_loss."""
    fd = _fd()
    dev = _dev()
    cams = [synthetic.make_camera(160, 120, theta_deg=-60.0 + 70.0 * v, time=0.15 + 0.3 * v).to(dev) for v in range(3)]
    ws = [_weights(120, 160, 40 + v) for v in range(3)]
    bg = torch.zeros(3, device=dev)
    pc = _model(n=1003)
    loss = lambda rs: sum((r["render"] * w).sum() + (r["alpha"] * wa).sum() for r, (w, wa) in zip(rs, ws))
    res_a = fd.render_views(cams, pc, _Pipe(), bg, stage="fine")
    assert all(r["alpha"].shape == (1, 120, 160) for r in res_a)
    loss(res_a).backward()
    ga = _param_grads(pc)
    va = [r["viewspace_points"].grad.clone() for r in res_a]
    for p in pc.parameters():
        p.grad = None
    res_b = [fd.render(c, pc, _Pipe(), bg, stage="fine") for c in cams]
    loss(res_b).backward()
    gb = _param_grads(pc)
    for v, (ra, rb) in enumerate(zip(res_a, res_b)):
        mid = _mid_share(ra["alpha"])
        print(f"view {v}: share of pixels with alpha in [0.05, 0.95] {mid:.2f}")
        assert mid >= 0.5
        for key in ("render", "depth", "radii", "visibility_filter", "alpha"):
            assert torch.equal(ra[key], rb[key]), key
    assert set(ga) == set(gb)
    worst = max((rel_l2(ga[k].cpu().numpy(), gb[k].cpu().numpy()), k) for k in ga)
    print(f"[3 views, alpha] batched node vs per-view graphs: worst gradient rel-L2 {worst[0]:.1e} ({worst[1]})")
    assert worst[0] < 2e-5
    for v in range(3):
        assert rel_l2(va[v].cpu().numpy(), res_b[v]["viewspace_points"].grad.cpu().numpy()) < 1e-6


# ---- 7. camera ------------------------------------------------------------------------------------------------------------------------------------

def test_camera_gradient_of_a_loss_on_alpha_is_the_twin_frames_colour_loss_gradient():
    """A frame whose camera tensors require grad, loss on alpha alone: dL/dviewmatrix and dL/dprojmatrix are the device's own colour-loss
    camera gradients of the twin frame (dL_dcolor = (G_A, 0, 0)) within 2e-5, the bound tests/test_gpu_camera_grad.py uses between device
    forms; alpha does not depend on the camera's position other than through the matrices: dL/dcampos is exactly zero."""
    R = _fd().rasterizer
    dev = _dev()
    sc, _, _, _, _ = _reference("A")
    H, W = sc["image_height"], sc["image_width"]
    ga = torch.tensor(np.random.default_rng(13).standard_normal((1, H, W)).astype(np.float32), device=dev)
    tw = _twin(sc)

    def settings(s):
        rs = _settings(s, dev)
        for k in ("viewmatrix", "projmatrix", "campos"):
            getattr(rs, k).requires_grad_(True)
        return rs

    t = _inputs(sc)
    rs_a = settings(sc)
    color, radii, depth, alpha = R.GaussianRasterizer(rs_a, render_alpha=True)(
        means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), shs=t["shs"], opacities=t["opacities"], scales=t["scales"],
        rotations=t["rotations"])
    assert type(alpha.grad_fn).__name__ == "_RasterizeGaussiansCameraBackward"
    (alpha * ga).sum().backward()
    rs_t = settings(tw)
    color_t, _, _ = R.GaussianRasterizer(rs_t)(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]),
                                               colors_precomp=torch.tensor(tw["colors_precomp"], device=dev), opacities=t["opacities"],
                                               scales=t["scales"], rotations=t["rotations"])
    # the twin's red channel is alpha on the device too (a float32 sum of the weights against 1 - the product: rounding apart)
    assert float((color_t[0:1] - alpha).detach().abs().max()) < 1e-5
    (color_t[0:1] * ga).sum().backward()
    torch.cuda.synchronize()
    for k in ("viewmatrix", "projmatrix"):
        a, b = getattr(rs_a, k).grad.cpu().numpy(), getattr(rs_t, k).grad.cpu().numpy()
        assert np.linalg.norm(b) > 0
        print(f"camera gradient of the alpha loss, {k}: rel-L2 vs the twin's colour loss {rel_l2(a, b):.1e}")
        assert rel_l2(a, b) < 2e-5, k
    assert rs_a.campos.grad is not None and not rs_a.campos.grad.any()


# ---- 8. a fit --------------------------------------------------------------------------------------------------------------------------------------

def test_a_mask_loss_on_alpha_moves_the_opacities_the_right_way():
    """Everything frozen but _opacity, 30 Adam steps on l1_loss(alpha, mask) towards a half-plane mask: the loss goes down (the sign)."""
    fd = _fd()
    dev = _dev()
    pc, cam, bg = _model(), _cam(), torch.zeros(3, device=dev)
    for p in pc.parameters():
        p.requires_grad_(False)
    pc._opacity.requires_grad_(True)
    mask = torch.zeros(1, 80, 96, device=dev)
    mask[:, :, :48] = 1.0
    opt = torch.optim.Adam([pc._opacity], lr=0.1)
    losses = []
    for _ in range(30):
        opt.zero_grad(set_to_none=True)
        loss = fd.losses.l1_loss(fd.render(cam, pc, _Pipe(), bg, stage="fine")["alpha"], mask)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print(f"mask loss on alpha: {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert losses[-1] < losses[0]
