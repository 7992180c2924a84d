"""The absolute screen-space gradients (fdgs_raster_bwd_abs, pipe.absgrad) on the GPU: every form of the blending backward against the
per-pixel float64 reference of tests/absgrad_common.py, the structure of the result, that not asking changes nothing, render() /
render_views on every route, and the densification statistic.

Bounds.  means2D_abs[:, :2] against the reference: group rel-L2 <= 1e-3, the project's gradient bound (tests/test_gpu_raster.py::
test_backward_parity); the signed gradients of the SAME call are held to the same oracle at the same bound, so asking does not degrade them
(an antialiased frame: means2D and the SH coefficients only -- the oracle on premultiplied opacities has the blend's share of the other
groups, not the compensation's own chain rule, which tests/test_gpu_antialias.py covers).  |signed| <= abs (1 + 1e-4) componentwise: both
are float32 sums of the same at most H W = 960 terms, and n 2^-24 = 5.7e-5.  The per-row maximum relative error is printed, not asserted.

Measured on MI355X over the 36 parity cases: means2D_abs rel-L2 1.5e-7 .. 2.3e-7, worst single row 4.6e-6 relative; the signed groups of the
same call 5.0e-7 .. 8.4e-7; render(): fused against two-node 5.0e-8 (fine), 2.0e-9 (coarse)."""
import importlib

import numpy as np
import pytest
import torch

import absgrad_common as AG
from conftest import set_knob
from scenes import rel_l2
from test_gpu_raster import _settings

pytestmark = pytest.mark.gpu
synthetic = importlib.import_module("4dgaussians_amd.synthetic")

GRAD_BOUND = 1e-3
LOSSES = {"color": (False, False), "color+depth": (True, False), "color+depth+alpha": (True, True)}


def _fd():
    return importlib.import_module("4dgaussians_amd")


def _dev():
    return torch.device("cuda:0")


def _call(sc, grads, with_depth, with_alpha, aa, absgrad=True, ppl=None):
    """rasterize_forward + rasterize_backward of the scene dict `sc` -> (gradient dict as numpy, radii, the state)."""
    R = _fd().rasterizer
    if ppl is not None:
        set_knob("rbwd_ppl", ppl)
    dev = _dev()
    t = {k: torch.tensor(sc[k], device=dev) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    kw = {k: True for k, v in (("want_alpha", with_alpha), ("antialiasing", aa), ("absgrad", absgrad)) if v}
    out = R.rasterize_forward(_settings(sc, dev, debug=False), t["means3D"], t["shs"], None, t["opacities"], t["scales"], t["rotations"], None,
                              expect_backward=True, **kw)
    state, radii = out[-1], out[1]
    dc, dd, ga = (torch.tensor(g, device=dev) for g in grads)
    bkw = {"grad_alpha": ga} if with_alpha else {}
    g = R.rasterize_backward(state, dc, dd if with_depth else None, **bkw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in g.items() if v is not None}, radii.cpu().numpy(), state


def _signed_reference(name, with_depth, with_alpha, aa):
    """The float64 oracle's full gradients of the same loss: its run on S plus, with alpha, its run on the twin (tests/test_gpu_alpha.py)."""
    dc, dd, ga = AG.image_grads(name)
    o, ot = AG.oracles(name, aa)
    ref = o.backward(dc, dd[0] if with_depth else None)
    if with_alpha:
        rt = ot.backward(np.concatenate([ga, np.zeros_like(dc[:2])]))
        ref = {k: (v if k in ("shs", "colors") else np.asarray(v, np.float64) + np.asarray(rt[k], np.float64)) for k, v in ref.items()}
    return ref


def _structure(g, radii, blended, tag):
    a, s = g["means2D_abs"], g["means2D"]
    assert a.shape == s.shape and a.dtype == np.float32
    assert not a[:, 2].any() and not np.signbit(a[:, 2]).any()                           # the third column: exactly +0
    dead = (radii == 0) | ~blended
    assert not a[dead].any() and not np.signbit(a[dead]).any(), tag                      # culled rows and rows no pixel blended: exactly +0
    assert (a >= 0).all() and (np.abs(s[:, :2]) <= a[:, :2] * (1 + 1e-4)).all(), tag


# ---- 1. parity -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("aa", [False, True], ids=["plain", "antialiased"])
@pytest.mark.parametrize("loss", sorted(LOSSES))
@pytest.mark.parametrize("ppl", [0, 2, 4])
@pytest.mark.parametrize("name", ["S", "L"])
def test_parity_with_the_per_pixel_reference(name, ppl, loss, aa):
    AG.assert_scene_condition(name)
    with_depth, with_alpha = LOSSES[loss]
    a_ref, s_ref, blended = AG.reference(name, with_depth, with_alpha, aa)
    g, radii, _ = _call(AG.scene(name), AG.image_grads(name), with_depth, with_alpha, aa, ppl=ppl)
    tag = f"{name} rbwd_ppl={ppl} {loss} {'aa' if aa else 'plain'}"
    a = g["means2D_abs"][:, :2].astype(np.float64)
    live = a_ref.sum(1) > 0
    row = np.abs(a - a_ref)[live].max(1) / a_ref[live].max(1)
    e_abs, e_sgn = rel_l2(a, a_ref), rel_l2(g["means2D"][:, :2], s_ref)
    print(f"[{tag}] means2D_abs rel-L2 {e_abs:.2e}, per-row max relative error {row.max():.2e} (median {np.median(row):.2e}); "
          f"signed means2D rel-L2 {e_sgn:.2e}")
    assert e_abs <= GRAD_BOUND and e_sgn <= GRAD_BOUND, (tag, e_abs, e_sgn)
    _structure(g, radii, blended, tag)
    # the signed gradients of the same call against the same oracle: asking does not degrade them
    ref = _signed_reference(name, with_depth, with_alpha, aa)
    groups = ("means2D", "shs") if aa else ("means2D", "means3D", "opacities", "scales", "rotations", "shs")
    errs = {k: rel_l2(g[k], np.asarray(ref[k]).reshape(g[k].shape)) for k in groups}
    print(f"[{tag}] signed groups vs float64 oracle: " + ", ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= GRAD_BOUND, (tag, errs)


# ---- 2. structure and edges ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ppl", [0, 2, 4])
def test_one_row(ppl):
    a_ref, s_ref, blended = AG.reference("1", True, True)
    g, radii, _ = _call(AG.scene("1"), AG.image_grads("1"), True, True, False, ppl=ppl)
    assert g["means2D_abs"].shape == (1, 3) and g["means2D_abs"][0, :2].min() > 0
    assert rel_l2(g["means2D_abs"][:, :2], a_ref) <= GRAD_BOUND
    _structure(g, radii, blended, f"one row rbwd_ppl={ppl}")


def test_culled_rows_and_an_empty_set():
    R = _fd().rasterizer
    dev = _dev()
    sc = dict(AG.scene("S"))
    sc["means3D"] = sc["means3D"].copy()
    sc["means3D"][::3] = 50.0                                      # every third row far outside the frustum
    g, radii, _ = _call(sc, AG.image_grads("S"), True, False, False)
    assert (radii[::3] == 0).all() and (radii > 0).any()
    _structure(g, radii, np.ones(len(radii), bool), "culled")
    assert g["means2D_abs"][radii > 0].any()
    # P = 0: an empty tensor, no launch fault
    z = lambda *s: torch.zeros(*s, device=dev)
    *_, state = R.rasterize_forward(_settings(sc, dev, debug=False), z(0, 3), z(0, 16, 3), None, z(0, 1), z(0, 3), z(0, 4), None, absgrad=True)
    g0 = R.rasterize_backward(state, z(3, 24, 40))
    torch.cuda.synchronize()
    assert g0["means2D_abs"].shape == (0, 3) and g0["means2D"].shape == (0, 3)


# ---- 3. not asking changes nothing ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ppl", [0, 2, 4])
def test_the_accumulator_slots(ppl, monkeypatch):
    R = _fd().rasterizer
    seen = []
    real = R.fill_raster_grads
    monkeypatch.setattr(R, "fill_raster_grads", lambda *a, **k: (lambda r: (seen.append(r[1]), r)[1])(real(*a, **k)))
    g, _, state = _call(AG.scene("L"), AG.image_grads("L"), True, False, False, absgrad=False, ppl=ppl)
    assert "means2D_abs" not in g and state.absgrad is False
    acc = seen[-1].cpu().numpy()
    assert acc.shape == (400, 16) and acc[:, :10].any() and not acc[:, 10:].any()        # slots 10..15: still the zeros they were filled with
    g, _, state = _call(AG.scene("L"), AG.image_grads("L"), True, False, False, ppl=ppl)
    acc = seen[-1].cpu().numpy()
    assert acc[:, 10].any() and acc[:, 11].any() and not acc[:, 12:].any()               # with the option: 10 and 11, nothing behind them
    W, H = 40, 24
    assert np.array_equal(g["means2D_abs"][:, 0], acc[:, 10] * np.float32(0.5) * np.float32(W))
    assert np.array_equal(g["means2D_abs"][:, 1], acc[:, 11] * np.float32(0.5) * np.float32(H))
    # a second backward of the same state fills its own accumulator: the same sums, not twice them
    dc, dd, _ = (torch.tensor(x, device=_dev()) for x in AG.image_grads("L"))
    g2 = R.rasterize_backward(state, dc, dd)["means2D_abs"].cpu().numpy()
    assert rel_l2(g2, g["means2D_abs"]) < 1e-5


# ---- 4. render() and render_views ---------------------------------------------------------------------------------------------------------------

class _Pipe:
    convert_SHs_python = compute_cov3D_python = debug = False

    def __init__(self, absgrad=True, **kw):
        self.absgrad = absgrad
        self.__dict__.update(kw)


def _model(n=1000):
    pc = synthetic.SynthModel(n, "dynerf_default", seed=23)
    with torch.no_grad():
        pc._scaling.add_(1.0)                     # large footprints: the rows whose signed sum cancels
    return pc.to(_dev())


def _cam(theta=15.0, time=0.3):
    return synthetic.make_camera(96, 80, theta_deg=theta, time=time).to(_dev())


def _weights(seed=4):
    return torch.randn(3, 80, 96, generator=torch.Generator().manual_seed(seed)).to(_dev())


def _frame(pc, stage="fine", pipe=None, w=None, **kw):
    res = _fd().render(_cam(), pc, pipe or _Pipe(), torch.zeros(3, device=_dev()), stage=stage, **kw)
    (res["render"] * (_weights() if w is None else w)).sum().backward()
    torch.cuda.synchronize()
    return res


def _check_sink(vsp, n):
    a, s = vsp.absgrad, vsp.grad
    assert a.shape == (n, 3) and a.dtype == torch.float32 and not a.requires_grad and a.device == s.device
    assert not a[:, 2].any() and bool((s[:, :2].abs() <= a[:, :2] * (1 + 1e-4)).all()) and a.any()
    return a.cpu().numpy()


@pytest.mark.parametrize("stage", ["fine", "coarse"])
def test_render_fused_and_two_node_routes_agree(stage, monkeypatch):
    fd = _fd()
    rows = {}
    for fused in (True, False):
        monkeypatch.setattr(fd.renderer, "FUSED_BACKWARD", fused)
        res = _frame(_model(), stage)
        rows[fused] = _check_sink(res["viewspace_points"], 1000)
    e = rel_l2(rows[True], rows[False])
    print(f"[{stage}] viewspace_points.absgrad, fused vs two-node: rel-L2 {e:.2e}")
    assert e <= GRAD_BOUND
    # the statistic differs from the signed one by much more than the bound: it is not the signed gradient under another name
    res = _frame(_model(), stage)
    s = res["viewspace_points"].grad.abs().cpu().numpy()
    assert rel_l2(rows[True], s) > 0.1
    # a pipe that does not ask: no attribute
    res = _frame(_model(), stage, _Pipe(False))
    assert not hasattr(res["viewspace_points"], "absgrad")


@pytest.mark.parametrize("kw", [dict(convert_SHs_python=True), dict(compute_cov3D_python=True)], ids=["python-sh", "python-cov3d"])
def test_render_python_branches_honour_the_option(kw):
    stage = "coarse" if "compute_cov3D_python" in kw else "fine"
    res = _frame(_model(), stage, _Pipe(**kw))
    _check_sink(res["viewspace_points"], 1000)


def test_render_camera_and_time_nodes_honour_the_option():
    fd = _fd()
    ref = _check_sink(_frame(_model())["viewspace_points"], 1000)
    for leaf in ("camera", "time"):
        pc, cam = _model(), _cam()
        if leaf == "camera":
            cam.world_view_transform = cam.world_view_transform.clone().requires_grad_(True)
        else:
            cam.time = torch.tensor([0.3], device=_dev(), requires_grad=True)
        res = fd.render(cam, pc, _Pipe(), torch.zeros(3, device=_dev()), stage="fine")
        assert leaf.capitalize() in type(res["render"].grad_fn).__name__
        (res["render"] * _weights()).sum().backward()
        assert rel_l2(_check_sink(res["viewspace_points"], 1000), ref) <= GRAD_BOUND


def test_render_through_the_implicit_permutation_returns_the_rows_in_model_order(monkeypatch):
    fd = _fd()
    rows, signed = {}, {}
    for implicit in (False, True):
        monkeypatch.setattr(fd.renderer, "IMPLICIT_ORDER_MIN_N", 0 if implicit else 1 << 30)
        pc = _model()
        assert not fd.deformation.spatial_order_hint(pc._xyz)           # an unordered model: with the switch on it IS read through the permutation
        res = _frame(pc)
        rows[implicit] = _check_sink(res["viewspace_points"], 1000)
        signed[implicit] = res["viewspace_points"].grad.cpu().numpy()
    assert rel_l2(rows[True], rows[False]) <= GRAD_BOUND and rel_l2(signed[True], signed[False]) <= GRAD_BOUND
    # ... and the same model pre-sorted: row i of the sorted model is row perm[i] of this one
    pc = _model()
    perm = fd.deformation.implicit_permutation(pc._xyz, pc._deformation.deformation_net.grid.aabb).long()
    with torch.no_grad():
        for k in ("_xyz", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest"):
            p = getattr(pc, k)
            p.copy_(p[perm].clone())
    monkeypatch.setattr(fd.renderer, "IMPLICIT_ORDER_MIN_N", 1 << 30)
    res = _frame(pc)
    assert rel_l2(_check_sink(res["viewspace_points"], 1000), rows[True][perm.cpu().numpy()]) <= GRAD_BOUND


def test_render_views_equals_two_render_calls(monkeypatch):
    fd = _fd()
    monkeypatch.setattr(fd.renderer, "IMPLICIT_ORDER_MIN_N", 1 << 30)
    bg = torch.zeros(3, device=_dev())
    cams = [_cam(-20.0, 0.2), _cam(35.0, 0.6)]
    ws = [_weights(40), _weights(41)]
    pc = _model()
    res_a = fd.render_views(cams, pc, _Pipe(), bg, stage="fine")
    sum((r["render"] * x).sum() for r, x in zip(res_a, ws)).backward()
    res_b = [fd.render(c, pc, _Pipe(), bg, stage="fine") for c in cams]
    sum((r["render"] * x).sum() for r, x in zip(res_b, ws)).backward()
    rows_a = [_check_sink(r["viewspace_points"], 1000) for r in res_a]
    rows_b = [_check_sink(r["viewspace_points"], 1000) for r in res_b]
    for a, b in zip(rows_a, rows_b):
        assert rel_l2(a, b) <= GRAD_BOUND
    assert rel_l2(rows_a[0], rows_a[1]) > 0.1                            # every view's sink got its OWN rows


def test_a_second_backward_of_a_retained_graph_overwrites(monkeypatch):
    fd = _fd()
    for fused in (True, False):
        monkeypatch.setattr(fd.renderer, "FUSED_BACKWARD", fused)
        pc = _model()
        res = fd.render(_cam(), pc, _Pipe(), torch.zeros(3, device=_dev()), stage="fine")
        loss = (res["render"] * _weights()).sum()
        loss.backward(retain_graph=True)
        first = res["viewspace_points"].absgrad.clone()
        signed = res["viewspace_points"].grad.clone()
        loss.backward()
        vsp = res["viewspace_points"]
        assert rel_l2(vsp.absgrad.cpu().numpy(), first.cpu().numpy()) < 1e-5          # assigned: the same sums, not twice them ...
        assert rel_l2(vsp.grad.cpu().numpy(), 2.0 * signed.cpu().numpy()) < 1e-5      # ... while .grad accumulates, as a gradient does


# ---- 5. densification -----------------------------------------------------------------------------------------------------------------------------

def test_densification_statistic_from_absgrad():
    fd = _fd()
    res = _frame(_model())
    vsp, vis, radii = res["viewspace_points"], res["visibility_filter"], res["radii"]
    n = vsp.shape[0]
    pc = type("Stats", (), {})()
    pc.xyz_gradient_accum, pc.denom, pc.max_radii2D = torch.zeros(n, 1, device=_dev()), torch.zeros(n, 1, device=_dev()), torch.zeros(n, device=_dev())
    fd.densify.add_densification_stats(pc, vsp.absgrad, vis, radii)
    torch.cuda.synchronize()
    want = torch.where(vis, vsp.absgrad[:, :2].double().norm(dim=1), torch.zeros(n, device=_dev(), dtype=torch.float64))
    assert vis.any() and rel_l2(pc.xyz_gradient_accum[:, 0].cpu().numpy(), want.cpu().numpy()) < 1e-6
    assert torch.equal(pc.denom[:, 0], vis.float())
    assert float(pc.xyz_gradient_accum.sum()) > 2.0 * float(torch.where(vis, vsp.grad[:, :2].norm(dim=1), torch.zeros(n, device=_dev())).sum())
