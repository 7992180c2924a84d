"""The frame options together, on the device: the one frame no other test renders -- alpha + antialiasing + camera leaves + a time leaf --
through the fused node against the two-node form, and render_views() of three such cameras (alpha + antialiasing) against per-view
render() with the summed loss.  Run with -m gpu on MI355X.

Bounds, as tests/test_gpu_alpha.py::test_render_with_alpha_fused_node_equals_two_node_form and
tests/test_gpu_time_grad.py::test_render_fused_against_two_node_with_a_time_leaf hold the same routes to: images bit-equal (the forward is
the same calls on the same inputs), gradients 2e-5 rel-L2 (float atomics in launch order), the screen-space gradient 1e-6 (no atomics
between the two forms of one frame).

Measured on MI355X: the joint frame fused against two-node: model gradients 3.9e-7, camera 4.3e-7, dL/dt 8.1e-8, screen-space 6.1e-8;
three views against per-view render(): model gradients 6.0e-7, screen-space 1.3e-7."""
import importlib

import pytest
import torch

from time_grad_common import rel_l2

pytestmark = pytest.mark.gpu
W_, H_, N_ = 100, 76, 1000          # (no multiple of the 16 x 16 tile; 35 tiles)
CAM_KEYS = ("world_view_transform", "full_proj_transform", "camera_center")


class _Pipe:
    convert_SHs_python = compute_cov3D_python = debug = False
    render_alpha = antialiasing = True


def _fd():
    return importlib.import_module("4dgaussians_amd")


def _model(dev):
    pc = _fd().synthetic.SynthModel(N_, "dynerf_default", seed=23)
    with torch.no_grad():
        pc._scaling.add_(1.0)
    return pc.to(dev)


def _weights(dev, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(c, H_, W_, generator=gen).to(dev) for c in (3, 1, 1)]


def _loss(res, weights):
    return sum((res[k] * w).sum() for k, w in zip(("render", "depth", "alpha"), weights))


def _param_grads(pc):
    return {k: p.grad.clone() for k, p in pc.named_parameters() if p.grad is not None}


def _worst(ga, gb):
    assert set(ga) == set(gb)
    return max((rel_l2(ga[k].cpu().numpy(), gb[k].cpu().numpy()), k) for k in ga)


def test_alpha_antialiasing_camera_and_time_leaves_in_one_frame_fused_against_two_node(monkeypatch):
    fd, dev = _fd(), torch.device("cuda:0")

    def run(fused):
        monkeypatch.setattr(fd.renderer, "FUSED_BACKWARD", fused)
        pc = _model(dev)
        cam = fd.synthetic.make_camera(W_, H_, theta_deg=-35.0, time=0.45).to(dev)
        for k in CAM_KEYS:
            setattr(cam, k, getattr(cam, k).clone().requires_grad_(True))
        cam.time = torch.tensor(0.45, device=dev, requires_grad=True)
        res = fd.render(cam, pc, _Pipe(), torch.zeros(3, device=dev), stage="fine")
        _loss(res, _weights(dev, 4)).backward()
        torch.cuda.synchronize()
        return res, _param_grads(pc), {k: getattr(cam, k).grad for k in CAM_KEYS}, cam.time.grad

    (ra, ga, ca, ta), (rb, gb, cb, tb) = run(True), run(False)
    assert type(ra["render"].grad_fn).__name__ == "_FusedRenderTimeFunctionBackward"
    assert type(rb["render"].grad_fn).__name__ == "_RasterizeGaussiansCameraBackward"
    for k in ("render", "depth", "alpha", "radii"):
        assert torch.equal(ra[k], rb[k]), k
    assert int((ra["radii"] > 0).sum()) > 0
    assert ta.shape == tb.shape == () and [tuple(ca[k].shape) for k in CAM_KEYS] == [tuple(cb[k].shape) for k in CAM_KEYS] == [(4, 4), (4, 4), (3,)]
    e_time = abs(float(ta) - float(tb)) / abs(float(tb))
    worst_model, worst_cam = _worst(ga, gb), _worst(ca, cb)
    e_vs = rel_l2(ra["viewspace_points"].grad.cpu().numpy(), rb["viewspace_points"].grad.cpu().numpy())
    print(f"fused vs two-node, alpha + antialiasing + camera + time leaves: model {worst_model[0]:.1e} ({worst_model[1]}), camera {worst_cam[0]:.1e} "
          f"({worst_cam[1]}), dL/dt {float(ta):.6e} vs {float(tb):.6e} rel {e_time:.1e}, viewspace {e_vs:.1e}")
    assert all(float(c.abs().sum()) > 0 for c in ca.values()) and all(float(c.abs().sum()) > 0 for c in cb.values())
    assert float(ta.abs()) > 0 and float(tb.abs()) > 0
    assert worst_model[0] < 2e-5 and worst_cam[0] < 2e-5 and e_time < 2e-5
    assert e_vs < 1e-6


def test_render_views_with_alpha_and_antialiasing_equals_per_view_render_with_summed_loss():
    fd, dev = _fd(), torch.device("cuda:0")
    cams = [fd.synthetic.make_camera(W_, H_, theta_deg=-60.0 + 70.0 * v, time=0.15 + 0.3 * v).to(dev) for v in range(3)]
    ws = [_weights(dev, 40 + v) for v in range(3)]
    bg = torch.zeros(3, device=dev)
    pc = _model(dev)
    loss = lambda rs: sum(_loss(r, w) for r, w in zip(rs, ws))
    res_a = fd.render_views(cams, pc, _Pipe(), bg, stage="fine")
    assert all(r["alpha"].shape == (1, H_, W_) for r in res_a)
    loss(res_a).backward()
    ga = _param_grads(pc)
    for p in pc.parameters():
        p.grad = None
    res_b = [fd.render(c, pc, _Pipe(), bg, stage="fine") for c in cams]
    loss(res_b).backward()
    torch.cuda.synchronize()
    gb = _param_grads(pc)
    for ra, rb in zip(res_a, res_b):
        for k in ("render", "depth", "alpha", "radii", "visibility_filter"):
            assert torch.equal(ra[k], rb[k]), k
        assert int((ra["radii"] > 0).sum()) > 0
    worst = _worst(ga, gb)
    e_vs = max(rel_l2(ra["viewspace_points"].grad.cpu().numpy(), rb["viewspace_points"].grad.cpu().numpy()) for ra, rb in zip(res_a, res_b))
    print(f"[3 views, alpha + antialiasing] batched node vs per-view graphs: worst gradient rel-L2 {worst[0]:.1e} ({worst[1]}), viewspace {e_vs:.1e}")
    assert worst[0] < 2e-5 and e_vs < 2e-5
