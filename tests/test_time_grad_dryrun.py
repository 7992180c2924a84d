"""Host plumbing of the time's gradient (CPU, no kernels), on the fake library of tests/test_host_dryrun.py: which calls ask for
fdgs_deform_time_grad, behind which fdgs_deform_bwd and on which (p, g), and where the gradient arrives.  Nothing is computed."""
import ctypes
import importlib

import pytest
import torch

import test_camera_grad_dryrun as CD
import test_host_dryrun as D
from test_host_dryrun import PARENT_CALLS, _Pipe, _calls_of, _cam, _model

fdgs = importlib.import_module("4dgaussians_amd")
R = fdgs.rasterizer


class _TimeFake(CD._CamFake):
    """The camera dry run's fake, which also answers the scratch size of fdgs_deform_time_grad and notes the (p, g) of every deformation
    backward and time-gradient call."""

    def __init__(self):
        super().__init__()
        self.pg = []       # ("deform_bwd" | "time_grad", p object, g object)

    def __getattr__(self, name):
        fn = super().__getattr__(name)

        def wrapped(*a):
            if name == "fdgs_deform_time_grad_scratch_bytes":
                self.calls.append(name)
                a[-1].value = 512
                return 0
            if name == "fdgs_deform_bwd":
                self.pg.append(("deform_bwd", a[1], a[2]))
            elif name == "fdgs_deform_time_grad":
                self.pg.append(("time_grad", a[1], a[2]))
                assert a[3] is not None and a[3].value and a[4] is not None and a[4].value      # scratch and d_time
            return fn(*a)
        return wrapped


@pytest.fixture
def fake(monkeypatch):
    f = _TimeFake()
    monkeypatch.setattr(fdgs._lib, "lib", lambda: f)
    monkeypatch.setattr(fdgs._lib, "stream_ptr", lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(R, "stream_ptr", lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(fdgs.deformation, "stream_ptr", lambda: ctypes.c_void_p(0), raising=False)
    monkeypatch.setattr(R, "_pinned_words", lambda n: torch.zeros(n, dtype=torch.int32))
    monkeypatch.setattr(R, "_current_stream", lambda dev: type("S", (), {"synchronize": lambda self: None})())
    monkeypatch.setattr(R, "_tls", __import__("threading").local())
    monkeypatch.setattr(R, "_seen", {})
    monkeypatch.setattr(R, "_size_cache", {})
    monkeypatch.setattr(R, "_is_hip_device", lambda dev: True)
    monkeypatch.setattr(fdgs.deformation, "_is_hip_device", lambda dev: True)
    return f


def _paired_time(fake, n_pairs):
    """One fdgs_deform_time_grad directly behind each fdgs_deform_bwd, on that call's p and g."""
    assert len(fake.pg) == 2 * n_pairs, [k for k, _, _ in fake.pg]
    for (k0, p0, g0), (k1, p1, g1) in zip(fake.pg[0::2], fake.pg[1::2]):
        assert (k0, k1) == ("deform_bwd", "time_grad") and p0 is p1 and g0 is g1
    calls = [c for c in fake.calls if c in ("fdgs_deform_bwd", "fdgs_deform_time_grad")]
    assert calls == ["fdgs_deform_bwd", "fdgs_deform_time_grad"] * n_pairs


def _deform_inputs(n=200):
    g = torch.Generator().manual_seed(5)
    return [torch.randn(n, 3, generator=g).requires_grad_(True), torch.rand(n, 3, generator=g).requires_grad_(True),
            torch.randn(n, 4, generator=g).requires_grad_(True), torch.rand(n, 1, generator=g).requires_grad_(True),
            torch.randn(n, 16, 3, generator=g).requires_grad_(True)]


def _deform_calls(fake, time):
    net = _model(50)._deformation
    ins = _deform_inputs()
    fake.calls.clear()
    out = fdgs.deformation.deform(net, *ins[:4], shs=ins[4], time=time, activate=True)
    sum(o.sum() for o in out).backward()
    return " ".join(c[len("fdgs_"):] for c in fake.calls), ins, out


@pytest.mark.parametrize("n", D.SIZES)
@pytest.mark.parametrize("entry", ["render_backward", "render_views", "render_nograd"])
def test_a_float_time_makes_the_calls_of_the_parent(fake, entry, n):
    assert _calls_of(fake, entry, n) == PARENT_CALLS[entry, n]
    assert not any("time_grad" in c for c in fake.calls)


@pytest.mark.parametrize("n", D.SIZES)
def test_a_time_tensor_that_does_not_require_grad_makes_the_calls_of_the_parent(fake, n):
    pc = _model(n)
    cam = _cam(0.5)
    cam.time = torch.tensor(0.5)
    fake.calls.clear()
    res = fdgs.render(cam, pc, _Pipe(), torch.zeros(3), stage="fine")
    assert type(res["render"].grad_fn).__name__ == "_FusedRenderFunctionBackward"
    res["render"].sum().backward()
    assert " ".join(c[len("fdgs_"):] for c in fake.calls) == PARENT_CALLS["render_backward", n]


@pytest.mark.parametrize("n", D.SIZES)
def test_a_time_leaf_outside_grad_mode_makes_the_calls_of_the_no_grad_frame(fake, n):
    pc = _model(n)
    cam = _cam(0.5)
    cam.time = torch.tensor(0.5, requires_grad=True)
    fake.calls.clear()
    with torch.no_grad():
        fdgs.render(cam, pc, _Pipe(), torch.zeros(3), stage="fine")
        fake.calls.append("fdgs_--")
        cam.time = torch.tensor(0.25, requires_grad=True)
        fdgs.render(cam, pc, _Pipe(), torch.zeros(3), stage="fine")
    assert " ".join(c[len("fdgs_"):] for c in fake.calls) == PARENT_CALLS["render_nograd", n]


@pytest.mark.parametrize("n", D.SIZES)
def test_render_views_keeps_taking_the_times_as_numbers(fake, n):
    cams = [_cam(0.1 * i, 10.0 * i) for i in range(3)]
    leaf = torch.tensor(0.1, requires_grad=True)
    cams[1].time = leaf
    fake.calls.clear()
    res = fdgs.render_views(cams, _model(n, "dnerf_bouncingballs", seed=2), _Pipe(), torch.zeros(3), stage="fine")
    sum(r["render"].sum() for r in res).backward()
    assert " ".join(c[len("fdgs_"):] for c in fake.calls) == PARENT_CALLS["render_views", n] and leaf.grad is None


def test_deform_without_a_time_leaf_makes_the_calls_it_made(fake):
    want = "deform_saved_bytes deform_pack_bytes deform_fwd deform_bwd_scratch_bytes deform_bwd"
    calls, _, out = _deform_calls(fake, 0.3)
    assert calls == want and type(out[0].grad_fn).__name__ == "_DeformFunctionBackward"
    calls, _, out = _deform_calls(fake, torch.rand(200, 1))
    assert calls == want and type(out[0].grad_fn).__name__ == "_DeformFunctionBackward"
    with torch.no_grad():
        net = _model(50)._deformation
        ins = [x.detach() for x in _deform_inputs()]
        fake.calls.clear()
        fdgs.deformation.deform(net, *ins[:4], shs=ins[4], time=torch.rand(200, 1, requires_grad=True), activate=True)
    assert [c for c in fake.calls if "time_grad" in c] == []


@pytest.mark.parametrize("shape", [(200, 1), (), (1,)])
def test_deform_with_a_time_leaf(fake, shape):
    T = torch.full(shape, 0.3).requires_grad_(True) if shape != (200, 1) else torch.rand(200, 1).requires_grad_(True)
    calls, ins, out = _deform_calls(fake, T)
    assert calls == "deform_saved_bytes deform_pack_bytes deform_fwd deform_bwd_scratch_bytes deform_bwd deform_time_grad_scratch_bytes deform_time_grad"
    assert type(out[0].grad_fn).__name__ == "_DeformTimeFunctionBackward"
    _paired_time(fake, 1)
    assert T.grad is not None and T.grad.shape == T.shape and all(x.grad is not None and x.grad.shape == x.shape for x in ins)
    p = fake.pg[0][1]
    # one frame time goes down by value (the scalar path), per-Gaussian times as an array
    assert bool(p.time) == (shape == (200, 1)) and (p.time_scalar == pytest.approx(0.3) if shape != (200, 1) else True)


class _AlphaPipe(_Pipe):
    render_alpha = True


@pytest.mark.parametrize("route", ["fused", "two_node", "override_color"])
@pytest.mark.parametrize("frozen", [False, True])
def test_render_with_a_time_leaf(fake, monkeypatch, route, frozen):
    monkeypatch.setattr(fdgs.renderer, "FUSED_BACKWARD", route != "two_node")
    pc = _model(300)
    if frozen:
        pc.requires_grad_(False)
    delta = fdgs.TimeDelta()
    cam = delta.camera(_cam(0.5))
    fake.calls.clear()
    res = fdgs.render(cam, pc, _Pipe(), torch.zeros(3), stage="fine", override_color=torch.rand(300, 3) if route == "override_color" else None)
    res["render"].sum().backward()
    _paired_time(fake, 1)
    assert delta.offset.grad is not None and delta.offset.grad.shape == (1,)
    assert (pc._xyz.grad is None) == frozen and res["viewspace_points"].grad.shape == (300, 3)
    assert fake.pg[0][1].time_scalar == pytest.approx(0.5) and not fake.pg[0][1].time
    if route == "fused":
        assert type(res["render"].grad_fn).__name__ == "_FusedRenderTimeFunctionBackward"
        assert " ".join(c[5:] for c in fake.calls if c.endswith("_bwd") or c.endswith("_grad")) == "raster_bwd deform_bwd deform_time_grad"


def test_render_with_time_and_camera_leaves_and_alpha_in_one_frame(fake):
    pc = _model(300)
    pose, delta = fdgs.PoseDelta(), fdgs.TimeDelta(n_cameras=3)
    cam = delta.camera(pose.pose(_cam(0.5)), index=2)
    fake.calls.clear()
    res = fdgs.render(cam, pc, _AlphaPipe(), torch.zeros(3), stage="fine")
    assert type(res["render"].grad_fn).__name__ == "_FusedRenderTimeFunctionBackward" and res["alpha"].shape == (1, 48, 64)
    (res["render"].sum() + res["alpha"].sum() + res["depth"].sum()).backward()
    _paired_time(fake, 1)
    assert [k for k, _ in fake.acc_order] == ["camera_grad"]          # (fdgs_raster_bwd_alpha in front of it: asserted by name below)
    assert " ".join(c[5:] for c in fake.calls if c.endswith("_bwd") or c.endswith("_bwd_alpha") or c.endswith("_grad")) == \
        "raster_bwd_alpha camera_grad deform_bwd deform_time_grad"
    assert pose.omega.grad.shape == (3,) and pose.tau.grad.shape == (3,) and delta.offset.grad.shape == (3,)
    assert float(delta.offset.grad[:2].abs().sum()) == 0.0 and pc._xyz.grad is not None


@pytest.mark.parametrize("fused", [True, False])
def test_the_coarse_stage_gives_the_time_a_zero_gradient(fake, monkeypatch, fused):
    monkeypatch.setattr(fdgs.renderer, "FUSED_BACKWARD", fused)
    pc = _model(300)
    delta = fdgs.TimeDelta()
    res = fdgs.render(delta.camera(_cam(0.5)), pc, _Pipe(), torch.zeros(3), stage="coarse")
    res["render"].sum().backward()
    assert delta.offset.grad is not None and float(delta.offset.grad.abs().sum()) == 0.0
    assert not any("time_grad" in c for c in fake.calls) and pc._xyz.grad is not None


def test_time_delta_at_zero_is_the_identity_and_composes_with_pose_delta():
    cam = _cam(0.37)
    delta = fdgs.TimeDelta(n_cameras=2)
    assert fdgs.TimeDelta is fdgs.camera.TimeDelta and tuple(delta.offset.shape) == (2,) and float(delta.offset.detach().abs().sum()) == 0.0
    moved = delta.camera(cam, index=1)
    assert isinstance(moved, fdgs.camera.PosedCamera) and moved.time.shape == () and moved.time.requires_grad
    assert float(moved.time.detach()) == float(torch.tensor(float(cam.time)))
    for k in ("world_view_transform", "full_proj_transform", "camera_center"):
        assert getattr(moved, k) is getattr(cam, k)
    assert (moved.image_height, moved.image_width, moved.FoVx, moved.FoVy) == (cam.image_height, cam.image_width, cam.FoVx, cam.FoVy)
    with torch.no_grad():
        delta.offset[1] = 0.05
    assert float(delta.camera(cam, index=1).time.detach()) == pytest.approx(0.42, abs=1e-6)
    assert float(delta.camera(cam, index=0).time.detach()) == float(moved.time.detach())
    # behind a PoseDelta: the pose tensors keep their graph, the time gets its own
    pose = fdgs.PoseDelta()
    both = delta.camera(pose.pose(cam), index=1)
    assert both.world_view_transform.grad_fn is not None and both.time.grad_fn is not None
    (both.world_view_transform.sum() + 2.0 * both.time).backward()
    assert pose.tau.grad is not None and delta.offset.grad.tolist() == [0.0, 2.0]
    # ... and in front of one
    again = pose.pose(delta.camera(cam, index=0))
    assert again.time.requires_grad and again.world_view_transform.grad_fn is not None
