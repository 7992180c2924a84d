"""Host plumbing of the camera's gradient (CPU, no kernels), on the fake library of tests/test_host_dryrun.py: which frames call
fdgs_camera_grad, behind which fdgs_raster_bwd and on which accumulator, and where the gradients arrive.  Nothing is computed."""
import ctypes
import importlib

import pytest
import torch

import test_host_dryrun as D
from test_host_dryrun import PARENT_CALLS, _Pipe, _calls_of, _cam, _model

fdgs = importlib.import_module("4dgaussians_amd")
R = fdgs.rasterizer


class _CamFake(D._FakeLib):
    """The fake library, which also answers the scratch size of fdgs_camera_grad and notes the accumulator of every backward call."""

    def __init__(self):
        super().__init__()
        self.acc_order = []        # ("raster_bwd" | "camera_grad", accumulator address)

    def __getattr__(self, name):
        fn = super().__getattr__(name)

        def wrapped(*a):
            if name == "fdgs_camera_grad_scratch_bytes":
                self.calls.append(name)
                a[-1].value = 128
                return 0
            if name == "fdgs_raster_bwd":
                self.acc_order.append(("raster_bwd", int(a[6].scratch_acc or 0)))
            elif name == "fdgs_camera_grad":
                self.acc_order.append(("camera_grad", int(getattr(a[3], "value", a[3]) or 0)))
                assert a[2] is not None and a[4] is not None and a[5] is not None
            return fn(*a)
        return wrapped


@pytest.fixture
def fake(monkeypatch):
    """The installation of test_host_dryrun's fixture, with the fake above."""
    f = _CamFake()
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


def _paired(fake, n_pairs):
    """One fdgs_camera_grad directly behind each fdgs_raster_bwd, on that call's accumulator."""
    assert len(fake.acc_order) == 2 * n_pairs, fake.acc_order
    for (k0, a0), (k1, a1) in zip(fake.acc_order[0::2], fake.acc_order[1::2]):
        assert (k0, k1) == ("raster_bwd", "camera_grad") and a0 == a1 != 0
    calls = [c for c in fake.calls if c in ("fdgs_raster_bwd", "fdgs_camera_grad", "fdgs_deform_bwd")]
    for i, c in enumerate(calls):
        if c == "fdgs_raster_bwd":
            assert calls[i + 1] == "fdgs_camera_grad"


def _raster_inputs(n=200, grad=True):
    g = torch.Generator().manual_seed(3)
    t = dict(means3D=torch.randn(n, 3, generator=g), means2D=torch.zeros(n, 3), opacities=torch.rand(n, 1, generator=g),
             shs=torch.randn(n, 16, 3, generator=g), scales=torch.rand(n, 3, generator=g), rotations=torch.randn(n, 4, generator=g))
    return {k: v.requires_grad_(grad) for k, v in t.items()}


def _settings(cam, leaves=()):
    ts = dict(viewmatrix=cam.world_view_transform.clone(), projmatrix=cam.full_proj_transform.clone(), campos=cam.camera_center.clone())
    for k in leaves:
        ts[k].requires_grad_(True)
    return R.GaussianRasterizationSettings(image_height=48, image_width=64, tanfovx=0.36, tanfovy=0.27, bg=torch.zeros(3), scale_modifier=1.0,
                                           sh_degree=3, prefiltered=False, debug=False, **ts)


@pytest.mark.parametrize("n", D.SIZES)
@pytest.mark.parametrize("entry", ["render_backward", "render_views", "render_nograd"])
def test_without_requires_grad_on_the_camera_the_calls_are_what_they_were(fake, entry, n):
    assert _calls_of(fake, entry, n) == PARENT_CALLS[entry, n]
    assert "fdgs_camera_grad" not in fake.calls and not any("camera" in c for c in fake.calls)


def test_rasterizer_without_camera_leaves_runs_the_node_it_always_ran(fake):
    t = _raster_inputs()
    color, radii, depth = R.GaussianRasterizer(_settings(_cam()))(**t)
    assert type(color.grad_fn).__name__ == "_RasterizeGaussiansBackward"
    color.sum().backward()
    assert not any("camera" in c for c in fake.calls) and fake.calls[-1] == "fdgs_raster_bwd"
    # leaves that require grad, but no grad mode: no camera path either
    with torch.no_grad():
        color, _, _ = R.GaussianRasterizer(_settings(_cam(), ("viewmatrix", "projmatrix", "campos")))(**_raster_inputs(grad=False))
    assert color.grad_fn is None and not any("camera" in c for c in fake.calls)
    # render_views keeps ignoring requires_grad on a camera
    cam = _cam()
    cam.world_view_transform = cam.world_view_transform.clone().requires_grad_(True)
    fake.calls.clear()
    res = fdgs.render_views([cam, _cam(0.2)], _model(300), _Pipe(), torch.zeros(3), stage="fine")
    sum(r["render"].sum() for r in res).backward()
    assert "fdgs_camera_grad" not in fake.calls and cam.world_view_transform.grad is None


@pytest.mark.parametrize("leaves", [("viewmatrix", "projmatrix", "campos"), ("campos",), ("viewmatrix",)])
@pytest.mark.parametrize("frozen", [False, True])
def test_rasterizer_with_camera_leaves(fake, leaves, frozen):
    t = _raster_inputs(grad=not frozen)
    s = _settings(_cam(), leaves)
    color, radii, depth = R.GaussianRasterizer(s)(**t)
    assert type(color.grad_fn).__name__ == "_RasterizeGaussiansCameraBackward"
    (color.sum() + depth.sum()).backward()
    _paired(fake, 1)
    assert fake.acc_seen[-1][1] == 1          # a camera-only frame allocates the forward's accumulator like a training frame
    for k in ("viewmatrix", "projmatrix", "campos"):
        g = getattr(s, k).grad
        assert (g is not None and g.shape == getattr(s, k).shape) if k in leaves else g is None
    assert all((v.grad is None) == frozen for v in t.values())


def test_rasterize_backward_keyword(fake):
    t = _raster_inputs(grad=False)
    _, _, _, state = R.rasterize_forward(_settings(_cam()), t["means3D"], t["shs"], None, t["opacities"], t["scales"], t["rotations"], None,
                                         expect_backward=True)
    g = R.rasterize_backward(state, torch.ones(3, 48, 64))
    assert not {"viewmatrix", "projmatrix", "campos"} & set(g) and "fdgs_camera_grad" not in fake.calls
    _, _, _, state = R.rasterize_forward(_settings(_cam()), t["means3D"], t["shs"], None, t["opacities"], t["scales"], t["rotations"], None,
                                         expect_backward=True)
    fake.acc_order.clear()
    fake.calls.clear()
    g = R.rasterize_backward(state, torch.ones(3, 48, 64), camera=True)
    assert g["viewmatrix"].shape == (4, 4) and g["projmatrix"].shape == (4, 4) and g["campos"].shape == (3,)
    _paired(fake, 1)


@pytest.mark.parametrize("stage", ["fine", "coarse"])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("frozen", [False, True])
def test_render_with_a_pose_delta(fake, monkeypatch, stage, fused, frozen):
    monkeypatch.setattr(fdgs.renderer, "FUSED_BACKWARD", fused)
    pc = _model(300)
    if frozen:
        pc.requires_grad_(False)
    delta = fdgs.camera.PoseDelta()
    cam = delta.pose(_cam(0.5))
    fake.calls.clear()
    res = fdgs.render(cam, pc, _Pipe(), torch.zeros(3), stage=stage)
    res["render"].sum().backward()
    _paired(fake, 1)
    assert delta.omega.grad.shape == (3,) and delta.tau.grad.shape == (3,)
    assert (pc._xyz.grad is None) == frozen and res["viewspace_points"].grad.shape == (300, 3)
    if stage == "fine" and fused:
        assert type(res["render"].grad_fn).__name__ == "_FusedRenderCameraFunctionBackward"
        assert " ".join(c[5:] for c in fake.calls if c.endswith("_bwd") or c == "fdgs_camera_grad") == "raster_bwd camera_grad deform_bwd"


def test_render_with_plain_camera_leaves_and_panoptic_settings(fake):
    pc = _model(300)
    cam = _cam(0.5)
    for k in ("world_view_transform", "full_proj_transform", "camera_center"):
        setattr(cam, k, getattr(cam, k).clone().requires_grad_(True))
    fdgs.render(cam, pc, _Pipe(), torch.zeros(3), stage="fine")["render"].sum().backward()
    assert cam.world_view_transform.grad.shape == (4, 4) and cam.full_proj_transform.grad.shape == (4, 4) and cam.camera_center.grad.shape == (3,)
    _paired(fake, 1)
    # a "PanopticSports" dict camera works through the settings it brings along
    s = _settings(_cam(), ("viewmatrix", "campos"))
    fake.acc_order.clear()
    fake.calls.clear()
    fdgs.render({"camera": s, "time": 0.5}, pc, _Pipe(), torch.zeros(3), stage="fine", cam_type="PanopticSports")["render"].sum().backward()
    assert s.viewmatrix.grad.shape == (4, 4) and s.campos.grad.shape == (3,) and s.projmatrix.grad is None
    _paired(fake, 1)
