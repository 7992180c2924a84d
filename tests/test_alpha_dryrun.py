"""Host plumbing of the accumulated-alpha image (CPU, no kernels), on the fake library of tests/test_host_dryrun.py: a frame that asks
(GaussianRasterizer(render_alpha=True), pipe.render_alpha) makes the *_alpha calls with a non-NULL image on every path, its backward hands
dL_dalpha over exactly when alpha reached the loss, and a frame that does not ask makes the calls it always made.  Nothing is computed."""
import ctypes
import importlib

import pytest
import torch

import test_camera_grad_dryrun as CG
import test_host_dryrun as D
from test_host_dryrun import PARENT_CALLS, _calls_of, _cam, _model

fdgs = importlib.import_module("4dgaussians_amd")
R = fdgs.rasterizer
OLD = {"fdgs_render_fwd", "fdgs_raster_fwd_capacity", "fdgs_raster_bwd"}


def _addr(x):
    return int(getattr(x, "value", x) or 0)


class _AlphaFake(CG._CamFake):
    """The fake library, which also stands in for the three alpha entry points and notes the alpha pointer each of them got."""

    def __init__(self):
        super().__init__()
        self.alpha = []            # (entry point, address of out_alpha / dL_dalpha -- 0: NULL)

    def __getattr__(self, name):
        fn = super().__getattr__(name)

        def wrapped(*a):
            if name == "fdgs_render_fwd_alpha":
                assert len(a) == 9
                self.alpha.append(("render_fwd_alpha", _addr(a[8])))
            elif name == "fdgs_raster_fwd_capacity_alpha":       # (the fake delivers the count at once, as for fdgs_raster_fwd_capacity)
                assert len(a) == 11
                ctypes.cast(a[6], ctypes.POINTER(ctypes.c_uint32))[0] = self.pair_count
                self.alpha.append(("raster_fwd_capacity_alpha", _addr(a[10])))
            elif name == "fdgs_raster_bwd_alpha":
                assert len(a) == 8 and a[6].dL_dcolor and a[6].scratch_acc
                self.alpha.append(("raster_bwd_alpha", _addr(a[7])))
                self.acc_order.append(("raster_bwd", int(a[6].scratch_acc or 0)))
            return fn(*a)
        return wrapped


@pytest.fixture
def fake(monkeypatch):
    """The installation of test_host_dryrun's fixture, with the fake above."""
    f = _AlphaFake()
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


class _Pipe(D._Pipe):
    render_alpha = True


def _no_old_call(fake):
    assert not OLD & set(fake.calls), OLD & set(fake.calls)


def _names(fake):
    return [n for n, _ in fake.alpha]


LOSSES = {"color": (False, lambda c, d, a: c.sum()), "alpha": (True, lambda c, d, a: a.sum()),
          "color+alpha": (True, lambda c, d, a: c.sum() + 2.0 * a.sum()), "depth": (False, lambda c, d, a: d.sum()),
          "depth+alpha": (True, lambda c, d, a: d.sum() + a.sum())}


@pytest.mark.parametrize("loss", sorted(LOSSES))
def test_rasterizer_with_alpha_makes_the_alpha_calls_and_hands_dL_dalpha_over_when_alpha_reached_the_loss(fake, loss):
    reached, f = LOSSES[loss]
    for frame in range(2):                   # the first frame of a (size, count) takes the staged path, the second the one-call path
        t = CG._raster_inputs()
        out = R.GaussianRasterizer(CG._settings(_cam()), render_alpha=True)(**t)
        assert len(out) == 4
        color, radii, depth, alpha = out
        assert alpha.shape == (1, 48, 64) and alpha.dtype == torch.float32 and alpha.grad_fn is color.grad_fn
        assert fake.alpha[-1][0] == ("render_fwd_alpha", "raster_fwd_capacity_alpha")[frame] and fake.alpha[-1][1] == alpha.data_ptr()
        f(color, depth, alpha).backward()
        name, addr = fake.alpha[-1]
        assert name == "raster_bwd_alpha" and (addr != 0) == reached
        assert all(v.grad is not None for v in t.values())
    _no_old_call(fake)
    assert _names(fake) == ["render_fwd_alpha", "raster_bwd_alpha", "raster_fwd_capacity_alpha", "raster_bwd_alpha"]


def test_no_image_in_the_loss_makes_no_backward_call(fake):
    t = CG._raster_inputs()
    color, radii, depth, alpha = R.GaussianRasterizer(CG._settings(_cam()), render_alpha=True)(**t)
    (t["means3D"].sum() + 0.0 * color.detach().sum()).backward()
    assert _names(fake) == ["render_fwd_alpha"]


def test_rasterizer_with_camera_leaves_and_alpha(fake):
    t = CG._raster_inputs()
    s = CG._settings(_cam(), ("viewmatrix", "projmatrix", "campos"))
    color, radii, depth, alpha = R.GaussianRasterizer(s, render_alpha=True)(**t)
    assert type(alpha.grad_fn).__name__ == "_RasterizeGaussiansCameraBackward"
    alpha.sum().backward()
    CG._paired(fake, 1)                      # fdgs_camera_grad directly behind the alpha backward, on its accumulator
    assert fake.alpha[-1][0] == "raster_bwd_alpha" and fake.alpha[-1][1] != 0
    assert all(getattr(s, k).grad is not None for k in ("viewmatrix", "projmatrix", "campos"))
    _no_old_call(fake)


@pytest.mark.parametrize("n", D.SIZES)
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("loss", ["render", "alpha", "render+alpha"])
def test_render_with_alpha(fake, monkeypatch, fused, loss, n):
    monkeypatch.setattr(fdgs.renderer, "FUSED_BACKWARD", fused)
    pc = _model(n)
    res = fdgs.render(_cam(0.5), pc, _Pipe(), torch.zeros(3), stage="fine")
    assert set(res) == {"render", "viewspace_points", "visibility_filter", "radii", "depth", "alpha"}
    assert res["alpha"].shape == (1, 48, 64) and res["alpha"].requires_grad
    sum(res[k].sum() for k in loss.split("+")).backward()
    assert _names(fake) == ["render_fwd_alpha", "raster_bwd_alpha"]
    assert fake.alpha[0][1] == res["alpha"].data_ptr() and (fake.alpha[1][1] != 0) == ("alpha" in loss)
    assert pc._xyz.grad.shape == (n, 3) and res["viewspace_points"].grad.shape == (n, 3)
    _no_old_call(fake)
    # the frame makes the calls of a frame without alpha, the three entry points swapped for their alpha forms
    swapped = " ".join(c[len("fdgs_"):].replace("_alpha", "") for c in fake.calls)
    if fused:
        assert swapped == PARENT_CALLS["render_backward", n]


def test_render_with_alpha_and_a_camera_that_asks_for_its_gradient(fake):
    pc = _model(300)
    cam = _cam(0.5)
    for k in ("world_view_transform", "full_proj_transform", "camera_center"):
        setattr(cam, k, getattr(cam, k).clone().requires_grad_(True))
    res = fdgs.render(cam, pc, _Pipe(), torch.zeros(3), stage="fine")
    assert type(res["alpha"].grad_fn).__name__ == "_FusedRenderCameraFunctionBackward"
    res["alpha"].sum().backward()
    CG._paired(fake, 1)
    assert _names(fake) == ["render_fwd_alpha", "raster_bwd_alpha"] and fake.alpha[1][1] != 0
    assert cam.world_view_transform.grad is not None and pc._xyz.grad is not None
    _no_old_call(fake)


@pytest.mark.parametrize("stage,kw", [("coarse", {}), ("fine", {"override_color": True}), ("coarse", {"cov3d": True}), ("fine", {"sh": True})])
def test_the_two_node_branches_of_render_return_alpha(fake, stage, kw):
    pc = _model(300)
    pipe = _Pipe()
    pipe.compute_cov3D_python, pipe.convert_SHs_python = bool(kw.get("cov3d")), bool(kw.get("sh"))
    if kw.get("cov3d"):
        pc.get_covariance = lambda s=1.0: torch.rand(300, 6, requires_grad=True)
    oc = torch.rand(300, 3) if kw.get("override_color") else None
    res = fdgs.render(_cam(0.5), pc, pipe, torch.zeros(3), override_color=oc, stage=stage)
    assert res["alpha"].shape == (1, 48, 64)
    (res["render"].sum() + res["alpha"].sum()).backward()
    assert _names(fake) == ["render_fwd_alpha", "raster_bwd_alpha"] and fake.alpha[1][1] != 0
    _no_old_call(fake)


def test_render_views_with_alpha(fake):
    pc = _model(300, "dnerf_bouncingballs", seed=2)
    res = fdgs.render_views([_cam(0.1 * i, 10.0 * i) for i in range(3)], pc, _Pipe(), torch.zeros(3), stage="fine")
    assert all(r["alpha"].shape == (1, 48, 64) for r in res)
    assert _names(fake) == ["render_fwd_alpha", "raster_fwd_capacity_alpha", "raster_fwd_capacity_alpha"]
    assert [a for _, a in fake.alpha] == [r["alpha"].data_ptr() for r in res]          # every view renders into its slice of [V,1,H,W]
    assert res[1]["alpha"].data_ptr() - res[0]["alpha"].data_ptr() == 48 * 64 * 4
    (res[0]["render"].sum() + res[2]["alpha"].sum()).backward()
    bwd = fake.alpha[3:]
    assert [n for n, _ in bwd] == ["raster_bwd_alpha"] * 3 and all(a != 0 for _, a in bwd)      # (one [V,1,H,W] gradient: every view gets its slice)
    assert len({a for _, a in bwd}) == 3
    _no_old_call(fake)
    # alpha not in the loss: NULL for every view
    res = fdgs.render_views([_cam(0.1 * i, 10.0 * i) for i in range(3)], pc, _Pipe(), torch.zeros(3), stage="fine")
    sum(r["render"].sum() for r in res).backward()
    assert [x for x in fake.alpha[-3:]] == [("raster_bwd_alpha", 0)] * 3


def test_no_grad_frames_with_alpha(fake):
    pc = _model(300)
    with torch.no_grad():
        a = fdgs.render(_cam(0.5), pc, _Pipe(), torch.zeros(3), stage="fine")
        b = fdgs.render(_cam(0.25), pc, _Pipe(), torch.zeros(3), stage="fine")
    assert a["alpha"].grad_fn is None and not a["alpha"].requires_grad and b["alpha"].shape == (1, 48, 64)
    assert fake.alpha == [("render_fwd_alpha", a["alpha"].data_ptr()), ("raster_fwd_capacity_alpha", b["alpha"].data_ptr())]
    _no_old_call(fake)


def test_a_speculative_frame_with_alpha_that_overflows_is_finished_exactly_with_alpha(fake):
    fake.record = True
    pc = _model(300)
    cam = _cam(0.5)
    settings = R.GaussianRasterizationSettings(48, 64, 0.36, 0.27, torch.zeros(3), 1.0, cam.world_view_transform, cam.full_proj_transform, 3,
                                               cam.camera_center, False, False)
    args = (settings, pc.get_xyz.detach(), torch.rand(300, 16, 3), None, torch.rand(300, 1), torch.rand(300, 3), torch.rand(300, 4), None)
    color, radii, depth, alpha, first = R.rasterize_forward(*args, want_alpha=True)
    assert first.with_alpha and first.capacity == 7
    cap = (int(7 * R.CAPACITY_SLACK) + 8192) // 4096 * 4096
    fake.pair_count = cap + 1234
    fake.calls.clear()
    fake.alpha.clear()
    reruns = R.capacity_reruns
    out = tuple(torch.empty(s, dtype=dt) for s, dt in (((3, 48, 64), torch.float32), ((300,), torch.int32), ((1, 48, 64), torch.float32),
                                                       ((1, 48, 64), torch.float32)))
    color, radii, depth, alpha, state = R.rasterize_forward(*args, out=out, want_alpha=True)
    assert alpha is out[3] and color is out[0]
    assert " ".join(c[len("fdgs_"):] for c in fake.calls) == D.PARENT_RERUN_CALLS.replace("raster_fwd_capacity", "raster_fwd_capacity_alpha").replace(
        "render_fwd", "render_fwd_alpha")
    assert fake.alpha == [("raster_fwd_capacity_alpha", alpha.data_ptr()), ("render_fwd_alpha", alpha.data_ptr())]
    assert R.capacity_reruns == reruns + 1 and state.capacity == cap + 1234 and state.with_alpha
    # a state rendered without alpha refuses an alpha gradient instead of dropping it
    *_, plain = R.rasterize_forward(*args)
    assert not plain.with_alpha
    with pytest.raises(fdgs._lib.FdgsError):
        R.rasterize_backward(plain, torch.ones(3, 48, 64), grad_alpha=torch.ones(1, 48, 64))


@pytest.mark.parametrize("n", D.SIZES)
@pytest.mark.parametrize("entry", ["render_backward", "render_views", "render_nograd"])
def test_without_render_alpha_the_calls_are_what_they_were(fake, entry, n):
    assert _calls_of(fake, entry, n) == PARENT_CALLS[entry, n]
    assert fake.alpha == [] and not any("alpha" in c for c in fake.calls)


def test_rasterizer_without_alpha_returns_the_triple_and_runs_the_calls_it_always_ran(fake):
    t = CG._raster_inputs()
    out = R.GaussianRasterizer(CG._settings(_cam()))(**t)
    assert len(out) == 3
    out[0].sum().backward()
    assert fake.alpha == [] and fake.calls[-1] == "fdgs_raster_bwd"
    out = R.GaussianRasterizer(CG._settings(_cam()), render_alpha=False)(**t)
    assert len(out) == 3 and fake.alpha == []
