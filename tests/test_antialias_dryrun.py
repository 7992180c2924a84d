"""Host plumbing of the opacity compensation (CPU, no kernels), on the fake library of tests/test_host_dryrun.py: a frame that asks
(pipe.antialiasing, rasterize_forward(antialiasing=True), GaussianRasterizer.antialiasing) makes the *_aa calls and no old call of the same
stage on every path, its backward and camera gradient follow the state, alpha and antialiasing together pass both, and a frame that does
not ask makes the calls it always made.  Nothing is computed."""
import ctypes
import importlib

import pytest
import torch

import test_alpha_dryrun as A
import test_camera_grad_dryrun as CG
import test_host_dryrun as D
from test_host_dryrun import PARENT_CALLS, _calls_of, _cam, _model

fdgs = importlib.import_module("4dgaussians_amd")
R, P, C = fdgs.rasterizer, fdgs.playback, fdgs.compose
# the stages that have an antialiased form, and the calls of those stages a frame that asks must not make
OLD = {"fdgs_preprocess_fwd", "fdgs_raster_fwd_capacity", "fdgs_raster_fwd_capacity_alpha", "fdgs_raster_bwd", "fdgs_raster_bwd_alpha",
       "fdgs_camera_grad"}
_addr = A._addr


class _AAFake(A._AlphaFake):
    """The fake library, which also stands in for the four device entry points of the antialiased family."""

    def __init__(self):
        super().__init__()
        self.aa = []               # (entry point, address of out_alpha / dL_dalpha where it has one -- 0: NULL)

    def __getattr__(self, name):
        fn = super().__getattr__(name)

        def wrapped(*a):
            if name == "fdgs_preprocess_fwd_aa":
                assert len(a) == 4
                self.aa.append(("preprocess_fwd_aa", 0))
            elif name == "fdgs_raster_fwd_capacity_aa":          # (the fake delivers the count at once, as for fdgs_raster_fwd_capacity)
                assert len(a) == 11
                ctypes.cast(a[6], ctypes.POINTER(ctypes.c_uint32))[0] = self.pair_count
                self.aa.append(("raster_fwd_capacity_aa", _addr(a[10])))
            elif name == "fdgs_raster_bwd_aa":
                assert len(a) == 8 and a[6].dL_dcolor and a[6].scratch_acc
                self.aa.append(("raster_bwd_aa", _addr(a[7])))
                self.acc_order.append(("raster_bwd", int(a[6].scratch_acc or 0)))
            elif name == "fdgs_camera_grad_aa":
                assert len(a) == 6 and a[2] is not None and a[4] is not None and a[5] is not None
                self.aa.append(("camera_grad_aa", 0))
                self.acc_order.append(("camera_grad", int(getattr(a[3], "value", a[3]) or 0)))
            return fn(*a)
        return wrapped


@pytest.fixture
def fake(monkeypatch):
    f = _AAFake()
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
    antialiasing = True


class _PipeBoth(_Pipe):
    render_alpha = True


class _PipeOff(D._Pipe):
    antialiasing = False


def _names(fake):
    return [n for n, _ in fake.aa]


def _no_old_call(fake):
    assert not OLD & set(fake.calls), OLD & set(fake.calls)


def _swapped(fake):
    """The calls with the antialiased names put back to the plain ones: what the frame would have called without the switch."""
    return " ".join(c[len("fdgs_"):].replace("_aa", "") for c in fake.calls)


@pytest.mark.parametrize("n", D.SIZES)
@pytest.mark.parametrize("fused", [True, False])
def test_render_fused_and_two_node(fake, monkeypatch, fused, n):
    monkeypatch.setattr(fdgs.renderer, "FUSED_BACKWARD", fused)
    pc = _model(n)
    res = fdgs.render(_cam(0.5), pc, _Pipe(), torch.zeros(3), stage="fine")
    assert set(res) == {"render", "viewspace_points", "visibility_filter", "radii", "depth"}
    res["render"].sum().backward()
    assert _names(fake) == ["preprocess_fwd_aa", "raster_bwd_aa"] and fake.aa[1][1] == 0
    assert pc._xyz.grad.shape == (n, 3) and pc._opacity.grad is not None
    _no_old_call(fake)
    if fused:
        assert _swapped(fake) == PARENT_CALLS["render_backward", n]
    # the second frame of the size takes the one-call path
    with torch.no_grad():
        fdgs.render(_cam(0.25), pc, _Pipe(), torch.zeros(3), stage="fine")
    assert _names(fake)[-1] == "raster_fwd_capacity_aa" and fake.aa[-1][1] == 0
    _no_old_call(fake)


def test_render_with_a_camera_that_asks_for_its_gradient(fake):
    pc = _model(300)
    cam = _cam(0.5)
    for k in ("world_view_transform", "full_proj_transform", "camera_center"):
        setattr(cam, k, getattr(cam, k).clone().requires_grad_(True))
    res = fdgs.render(cam, pc, _Pipe(), torch.zeros(3), stage="fine")
    assert type(res["render"].grad_fn).__name__ == "_FusedRenderCameraFunctionBackward"
    res["render"].sum().backward()
    CG._paired(fake, 1)
    assert _names(fake) == ["preprocess_fwd_aa", "raster_bwd_aa", "camera_grad_aa"]
    assert cam.world_view_transform.grad is not None
    _no_old_call(fake)


def test_render_with_a_time_that_asks_for_its_gradient(fake):
    pc = _model(300)
    cam = _cam(0.5)
    cam.time = torch.tensor([0.5], requires_grad=True)
    res = fdgs.render(cam, pc, _Pipe(), torch.zeros(3), stage="fine")
    assert type(res["render"].grad_fn).__name__ == "_FusedRenderTimeFunctionBackward"
    res["render"].sum().backward()
    assert _names(fake) == ["preprocess_fwd_aa", "raster_bwd_aa"] and cam.time.grad is not None
    _no_old_call(fake)


@pytest.mark.parametrize("stage,kw", [("coarse", {}), ("fine", {"override_color": True}), ("coarse", {"cov3d": True}), ("fine", {"sh": True})])
def test_the_two_node_branches_of_render(fake, stage, kw):
    pc = _model(300)
    pipe = _Pipe()
    pipe.compute_cov3D_python, pipe.convert_SHs_python = bool(kw.get("cov3d")), bool(kw.get("sh"))
    if kw.get("cov3d"):
        pc.get_covariance = lambda s=1.0: torch.rand(300, 6, requires_grad=True)
    oc = torch.rand(300, 3) if kw.get("override_color") else None
    res = fdgs.render(_cam(0.5), pc, pipe, torch.zeros(3), override_color=oc, stage=stage)
    res["render"].sum().backward()
    assert _names(fake) == ["preprocess_fwd_aa", "raster_bwd_aa"]
    _no_old_call(fake)


@pytest.mark.parametrize("n", D.SIZES)
def test_render_views(fake, n):
    pc = _model(n, "dnerf_bouncingballs", seed=2)
    res = fdgs.render_views([_cam(0.1 * i, 10.0 * i) for i in range(3)], pc, _Pipe(), torch.zeros(3), stage="fine")
    sum(r["render"].sum() for r in res).backward()
    assert _names(fake) == ["preprocess_fwd_aa", "raster_fwd_capacity_aa", "raster_fwd_capacity_aa"] + ["raster_bwd_aa"] * 3
    _no_old_call(fake)
    assert _swapped(fake) == PARENT_CALLS["render_views", n]


def test_rasterizer_attribute_keyword_and_state(fake):
    for frame in range(2):
        t = CG._raster_inputs()
        r = R.GaussianRasterizer(CG._settings(_cam()))
        r.antialiasing = True
        out = r(**t)
        assert len(out) == 3
        out[0].sum().backward()
        assert all(v.grad is not None for v in t.values())
    assert _names(fake) == ["preprocess_fwd_aa", "raster_bwd_aa", "raster_fwd_capacity_aa", "raster_bwd_aa"]
    _no_old_call(fake)
    t = CG._raster_inputs(grad=False)
    s = CG._settings(_cam())
    *_, st = R.rasterize_forward(s, t["means3D"], t["shs"], None, t["opacities"], t["scales"], t["rotations"], None, antialiasing=True)
    assert st.antialiasing is True and not st.with_alpha
    *_, st = R.rasterize_forward(s, t["means3D"], t["shs"], None, t["opacities"], t["scales"], t["rotations"], None)
    assert st.antialiasing is False
    out = R.rasterize_gaussians(t["means3D"], t["means2D"], t["shs"], None, t["opacities"], t["scales"], t["rotations"], None, s, antialiasing=True)
    assert len(out) == 3 and fake.calls[-2] == "fdgs_raster_fwd_capacity_aa"


def test_rasterizer_with_camera_leaves(fake):
    t = CG._raster_inputs()
    s = CG._settings(_cam(), ("viewmatrix", "projmatrix", "campos"))
    r = R.GaussianRasterizer(s)
    r.antialiasing = True
    color, radii, depth = r(**t)
    color.sum().backward()
    CG._paired(fake, 1)
    assert _names(fake) == ["preprocess_fwd_aa", "raster_bwd_aa", "camera_grad_aa"]
    assert all(getattr(s, k).grad is not None for k in ("viewmatrix", "projmatrix", "campos"))
    _no_old_call(fake)


@pytest.mark.parametrize("loss", ["render", "alpha", "render+alpha"])
def test_alpha_and_antialiasing_together_pass_both(fake, loss):
    pc = _model(300)
    res = fdgs.render(_cam(0.5), pc, _PipeBoth(), torch.zeros(3), stage="fine")
    assert res["alpha"].shape == (1, 48, 64)
    sum(res[k].sum() for k in loss.split("+")).backward()
    # the staged frame blends with fdgs_render_fwd_alpha (unchanged: it reads recB); the backward is the antialiased one, with dL_dalpha
    assert _names(fake) == ["preprocess_fwd_aa", "raster_bwd_aa"] and (fake.aa[1][1] != 0) == ("alpha" in loss)
    assert fake.alpha == [("render_fwd_alpha", res["alpha"].data_ptr())]
    with torch.no_grad():
        b = fdgs.render(_cam(0.25), pc, _PipeBoth(), torch.zeros(3), stage="fine")
    assert fake.aa[-1] == ("raster_fwd_capacity_aa", b["alpha"].data_ptr())
    _no_old_call(fake)


def test_a_speculative_antialiased_frame_that_overflows_is_finished_exactly(fake):
    pc = _model(300)
    cam = _cam(0.5)
    settings = R.GaussianRasterizationSettings(48, 64, 0.36, 0.27, torch.zeros(3), 1.0, cam.world_view_transform, cam.full_proj_transform, 3,
                                               cam.camera_center, False, False)
    args = (settings, pc.get_xyz.detach(), torch.rand(300, 16, 3), None, torch.rand(300, 1), torch.rand(300, 3), torch.rand(300, 4), None)
    R.rasterize_forward(*args, antialiasing=True)
    cap = (int(7 * R.CAPACITY_SLACK) + 8192) // 4096 * 4096
    fake.pair_count = cap + 1234
    fake.calls.clear()
    *_, state = R.rasterize_forward(*args, antialiasing=True)
    # stages 3-4 run again on the geom the antialiased projection left: no second projection, the plain sort and blend
    assert " ".join(c[len("fdgs_"):] for c in fake.calls) == D.PARENT_RERUN_CALLS.replace("raster_fwd_capacity", "raster_fwd_capacity_aa")
    assert state.capacity == cap + 1234 and state.antialiasing


def _baked(kind, n):
    if kind == "baked":
        return P.bake(_model(n), D.TIMES), n
    if kind == "sparse":
        return P.bake_sparse(_model(n), D.TIMES, tol=-1.0), n
    return C.compose(D._two_baked(n), [None, C.Placement(translation=(0.5, 0.0, -0.25), scale=0.5, time_offset=0.1)]), 2 * n


@pytest.mark.parametrize("n", D.SIZES)
@pytest.mark.parametrize("kind", ["baked", "sparse", "composite"])
def test_playback_render(fake, kind, n):
    obj, rows = _baked(kind, n)
    entry = {"baked": "baked_render", "sparse": "sparse_render", "composite": "composite_render"}[kind]
    fake.calls.clear()
    fake.aa.clear()
    obj.render(_cam(0.5), _Pipe(), torch.zeros(3), rgb8="trunc" if kind != "sparse" else "round")
    fake.calls.append("fdgs_--")
    out = obj.render(_cam(0.25), _Pipe(), torch.zeros(3), override_color=D._colors(rows))
    assert out["radii"].shape == (rows,)
    assert _names(fake) == ["preprocess_fwd_aa", "raster_fwd_capacity_aa"]
    _no_old_call(fake)
    assert _swapped(fake) == PARENT_CALLS[entry, n]
    # the same object, a pipe that does not ask: the old calls
    fake.calls.clear()
    obj.render(_cam(0.5), _PipeOff(), torch.zeros(3))
    assert not any(c.endswith("_aa") for c in fake.calls) and "fdgs_raster_fwd_capacity" in fake.calls


@pytest.mark.parametrize("method", ["render_pick", "render_contrib", "render_features", "render_motion"])
def test_replay_methods_project_with_the_compensation_and_replay_unchanged(fake, method):
    baked = P.bake(_model(300), D.TIMES)
    fake.calls.clear()
    kw = {"render_features": dict(values=torch.rand(300, 2)), "render_motion": dict(toward_time=0.7)}.get(method, {})
    getattr(baked, method)(_cam(0.5), _Pipe(), torch.zeros(3), **kw)
    assert _names(fake) == ["preprocess_fwd_aa"]
    _no_old_call(fake)
    replay = {"render_pick": "fdgs_render_pick", "render_contrib": "fdgs_render_contrib", "render_features": "fdgs_render_features",
              "render_motion": "fdgs_render_fwd"}[method]
    assert replay in fake.calls


@pytest.mark.parametrize("pipe", [D._Pipe, _PipeOff], ids=["absent", "False"])
@pytest.mark.parametrize("n", D.SIZES)
@pytest.mark.parametrize("entry", sorted(D._RUNS))
def test_without_the_switch_the_calls_are_what_they_were(fake, monkeypatch, entry, n, pipe):
    monkeypatch.setattr(D, "_Pipe", pipe)
    assert _calls_of(fake, entry, n) == PARENT_CALLS[entry, n]
    assert fake.aa == [] and not any(c.endswith("_aa") for c in fake.calls)
