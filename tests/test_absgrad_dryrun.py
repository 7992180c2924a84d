"""Host plumbing of the absolute screen-space gradients (CPU, no kernels), on the fake library of tests/test_host_dryrun.py as
tests/test_antialias_dryrun.py extends it: a frame that asks (pipe.absgrad, GaussianRasterizer.absgrad, the absgrad keyword) makes
fdgs_raster_bwd_abs -- with a non-NULL output, the frame's antialiasing case and the alpha gradient exactly where alpha reached the loss -- in
place of every other form of the backward on every route, and its gradient sink carries `.absgrad`; a frame that does not ask makes exactly
the calls it made and its sink carries nothing.  Nothing is computed."""
import importlib
import itertools

import pytest
import torch

import test_alpha_dryrun as A
import test_camera_grad_dryrun as CG
import test_frame_options_dryrun as FO
import test_host_dryrun as D
from test_antialias_dryrun import _AAFake
from test_host_dryrun import PARENT_CALLS, _calls_of, _cam, _model

fdgs = importlib.import_module("4dgaussians_amd")
R = fdgs.rasterizer
OTHER_BACKWARDS = {"fdgs_raster_bwd", "fdgs_raster_bwd_alpha", "fdgs_raster_bwd_aa"}


class _AbsFake(_AAFake):
    """The fake library, which also stands in for fdgs_raster_bwd_abs and notes what it was handed."""

    def __init__(self):
        super().__init__()
        self.abs = []              # (address of dL_dalpha -- 0: NULL, antialiased, address of dL_dmeans2D_abs)

    def __getattr__(self, name):
        fn = super().__getattr__(name)

        def wrapped(*a):
            if name == "fdgs_raster_bwd_abs":
                assert len(a) == 10 and a[6].dL_dcolor and a[6].scratch_acc and a[6].dL_dmeans2D
                self.abs.append((A._addr(a[7]), int(a[8]), A._addr(a[9])))
                self.acc_order.append(("raster_bwd", int(a[6].scratch_acc or 0)))
            return fn(*a)
        return wrapped


@pytest.fixture
def fake(monkeypatch):
    import ctypes
    f = _AbsFake()
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


def _ask(monkeypatch):
    """tests/test_frame_options_dryrun.py's frames, asking: its pipes gain absgrad = True, and so does the rasterizer it builds itself."""
    monkeypatch.setattr(FO, "_pipe", lambda alpha, aa: type("Pipe", (D._Pipe,), {"render_alpha": alpha, "antialiasing": aa, "absgrad": True})())
    monkeypatch.setattr(R.GaussianRasterizer, "absgrad", True)


def _expected(route, alpha, aa, cam, time):
    """The calls of the frame without the option, every form of the backward swapped for the one entry point."""
    swap = {FO._entry("raster_bwd", alpha, aa): "raster_bwd_abs"}
    return [swap.get(c, c) for c in FO.expected_calls(route, alpha, aa, cam, time)]


def _sinks(frame):
    return [t for k, t in frame.asked.items() if k.startswith("viewspace_points") or k == "means2D"]


def _camera_behind_its_backward(fake):
    """One camera-gradient call directly behind each backward, on that call's accumulator (CG._paired, for the names of this family)."""
    assert len(fake.acc_order) % 2 == 0 and fake.acc_order
    for (k0, a0), (k1, a1) in zip(fake.acc_order[0::2], fake.acc_order[1::2]):
        assert (k0, k1) == ("raster_bwd", "camera_grad") and a0 == a1 != 0


def _cases():
    for route, (alpha, aa), leaves in itertools.product(FO.ROUTES, itertools.product((False, True), repeat=2), FO.LEAVES):
        cam, time = FO.LEAVES[leaves]
        if (route == "rasterizer" and time) or (route == "views" and (cam or time)):
            continue
        yield pytest.param(route, alpha, aa, cam, time, id=f"{route}-alpha{int(alpha)}-aa{int(aa)}-{leaves}")


@pytest.mark.parametrize("route,alpha,aa,cam,time", list(_cases()))
def test_a_frame_that_asks_makes_the_one_backward_call_on_every_route(fake, monkeypatch, route, alpha, aa, cam, time):
    _ask(monkeypatch)
    frame = FO._Frame(route, alpha, aa, cam, time, monkeypatch)
    assert FO._nodes(*frame.images[0][:2]) == FO.expected_nodes(route, cam, time)      # the node classes a frame always recorded
    sinks = _sinks(frame)
    assert len(sinks) == len(frame.images) and not any(hasattr(s, "absgrad") for s in sinks)
    frame.loss().backward()
    assert FO._calls(fake) == _expected(route, alpha, aa, cam, time)
    assert not OTHER_BACKWARDS & set(fake.calls)
    views = len(frame.images)
    assert len(fake.abs) == views
    for ga, flag, out in fake.abs:
        assert flag == int(aa) and out != 0 and (ga != 0) == alpha       # (the loss saw alpha where there is one)
    # every view's own sink carries its own rows: [P,3] float32, the buffer the call of that view wrote
    rows = [s.absgrad for s in sinks]
    assert all(r.shape == (300, 3) and r.dtype == torch.float32 and not r.requires_grad for r in rows)
    assert sorted(r.data_ptr() for r in rows) == sorted(out for _, _, out in fake.abs) and len({r.data_ptr() for r in rows}) == views
    if cam:
        _camera_behind_its_backward(fake)
    frame.check_gradients()


@pytest.mark.parametrize("route,cam,time", FO.FULL)
def test_a_second_backward_assigns_a_fresh_tensor(fake, monkeypatch, route, cam, time):
    _ask(monkeypatch)
    frame = FO._Frame(route, True, True, cam, time, monkeypatch)
    sink, = _sinks(frame)
    loss = frame.loss()
    loss.backward(retain_graph=True)
    first = sink.absgrad
    loss.backward()
    assert sink.absgrad is not first and sink.absgrad.data_ptr() == fake.abs[-1][2] != first.data_ptr() == fake.abs[0][2]
    assert len(fake.abs) == 2


@pytest.mark.parametrize("route", ["fused", "views"])
def test_through_the_implicit_permutation_the_rows_go_back_through_the_scatter(fake, route):
    """N = 8200 (a random cube above IMPLICIT_ORDER_MIN_N): the node's inputs are the permuted sinks; the caller's own leaves get the rows,
    through one more fdgs_permute_rows call per backward (one call moves every view's rows)."""
    n = 8200
    pipe = type("Pipe", (D._Pipe,), {"absgrad": True})()
    if route == "fused":
        pc = _model(n)
        fake.calls.clear()
        res = [fdgs.render(_cam(0.5), pc, pipe, torch.zeros(3), stage="fine")]
        parent = PARENT_CALLS["render_backward", n]
    else:
        pc = _model(n, "dnerf_bouncingballs", seed=2)
        fake.calls.clear()
        res = fdgs.render_views([_cam(0.1 * i, 10.0 * i) for i in range(3)], pc, pipe, torch.zeros(3), stage="fine")
        parent = PARENT_CALLS["render_views", n]
    sum(r["render"].sum() for r in res).backward()
    calls = " ".join(c[len("fdgs_"):] for c in fake.calls)
    want = parent.replace("raster_bwd", "raster_bwd_abs")
    head, tail = want.rsplit("deform_bwd", 1)
    assert calls == head + "deform_bwd permute_rows" + tail           # the scatter of the absolute rows, then the signed gradients' own
    for r in res:
        s = r["viewspace_points"]
        assert s.absgrad.shape == (n, 3) and s.grad.shape == (n, 3)
        assert s.absgrad.data_ptr() not in {out for _, _, out in fake.abs}      # (the scattered copy, not the buffer in kernel order)


@pytest.mark.parametrize("stage,kw", [("coarse", {}), ("fine", {"override_color": True}), ("coarse", {"cov3d": True}), ("fine", {"sh": True})])
def test_the_two_node_branches_of_render(fake, stage, kw):
    pc = _model(300)
    pipe = type("Pipe", (D._Pipe,), {"absgrad": True})()
    pipe.compute_cov3D_python, pipe.convert_SHs_python = bool(kw.get("cov3d")), bool(kw.get("sh"))
    if kw.get("cov3d"):
        pc.get_covariance = lambda s=1.0: torch.rand(300, 6, requires_grad=True)
    oc = torch.rand(300, 3) if kw.get("override_color") else None
    res = fdgs.render(_cam(0.5), pc, pipe, torch.zeros(3), override_color=oc, stage=stage)
    res["render"].sum().backward()
    assert len(fake.abs) == 1 and fake.abs[0][:2] == (0, 0) and not OTHER_BACKWARDS & set(fake.calls)
    assert res["viewspace_points"].absgrad.data_ptr() == fake.abs[0][2] and res["viewspace_points"].grad is not None


def test_rasterizer_attribute_keyword_state_and_backward(fake):
    t = CG._raster_inputs()
    s = CG._settings(_cam())
    r = R.GaussianRasterizer(s)
    assert r.absgrad is False
    r.absgrad = True
    out = r(**t)
    assert len(out) == 3
    out[0].sum().backward()
    assert t["means2D"].absgrad.shape == (200, 3) and t["means2D"].grad is not None and fake.calls[-1] == "fdgs_raster_bwd_abs"
    t = CG._raster_inputs(grad=False)
    args = (s, t["means3D"], t["shs"], None, t["opacities"], t["scales"], t["rotations"], None)
    *_, st = R.rasterize_forward(*args, absgrad=True)
    assert st.absgrad is True and not st.with_alpha and not st.antialiasing and st.options == (False, False, True)
    g = R.rasterize_backward(st, torch.ones(3, 48, 64))
    assert g["means2D_abs"].shape == (200, 3) and fake.abs[-1] == (0, 0, g["means2D_abs"].data_ptr())
    *_, st = R.rasterize_forward(*args, antialiasing=True, absgrad=True)
    g = R.rasterize_backward(st, torch.ones(3, 48, 64), torch.ones(1, 48, 64))
    assert fake.abs[-1] == (0, 1, g["means2D_abs"].data_ptr())
    *_, st = R.rasterize_forward(*args)
    assert st.absgrad is False and "means2D_abs" not in R.rasterize_backward(st, torch.ones(3, 48, 64))
    assert fake.calls[-1] == "fdgs_raster_bwd"
    # a state that asked is never handed to the backward without its buffer (a NULL would silently be the other call)
    *_, st = R.rasterize_forward(*args, absgrad=True)
    gr, _ = R.fill_raster_grads(st, torch.ones(3, 48, 64), None, torch.empty(200, 3))
    with pytest.raises(fdgs._lib.FdgsError):
        R.raster_bwd_call(fake, st, gr)
    out = R.rasterize_gaussians(t["means3D"], t["means2D"], t["shs"], None, t["opacities"], t["scales"], t["rotations"], None, s, absgrad=True)
    assert len(out) == 3


def test_the_forward_of_a_frame_that_asks_is_the_forward_it_would_be_without(fake):
    pc = _model(300)
    pipe = type("Pipe", (D._Pipe,), {"absgrad": True})()
    with torch.no_grad():
        fdgs.render(_cam(0.5), pc, pipe, torch.zeros(3), stage="fine")
        fake.calls.append("fdgs_--")
        res = fdgs.render(_cam(0.25), pc, pipe, torch.zeros(3), stage="fine")
    assert " ".join(c[len("fdgs_"):] for c in fake.calls) == PARENT_CALLS["render_nograd", 300]
    assert not hasattr(res["viewspace_points"], "absgrad")
    # playback has no backward: the option of the pipe is not its business
    baked = fdgs.playback.bake(pc, D.TIMES)
    fake.calls.clear()
    baked.render(_cam(0.5), pipe, torch.zeros(3))
    assert fake.calls == ["fdgs_state_blend", "fdgs_raster_fwd_capacity", "fdgs_pair_count_wait"][-len(fake.calls):] and fake.calls


@pytest.mark.parametrize("pipe", [D._Pipe, type("PipeOff", (D._Pipe,), {"absgrad": False})], ids=["absent", "False"])
@pytest.mark.parametrize("n", D.SIZES)
@pytest.mark.parametrize("entry", sorted(D._RUNS))
def test_without_the_option_the_calls_are_what_they_were(fake, monkeypatch, entry, n, pipe):
    monkeypatch.setattr(D, "_Pipe", pipe)
    assert _calls_of(fake, entry, n) == PARENT_CALLS[entry, n]
    assert fake.abs == [] and "fdgs_raster_bwd_abs" not in fake.calls


@pytest.mark.parametrize("route", FO.ROUTES)
def test_without_the_option_the_sink_carries_no_absgrad(fake, monkeypatch, route):
    frame = FO._Frame(route, True, True, False, False, monkeypatch)
    frame.loss().backward()
    assert FO._calls(fake) == FO.expected_calls(route, True, True, False, False) and fake.abs == []
    assert not any(hasattr(s, "absgrad") for s in _sinks(frame))
