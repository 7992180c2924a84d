"""Host plumbing of the frame options (CPU, no kernels), on the fake library of tests/test_host_dryrun.py as tests/test_antialias_dryrun.py
extends it: for every combination of {alpha, antialiasing} x {no leaf, camera leaves, time leaf, both} on every route -- GaussianRasterizer
directly, render() with the fused node, render() in the two-node form, render_views() -- the ordered C calls are the ones the dispatch rule
below predicts, the alpha pointer is NULL exactly where it must be, the graph holds the node classes it always held and every gradient
lands on the input that asked, in its shape.  Nothing is computed."""
import importlib
import itertools

import pytest
import torch

import test_camera_grad_dryrun as CG
import test_host_dryrun as D
from test_antialias_dryrun import fake        # noqa: F401  (the fixture: _AAFake installed as the library)
from test_host_dryrun import _cam, _model

fdgs = importlib.import_module("4dgaussians_amd")
R = fdgs.rasterizer

# ---- the dispatch rule, stated on its own: stage -> the entry point of a (plain, alpha, antialiased, alpha + antialiased) frame -------------
# antialiased: the _aa entry, which always takes the alpha pointer (NULL where the frame has no alpha); alpha only: the _alpha entry, with
# the pointer; neither: the plain entry, without the argument.  The projection and the camera gradient have only plain and _aa forms, the
# blend only plain and _alpha (the projection carries the compensation).
RULE = {
    "preprocess_fwd": ("preprocess_fwd", "preprocess_fwd", "preprocess_fwd_aa", "preprocess_fwd_aa"),
    "render_fwd": ("render_fwd", "render_fwd_alpha", "render_fwd", "render_fwd_alpha"),
    "raster_fwd_capacity": ("raster_fwd_capacity", "raster_fwd_capacity_alpha", "raster_fwd_capacity_aa", "raster_fwd_capacity_aa"),
    "raster_bwd": ("raster_bwd", "raster_bwd_alpha", "raster_bwd_aa", "raster_bwd_aa"),
    "camera_grad": ("camera_grad", "camera_grad", "camera_grad_aa", "camera_grad_aa"),
}
ROUTES = ("rasterizer", "fused", "two_node", "views")
LEAVES = {"none": (False, False), "camera": (True, False), "time": (False, True), "camera+time": (True, True)}
CAM_LEAVES = ("world_view_transform", "camera_center")        # full_proj_transform stays a plain tensor: it must not gain a gradient
_DEFORM_FWD = ["deform_saved_bytes", "deform_pack_bytes", "deform_fwd"]


def _entry(stage, alpha, aa):
    return RULE[stage][int(alpha) + 2 * int(aa)]


def _exact(alpha, aa):
    """The first frame of a (size, count): the staged forward."""
    return ["geom_bytes", "img_bytes", _entry("preprocess_fwd", alpha, aa), "bin_prepare", "binning_bytes", "bin_sort", _entry("render_fwd", alpha, aa)]


def _raster_bwd(alpha, aa, cam):
    """fdgs_camera_grad directly behind its fdgs_raster_bwd where a camera leaf exists."""
    return [_entry("raster_bwd", alpha, aa)] + (["camera_grad_scratch_bytes", _entry("camera_grad", alpha, aa)] if cam else [])


def _deform_bwd(time):
    """fdgs_deform_time_grad directly behind its fdgs_deform_bwd where a time leaf exists."""
    return ["deform_bwd"] + (["deform_time_grad_scratch_bytes", "deform_time_grad"] if time else [])


def expected_calls(route, alpha, aa, cam, time):
    if route == "rasterizer":
        return _exact(alpha, aa) + _raster_bwd(alpha, aa, cam)
    if route == "fused":
        return _DEFORM_FWD + _exact(alpha, aa) + ["deform_bwd_scratch_bytes", "tuning_get"] + _raster_bwd(alpha, aa, cam) + _deform_bwd(time)
    if route == "two_node":
        return _DEFORM_FWD + _exact(alpha, aa) + _raster_bwd(alpha, aa, cam) + ["deform_bwd_scratch_bytes"] + _deform_bwd(time)
    capacity = [_entry("raster_fwd_capacity", alpha, aa), "pair_count_wait"]          # views 2 and 3: the one-call forward
    return (_DEFORM_FWD + _exact(alpha, aa) + _DEFORM_FWD + ["binning_bytes"] + capacity + _DEFORM_FWD + capacity
            + ["deform_bwd_scratch_bytes"] + 3 * (["tuning_get"] + _raster_bwd(alpha, aa, False) + ["deform_bwd"]))


def expected_nodes(route, cam, time):
    """The node classes the parent records for such a frame."""
    if route == "rasterizer":
        return {"_RasterizeGaussiansCameraBackward" if cam else "_RasterizeGaussiansBackward"}
    if route == "fused":
        return {"_FusedRenderTimeFunctionBackward" if time else "_FusedRenderCameraFunctionBackward" if cam else "_FusedRenderFunctionBackward"}
    if route == "two_node":
        return {"_RasterizeGaussiansCameraBackward" if cam else "_RasterizeGaussiansBackward",
                "_DeformTimeFunctionBackward" if time else "_DeformFunctionBackward"}
    return {"_FusedRenderViewsFunctionBackward"}


def _nodes(*tensors):
    """The names of this package's autograd nodes in the graph behind `tensors`."""
    seen, todo, names = set(), [t.grad_fn for t in tensors if t.grad_fn is not None], set()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if type(fn).__name__.startswith("_") and type(fn).__name__.endswith("Backward"):
            names.add(type(fn).__name__)
        todo += [f for f, _ in fn.next_functions]
    return names


def _pipe(alpha, aa):
    return type("Pipe", (D._Pipe,), {"render_alpha": alpha, "antialiasing": aa})()


class _Frame:
    """One frame of a route: its images (colour, depth, alpha or None) per view, the inputs that asked for a gradient, those that did not."""

    def __init__(self, route, alpha, aa, cam_leaf, time_leaf, monkeypatch):
        self.asked, self.silent = {}, {}
        bg = self.silent["bg"] = torch.zeros(3)
        if route == "rasterizer":
            t = CG._raster_inputs(n=300)
            s = CG._settings(_cam(), ("viewmatrix", "campos") if cam_leaf else ())
            r = R.GaussianRasterizer(s, render_alpha=alpha)
            r.antialiasing = aa
            color, radii, depth, *a = r(**t)
            self.images = [(color, depth, a[0] if a else None)]
            self.asked.update(t)
            cams = {"viewmatrix": s.viewmatrix, "campos": s.campos, "projmatrix": s.projmatrix}
            (self.asked if cam_leaf else self.silent).update({k: cams[k] for k in ("viewmatrix", "campos")})
            self.silent["projmatrix"] = cams["projmatrix"]
            return
        monkeypatch.setattr(fdgs.renderer, "FUSED_BACKWARD", route != "two_node")
        pc = _model(300)
        # what a fine frame reads: the model's six arrays and the planes and MLP tensors of its deformation network; the model's other
        # parameters (the reference's unused timenet) are in no frame's graph
        planes, mlp = fdgs.deformation._collect(pc._deformation)
        read = [pc._xyz, pc._scaling, pc._rotation, pc._opacity, pc._features_dc, pc._features_rest, *planes, *mlp]
        for k, p in pc.named_parameters():
            (self.asked if any(p is q for q in read) else self.silent)[k] = p
        assert len(self.asked) == len(read)
        if route == "views":
            cams = [_cam(0.1 * i, 10.0 * i) for i in range(3)]
            res = fdgs.render_views(cams, pc, _pipe(alpha, aa), bg, stage="fine")
        else:
            cam = _cam(0.5)
            for k in CAM_LEAVES if cam_leaf else ():
                setattr(cam, k, getattr(cam, k).clone().requires_grad_(True))
            if time_leaf:
                cam.time = torch.tensor([0.5], requires_grad=True)
                self.asked["time"] = cam.time
            (self.asked if cam_leaf else self.silent).update({k: getattr(cam, k) for k in CAM_LEAVES})
            self.silent["full_proj_transform"] = cam.full_proj_transform
            res = [fdgs.render(cam, pc, _pipe(alpha, aa), bg, stage="fine")]
        for v, r in enumerate(res):
            assert set(r) == {"render", "viewspace_points", "visibility_filter", "radii", "depth"} | ({"alpha"} if alpha else set())
            self.asked[f"viewspace_points[{v}]"] = r["viewspace_points"]
        self.images = [(r["render"], r["depth"], r.get("alpha")) for r in res]

    def loss(self, color=True, depth=True, alpha=True):
        terms = [img.sum() for view in self.images for img, use in zip(view, (color, depth, alpha)) if use and img is not None]
        return sum(terms[1:], terms[0])

    def check_gradients(self):
        for k, t in self.asked.items():
            assert t.grad is not None and t.grad.shape == t.shape, k
        for k, t in self.silent.items():
            assert t.grad is None, k


def _calls(fake):
    return [c[len("fdgs_"):] for c in fake.calls]


def _alpha_pointers(fake):
    """(forward, backward): the alpha pointers the entry points that take one were handed, in call order."""
    took = fake.alpha + [e for e in fake.aa if e[0] in ("raster_fwd_capacity_aa", "raster_bwd_aa")]
    return [a for n, a in took if "bwd" not in n], [a for n, a in took if "bwd" in n]


def _cases():
    for route, (alpha, aa), leaves in itertools.product(ROUTES, itertools.product((False, True), repeat=2), LEAVES):
        cam, time = LEAVES[leaves]
        if (route == "rasterizer" and time) or (route == "views" and (cam or time)):
            continue        # the rasterizer has no time; render_views takes times as numbers and ignores requires_grad on a camera
        yield pytest.param(route, alpha, aa, cam, time, id=f"{route}-alpha{int(alpha)}-aa{int(aa)}-{leaves}")


@pytest.mark.parametrize("route,alpha,aa,cam,time", list(_cases()))
def test_every_frame_makes_the_calls_the_rule_predicts_and_every_gradient_lands_where_it_was_asked(fake, monkeypatch, route, alpha, aa, cam, time):
    frame = _Frame(route, alpha, aa, cam, time, monkeypatch)
    assert _nodes(*frame.images[0][:2]) == expected_nodes(route, cam, time)
    frame.loss().backward()
    assert _calls(fake) == expected_calls(route, alpha, aa, cam, time)
    fwd, bwd = _alpha_pointers(fake)
    views = len(frame.images)
    # the forward entries that take the pointer: the blend of the staged frame (alpha frames only), the one-call forward of views 2 and 3
    assert len(fwd) == (1 if alpha else 0) + (views - 1 if alpha or aa else 0) and all((a != 0) == alpha for a in fwd)
    assert len(bwd) == (views if alpha or aa else 0) and all((a != 0) == alpha for a in bwd)       # (the loss saw alpha where there is one)
    if alpha:
        assert fwd == [view[2].data_ptr() for view in frame.images]
    if cam:
        CG._paired(fake, 1)
    frame.check_gradients()


# ---- losses that see only part of the frame, on the frame that asks for everything ------------------------------------------------------

FULL = [pytest.param("rasterizer", True, False, id="rasterizer"), pytest.param("fused", True, True, id="fused"),
        pytest.param("two_node", True, True, id="two_node")]


@pytest.mark.parametrize("route,cam,time", FULL)
@pytest.mark.parametrize("sees", ["depth", "alpha"])
def test_a_loss_that_sees_only_depth_or_only_alpha(fake, monkeypatch, route, cam, time, sees):
    frame = _Frame(route, True, True, cam, time, monkeypatch)
    frame.loss(color=False, depth=sees == "depth", alpha=sees == "alpha").backward()
    assert _calls(fake) == expected_calls(route, True, True, cam, time)
    fwd, bwd = _alpha_pointers(fake)
    assert fwd == [frame.images[0][2].data_ptr()] and len(bwd) == 1 and (bwd[0] != 0) == (sees == "alpha")
    frame.check_gradients()


@pytest.mark.parametrize("route,cam,time", FULL + [pytest.param("views", False, False, id="views")])
def test_a_backward_that_no_image_reached_returns_without_a_call(fake, monkeypatch, route, cam, time):
    frame = _Frame(route, True, True, cam, time, monkeypatch)
    node = frame.images[0][0].grad_fn
    while type(node).__name__ not in expected_nodes(route, cam, time):          # (render_views: behind the select of the view's slice)
        node = node.next_functions[0][0]
    before = list(fake.calls)
    n_outputs = {"rasterizer": 4, "two_node": 4, "fused": 5, "views": 4}[route]
    grads = node.apply(*[None] * n_outputs)
    assert fake.calls == before
    assert len(grads) == len(node.needs_input_grad) and all(g is None for g in grads)          # one None per input of the node


@pytest.mark.parametrize("route,cam,time", FULL)
def test_a_second_backward_of_the_same_state_gets_a_fresh_accumulator(fake, monkeypatch, route, cam, time):
    seen = []
    real = R.raster_bwd_call
    monkeypatch.setattr(R, "raster_bwd_call", lambda L, state, g, *a: (seen.append((int(g.scratch_acc or 0), int(g.scratch_acc_zeroed))), real(L, state, g, *a))[1])
    frame = _Frame(route, True, True, cam, time, monkeypatch)
    loss = frame.loss()
    loss.backward(retain_graph=True)
    loss.backward()
    (a0, z0), (a1, z1) = seen
    assert a0 != 0 and a1 != 0 and (z0, z1) == (1, 0)
    frame.check_gradients()
