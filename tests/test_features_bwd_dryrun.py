"""Host plumbing of render_features(differentiable=True), dry (CPU, no kernels): Baked / SparseBaked / Composite against the fake library
of tests/test_host_dryrun.py.  What is pinned: a differentiable frame makes the call sequence of a plain one; `.backward()` adds exactly
ONE fdgs_render_features_bwd and nothing else, handed C, rows = N, the row-map pointer (NULL for rows stored in the model's order), a
negative min_alpha unless `normalize` with the alpha pointer = out["alpha"], and the frame state's capacity; under no_grad, or with values
that do not require grad, nothing is attached and no backward call can follow."""
import importlib
import types

import pytest
import torch

from test_host_dryrun import TIMES, _Pipe, _cam, _model, _two_baked, fake  # noqa: F401  (`fake` is the fixture)

fdgs = importlib.import_module("4dgaussians_amd")
P, C = fdgs.playback, fdgs.compose
BWD = "fdgs_render_features_bwd"


def _recording(fake):
    """The fake keeps, per fdgs_render_features_bwd, its arguments behind the stream as a namespace (pointers as integers or None), and
    the capacity each fdgs_render_features was handed."""
    log = types.SimpleNamespace(calls=[], forward_R=[])

    def addr(v):
        return getattr(v, "value", v)

    def note(self, name, a):
        if name == "fdgs_render_features":
            log.forward_R.append(int(a[5]))
        elif name == BWD:
            assert len(a) == 14
            log.calls.append(types.SimpleNamespace(dims=(a[1].P, a[1].W, a[1].H), R=int(a[5]), C=a[6], grad=addr(a[7]), alpha=addr(a[8]),
                                                   min_alpha=float(a[9]), row_map=addr(a[10]), rows=a[11], dvalues=addr(a[12]), stride=a[13]))
    fake._note = types.MethodType(note, fake)
    fake.record = True
    return log


def _sequence(fake):
    out = list(fake.calls)
    fake.calls.clear()
    return out


def _objects(n):
    baked = P.bake(_model(n), TIMES)
    sparse = P.bake_sparse(_model(n), TIMES, tol=-1.0)
    scene = C.compose(_two_baked(n), [None, C.Placement(translation=(0.5, 0.0, -0.25), scale=0.5, time_offset=0.1)])
    return {"Baked": (baked, n), "SparseBaked": (sparse, n), "Composite": (scene, 2 * n)}


@pytest.mark.parametrize("n", [300, 8200])
@pytest.mark.parametrize("kind", ["Baked", "SparseBaked", "Composite"])
def test_a_differentiable_frame_is_a_plain_frame_and_backward_is_one_call(fake, kind, n):
    log = _recording(fake)
    obj, rows = _objects(n)[kind]
    fake.calls.clear()
    values = torch.rand(rows, 9, requires_grad=True)
    # two frames first, so that the two compared are both speculative frames whose buffer sizes are known (the first frame of a size is
    # exact and the second asks for the capacity's binning size: other sequences)
    obj.render_features(_cam(0.25), _Pipe(), torch.zeros(3), values)
    obj.render_features(_cam(0.25), _Pipe(), torch.zeros(3), values)
    fake.calls.clear()
    plain_out = obj.render_features(_cam(0.25), _Pipe(), torch.zeros(3), values)
    plain = _sequence(fake)
    out = obj.render_features(_cam(0.25), _Pipe(), torch.zeros(3), values, differentiable=True)
    assert _sequence(fake) == plain and BWD not in plain and plain[-1] == "fdgs_render_features"
    assert plain_out["features"].grad_fn is None and not plain_out["features"].requires_grad      # the default: as before
    assert out["features"].requires_grad and out["features"].grad_fn is not None
    assert set(out) == set(plain_out) and out["features"].shape == (9, 48, 64)
    for key, value in out.items():
        if key != "features" and torch.is_tensor(value):
            assert not value.requires_grad and value.grad_fn is None, key
    grad = torch.rand(9, 48, 64)
    out["features"].backward(grad, retain_graph=True)
    assert _sequence(fake) == [BWD]                                  # exactly one call, and no other
    call, = log.calls
    assert call.dims == (rows, 64, 48) and call.R == log.forward_R[-1] == 8192          # the state's capacity, as the forward's pass
    assert (call.C, call.rows, call.stride) == (9, rows, 9)
    assert call.grad == grad.data_ptr()                              # a contiguous float32 gradient is read in place
    assert call.min_alpha < 0.0 and call.alpha is None               # raw sums: no alpha image
    if n == 8200:
        assert call.row_map == obj._pick_row_map.data_ptr()
    else:
        assert call.row_map is None and obj._pick_row_map is None    # rows in the model's order: a NULL row map
    assert values.grad is not None and values.grad.shape == values.shape and values.grad.dtype == torch.float32
    # a second backward of the retained graph: the same call once more, nothing was consumed
    out["features"].backward(grad)
    assert _sequence(fake) == [BWD] and log.calls[1].R == call.R and log.calls[1].row_map == call.row_map


def test_normalize_hands_over_the_alpha_image_and_min_alpha(fake):
    log = _recording(fake)
    n = 300
    baked = P.bake(_model(n), TIMES)
    column = torch.rand(n, 12)[:, 3].requires_grad_()               # [N] with stride 12: one channel
    out = baked.render_features(_cam(0.5), _Pipe(), torch.zeros(3), column, normalize=True, min_alpha=0.25, differentiable=True)
    fake.calls.clear()
    out["features"].sum().backward()
    assert _sequence(fake) == [BWD]
    call, = log.calls
    assert call.min_alpha == 0.25 and call.alpha == out["alpha"].data_ptr()
    assert (call.C, call.rows, call.stride) == (1, n, 1) and call.R == log.forward_R[-1] == fake.pair_count      # the exact path's count
    assert column.grad.shape == (n,)                                 # in the shape of `values`


def test_a_frame_rendered_in_between_does_not_change_what_the_backward_is_handed(fake):
    log = _recording(fake)
    n = 300
    sb = P.bake_sparse(_model(n), TIMES, tol=-1.0)
    values = torch.rand(n, 4, requires_grad=True)
    out = sb.render_features(_cam(0.25), _Pipe(), torch.zeros(3), values, differentiable=True)
    fn = out["features"].grad_fn
    state = fn.frame.rstate
    kept = (state.geom.data_ptr(), state.binning.data_ptr(), state.img.data_ptr(), state.capacity)
    sb.render(_cam(0.75, theta=20.0), _Pipe(), torch.zeros(3))       # another time and view
    fake.calls.clear()
    out["features"].sum().backward()
    assert _sequence(fake) == [BWD]
    assert (state.geom.data_ptr(), state.binning.data_ptr(), state.img.data_ptr(), state.capacity) == kept and log.calls[0].R == kept[3]


def test_without_grad_nothing_is_attached(fake):
    log = _recording(fake)
    n = 300
    for obj, rows in _objects(n).values():
        needs = torch.rand(rows, 3, requires_grad=True)
        with torch.no_grad():
            out = obj.render_features(_cam(0.5), _Pipe(), torch.zeros(3), needs, differentiable=True)
        assert out["features"].grad_fn is None and not out["features"].requires_grad
        out = obj.render_features(_cam(0.5), _Pipe(), torch.zeros(3), torch.rand(rows, 3), differentiable=True)
        assert out["features"].grad_fn is None and not out["features"].requires_grad
        assert out["alpha"].grad_fn is None
    assert BWD not in fake.calls and log.calls == []
    # a graph whose features did not enter the loss: the gradient is None, and None costs no launch
    baked, rows = _objects(n)["Baked"]
    needs = torch.rand(rows, 3, requires_grad=True)
    out = baked.render_features(_cam(0.5), _Pipe(), torch.zeros(3), needs, differentiable=True)
    fake.calls.clear()
    assert out["features"].grad_fn.apply(None) == (None, None) and fake.calls == []
