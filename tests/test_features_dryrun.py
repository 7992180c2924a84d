"""Host plumbing of render_features, dry (CPU, no kernels): Baked / SparseBaked / Composite.render_features against the fake library of
tests/test_host_dryrun.py.  What is pinned: a features frame is the state launches of its one state_at call, ONE rasterizer front half
(exact or capacity) and ONE fdgs_render_features -- no second projection, sort or render_fwd --, and what that call is handed: C, the
tensor's own address and row stride (the values are read in place), the number of rows, the row-map pointer (NULL for rows stored in the
model's order), a negative min_alpha unless `normalize`, and the output pointers."""
import importlib
import types

import pytest
import torch

from test_host_dryrun import TIMES, _CAP, _EXACT, _Pipe, _cam, _model, _two_baked, fake  # noqa: F401  (`fake` is the fixture)

fdgs = importlib.import_module("4dgaussians_amd")
P, C = fdgs.playback, fdgs.compose
_FRONT_HALF = ("preprocess_fwd", "bin_prepare", "bin_sort", "raster_fwd_capacity", "render_fwd")
FEATURE_KEYS = {"features", "alpha"}
RENDER_KEYS = {"render", "viewspace_points", "visibility_filter", "radii", "depth"}


def _recording(fake):
    """The fake keeps, per fdgs_render_features, its arguments behind the stream as a namespace (pointers as integers or None)."""
    log = types.SimpleNamespace(calls=[], capacity=[])

    def addr(v):
        return getattr(v, "value", v)

    def note(self, name, a):
        if name == "fdgs_raster_fwd_capacity":
            log.capacity.append(int(a[5]))
        elif name == "fdgs_render_features":
            assert len(a) == 14
            log.calls.append(types.SimpleNamespace(dims=(a[1].P, a[1].W, a[1].H), R=int(a[5]), C=a[6], values=addr(a[7]), stride=a[8], rows=a[9],
                                                   row_map=addr(a[10]), min_alpha=float(a[11]), features=addr(a[12]), alpha=addr(a[13])))
    fake._note = types.MethodType(note, fake)
    fake.record = True
    return log


def _calls(fake):
    out = " ".join(c[len("fdgs_"):] for c in fake.calls)
    fake.calls.clear()
    return out


def _check_frame(calls, state_calls, exact, n_perm, extra=""):
    front = _EXACT if exact else _CAP
    assert calls == f"{state_calls}{front}{' permute_rows' * n_perm}{extra} render_features", calls
    for name in _FRONT_HALF:                                     # exactly one front half, and its one blend
        assert calls.split().count(name) == (1 if name in front.split() else 0), name


def _check_outputs(out, n, c, call):
    assert set(out) >= RENDER_KEYS | FEATURE_KEYS and out["viewspace_points"] is None and out["radii"].shape == (n,)
    assert out["features"].shape == (c, 48, 64) and out["alpha"].shape == (1, 48, 64)
    assert out["features"].dtype == out["alpha"].dtype == torch.float32
    assert out["features"].is_contiguous() and out["alpha"].is_contiguous()
    assert (call.features, call.alpha) == (out["features"].data_ptr(), out["alpha"].data_ptr())


@pytest.mark.parametrize("n", [300, 8200])
def test_baked_render_features_is_one_front_half_and_one_pass(fake, n):
    log = _recording(fake)
    baked = P.bake(_model(n), TIMES)
    permuted = n == 8200
    assert (baked.perm is not None) == permuted and baked._pick_row_map is None
    fake.calls.clear()
    nbytes = baked.nbytes
    wide = torch.rand(n, 12)
    values = wide[:, 1:10]                                       # nine channels of a wider array: read in place, row stride 12
    out = baked.render_features(_cam(0.25), _Pipe(), torch.zeros(3), values)
    _check_frame(_calls(fake), "state_blend ", True, int(permuted))
    assert set(out) == RENDER_KEYS | FEATURE_KEYS and baked.nbytes == nbytes
    call, = log.calls
    assert call.R == fake.pair_count == 7 and call.dims == (n, 64, 48)          # exact path: laid out for the true pair count
    assert (call.C, call.values, call.stride, call.rows) == (9, values.data_ptr(), 12, n) and values.data_ptr() == wide.data_ptr() + 4
    assert call.min_alpha < 0.0                                  # raw sums unless asked to normalize
    _check_outputs(out, n, 9, call)
    if permuted:
        assert baked._pick_row_map.dtype == torch.int32 and torch.equal(baked._pick_row_map, baked.perm.to(torch.int32))
        assert call.row_map == baked._pick_row_map.data_ptr()
    else:
        assert call.row_map is None and baked._pick_row_map is None                  # rows in the model's order: a NULL row map
    kept = baked._pick_row_map
    # the next frame of this size is speculative: one capacity frame, and the pass gets THAT capacity; at a baked timestamp: no blend
    column = wide[:, 3]                                          # [N] with stride 12: one channel
    out = baked.render_features(_cam(0.5, theta=20.0), _Pipe(), torch.zeros(3), column, normalize=True, rgb8="trunc")
    _check_frame(_calls(fake), "", False, int(permuted), extra=" image_rgb8")
    call = log.calls[1]
    assert call.R == log.capacity[0] == 8192 and "rgb8" in out
    assert (call.C, call.values, call.stride, call.rows) == (1, column.data_ptr(), 12, n)
    assert abs(call.min_alpha - 1e-4) < 1e-10 and call.row_map == log.calls[0].row_map
    _check_outputs(out, n, 1, call)
    assert baked._pick_row_map is kept                                               # built once
    plain = torch.rand(n, 3)
    baked.render_features(_cam(0.75), _Pipe(), torch.zeros(3), plain, normalize=True, min_alpha=0.25)
    assert (log.calls[2].C, log.calls[2].stride, log.calls[2].min_alpha) == (3, 3, 0.25)
    baked.render_features(_cam(0.75), _Pipe(), torch.zeros(3), plain, min_alpha=0.25)
    assert log.calls[3].min_alpha < 0.0


@pytest.mark.parametrize("n", [300, 8200])
def test_sparse_render_features_scatters_first_and_leaves_the_state_truthful(fake, n):
    log = _recording(fake)
    sb = P.bake_sparse(_model(n), TIMES, tol=-1.0)
    fake.calls.clear()
    values = torch.rand(n, 17)
    out = sb.render_features(_cam(0.25), _Pipe(), torch.zeros(3), values)
    _check_frame(_calls(fake), "state_scatter ", True, int(n == 8200))
    assert sb.launches == 1 and sb._shown == P.locate(TIMES, 0.25)
    call, = log.calls
    assert (call.C, call.values, call.stride, call.rows) == (17, values.data_ptr(), 17, n)
    _check_outputs(out, n, 17, call)
    assert (call.row_map is None) == (sb.perm is None)
    sb.render(_cam(0.25), _Pipe(), torch.zeros(3))                   # the working state holds the frame's time: no state launch
    assert _calls(fake) == f"{_CAP}{' permute_rows' * int(n == 8200)}" and sb.launches == 1


@pytest.mark.parametrize("n", [300, 8200])
def test_composite_render_features_places_first_and_hands_over_the_scene_row_map(fake, n):
    log = _recording(fake)
    models = _two_baked(n)
    scene = C.compose(models, [None, C.Placement(translation=(0.5, 0.0, -0.25), scale=0.5, time_offset=0.1)])
    fake.calls.clear()
    launches = scene.launches
    values = scene.model_indicator()
    assert values.shape == (2 * n, 2) and torch.equal(values[:n, 0], torch.ones(n)) and torch.equal(values[n:, 1], torch.ones(n))
    out = scene.render_features(_cam(0.25), _Pipe(), torch.zeros(3), values)
    _check_frame(_calls(fake), "state_place state_place ", True, 2 * int(n == 8200))
    assert scene.launches == launches + 2
    call, = log.calls
    assert call.R == 7 and call.dims == (2 * n, 64, 48) and (call.C, call.values, call.stride, call.rows) == (2, values.data_ptr(), 2, 2 * n)
    _check_outputs(out, 2 * n, 2, call)
    if n == 8200:
        want = torch.cat([models[0].perm.to(torch.int32), models[1].perm.to(torch.int32) + n])
        assert torch.equal(scene._pick_row_map, want) and call.row_map == scene._pick_row_map.data_ptr()
    else:
        assert call.row_map is None and scene._pick_row_map is None
    scene.render(_cam(0.25), _Pipe(), torch.zeros(3))
    assert _calls(fake) == f"{_CAP}{' permute_rows' * 2 * int(n == 8200)}" and scene.launches == launches + 2


def test_render_features_refuses_what_it_cannot_do(fake):
    n = 300
    baked = P.bake(_model(n), TIMES)
    sb = P.bake_sparse(_model(n), TIMES, tol=-1.0)
    scene = C.compose([baked])
    fake.calls.clear()
    good = torch.rand(n, 4)
    bad = {"rows": torch.rand(n + 1, 4), "dtype": good.double(), "dims": torch.rand(n, 2, 2), "scalar": torch.tensor(1.0),
           "no channels": torch.rand(n, 0), "last stride": torch.rand(n, 8)[:, ::2], "transposed": torch.rand(4, n).t(),
           "expanded": torch.rand(1, 4).expand(n, 4), "not a tensor": [[0.0] * 4] * n}
    for obj in (baked, sb, scene):
        for what, values in bad.items():
            with pytest.raises(ValueError, match="values"):
                obj.render_features(_cam(0.5), _Pipe(), torch.zeros(3), values)
        for m in (-1.0, float("nan")):
            with pytest.raises(ValueError, match="min_alpha"):
                obj.render_features(_cam(0.5), _Pipe(), torch.zeros(3), good, normalize=True, min_alpha=m)
        for flag in ("convert_SHs_python", "compute_cov3D_python"):
            pipe = _Pipe()
            setattr(pipe, flag, True)
            with pytest.raises(NotImplementedError):
                obj.render_features(_cam(0.5), pipe, torch.zeros(3), good)
    assert fake.calls == []                                         # refused before anything was launched
