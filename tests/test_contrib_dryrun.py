"""Host plumbing of render_contrib, dry (CPU, no kernels): Baked / SparseBaked / Composite.render_contrib against the fake library of
tests/test_host_dryrun.py.  What is pinned: a contribution frame is the state launches of its one state_at call, ONE rasterizer front half
(exact or capacity) and ONE fdgs_render_contrib -- no second projection, sort or render_fwd --, and what that call is handed: the owner's
row-map pointer (NULL for rows stored in the model's order), the pair count the state's buffers are laid out for, the pixel-weight pointer
(NULL without one) and the `into` buffer's pointer, which a second call reuses and does not clear."""
import importlib
import types

import pytest
import torch

from test_host_dryrun import TIMES, _CAP, _EXACT, _Pipe, _cam, _model, _two_baked, fake  # noqa: F401  (`fake` is the fixture)

fdgs = importlib.import_module("4dgaussians_amd")
P, C = fdgs.playback, fdgs.compose
_CAP_AGAIN = "raster_fwd_capacity pair_count_wait"             # (the size of a binning buffer of that capacity is cached by then)
_FRONT_HALF = ("preprocess_fwd", "bin_prepare", "bin_sort", "raster_fwd_capacity", "render_fwd")
RENDER_KEYS = {"render", "viewspace_points", "visibility_filter", "radii", "depth"}
W, H = 64, 48


def _ptr(v):
    return None if v is None else (v.value if hasattr(v, "value") else int(v))


def _recording(fake):
    """The fake keeps, per fdgs_render_contrib: (num_rendered, pixel-weight pointer or None, row-map pointer or None, (P, W, H), rows
    pointer), and the capacity of every capacity frame."""
    log = types.SimpleNamespace(contrib=[], capacity=[])

    def note(self, name, a):
        if name == "fdgs_raster_fwd_capacity":
            log.capacity.append(int(a[5]))
        elif name == "fdgs_render_contrib":
            assert len(a) == 9
            log.contrib.append((int(a[5]), _ptr(a[6]), _ptr(a[7]), (a[1].P, a[1].W, a[1].H), _ptr(a[8])))
    fake._note = types.MethodType(note, fake)
    fake.record = True
    return log


def _calls(fake):
    out = " ".join(c[len("fdgs_"):] for c in fake.calls)
    fake.calls.clear()
    return out


def _check_contrib_frame(calls, state_calls, exact, n_perm, extra=""):
    front = _EXACT if exact else _CAP
    assert calls == f"{state_calls}{front}{' permute_rows' * n_perm}{extra} render_contrib", calls
    for name in _FRONT_HALF:                                     # exactly one front half, and its one blend
        assert calls.split().count(name) == (1 if name in front.split() else 0), name


@pytest.mark.parametrize("n", [300, 8200])
def test_baked_render_contrib_is_one_front_half_and_one_contrib(fake, n):
    log = _recording(fake)
    baked = P.bake(_model(n), TIMES)
    permuted = n == 8200
    assert (baked.perm is not None) == permuted and baked._pick_row_map is None
    fake.calls.clear()
    nbytes = baked.nbytes
    out = baked.render_contrib(_cam(0.25), _Pipe(), torch.zeros(3))
    _check_contrib_frame(_calls(fake), "state_blend ", True, int(permuted))
    assert set(out) == RENDER_KEYS | {"contribution"} and out["viewspace_points"] is None and baked.nbytes == nbytes
    acc = out["contribution"]
    assert isinstance(acc, P.Contribution) and acc.N == n and acc.frames == 1 and acc.rows.shape == (n, 4) and acc.rows.dtype == torch.int32
    assert acc.rows.is_contiguous() and not acc.rows.any() and out["radii"].shape == (n,)
    # exact path: the state is laid out for the true pair count, 7; no pixel weight: NULL
    (r0, w0, map0, dims0, rows0), = log.contrib
    assert r0 == fake.pair_count == 7 and w0 is None and dims0 == (n, W, H) and rows0 == acc.rows.data_ptr()
    if permuted:
        assert baked._pick_row_map.dtype == torch.int32 and torch.equal(baked._pick_row_map, baked.perm.to(torch.int32))
        assert map0 == baked._pick_row_map.data_ptr()
    else:
        assert map0 is None and baked._pick_row_map is None                          # rows in the model's order: a NULL row map
    kept = baked._pick_row_map
    # a second pass INTO the same Contribution: the same buffer, not cleared; the next frame of this size is speculative: one capacity
    # frame, and the pass gets THAT capacity; at a baked timestamp: no blend
    acc.rows[5, 2] = 41                                                              # (stands in for what the first pass accumulated)
    weight = torch.rand(H, W)
    out = baked.render_contrib(_cam(0.5, theta=20.0), _Pipe(), torch.zeros(3), into=acc, pixel_weight=weight, rgb8="trunc")
    _check_contrib_frame(_calls(fake), "", False, int(permuted), extra=" image_rgb8")
    r1, w1, map1, dims1, rows1 = log.contrib[1]
    assert r1 == log.capacity[0] == 8192 and w1 == weight.data_ptr() and map1 == map0 and dims1 == dims0 and rows1 == rows0 and "rgb8" in out
    assert out["contribution"] is acc and acc.frames == 2 and int(acc.rows[5, 2]) == 41 and int(acc.rows.sum()) == 41
    assert baked._pick_row_map is kept                                               # built once (shared with render_pick)
    out = baked.render_contrib(_cam(0.75), _Pipe(), torch.zeros(3), into=acc, pixel_weight=weight.reshape(1, H, W))
    assert _calls(fake) == f"state_blend {_CAP_AGAIN}{' permute_rows' * int(permuted)} render_contrib"
    assert log.contrib[2][1] == weight.data_ptr() and log.contrib[2][4] == rows0 and acc.frames == 3
    fresh = baked.render_contrib(_cam(0.75), _Pipe(), torch.zeros(3))["contribution"]
    assert fresh is not acc and fresh.frames == 1 and log.contrib[3][4] == fresh.rows.data_ptr() != rows0
    fake.calls.clear()
    baked.render_pick(_cam(0.75), _Pipe(), torch.zeros(3))                           # the pick shares the row map
    assert baked._pick_row_map is kept


@pytest.mark.parametrize("n", [300, 8200])
def test_sparse_render_contrib_scatters_first_and_leaves_the_state_truthful(fake, n):
    log = _recording(fake)
    sb = P.bake_sparse(_model(n), TIMES, tol=-1.0)
    fake.calls.clear()
    out = sb.render_contrib(_cam(0.25), _Pipe(), torch.zeros(3))
    _check_contrib_frame(_calls(fake), "state_scatter ", True, int(n == 8200))
    assert sb.launches == 1 and sb._shown == P.locate(TIMES, 0.25)
    assert out["contribution"].N == n and log.contrib[0][4] == out["contribution"].rows.data_ptr() and log.contrib[0][0] == 7
    assert (log.contrib[0][2] is None) == (sb.perm is None)
    sb.render(_cam(0.25), _Pipe(), torch.zeros(3))                   # the working state holds the frame's time: no state launch
    assert _calls(fake) == f"{_CAP}{' permute_rows' * int(n == 8200)}" and sb.launches == 1


@pytest.mark.parametrize("n", [300, 8200])
def test_composite_render_contrib_places_first_and_hands_over_the_scene_row_map(fake, n):
    log = _recording(fake)
    models = _two_baked(n)
    scene = C.compose(models, [None, C.Placement(translation=(0.5, 0.0, -0.25), scale=0.5, time_offset=0.1)])
    fake.calls.clear()
    launches = scene.launches
    out = scene.render_contrib(_cam(0.25), _Pipe(), torch.zeros(3))
    _check_contrib_frame(_calls(fake), "state_place state_place ", True, 2 * int(n == 8200))
    assert scene.launches == launches + 2
    (r, w, rmap, dims, rows), = log.contrib
    acc = out["contribution"]
    assert r == 7 and w is None and dims == (2 * n, W, H) and acc.N == 2 * n and rows == acc.rows.data_ptr() and out["radii"].shape == (2 * n,)
    if n == 8200:
        want = torch.cat([models[0].perm.to(torch.int32), models[1].perm.to(torch.int32) + n])
        assert scene._pick_row_map.dtype == torch.int32 and torch.equal(scene._pick_row_map, want) and rmap == scene._pick_row_map.data_ptr()
    else:
        assert rmap is None and scene._pick_row_map is None
    scene.render(_cam(0.25), _Pipe(), torch.zeros(3))
    assert _calls(fake) == f"{_CAP}{' permute_rows' * 2 * int(n == 8200)}" and scene.launches == launches + 2
    assert not hasattr(scene, "select_rows") and not hasattr(P.SparseBaked, "select_rows")        # out of scope: select per model


def test_contribution_loops_render_contrib_over_cameras_and_times(fake):
    log = _recording(fake)
    baked = P.bake(_model(300), TIMES)
    cams = [_cam(0.0), _cam(0.5, theta=20.0), _cam(1.0, theta=40.0)]
    fake.calls.clear()
    acc = P.contribution(baked, cams, _Pipe(), torch.zeros(3))
    assert isinstance(acc, P.Contribution) and acc.N == 300 and acc.frames == 3
    assert fake.calls.count("fdgs_render_contrib") == 3 and fake.calls.count("fdgs_state_blend") == 0       # each at its own, baked, time
    assert {c[4] for c in log.contrib} == {acc.rows.data_ptr()}
    fake.calls.clear()
    again = P.contribution(baked, cams[:2], _Pipe(), torch.zeros(3), times=[0.25, 0.5, 0.75], into=acc, pixel_weight=torch.ones(H, W))
    assert again is acc and acc.frames == 3 + 6
    assert fake.calls.count("fdgs_render_contrib") == 6 and fake.calls.count("fdgs_state_blend") == 4       # 0.25 and 0.75 lie in between
    assert all(c[4] == acc.rows.data_ptr() and c[1] is not None for c in log.contrib[3:])
    assert cams[0].time == 0.0                                                       # the cameras keep their own times


def test_render_contrib_refuses_what_it_cannot_do(fake):
    baked = P.bake(_model(300), TIMES)
    sb = P.bake_sparse(_model(300), TIMES, tol=-1.0)
    scene = C.compose([baked])
    fake.calls.clear()
    for obj in (baked, sb, scene):
        for bad in (torch.ones(H, W + 1), torch.ones(W, H), torch.ones(3, H, W), torch.ones(H * W), torch.ones(H, W, dtype=torch.float64),
                    torch.ones(H, W, dtype=torch.int32), torch.ones(H, W, device="meta"), [[1.0] * W] * H):
            with pytest.raises(ValueError, match="pixel_weight"):
                obj.render_contrib(_cam(0.5), _Pipe(), torch.zeros(3), pixel_weight=bad)
        for bad in (P.Contribution(obj.N + 1, obj.device), P.Contribution(obj.N, torch.device("meta")), torch.zeros(obj.N, 4, dtype=torch.int32)):
            with pytest.raises(ValueError, match="into"):
                obj.render_contrib(_cam(0.5), _Pipe(), torch.zeros(3), into=bad)
        for flag in ("convert_SHs_python", "compute_cov3D_python"):
            pipe = _Pipe()
            setattr(pipe, flag, True)
            with pytest.raises(NotImplementedError, match="need the live model"):
                obj.render_contrib(_cam(0.5), pipe, torch.zeros(3))
    assert fake.calls == []                                         # refused before anything was launched
