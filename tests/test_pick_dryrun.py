"""Host plumbing of render_pick, dry (CPU, no kernels): Baked / SparseBaked / Composite.render_pick against the fake library of
tests/test_host_dryrun.py.  What is pinned: a pick frame is the state launches of its one state_at call, ONE rasterizer front half (exact
or capacity) and ONE fdgs_render_pick -- no second projection, sort or render_fwd --, and what that call is handed: the row-map pointer
(NULL for rows stored in the model's order), alpha_cut, and the pair count the state's buffers are laid out for."""
import importlib
import types

import pytest
import torch

from test_host_dryrun import TIMES, _CAP, _EXACT, _Pipe, _cam, _model, _two_baked, fake  # noqa: F401  (`fake` is the fixture)

fdgs = importlib.import_module("4dgaussians_amd")
P, C = fdgs.playback, fdgs.compose
_CAP_AGAIN = "raster_fwd_capacity pair_count_wait"             # (the size of a binning buffer of that capacity is cached by then)
_FRONT_HALF = ("preprocess_fwd", "bin_prepare", "bin_sort", "raster_fwd_capacity", "render_fwd")
PICK_KEYS = {"pick_id", "pick_weight", "surface_id", "surface_depth"}
RENDER_KEYS = {"render", "viewspace_points", "visibility_filter", "radii", "depth"}


def _recording(fake):
    """The fake keeps, per fdgs_render_pick: (num_rendered, alpha_cut, row-map pointer or None, (P, W, H), the four output pointers), and
    the capacity of every capacity frame."""
    log = types.SimpleNamespace(pick=[], capacity=[])

    def note(self, name, a):
        if name == "fdgs_raster_fwd_capacity":
            log.capacity.append(int(a[5]))
        elif name == "fdgs_render_pick":
            out = a[8]
            log.pick.append((int(a[5]), float(a[6]), None if a[7] is None else a[7].value, (a[1].P, a[1].W, a[1].H),
                             (out.pick_id, out.pick_weight, out.surface_id, out.surface_depth)))
    fake._note = types.MethodType(note, fake)
    fake.record = True
    return log


def _calls(fake):
    out = " ".join(c[len("fdgs_"):] for c in fake.calls)
    fake.calls.clear()
    return out


def _check_pick_frame(calls, state_calls, exact, n_perm, extra=""):
    front = _EXACT if exact else _CAP
    assert calls == f"{state_calls}{front}{' permute_rows' * n_perm}{extra} render_pick", calls
    for name in _FRONT_HALF:                                     # exactly one front half, and its one blend
        assert calls.split().count(name) == (1 if name in front.split() else 0), name


def _check_outputs(out, n, ptrs):
    assert set(out) >= RENDER_KEYS | PICK_KEYS and out["viewspace_points"] is None and out["radii"].shape == (n,)
    assert out["pick_id"].shape == out["surface_id"].shape == out["pick_weight"].shape == (48, 64) and out["surface_depth"].shape == (1, 48, 64)
    assert out["pick_id"].dtype == out["surface_id"].dtype == torch.int32
    assert out["pick_weight"].dtype == out["surface_depth"].dtype == torch.float32
    assert ptrs == (out["pick_id"].data_ptr(), out["pick_weight"].data_ptr(), out["surface_id"].data_ptr(), out["surface_depth"].data_ptr())
    assert all(out[k].is_contiguous() for k in PICK_KEYS)


@pytest.mark.parametrize("n", [300, 8200])
def test_baked_render_pick_is_one_front_half_and_one_pick(fake, n):
    log = _recording(fake)
    baked = P.bake(_model(n), TIMES)
    permuted = n == 8200
    assert (baked.perm is not None) == permuted and baked._pick_row_map is None
    fake.calls.clear()
    nbytes = baked.nbytes
    out = baked.render_pick(_cam(0.25), _Pipe(), torch.zeros(3))
    _check_pick_frame(_calls(fake), "state_blend ", True, int(permuted))
    assert set(out) == RENDER_KEYS | PICK_KEYS and baked.nbytes == nbytes
    # exact path: the state is laid out for the true pair count, 7; alpha_cut defaults to the median
    (r0, cut0, map0, dims0, ptrs0), = log.pick
    assert r0 == fake.pair_count == 7 and cut0 == 0.5 and dims0 == (n, 64, 48)
    _check_outputs(out, n, ptrs0)
    if permuted:
        assert baked._pick_row_map.dtype == torch.int32 and torch.equal(baked._pick_row_map, baked.perm.to(torch.int32))
        assert map0 == baked._pick_row_map.data_ptr()
    else:
        assert map0 is None and baked._pick_row_map is None                          # rows in the model's order: a NULL row map
    kept = baked._pick_row_map
    # the next frame of this size is speculative: one capacity frame, and the pick gets THAT capacity; at a baked timestamp: no blend
    out = baked.render_pick(_cam(0.5, theta=20.0), _Pipe(), torch.zeros(3), alpha_cut=1.0, rgb8="trunc")
    _check_pick_frame(_calls(fake), "", False, int(permuted), extra=" image_rgb8")
    r1, cut1, map1, dims1, ptrs1 = log.pick[1]
    assert r1 == log.capacity[0] == 8192 and cut1 == 1.0 and map1 == map0 and dims1 == dims0 and "rgb8" in out
    _check_outputs(out, n, ptrs1)
    assert baked._pick_row_map is kept                                               # built once
    baked.render_pick(_cam(0.75), _Pipe(), torch.zeros(3), alpha_cut=1.0 / 255.0)
    assert _calls(fake) == f"state_blend {_CAP_AGAIN}{' permute_rows' * int(permuted)} render_pick"
    assert abs(log.pick[2][1] - 1.0 / 255.0) < 1e-12


@pytest.mark.parametrize("n", [300, 8200])
def test_sparse_render_pick_scatters_first_and_leaves_the_state_truthful(fake, n):
    log = _recording(fake)
    sb = P.bake_sparse(_model(n), TIMES, tol=-1.0)
    fake.calls.clear()
    out = sb.render_pick(_cam(0.25), _Pipe(), torch.zeros(3))
    _check_pick_frame(_calls(fake), "state_scatter ", True, int(n == 8200))
    assert sb.launches == 1 and sb._shown == P.locate(TIMES, 0.25)
    _check_outputs(out, n, log.pick[0][4])
    assert (log.pick[0][2] is None) == (sb.perm is None)
    sb.render(_cam(0.25), _Pipe(), torch.zeros(3))                   # the working state holds the frame's time: no state launch
    assert _calls(fake) == f"{_CAP}{' permute_rows' * int(n == 8200)}" and sb.launches == 1


@pytest.mark.parametrize("n", [300, 8200])
def test_composite_render_pick_places_first_and_hands_over_the_scene_row_map(fake, n):
    log = _recording(fake)
    models = _two_baked(n)
    scene = C.compose(models, [None, C.Placement(translation=(0.5, 0.0, -0.25), scale=0.5, time_offset=0.1)])
    fake.calls.clear()
    launches = scene.launches
    out = scene.render_pick(_cam(0.25), _Pipe(), torch.zeros(3), alpha_cut=0.75)
    _check_pick_frame(_calls(fake), "state_place state_place ", True, 2 * int(n == 8200))
    assert scene.launches == launches + 2
    (r, cut, rmap, dims, ptrs), = log.pick
    assert r == 7 and cut == 0.75 and dims == (2 * n, 64, 48)
    _check_outputs(out, 2 * n, ptrs)
    if n == 8200:
        want = torch.cat([models[0].perm.to(torch.int32), models[1].perm.to(torch.int32) + n])
        assert scene._pick_row_map.dtype == torch.int32 and torch.equal(scene._pick_row_map, want) and rmap == scene._pick_row_map.data_ptr()
    else:
        assert rmap is None and scene._pick_row_map is None
    scene.render(_cam(0.25), _Pipe(), torch.zeros(3))
    assert _calls(fake) == f"{_CAP}{' permute_rows' * 2 * int(n == 8200)}" and scene.launches == launches + 2


def test_render_pick_refuses_what_it_cannot_do(fake):
    baked = P.bake(_model(300), TIMES)
    sb = P.bake_sparse(_model(300), TIMES, tol=-1.0)
    scene = C.compose([baked])
    fake.calls.clear()
    for obj in (baked, sb, scene):
        for cut in (0.0, -1.0, 1.5, float("nan")):
            with pytest.raises(ValueError, match="alpha_cut"):
                obj.render_pick(_cam(0.5), _Pipe(), torch.zeros(3), alpha_cut=cut)
        for flag in ("convert_SHs_python", "compute_cov3D_python"):
            pipe = _Pipe()
            setattr(pipe, flag, True)
            with pytest.raises(NotImplementedError):
                obj.render_pick(_cam(0.5), pipe, torch.zeros(3))
    assert fake.calls == []                                         # refused before anything was launched
