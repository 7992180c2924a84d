"""Host plumbing of render_motion, dry (CPU, no kernels): Baked / SparseBaked / Composite.render_motion against the fake library of
tests/test_host_dryrun.py.  What is pinned: a motion frame is ONE rasterizer front half -- no second projection, sort or capacity frame --
followed by geom_field, motion_rows, one more render_fwd over the same buffers and motion_resolve; the state launches of its two state_at
calls come first; and the objects' bookkeeping of what their state holds stays truthful."""
import importlib
import types

import pytest
import torch

from test_host_dryrun import TIMES, _CAP, _EXACT, _Pipe, _cam, _model, _two_baked, fake  # noqa: F401  (`fake` is the fixture)

fdgs = importlib.import_module("4dgaussians_amd")
P, C = fdgs.playback, fdgs.compose
_TAIL = "geom_field motion_rows render_fwd motion_resolve"
_CAP_AGAIN = "raster_fwd_capacity pair_count_wait"             # (the size of a binning buffer of that capacity is cached by then)
_FRONT_HALF_ONLY = ("preprocess_fwd", "bin_prepare", "bin_sort", "raster_fwd_capacity")


def _recording(fake):
    """The fake keeps, per call: the frame's bg pointer (front half), (num_rendered, acc_zero, bg) of every render_fwd, and
    (N, stride, W, H) of every motion_rows."""
    log = types.SimpleNamespace(frame_bg=[], render_fwd=[], motion_rows=[], capacity=[])

    def note(self, name, a):
        if name in ("fdgs_preprocess_fwd", "fdgs_raster_fwd_capacity"):
            log.frame_bg.append(a[1].bg)
            if name == "fdgs_raster_fwd_capacity":
                log.capacity.append(int(a[5]))
        elif name == "fdgs_render_fwd":
            log.render_fwd.append((int(a[5]), a[1].acc_zero, a[1].bg, a[1].P, a[1].W, a[1].H))
        elif name == "fdgs_motion_rows":
            log.motion_rows.append((a[1], a[11], a[8], a[9]))
    fake._note = types.MethodType(note, fake)
    fake.record = True
    return log


def _calls(fake):
    out = " ".join(c[len("fdgs_"):] for c in fake.calls)
    fake.calls.clear()
    return out


def _check_motion_frame(calls, state_calls, exact, permuted, n_perm=1):
    perm = " permute_rows" * n_perm if permuted else ""
    assert calls == f"{state_calls}{_EXACT if exact else _CAP}{perm} {_TAIL}", calls
    for name in _FRONT_HALF_ONLY:                                # exactly one front half
        assert calls.split().count(name) == (1 if name in (_EXACT if exact else _CAP).split() else 0), name


@pytest.mark.parametrize("n", [300, 8200])
def test_baked_render_motion_is_one_front_half_and_one_more_blend(fake, n):
    log = _recording(fake)
    baked = P.bake(_model(n), TIMES)
    assert (baked.perm is not None) == (n == 8200)
    fake.calls.clear()
    nbytes = baked.nbytes
    out = baked.render_motion(_cam(0.5), _Pipe(), torch.zeros(3), toward_time=0.25, rgb8=None)
    _check_motion_frame(_calls(fake), "state_blend ", True, n == 8200)
    assert set(out) == {"render", "viewspace_points", "visibility_filter", "radii", "depth", "motion_raw", "motion", "alpha"}
    assert out["motion_raw"].shape == (3, 48, 64) and out["motion"].shape == (2, 48, 64) and out["alpha"].shape == (1, 48, 64)
    assert out["radii"].shape == (n,) and out["viewspace_points"] is None and baked.nbytes == nbytes
    # exact path: the frame's blend and the extra one are laid out for the true pair count, 7
    (r0, acc0, bg0, *_), (r1, acc1, bg1, p1, w1, h1) = log.render_fwd
    assert r0 == r1 == fake.pair_count == 7 and acc0 is None and acc1 is None
    assert bg0 == log.frame_bg[0] and bg1 is not None and bg1 != bg0 and (p1, w1, h1) == (n, 64, 48)
    assert log.motion_rows == [(n, 4, 64, 48)]
    # the next frame of this size is speculative: one capacity frame, and the extra blend gets THAT capacity
    out = baked.render_motion(_cam(0.5, theta=20.0), _Pipe(), torch.zeros(3), toward=_cam(0.75, theta=25.0), rgb8="trunc")
    calls = _calls(fake)
    perm = " permute_rows" if n == 8200 else ""
    assert calls == f"state_blend {_CAP}{perm} image_rgb8 {_TAIL}", calls
    assert calls.split().count("render_fwd") == 1 and "preprocess_fwd" not in calls and "bin_sort" not in calls
    assert len(log.render_fwd) == 3 and log.render_fwd[2][0] == log.capacity[0] == 8192 and log.render_fwd[2][1] is None
    assert log.render_fwd[2][2] == bg1 != log.frame_bg[1]            # the object's own three zeros, again
    assert log.motion_rows[1] == (n, 4, 64, 48) and "rgb8" in out
    # a frame toward a baked timestamp, at a baked timestamp: no blend at all
    baked.render_motion(_cam(0.5), _Pipe(), torch.zeros(3), toward_time=1.0)
    assert _calls(fake) == f"{_CAP_AGAIN}{perm} {_TAIL}"


@pytest.mark.parametrize("n", [300, 8200])
def test_sparse_render_motion_scatters_first_and_leaves_the_state_truthful(fake, n):
    _recording(fake)
    sb = P.bake_sparse(_model(n), TIMES, tol=-1.0)
    fake.calls.clear()
    sb.render_motion(_cam(0.5), _Pipe(), torch.zeros(3), toward_time=0.25)
    _check_motion_frame(_calls(fake), "state_scatter state_scatter ", True, n == 8200)
    assert sb.launches == 2 and sb._shown == P.locate(TIMES, 0.5)
    perm = " permute_rows" if n == 8200 else ""
    sb.render(_cam(0.5), _Pipe(), torch.zeros(3))                    # the working state holds the frame's time: no state launch
    assert _calls(fake) == f"{_CAP}{perm}" and sb.launches == 2
    sb.render_motion(_cam(0.5), _Pipe(), torch.zeros(3), toward=_cam(0.5, theta=30.0))       # the same time on both sides: none either
    assert _calls(fake) == f"{_CAP_AGAIN}{perm} {_TAIL}" and sb.launches == 2


@pytest.mark.parametrize("n", [300, 8200])
def test_composite_render_motion_places_first_and_leaves_the_state_truthful(fake, n):
    log = _recording(fake)
    scene = C.compose(_two_baked(n), [None, C.Placement(translation=(0.5, 0.0, -0.25), scale=0.5, time_offset=0.1)])
    fake.calls.clear()
    launches = scene.launches
    out = scene.render_motion(_cam(0.5), _Pipe(), torch.zeros(3), toward_time=0.25)
    _check_motion_frame(_calls(fake), "state_place state_place state_place state_place ", True, n == 8200, n_perm=2)
    assert scene.launches == launches + 4 and out["radii"].shape == (2 * n,) and log.motion_rows == [(2 * n, 4, 64, 48)]
    perm = " permute_rows" * 2 if n == 8200 else ""
    scene.render(_cam(0.5), _Pipe(), torch.zeros(3))
    assert _calls(fake) == f"{_CAP}{perm}" and scene.launches == launches + 4


def test_render_motion_refuses_what_it_cannot_do(fake):
    baked = P.bake(_model(300), TIMES)
    sb = P.bake_sparse(_model(300), TIMES, tol=-1.0)
    scene = C.compose([baked])
    fake.calls.clear()
    for obj in (baked, sb, scene):
        with pytest.raises(ValueError, match="toward"):
            obj.render_motion(_cam(0.5), _Pipe(), torch.zeros(3))
        with pytest.raises(ValueError, match="image size"):
            obj.render_motion(_cam(0.5), _Pipe(), torch.zeros(3), toward=fdgs.synthetic.make_camera(48, 64, theta_deg=10.0, time=0.25))
        pipe = _Pipe()
        pipe.convert_SHs_python = True
        with pytest.raises(NotImplementedError):
            obj.render_motion(_cam(0.5), pipe, torch.zeros(3), toward_time=0.25)
    assert fake.calls == []                                         # refused before anything was launched
