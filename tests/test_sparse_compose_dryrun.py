"""Dry run of a composite over one dense and one sparse bake (CPU, no kernels) against the fake library of tests/test_host_dryrun.py:
the ordered fdgs_* calls of compose(..., allow_sparse=True) and of three frames, and the sizes, masks and blend arguments the two place
entry points are handed."""
import importlib

import pytest
import torch

from test_host_dryrun import _CAP, _EXACT, TIMES, _cam, _model, _Pipe, fake  # noqa: F401  (`fake` is the fixture)

fdgs = importlib.import_module("4dgaussians_amd")
P, C = fdgs.playback, fdgs.compose
ALL = 31


def _calls(fake):
    out = " ".join(c[len("fdgs_"):] for c in fake.calls)
    fake.calls.clear()
    return out


def test_compose_and_three_frames_over_one_dense_and_one_sparse_model(fake):
    n = 300
    dense = P.bake(_model(n, "dnerf_bouncingballs", seed=2), TIMES)           # three heads on: opacity and SH are placed by compose()
    sparse = P.bake_sparse(_model(n, seed=1), TIMES, tol=-1.0)                # dynerf_default, five heads on, every row dynamic
    assert dense.head_on == (1, 1, 1, 0, 0) and sparse.head_on == (1, 1, 1, 1, 1) and sparse.D == n
    placed = []

    def note(name, a):
        if name == "fdgs_state_place":
            placed.append(("place", a[2], a[3], a[5] is None, a[6]))                      # N, mask, no blend, w
        elif name == "fdgs_state_place_rows":
            placed.append(("rows", a[2], a[4], a[5], a[7] is None, a[8]))                 # D, N, mask, no blend, w
    fake.record, fake._note = True, note
    fake.calls.clear()
    scene = C.compose([dense, sparse], [None, C.Placement(translation=(0.5, 0.0, -0.25), scale=0.5)], allow_sparse=True)
    # the dense model's static fields, then ALL fields of the sparse model's working state, every row
    assert _calls(fake) == "state_place state_place" and placed == [("place", n, 0b11000, True, 0.0), ("place", n, ALL, True, 0.0)]
    assert scene.N == 2 * n and scene.launches == 2 and scene.nbytes == C.compose_bytes([n, n])
    del placed[:]
    out = scene.render(_cam(0.5), _Pipe(), torch.zeros(3))                                # a baked timestamp: copies
    assert out["radii"].shape == (2 * n,) and out["viewspace_points"] is None
    assert _calls(fake) == f"state_place state_place_rows {_EXACT}"
    assert placed == [("place", n, 0b00111, True, 0.0), ("rows", n, n, ALL, True, 0.0)] and scene.launches == 4
    del placed[:]
    scene.render(_cam(0.25), _Pipe(), torch.zeros(3))                                     # between two timestamps: the blend, fused
    assert _calls(fake) == f"state_place state_place_rows {_CAP}"
    assert placed == [("place", n, 0b00111, False, 0.5), ("rows", n, n, ALL, False, 0.5)] and scene.launches == 6
    del placed[:]
    scene.render(_cam(0.25, theta=40.0), _Pipe(), torch.zeros(3))                         # the same time again: the rasterizer alone
    # (the third forward at one size asks for no buffer size again, as the third view of render_views does not)
    assert _calls(fake) == "raster_fwd_capacity pair_count_wait" and placed == [] and scene.launches == 6
    assert sparse.launches == 0                                                           # the composite never drives the model itself


def test_a_sparse_model_without_dynamic_rows_is_placed_once(fake):
    n = 300
    sparse = P.bake_sparse(_model(n, seed=1), TIMES, tol=float("inf"))
    assert sparse.D == 0
    fake.calls.clear()
    scene = C.compose([sparse], allow_sparse=True)
    assert _calls(fake) == "state_place" and scene.launches == 1
    for t in (0.5, 0.25):
        scene.state_at(t)
    assert _calls(fake) == "" and scene.launches == 1
    with pytest.raises(TypeError, match="Baked"):
        C.compose([sparse])
