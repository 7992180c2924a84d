"""Composites of sparse bakes on the device (fdgs.compose with allow_sparse=True, fdgs_state_place_rows in csrc/compose.hip).  Every
comparison here is EXACT: the kernel runs the functions its host twin runs (csrc/compose_ops.h, compiled without contraction), a sparse
bake's compact rows are rows of the dense bake's frames, and the forward has no atomics on its image path."""
import itertools
import math

import numpy as np
import pytest
import torch

from test_compose_host import ALL, KEYS, general_placement, host_place
from test_gpu_compose import _settings
from test_gpu_playback import TIMES, _baked, _cam, _cpu_state, _dev, _model, _same_frame, _timing_rows
from test_gpu_sparse_playback import _ibits, _sparse, _tolerances, lists_of
from test_sparse_playback_host import CANARY, WIDTH, bits, blend_states

import importlib

pytestmark = pytest.mark.gpu
fdgs = importlib.import_module("4dgaussians_amd")
C, P, syn = fdgs.compose, fdgs.playback, fdgs.synthetic
NEAR_ONE = float(np.nextafter(np.float32(1), np.float32(0)))
MODES = ("points", "rigid")
DEGREES = (0, 3)
BLENDS = ((False, 0.0), (True, 0.0), (True, 0.25), (True, NEAR_ONE))
PLACE_MASKS = (ALL, 0b10101, 0b01011)
DESTS = ((0, 0), (4099, 0), (4099, 1), (0, 3))          # (rows before the model's row 0, floats past a 16-byte boundary)
# for the largest size: twelve cases in which every axis takes each of its values
REDUCED = [(MODES[i % 2], BLENDS[i % 4], DEGREES[(i // 2) % 2], PLACE_MASKS[i % 3], DESTS[(i + i // 4) % 4]) for i in range(12)]
CANARY_I32 = int(np.uint32(CANARY).view(np.int32))


# ---- 1. the kernel against its twin ------------------------------------------------------------------------------------------------------

def compact_ptrs(state, mask, ptr):
    """fdgs_state_arrays over a {field: array} of compact rows: the pointers of the fields `mask` selects."""
    s = fdgs._lib.StateArrays()
    for h, k in enumerate(P.FIELDS):
        if mask >> h & 1:
            setattr(s, k, ptr(state[k]))
    return s


def dest_ptrs(bufs, mask, row_off, shift, ptr):
    """... over flat buffers in which the model's row 0 starts `shift` floats past the (aligned) start plus `row_off` rows."""
    s = fdgs._lib.StateArrays()
    for h, k in enumerate(P.FIELDS):
        if mask >> h & 1:
            setattr(s, k, ptr(bufs[k]) + 4 * (shift + row_off * WIDTH[k]))
    return s


@pytest.mark.parametrize("D", [1, 63, 64, 65, 257, 4099])
def test_place_rows_equals_its_twin(D):
    """Around the 64-row SH tile and the 256 rows a workgroup takes without the SH stream; destinations on a 16-byte boundary (float4
    stores) and 1 or 3 floats past one (single-float stores), behind 0 or 4099 other rows.  The whole destination buffers are compared:
    the listed rows, the unlisted rows, the unselected fields and the floats around the model's rows."""
    L = fdgs._lib
    lib, stream = L.lib(), L.stream_ptr()
    a, b, _, _, _ = blend_states(D, seed=500 + D)
    da, db = ({k: torch.from_numpy(v).to(_dev()) for k, v in s.items()} for s in (a, b))
    assert all(v.data_ptr() % 16 == 0 for s in (da, db) for v in s.values())
    cases = list(itertools.product(MODES, BLENDS, DEGREES, PLACE_MASKS, DESTS)) if D <= 257 else REDUCED
    for axis, values in enumerate((MODES, BLENDS, DEGREES, PLACE_MASKS, DESTS)):
        assert {c[axis] for c in cases} == set(values)
    np_ptr, dev_ptr = (lambda x: x.ctypes.data), (lambda x: x.data_ptr())
    for N in (D, 2 * D + 3):
        for name, rows in lists_of(D, N).items():
            assert len(rows) == D and (np.diff(rows) > 0).all() and 0 <= rows[0] and rows[-1] < N
            drows = torch.from_numpy(rows).to(_dev())
            for mode, (blend, w), deg, mask, (row_off, shift) in cases:
                ps = general_placement(mode).struct(deg)
                floats = {k: shift + (row_off + N + 3) * wd for k, wd in WIDTH.items()}
                hbuf = {k: np.full(n, CANARY, np.uint32) for k, n in floats.items()}
                dbuf = {k: torch.full((n,), CANARY_I32, dtype=torch.int32, device=_dev()) for k, n in floats.items()}
                assert dbuf["shs"].data_ptr() % 16 == 0
                rc = lib.fdgs_state_place_rows_host(ps, D, rows.ctypes.data, N, mask, compact_ptrs(a, mask, np_ptr),
                                                    compact_ptrs(b, mask, np_ptr) if blend else None, w, dest_ptrs(hbuf, mask, row_off, shift, np_ptr))
                assert rc == 0, lib.fdgs_last_error()
                L.check(lib.fdgs_state_place_rows(stream, ps, D, drows.data_ptr(), N, mask, compact_ptrs(da, mask, dev_ptr),
                                                  compact_ptrs(db, mask, dev_ptr) if blend else None, w, dest_ptrs(dbuf, mask, row_off, shift, dev_ptr)))
                case = (N, name, mode, blend, w, deg, mask, row_off, shift)
                for h, k in enumerate(P.FIELDS):
                    assert np.array_equal(dbuf[k].cpu().numpy().view(np.uint32), hbuf[k]), (case, k)              # bit for bit, canary included
                    written = int((hbuf[k] != CANARY).sum())
                    assert written == (D * WIDTH[k] if mask >> h & 1 else 0), (case, k)
                    lo = shift + row_off * WIDTH[k]
                    assert (hbuf[k][:lo] == CANARY).all() and (hbuf[k][lo + N * WIDTH[k]:] == CANARY).all(), (case, k)
            assert np.array_equal(drows.cpu().numpy(), rows)
    for k in P.FIELDS:                                                                                          # the inputs are only read
        assert np.array_equal(bits(da[k].cpu().numpy()), bits(a[k])) and np.array_equal(bits(db[k].cpu().numpy()), bits(b[k])), k


# ---- 2. nothing to do ----------------------------------------------------------------------------------------------------------------------

def test_nothing_to_do_launches_nothing():
    lib, stream = fdgs._lib.lib(), fdgs._lib.stream_ptr()
    ps = general_placement().struct(3)
    rc = []
    rows = _timing_rows(lambda: rc.extend([lib.fdgs_state_place_rows(stream, ps, 0, None, 7, ALL, None, None, 0.0, None),
                                           lib.fdgs_state_place_rows(stream, ps, 0, None, 0, ALL, None, None, 0.0, None),
                                           lib.fdgs_state_place_rows(stream, ps, 3, None, 7, 0, None, None, 0.0, None)]))
    assert rc == [0, 0, 0] and "state_place_rows" not in rows, (rc, rows)


# ---- 3. tol < 0: the dense composite, bit for bit --------------------------------------------------------------------------------------------

SCENE = ((4099, "dynerf_default"), (8200, "dnerf_bouncingballs"))
BETWEEN = (0.3, 0.375, 0.8)


def _placements():
    return [general_placement(), general_placement(time_scale=1.5, time_offset=0.3, wrap="loop")]


def _same_state(a, b):
    for name, x, y in zip(P.FIELDS, a.arrays(), b.arrays()):
        assert x.shape == y.shape and torch.equal(_ibits(x), _ibits(y)), name


@pytest.mark.parametrize("mixed", [False, True])
def test_a_composite_of_all_dynamic_sparse_bakes_is_the_dense_composite(mixed):
    dense = [_baked(n, cfg) for n, cfg in SCENE]
    sparse = [_sparse(n, cfg, "all") for n, cfg in SCENE]
    assert dense[0].perm is None and dense[1].perm is not None and dense[1].head_on == (1, 1, 1, 0, 0) and all(s.D == s.N for s in sparse)
    ref = C.compose(dense, _placements())
    scene = C.compose([dense[0], sparse[1]] if mixed else sparse, _placements(), allow_sparse=True)
    assert scene.N == ref.N and scene.offsets == ref.offsets and scene.nbytes == ref.nbytes == C.compose_bytes([n for n, _ in SCENE])
    assert scene.active_sh_degree == ref.active_sh_degree
    pipe, bg = syn.PipelineParams(), torch.tensor([0.1, 0.2, 0.3], device=_dev())
    colors = torch.rand(scene.N, 3, generator=torch.Generator().manual_seed(9)).to(_dev())
    seen = 0
    for k, t in enumerate((*TIMES, *BETWEEN)):
        _same_state(scene.state_at(t), ref.state_at(t))
        cam = _cam(k, t)
        got, want = scene.render(cam, pipe, bg), ref.render(cam, pipe, bg)
        _same_frame(got, want)
        assert set(got) == set(want) and got["viewspace_points"] is None
        seen += int((got["radii"] > 0).sum())
        _same_frame(scene.render(cam, pipe, bg, override_color=colors), ref.render(cam, pipe, bg, override_color=colors))
    assert seen > scene.N // 2
    for mode in ("trunc", "round"):
        got, want = scene.render(_cam(2, 0.8), pipe, bg, rgb8=mode), ref.render(_cam(2, 0.8), pipe, bg, rgb8=mode)
        _same_frame(got, want)
        assert got["rgb8"].dtype == torch.uint8 and torch.equal(got["rgb8"], want["rgb8"])
    a, b = scene.render(_cam(1, 0.0), pipe, bg), scene.render(_cam(1, 1.0), pipe, bg)
    assert not torch.equal(a["render"], b["render"])


# ---- 4. quantile tolerances: every model's slice is its own sparse state, placed ------------------------------------------------------------

def test_a_composite_of_sparse_bakes_holds_each_models_sparse_state_placed():
    lib = fdgs._lib.lib()
    models = [_sparse(n, cfg, "quantile") for n, cfg in SCENE]
    for sb in models:
        assert 0 < sb.D <= sb.N / 2, (sb.D, sb.N)                   # the bound of _tolerances
    placements = _placements()
    scene = C.compose(models, placements, allow_sparse=True)
    assert scene.N == 12299 and scene.slices == (slice(0, 4099), slice(4099, 12299))
    pipe, bg = syn.PipelineParams(), torch.zeros(3, device=_dev())
    perm = models[1].perm.long()
    for k, t in enumerate((0.25, 0.375, 0.9, 0.0)):
        st = scene.state_at(t)
        parts = []
        for m, (sb, pl) in enumerate(zip(models, placements)):
            own, _ = sb.state_at(C.map_time(sb.times, t, pl))                         # the model's own (blended) sparse state
            parts.append(host_place(lib, pl.struct(sb.active_sh_degree), _cpu_state(own)))
            for key, x in zip(KEYS, st.arrays()):
                assert torch.equal(_ibits(x[scene.slices[m]].cpu()), _ibits(parts[m][key])), (t, m, key)       # bit for bit
        d = {key: torch.cat([p[key] for p in parts]).to(_dev()) for key in KEYS}
        cam = _cam(k, t)
        got = scene.render(cam, pipe, bg)
        with torch.no_grad():
            image, radii, depth = fdgs.GaussianRasterizer(_settings(cam, bg, scene.active_sh_degree))(
                means3D=d["xyz"], means2D=torch.zeros_like(d["xyz"]), shs=d["shs"], opacities=d["opacity"], scales=d["scales"], rotations=d["rot"])
        assert torch.equal(got["render"], image) and torch.equal(got["depth"], depth)
        assert torch.equal(got["radii"][scene.slices[0]], radii[:4099]) and torch.equal(got["radii"][scene.slices[1]][perm], radii[4099:])
        assert int((radii[:4099] > 0).sum()) > 0 and int((radii[4099:] > 0).sum()) > 0


# ---- 5. launch economy and independence -------------------------------------------------------------------------------------------------------

def test_launch_economy_and_the_models_stay_as_they_are():
    models = [P.bake_sparse(_model(n, cfg), TIMES, _tolerances(n, cfg)) for n, cfg in SCENE]
    models.append(P.bake_sparse(_model(4099, "dynerf_default"), TIMES, math.inf))
    assert all(0 < sb.D <= sb.N / 2 for sb in models[:2]) and models[2].D == 0 and all(sb.launches == 0 for sb in models)
    before = [[_ibits(x).clone() for x in sb._frame.arrays()] for sb in models]
    made = []
    rows = _timing_rows(lambda: made.append(C.compose(models, [general_placement(), None, general_placement("points")], allow_sparse=True)))
    scene = made[0]
    # compose(): one launch per sparse model, all fields of all its rows
    assert rows.get("state_place") == 3 and "state_place_rows" not in rows and scene.launches == 3, rows
    pipe, bg = syn.PipelineParams(), torch.zeros(3, device=_dev())
    quiet = lambda r: not any(k.startswith("deform") or k in ("state_blend", "state_scatter", "state_place") for k in r)
    rows = _timing_rows(lambda: scene.render(_cam(0, 0.25), pipe, bg))              # a baked time: one launch per model with dynamic rows
    assert rows.get("state_place_rows") == 2 and quiet(rows) and scene.launches == 5, rows
    first = scene.render(_cam(0, 0.25), pipe, bg)
    rows = _timing_rows(lambda: scene.render(_cam(1, 0.25), pipe, bg))              # the same time again, another camera
    assert "state_place_rows" not in rows and quiet(rows) and scene.launches == 5, rows
    rows = _timing_rows(lambda: scene.render(_cam(0, 0.8), pipe, bg))               # a time in between: the blend is fused
    assert rows.get("state_place_rows") == 2 and quiet(rows) and scene.launches == 7, rows
    scene.state_at(0.25)
    assert scene.launches == 9
    _same_frame(scene.render(_cam(0, 0.25), pipe, bg), first)
    # static rows are written by compose() alone: poison a model's rows, play on; only the dynamic rows of the fields whose head is on return
    for m, t in ((0, 0.5), (1, 1.0)):
        sb, sl = models[m], scene.slices[m]
        for x in scene._frame.arrays():
            x[sl] = float("nan")
        st = scene.state_at(t)
        dyn = torch.zeros(sb.N, dtype=torch.bool, device=_dev())
        dyn[sb.rows.long()] = True
        for h, x in enumerate(st.arrays()):
            nan_rows = torch.isnan(x[sl]).reshape(sb.N, -1)
            assert bool(nan_rows[~dyn].all()), (m, h)
            assert bool(nan_rows[dyn].all()) if not sb.head_on[h] else not bool(nan_rows[dyn].any()), (m, h)
    assert scene.launches == 13
    sl = scene.slices[2]                                                            # the model without dynamic rows never launches again
    scene._frame.xyz[sl] = float("nan")
    for t in (0.0, 0.3, 1.0):
        scene.state_at(t)
    assert bool(torch.isnan(scene._frame.xyz[sl]).all()) and scene.launches == 13 + 2 * 3
    # the composite only read its models
    for sb, kept in zip(models, before):
        assert sb.launches == 0
        for name, x, y in zip(P.FIELDS, sb._frame.arrays(), kept):
            assert torch.equal(_ibits(x), y), name
