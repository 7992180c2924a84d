"""Sparse baked playback on the device (fdgs.playback.bake_sparse, csrc/playback.hip).  Every comparison here is EXACT: the three kernels run
the functions their *_host twins run (csrc/playback_ops.h, compiled without contraction) or move bits, the deformation forward repeats bit
for bit, and a sparse frame is assembled from rows of the dense bake's frames.  The one inequality, |static row - dense frame| <= tol, is
the definition of a static row, taken in the float32 arithmetic fdgs_state_extent uses."""
import importlib
import functools
import math

import numpy as np
import pytest
import torch

from test_gpu_playback import CONFIGS, H, TIMES, W, _baked, _cam, _dev, _model, _same_frame, _timing_rows
from test_playback_host import WEIGHTS
from test_sparse_playback_host import ALL, CANARY, MASKS, WIDTH, bits, blend_states, random_state

pytestmark = pytest.mark.gpu
fdgs = importlib.import_module("4dgaussians_amd")
P, R, syn = fdgs.playback, fdgs.renderer, fdgs.synthetic
SPARE = 64                  # canary floats on either side of every array


# ---- the kernels against their twins ---------------------------------------------------------------------------------------------------

def layout(n):
    """Float offsets of the five [n, width] arrays in one flat buffer: SPARE floats before the first, after the last and between any two,
    every array on a 256-byte boundary."""
    offs, off = {}, SPARE
    for k, w in WIDTH.items():
        offs[k] = off
        off += (n * w + 63) // 64 * 64 + SPARE
    return offs, off


def host_buffer(n, state=None):
    """uint32 flat buffer of `layout(n)`: the canary everywhere, the bits of `state` in the arrays."""
    offs, total = layout(n)
    buf = np.full(total, CANARY, np.uint32)
    if state is not None:
        for k, w in WIDTH.items():
            buf[offs[k]:offs[k] + n * w] = bits(state[k]).reshape(-1)
    return buf


def to_device(buf):
    return torch.from_numpy(buf.view(np.int32)).to(_dev())


def state_ptrs(base, n, mask):
    offs, _ = layout(n)
    s = fdgs._lib.StateArrays()
    for h, k in enumerate(P.FIELDS):
        if mask >> h & 1:
            setattr(s, k, base + 4 * offs[k])
    return s


def same_bits(dev, host):
    return np.array_equal(dev.cpu().numpy().view(np.uint32), host)


def lists_of(D, N):
    """Strictly ascending lists of exactly D rows of N."""
    if N == D:
        return {"all": np.arange(D, dtype=np.int32)}
    g = np.random.default_rng(D)
    out = {"every_other": np.arange(0, 2 * D, 2, dtype=np.int32), "random": np.sort(g.choice(N, size=D, replace=False)).astype(np.int32)}
    if D == 1:
        out.update(first=np.array([0], np.int32), last=np.array([N - 1], np.int32))
    return out


@pytest.mark.parametrize("D", [1, 63, 64, 65, 4099])
def test_gather_and_scatter_equal_their_twins(D):
    L = fdgs._lib.lib()
    stream = fdgs._lib.stream_ptr()
    a, b, _, _, _ = blend_states(D, seed=11 + D)
    ha, hb = host_buffer(D, a), host_buffer(D, b)
    da, db = to_device(ha), to_device(hb)
    for N in (D, 2 * D + 3):
        hfull = host_buffer(N, random_state(N, 3 * N))
        dfull = to_device(hfull)
        clean_c, clean_o = host_buffer(D), host_buffer(N)
        for name, rows in lists_of(D, N).items():
            assert len(rows) == D and (np.diff(rows) > 0).all() and 0 <= rows[0] and rows[-1] < N
            drows = torch.from_numpy(rows).to(_dev())
            for mask in MASKS:
                hc, dc = clean_c.copy(), to_device(clean_c)
                assert L.fdgs_state_gather_host(D, rows.ctypes.data, N, mask, state_ptrs(hfull.ctypes.data, N, mask),
                                                state_ptrs(hc.ctypes.data, D, mask)) == 0
                fdgs._lib.check(L.fdgs_state_gather(stream, D, drows.data_ptr(), N, mask, state_ptrs(dfull.data_ptr(), N, mask),
                                                    state_ptrs(dc.data_ptr(), D, mask)))
                assert same_bits(dc, hc), (N, name, mask)                       # the listed rows, and the canary around them
                assert not np.array_equal(hc, clean_c)
                for w in (None, *WEIGHTS):
                    ho, do = clean_o.copy(), to_device(clean_o)
                    hb_, db_ = (None, None) if w is None else (state_ptrs(hb.ctypes.data, D, mask), state_ptrs(db.data_ptr(), D, mask))
                    assert L.fdgs_state_scatter_host(D, rows.ctypes.data, N, mask, state_ptrs(ha.ctypes.data, D, mask), hb_, w or 0.0,
                                                     state_ptrs(ho.ctypes.data, N, mask)) == 0
                    fdgs._lib.check(L.fdgs_state_scatter(stream, D, drows.data_ptr(), N, mask, state_ptrs(da.data_ptr(), D, mask), db_, w or 0.0,
                                                         state_ptrs(do.data_ptr(), N, mask)))
                    assert same_bits(do, ho), (N, name, mask, w)                # listed rows, unlisted rows and the canary, bit for bit
                    assert int((ho != CANARY).sum()) == D * sum(wd for h, wd in enumerate(P.FIELD_WIDTH) if mask >> h & 1)
    assert same_bits(da, ha) and same_bits(db, hb) and same_bits(dfull, hfull)  # the inputs are only read


@pytest.mark.parametrize("n", [1, 4099])
def test_extent_equals_its_twin_across_three_calls(n):
    L = fdgs._lib.lib()
    states = [random_state(n, 50 + n + k, payloads=(k == 3)) for k in range(4)]       # ref, then three `cur`; the last holds NaNs
    hs = [host_buffer(n, s) for s in states]
    ds = [to_device(h) for h in hs]
    for mask in MASKS:
        hext = np.full(SPARE + 5 * n + SPARE, CANARY, np.uint32)
        body = hext[SPARE:SPARE + 5 * n].reshape(n, 5)
        for h in range(5):
            if mask >> h & 1:
                body[:, h] = 0
        dext = to_device(hext)
        for k in (1, 2, 3):
            assert L.fdgs_state_extent_host(n, mask, state_ptrs(hs[0].ctypes.data, n, mask), state_ptrs(hs[k].ctypes.data, n, mask),
                                            hext.ctypes.data + 4 * SPARE) == 0
            fdgs._lib.check(L.fdgs_state_extent(fdgs._lib.stream_ptr(), n, mask, state_ptrs(ds[0].data_ptr(), n, mask),
                                                state_ptrs(ds[k].data_ptr(), n, mask), dext.data_ptr() + 4 * SPARE))
            assert same_bits(dext, hext), (mask, k)
        got = hext[SPARE:SPARE + 5 * n].reshape(n, 5)
        for h in range(5):
            assert (got[:, h] != CANARY).all() if mask >> h & 1 else (got[:, h] == CANARY).all()
        if n > 1 and mask == ALL:
            assert np.isposinf(got.view(np.float32)).any() and np.isfinite(got.view(np.float32)).any()


def test_nothing_to_do_launches_nothing():
    L = fdgs._lib.lib()
    stream = fdgs._lib.stream_ptr()
    rc = []
    rows = _timing_rows(lambda: rc.extend([L.fdgs_state_gather(stream, 0, None, 7, ALL, None, None),
                                           L.fdgs_state_scatter(stream, 0, None, 7, ALL, None, None, 0.0, None),
                                           L.fdgs_state_scatter(stream, 0, None, 0, ALL, None, None, 0.0, None),
                                           L.fdgs_state_gather(stream, 3, None, 7, 0, None, None),
                                           L.fdgs_state_extent(stream, 0, ALL, None, None, None),
                                           L.fdgs_state_extent(stream, 7, 0, None, None, None)]))
    assert rc == [0] * 6 and not any(k.startswith("state_") for k in rows), (rc, rows)


# ---- the guarantees of SparseBaked -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _extent(n, cfg):
    return P.motion_extent(_model(n, cfg), TIMES)


@functools.lru_cache(maxsize=None)
def _tolerances(n, cfg):
    """tol[h] = the ceil(0.9 n)-th smallest value of column h of the extents: at most 0.1 n rows exceed it, so over (at most) five heads
    at most n / 2 rows are dynamic."""
    ext, on = _extent(n, cfg), _baked(n, cfg).head_on
    k = math.ceil(0.9 * n)
    return tuple(float(torch.kthvalue(ext[:, h], k).values) if on[h] else 0.0 for h in range(5))


@functools.lru_cache(maxsize=None)
def _sparse(n, cfg, which):
    tol = {"quantile": _tolerances(n, cfg), "all": -1.0, "none": math.inf}[which] if isinstance(which, str) else which
    return P.bake_sparse(_model(n, cfg), TIMES, tol)


def _ibits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("n", [4099, 8200])
def test_sparse_frames_hold_what_the_guarantees_say(n, cfg):
    pc, baked, ext, tol = _model(n, cfg), _baked(n, cfg), _extent(n, cfg), _tolerances(n, cfg)
    assert (baked.perm is not None) == (n >= R.IMPLICIT_ORDER_MIN_N)
    on = baked.head_on
    # the extents, in the MODEL's order, are the extents of the dense frames: exactly
    assert ext.shape == (n, 5) and ext.dtype == torch.float32
    for h, name in enumerate(P.FIELDS):
        e = torch.zeros(n, device=_dev())
        if on[h]:
            f0 = getattr(baked.frames[0], name)
            for fr in baked.frames[1:]:
                e = torch.maximum(e, (getattr(fr, name) - f0).abs().reshape(n, -1).max(dim=1).values)
            if baked.perm is not None:
                model_order = torch.empty_like(e)
                model_order[baked.perm.long()] = e
                e = model_order
            assert float(e.max()) > 0
        assert torch.equal(ext[:, h], e), name
    sb = _sparse(n, cfg, "quantile")
    assert 0 < sb.D <= n / 2, (sb.D, n)
    assert sb.N == n and sb.times == tuple(TIMES) and sb.head_on == on and sb.tol == tol and sb.active_sh_degree == baked.active_sh_degree
    assert (sb.perm is None) == (baked.perm is None) and (sb.perm is None or torch.equal(sb.perm, baked.perm))
    assert sb.nbytes == P.sparse_bake_bytes(n, sb.D, len(TIMES), on) < baked.nbytes
    dyn_model = torch.zeros(n, dtype=torch.bool, device=_dev())
    for h in range(5):
        if on[h]:
            dyn_model |= ext[:, h] > tol[h]
    assert sb.dynamic.dtype == torch.bool and torch.equal(sb.dynamic, dyn_model)
    dyn = dyn_model if sb.perm is None else dyn_model[sb.perm.long()]              # in the stored row order
    assert sb.rows.dtype == torch.int32 and torch.equal(sb.rows.long(), torch.nonzero(dyn).reshape(-1)) and sb.D == int(dyn.sum())
    first = baked.frames[0]
    for k, t in enumerate(TIMES):
        st, where = sb.state_at(t)
        assert where == (k, k, 0.0)
        for h, name in enumerate(P.FIELDS):
            got, dense, f0 = getattr(st, name), getattr(baked.frames[k], name), getattr(first, name)
            assert torch.equal(_ibits(got)[dyn], _ibits(dense)[dyn]), (k, name)                    # 1. dynamic rows: the dense frame's bits
            assert torch.equal(_ibits(got)[~dyn], _ibits(f0)[~dyn]), (k, name)                     # 2. static rows: frame 0's bits
            if on[h]:
                assert bool(((got - dense).abs().reshape(n, -1).max(dim=1).values <= tol[h]).all()), (k, name)
            else:
                assert torch.equal(_ibits(got), _ibits(dense)), (k, name)
    for t in (0.3, 0.8):
        st, (i, j, w) = sb.state_at(t)
        assert i + 1 == j and 0.0 < w < 1.0
        dense = baked.blend(i, j, w)
        for h, name in enumerate(P.FIELDS):
            got = getattr(st, name)
            assert torch.equal(_ibits(got)[dyn], _ibits(getattr(dense, name))[dyn]), (t, name)     # 1. ... between timestamps: Baked.blend's
            assert torch.equal(_ibits(got)[~dyn], _ibits(getattr(first, name))[~dyn]), (t, name)
            if on[h]:
                assert not torch.equal(got[dyn], getattr(first, name)[dyn]), (t, name)


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("n", [4099, 8200])
def test_negative_and_infinite_tolerances(n, cfg):
    baked = _baked(n, cfg)
    pipe, bg = syn.PipelineParams(), torch.zeros(3, device=_dev())
    # 3. tol < 0: every row is dynamic, every frame is Baked.render's
    sb = _sparse(n, cfg, "all")
    assert sb.D == n and bool(sb.dynamic.all()) and sb.nbytes == P.sparse_bake_bytes(n, n, len(TIMES), baked.head_on)
    for k, t in enumerate((*TIMES, 0.3)):
        cam = _cam(k, t)
        _same_frame(sb.render(cam, pipe, bg), baked.render(cam, pipe, bg))
    a, b = sb.render(_cam(1, 0.0), pipe, bg), sb.render(_cam(1, 1.0), pipe, bg)
    assert not torch.equal(a["render"], b["render"])
    # 4. tol = inf: no row is dynamic, every frame is the frame at TIMES[0], nothing is launched
    sb = _sparse(n, cfg, "none")
    assert sb.D == 0 and not bool(sb.dynamic.any()) and sb.rows.numel() == 0
    assert sb.nbytes == P.sparse_bake_bytes(n, 0, len(TIMES), baked.head_on)
    for k, t in enumerate((*TIMES, 0.3)):
        _same_frame(sb.render(_cam(k, t), pipe, bg), baked.render(_cam(k, TIMES[0]), pipe, bg))
    assert sb.launches == 0
    with pytest.raises(MemoryError):
        P.bake_sparse(_model(n, cfg), TIMES, -1.0, max_bytes=P.sparse_bake_bytes(n, n, len(TIMES), baked.head_on) - 1)


def test_sparse_render_honours_the_arguments_of_render():
    """scaling_modifier, override_color, the PanopticSports dict camera and rgb8=, against Baked.render; through the permutation too."""
    for n in (4099, 8200):
        pc, baked, sb = _model(n, "dynerf_default"), _baked(n, "dynerf_default"), _sparse(n, "dynerf_default", "all")
        assert (sb.perm is not None) == (n >= R.IMPLICIT_ORDER_MIN_N)
        cam, bg = _cam(2, 0.5), torch.tensor([0.2, 0.4, 0.6], device=_dev())
        pipe = syn.PipelineParams()
        _same_frame(sb.render(cam, pipe, bg, scaling_modifier=0.7), baked.render(cam, pipe, bg, scaling_modifier=0.7))
        settings = fdgs.GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5), bg=bg, scale_modifier=1.0,
            viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=pc.active_sh_degree, campos=cam.camera_center,
            prefiltered=False, debug=False)
        dcam = {"camera": settings, "time": 0.3}
        _same_frame(sb.render(dcam, pipe, bg, cam_type="PanopticSports"), baked.render(dcam, pipe, bg, cam_type="PanopticSports"))
        colors = torch.rand(n, 3, generator=torch.Generator().manual_seed(4)).to(_dev())
        _same_frame(sb.render(cam, pipe, bg, override_color=colors), baked.render(cam, pipe, bg, override_color=colors))
        for mode in ("trunc", "round"):
            got, ref = sb.render(cam, pipe, bg, rgb8=mode), baked.render(cam, pipe, bg, rgb8=mode)
            _same_frame(got, ref)
            assert got["rgb8"].dtype == torch.uint8 and torch.equal(got["rgb8"], ref["rgb8"]) and set(got) == set(ref)
        assert "rgb8" not in sb.render(cam, pipe, bg) and sb.render(cam, pipe, bg)["viewspace_points"] is None
        _same_frame(sb.render(_cam(2, 0.3), pipe, bg, interp="nearest"), baked.render(_cam(2, 0.3), pipe, bg, interp="nearest"))
    pipe = syn.PipelineParams()
    pipe.convert_SHs_python = True
    with pytest.raises(NotImplementedError):
        sb.render(cam, pipe, bg)
    with pytest.raises(ValueError):
        sb.state_at(0.3, "cubic")


def test_a_sparse_frame_launches_one_scatter_and_nothing_else_for_the_state():
    n, cfg = 4099, "dynerf_default"
    baked = _baked(n, cfg)
    sb = P.bake_sparse(_model(n, cfg), TIMES, _tolerances(n, cfg))            # a fresh one: it holds the state at TIMES[0]
    assert 0 < sb.D <= n / 2 and sb.launches == 0
    pipe, bg = syn.PipelineParams(), torch.zeros(3, device=_dev())
    quiet = lambda rows: not any(k.startswith("deform") or k == "state_blend" for k in rows)
    rows = _timing_rows(lambda: sb.render(_cam(0, 0.0), pipe, bg))            # the time it holds: nothing to do
    assert "state_scatter" not in rows and quiet(rows) and sb.launches == 0, rows
    rows = _timing_rows(lambda: sb.render(_cam(0, 0.25), pipe, bg))           # a new baked time: one copy-scatter
    assert rows.get("state_scatter") == 1 and quiet(rows) and sb.launches == 1, rows
    rows = _timing_rows(lambda: sb.render(_cam(1, 0.25), pipe, bg))           # the same time again, another camera
    assert "state_scatter" not in rows and quiet(rows) and sb.launches == 1, rows
    rows = _timing_rows(lambda: sb.render(_cam(0, 0.8), pipe, bg))            # a time in between: one scatter with the blend fused
    assert rows.get("state_scatter") == 1 and quiet(rows) and sb.launches == 2, rows
    rows = _timing_rows(lambda: sb.render(_cam(0, 0.8), pipe, bg))
    assert "state_scatter" not in rows and quiet(rows), rows
    rows = _timing_rows(lambda: sb.render(_cam(0, 0.3), pipe, bg, interp="nearest"))
    assert rows.get("state_scatter") == 1 and quiet(rows) and sb.launches == 3, rows
    st, where = sb.state_at(0.3, "nearest")
    assert where == (1, 1, 0.0) and sb.launches == 3
    idx = sb.rows.long()
    for name in P.FIELDS:
        assert torch.equal(_ibits(getattr(st, name))[idx], _ibits(getattr(baked.frames[1], name))[idx]), name


def test_no_graph_is_recorded_and_compose_refuses_a_sparse_bake():
    pc = _model(4099, "dynerf_default")
    with torch.enable_grad():
        sb = P.bake_sparse(pc, TIMES[:2], 1e-3)
        ext = P.motion_extent(pc, TIMES[:2])
        out = sb.render(_cam(0, 0.1), syn.PipelineParams(), torch.zeros(3, device=_dev()))
    assert not ext.requires_grad and not any(a.requires_grad for a in sb.state_at(0.1)[0].arrays())
    assert all(not v.requires_grad and v.grad_fn is None for v in out.values() if isinstance(v, torch.Tensor))
    with pytest.raises(TypeError, match="Baked"):
        fdgs.compose.compose([sb])
