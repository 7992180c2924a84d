"""Scene composition on the device (fdgs.compose, csrc/compose.hip).  The place kernel runs the functions its host twin runs
(csrc/compose_ops.h, compiled without contraction) and the forward has no atomics on its image path, so every comparison with the host
twin, with Baked.render and with the rasterizer on host-placed arrays is EXACT.  The one tolerance is the equivariance test's, the bound
the project holds for HIP against the float64 oracle (tests/test_gpu_raster.py): PSNR > 80 dB, mean |dC| < 2e-6."""
import itertools
import math

import numpy as np
import pytest
import torch

from test_compose_host import ALL, D_GENERAL, KEYS, R_GENERAL, _psnr, general_placement, host_place, moved_camera
from test_gpu_playback import H, TIMES, W, _baked, _cam, _cpu_state, _dev, _model, _same_frame, _timing_rows
from test_playback_host import _state

import importlib

pytestmark = pytest.mark.gpu
fdgs = importlib.import_module("4dgaussians_amd")
C, P, syn = fdgs.compose, fdgs.playback, fdgs.synthetic
WIDTH = dict(zip(KEYS, P.FIELD_WIDTH))


def _settings(cam, bg, sh_degree):
    return fdgs.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5), bg=bg, scale_modifier=1.0,
        viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=sh_degree, campos=cam.camera_center,
        prefiltered=False, debug=False)


def device_place(pstruct, a, b, w, mask, n, row_off, shift):
    """fdgs_state_place into rows [row_off, row_off + n) of NaN-filled flat buffers that start `shift` floats past an aligned address.
    Returns per field the whole buffer (CPU) and the float range of the destination rows inside it."""
    L = fdgs._lib
    sa, sb, so = L.StateArrays(), L.StateArrays(), L.StateArrays()
    bufs, spans = {}, {}
    for h, (k, name) in enumerate(zip(KEYS, P.FIELDS)):
        wd = WIDTH[k]
        lo = shift + row_off * wd
        bufs[k] = torch.full((shift + (row_off + n + 3) * wd,), float("nan"), device=_dev())
        spans[k] = (lo, lo + n * wd)
        if mask >> h & 1:
            setattr(sa, name, a[k].data_ptr())
            setattr(so, name, bufs[k].data_ptr() + 4 * lo)
            if b is not None:
                setattr(sb, name, b[k].data_ptr())
    L.check(L.lib().fdgs_state_place(L.stream_ptr(), pstruct, n, mask, sa, sb if b is not None else None, w, so))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in bufs.items()}, spans


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4099])
def test_device_place_equals_host_place(n):
    """Around the 64-row tile; destinations at row offsets 0 and 4099 (3 * 4099 floats is not a multiple of 4: the small fields land on
    4-byte boundaries) and 1 or 3 floats past a 16-byte boundary (the SH stream's single-float head and tail)."""
    lib = fdgs._lib.lib()
    a, b = _state(n, seed=200 + n)
    da, db = ({k: v.to(_dev()) for k, v in s.items()} for s in (a, b))
    assert all(v.data_ptr() % 16 == 0 for s in (da, db) for v in s.values())
    near_one = float(np.nextafter(np.float32(1), np.float32(0)))
    blends = [(False, 0.0), (True, 0.0), (True, 0.25), (True, near_one)]
    dests = [(0, 0), (4099, 0), (4099, 1), (0, 3)]
    host = {}
    for mode, (blend, w), deg, mask, (row_off, shift) in itertools.product(("points", "rigid"), blends, (0, 3), (ALL, 0b10101, 0b01011), dests):
        ps = general_placement(mode).struct(deg)
        key = (mode, blend, w, deg)
        if key not in host:
            host[key] = host_place(lib, ps, a, b if blend else None, w)
        got, spans = device_place(ps, da, db if blend else None, w, mask, n, row_off, shift)
        for h, k in enumerate(KEYS):
            lo, hi = spans[k]
            if mask >> h & 1:
                assert torch.equal(got[k][lo:hi], host[key][k].reshape(-1)), (key, mask, row_off, shift, k)       # bit for bit
                assert bool(torch.isnan(got[k][:lo]).all()) and bool(torch.isnan(got[k][hi:]).all()), (key, mask, row_off, shift, k)
            else:
                assert bool(torch.isnan(got[k]).all()), (key, mask, row_off, shift, k)


@pytest.mark.parametrize("cfg", ["dynerf_default", "dnerf_bouncingballs"])
@pytest.mark.parametrize("n", [4099, 8200])
def test_identity_composite_of_one_model_is_baked_render(n, cfg):
    baked = _baked(n, cfg)
    scene = C.compose([baked])
    assert scene.N == n and scene.slices == (slice(0, n),) and scene.nbytes == C.compose_bytes([n]) and scene.active_sh_degree == baked.active_sh_degree
    assert all((x.data_ptr() - scene._storage.data_ptr()) % (4 * P.SLOT_ALIGN_FLOATS) == 0 for x in scene._frame.arrays())
    bg, pipe = torch.tensor([0.1, 0.2, 0.3], device=_dev()), syn.PipelineParams()
    seen = 0
    for k, t in enumerate((*TIMES, 0.375)):
        cam = _cam(k, t)
        want = baked.render(cam, pipe, bg)
        got = scene.render(cam, pipe, bg)
        _same_frame(got, want)
        assert got["viewspace_points"] is None and set(got) == set(want)
        seen += int((got["radii"] > 0).sum())
    assert seen > n // 2
    st = scene.state_at(0.375)
    ref, where = baked.state_at(0.375)
    assert where == (1, 2, 0.5)
    for x, y in zip(st.arrays(), ref.arrays()):
        assert torch.equal(x, y)
    colors = torch.rand(n, 3, generator=torch.Generator().manual_seed(4)).to(_dev())
    _same_frame(scene.render(_cam(2, 0.5), pipe, bg, override_color=colors, scaling_modifier=0.7, rgb8="trunc"),
                baked.render(_cam(2, 0.5), pipe, bg, override_color=colors, scaling_modifier=0.7))
    pipe.convert_SHs_python = True
    with pytest.raises(NotImplementedError):
        scene.render(_cam(0, 0.0), pipe, bg)


def _two_models():
    return [_baked(4099, "dynerf_default"), _baked(8200, "dnerf_bouncingballs")]


def _host_composite(models, placements, t):
    """The composite state at t from the host twin over host copies of the models' baked frames: dict of CPU tensors, rows concatenated."""
    lib = fdgs._lib.lib()
    parts = []
    for model, pl in zip(models, placements):
        i, j, w = P.locate(model.times, C.map_time(model.times, t, pl), "linear")
        a, b = _cpu_state(model.frames[i]), _cpu_state(model.frames[j])
        parts.append(host_place(lib, pl.struct(model.active_sh_degree), a, b if i != j else None, w if i != j else 0.0))
    return {k: torch.cat([p[k] for p in parts]) for k in KEYS}


def test_two_placed_models():
    models = _two_models()
    assert models[0].perm is None and models[1].perm is not None and models[1].head_on == (1, 1, 1, 0, 0)
    placements = [general_placement(), C.Placement(rotation=(0.6, 0.0, 0.8, 0.0), translation=(-0.7, 0.2, 0.1), scale=0.6)]
    scene = C.compose(models, placements)
    assert scene.N == 12299 and scene.offsets == (0, 4099) and scene.slices == (slice(0, 4099), slice(4099, 12299))
    assert scene.nbytes == C.compose_bytes([4099, 8200])
    with pytest.raises(MemoryError):
        C.compose(models, placements, max_bytes=scene.nbytes - 1)
    bg, pipe = torch.zeros(3, device=_dev()), syn.PipelineParams()
    for k, t in enumerate((0.25, 0.375, 0.9)):
        ref = _host_composite(models, placements, t)
        st = scene.state_at(t)
        for key, x in zip(KEYS, st.arrays()):
            assert tuple(x.shape) == tuple(ref[key].shape) and torch.equal(x.cpu(), ref[key]), (t, key)      # bit for bit
        cam = _cam(k, t)
        got = scene.render(cam, pipe, bg)
        d = {key: v.to(_dev()) for key, v in ref.items()}
        with torch.no_grad():
            image, radii, depth = fdgs.GaussianRasterizer(_settings(cam, bg, scene.active_sh_degree))(
                means3D=d["xyz"], means2D=torch.zeros_like(d["xyz"]), shs=d["shs"], opacities=d["opacity"], scales=d["scales"], rotations=d["rot"])
        assert torch.equal(got["render"], image) and torch.equal(got["depth"], depth)
        # radii: model 0 in its own (= the stored) order, model 1 scattered back from the permuted rows to its own order
        perm = models[1].perm.long()
        assert got["radii"].shape == (12299,) and torch.equal(got["radii"][scene.slices[0]], radii[:4099])
        assert torch.equal(got["radii"][scene.slices[1]][perm], radii[4099:])
        assert torch.equal(got["visibility_filter"], got["radii"] > 0)
        assert int((radii[:4099] > 0).sum()) > 0 and int((radii[4099:] > 0).sum()) > 0 and int((radii > 0).sum()) > 1000
    # override_color in the models' own order
    colors = torch.rand(12299, 3, generator=torch.Generator().manual_seed(9)).to(_dev())
    cam = _cam(1, 0.375)
    got = scene.render(cam, pipe, bg, override_color=colors)
    d = {key: v.to(_dev()) for key, v in _host_composite(models, placements, 0.375).items()}
    stored = torch.cat((colors[:4099], colors[4099:][perm]))
    with torch.no_grad():
        image, radii, depth = fdgs.GaussianRasterizer(_settings(cam, bg, scene.active_sh_degree))(
            means3D=d["xyz"], means2D=torch.zeros_like(d["xyz"]), colors_precomp=stored, opacities=d["opacity"], scales=d["scales"], rotations=d["rot"])
    assert torch.equal(got["render"], image) and torch.equal(got["radii"][scene.slices[1]][perm], radii[4099:])


def test_a_placed_model_is_the_model_seen_from_the_moved_camera():
    """Composite.render of a model placed by (R, d) against the float64 oracle's image of the UNPLACED baked state from the moved camera."""
    from oracle.raster_torch import rasterize
    baked = _baked(4099, "dynerf_default")
    cam = syn.make_camera(W, H, theta_deg=-73, time=TIMES[1]).to(_dev())
    bg, pipe = torch.zeros(3, device=_dev()), syn.PipelineParams()
    f = baked.frames[1]
    V, F, c = moved_camera(syn.make_camera(W, H, theta_deg=-73), R_GENERAL, D_GENERAL)
    dd = lambda x: x.double().to(_dev())
    want, _, want_radii = rasterize(means3D=dd(f.xyz), opacities=dd(f.opacity), viewmatrix=dd(V), projmatrix=dd(F), campos=dd(c), bg=dd(bg),
                                    image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
                                    sh_degree=baked.active_sh_degree, shs=dd(f.shs), scales=dd(f.scales), rotations=dd(f.rotations))
    assert int((want_radii > 0).sum()) > 500 and float(want.max()) > 0.3
    results = {}
    for mode in ("rigid", "points"):
        scene = C.compose([baked], [C.Placement(rotation=R_GENERAL, translation=D_GENERAL, mode=mode)])
        got = scene.render(cam, pipe, bg)["render"].double()
        diff = (got - want).abs()
        results[mode] = (_psnr(got, want), float(diff.mean()))
        print(f"[equivariance {mode}] psnr={results[mode][0]:.1f} dB mean|dC|={results[mode][1]:.3e} max|dC|={float(diff.max()):.3e}")
    assert results["rigid"][0] > 80.0 and results["rigid"][1] < 2e-6
    assert results["points"][0] < 40.0


def test_time_maps():
    models = _two_models()
    placements = [general_placement(time_offset=0.3, time_scale=1.5, wrap="loop"), general_placement("points", time_scale=-1.0, time_offset=0.1, wrap="pingpong")]
    scene = C.compose(models, placements)
    lib = fdgs._lib.lib()
    mapped = []
    for t in (0.1, 0.9, 0.5):
        st = scene.state_at(t)
        for m, (model, pl) in enumerate(zip(models, placements)):
            tm = C.map_time(model.times, t, pl)
            mapped.append(tm)
            own, _ = model.state_at(tm)                                                 # the model's own (blended) state at the mapped time
            ref = host_place(lib, pl.struct(model.active_sh_degree), _cpu_state(own))
            for key, x in zip(KEYS, st.arrays()):
                assert torch.equal(x[scene.slices[m]].cpu(), ref[key]), (t, m, key)
    assert mapped[:2] == [0.3 + 1.5 * 0.1, 0.0] and abs(mapped[2] - (1.5 * 0.9 + 0.3 - 1.0)) < 1e-12 and abs(mapped[3] - 0.8) < 1e-12       # looped / reflected


def test_launch_economy():
    models = _two_models()
    scene = C.compose(models, [general_placement(), general_placement()])
    assert scene.launches == 1                                   # compose(): the static opacity and SH of the dnerf model, once
    pipe, bg = syn.PipelineParams(), torch.zeros(3, device=_dev())
    rows = _timing_rows(lambda: scene.render(_cam(0, 0.3), pipe, bg))
    assert scene.launches == 3 and rows.get("state_place") == 2 and "state_blend" not in rows and not any(k.startswith("deform") for k in rows), rows
    first = scene.render(_cam(0, 0.3), pipe, bg)
    rows = _timing_rows(lambda: scene.render(_cam(1, 0.3), pipe, bg))                   # the same time again: nothing to place
    assert scene.launches == 3 and "state_place" not in rows, rows
    _same_frame(scene.render(_cam(0, 0.3), pipe, bg), first)
    # the static fields of the dnerf model are written by compose() alone: poison them, play on, they stay poisoned (and the rest does not)
    sl = scene.slices[1]
    keep = {name: getattr(scene._frame, name).clone() for name in P.FIELDS}
    scene._frame.opacity[sl] = float("nan")
    scene._frame.shs[sl] = float("nan")
    scene._frame.xyz[sl] = float("nan")
    before = scene.launches
    for n_new, t in enumerate((0.5, 0.6, 1.0), 1):
        st = scene.state_at(t)
        assert scene.launches <= before + 2 * n_new
        assert bool(torch.isnan(st.opacity[sl]).all()) and bool(torch.isnan(st.shs[sl]).all())
        assert not bool(torch.isnan(st.xyz).any())
        assert not bool(torch.isnan(st.opacity[scene.slices[0]]).any()) and not bool(torch.isnan(st.shs[scene.slices[0]]).any())
    assert scene.launches == before + 6
    scene._frame.opacity[sl] = keep["opacity"][sl]
    scene._frame.shs[sl] = keep["shs"][sl]
    # a model whose time stands still is placed once
    frozen = C.compose(models, [general_placement(time_scale=0.0, time_offset=0.4), None])
    base = frozen.launches
    for t in (0.1, 0.2, 0.7):
        frozen.state_at(t)
    assert frozen.launches == base + 1 + 3
