"""Baked playback on the device (fdgs.playback, csrc/playback.hip).  Every comparison here is EXACT: a baked frame is the state the live
no-grad frame rasterizes, the forward has no atomics on its image path, and the three playback kernels run the functions their *_host twins
run (csrc/playback_ops.h), compiled without contraction."""
import ctypes
import functools
import importlib
import math

import numpy as np
import pytest
import torch

from test_playback_host import boundary_image, host_blend, host_rgb8

pytestmark = pytest.mark.gpu
fdgs = importlib.import_module("4dgaussians_amd")
P, R, syn = fdgs.playback, fdgs.renderer, fdgs.synthetic
W, H = 96, 64
TIMES = [0.0, 0.25, 0.5, 1.0]
CONFIGS = ["dynerf_default", "dnerf_bouncingballs"]


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _model(n, cfg):
    pc = syn.SynthModel(n, cfg, seed=100 + n).to(_dev())
    with torch.no_grad():
        pc._scaling.add_(0.5)
    return pc


@functools.lru_cache(maxsize=None)
def _baked(n, cfg):
    return P.bake(_model(n, cfg), TIMES)


def _cam(k, t):
    return syn.make_camera(W, H, theta_deg=-140.0 + 67.0 * k, time=t).to(_dev())


def _live(cam, pc, **kw):
    with torch.no_grad():
        return fdgs.render(cam, pc, syn.PipelineParams(), torch.zeros(3, device=_dev()), stage="fine", **kw)


def _same_frame(a, b):
    assert torch.equal(a["render"], b["render"]) and torch.equal(a["depth"], b["depth"])
    assert a["radii"].dtype == b["radii"].dtype and torch.equal(a["radii"], b["radii"])
    assert torch.equal(a["visibility_filter"], b["visibility_filter"])


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("n", [4099, 8200])
def test_baked_frames_are_the_live_frames(n, cfg):
    pc = _model(n, cfg)
    if n >= R.IMPLICIT_ORDER_MIN_N:
        dn = pc._deformation.deformation_net
        perm = R._implicit_perm(pc, {"ordered": fdgs.deformation.spatial_order_hint(pc._xyz)}, dn)
        if perm is None:
            pytest.skip("renderer._implicit_perm returned no permutation for this model (FDGS_IMPLICIT_ORDER=0?)")
    baked = _baked(n, cfg)
    assert (baked.perm is not None) == (n >= R.IMPLICIT_ORDER_MIN_N) and baked.N == n and baked.times == tuple(TIMES)
    bg = torch.zeros(3, device=_dev())
    seen = 0
    for k, t in enumerate(TIMES):
        cam = _cam(k, t)
        live = _live(cam, pc)
        _same_frame(live, _live(cam, pc))                        # the premise: the live frame repeats bit for bit
        got = baked.render(cam, syn.PipelineParams(), bg)
        _same_frame(got, live)                                   # radii / visibility in the MODEL's order, permutation or not
        assert got["viewspace_points"] is None and set(got) == set(live)
        seen += int((got["radii"] > 0).sum())
    assert seen > n // 2                                         # (frames with something in them)
    # the same camera at two baked times gives two different frames: the time is honoured
    a, b = baked.render(_cam(1, 0.0), syn.PipelineParams(), bg), baked.render(_cam(1, 1.0), syn.PipelineParams(), bg)
    assert not torch.equal(a["render"], b["render"])


def test_baked_render_honours_the_arguments_of_render():
    """scaling_modifier, override_color and the PanopticSports dict camera, against the live frame; through the permutation too."""
    for n in (4099, 8200):
        pc, baked = _model(n, "dynerf_default"), _baked(n, "dynerf_default")
        cam, bg = _cam(2, 0.5), torch.tensor([0.2, 0.4, 0.6], device=_dev())
        pipe = syn.PipelineParams()
        with torch.no_grad():
            live = fdgs.render(cam, pc, pipe, bg, scaling_modifier=0.7, stage="fine")
        _same_frame(baked.render(cam, pipe, bg, scaling_modifier=0.7), live)
        settings = fdgs.GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5), bg=bg, scale_modifier=1.0,
            viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=pc.active_sh_degree, campos=cam.camera_center,
            prefiltered=False, debug=False)
        dcam = {"camera": settings, "time": 0.5}
        with torch.no_grad():
            live = fdgs.render(dcam, pc, pipe, bg, stage="fine", cam_type="PanopticSports")
        _same_frame(baked.render(dcam, pipe, bg, cam_type="PanopticSports"), live)
        colors = torch.rand(n, 3, generator=torch.Generator().manual_seed(4)).to(_dev())
        got = baked.render(cam, pipe, bg, override_color=colors)
        if baked.perm is None:
            with torch.no_grad():
                live = fdgs.render(cam, pc, pipe, bg, override_color=colors, stage="fine")
            _same_frame(got, live)
        else:
            # (render() does not read the model through the permutation on its override_color path, and the order of two splats of equal
            # depth follows the row order: the exact counterpart is the rasterizer on the stored rows with the colours in the stored order)
            f, perm = baked.frames[2], baked.perm.long()
            with torch.no_grad():
                image, radii, depth = fdgs.GaussianRasterizer(settings)(means3D=f.xyz, means2D=torch.zeros_like(f.xyz), colors_precomp=colors[perm],
                                                                        opacities=f.opacity, scales=f.scales, rotations=f.rotations)
            assert torch.equal(got["render"], image) and torch.equal(got["depth"], depth) and torch.equal(got["radii"][perm], radii)
            assert torch.equal(got["visibility_filter"], got["radii"] > 0) and int((radii > 0).sum()) > n // 4
    pipe = syn.PipelineParams()
    pipe.convert_SHs_python = True
    with pytest.raises(NotImplementedError):
        baked.render(cam, pipe, bg)


def test_static_heads_are_stored_once():
    n = 4099
    for cfg in CONFIGS:
        baked = _baked(n, cfg)
        on = fdgs.deformation._head_on(syn.deform_args(cfg))
        assert baked.head_on == tuple(on) and baked.nbytes == P.bake_bytes(n, len(TIMES), on)
        for h, name in enumerate(P.FIELDS):
            ptrs = [getattr(f, name).data_ptr() for f in baked.frames]
            assert all(q % 16 == 0 for q in ptrs), name                      # every slot on a 16-byte boundary (3 * 4099 floats is not)
            assert len(set(ptrs)) == (len(TIMES) if on[h] else 1), name
            lo, hi = baked._storage.data_ptr(), baked._storage.data_ptr() + baked.nbytes
            assert all(lo <= q and q + 4 * n * P.FIELD_WIDTH[h] <= hi for q in ptrs), name
    baked = _baked(n, "dnerf_bouncingballs")
    assert all(f.opacity is baked.frames[0].opacity and f.shs is baked.frames[0].shs for f in baked.frames)      # one storage for all frames
    assert baked.nbytes < _baked(n, "dynerf_default").nbytes // 2
    pc = _model(n, "dnerf_bouncingballs")
    assert torch.equal(baked.frames[3].shs, torch.cat((pc._features_dc, pc._features_rest), 1).detach())
    with pytest.raises(MemoryError):
        P.bake(pc, TIMES, max_bytes=baked.nbytes - 1)


def _cpu_state(frame):
    return dict(xyz=frame.xyz.cpu(), scales=frame.scales.cpu(), opacity=frame.opacity.cpu(), shs=frame.shs.cpu(), rot=frame.rotations.cpu())


@pytest.mark.parametrize("cfg", CONFIGS)
def test_blend_on_the_device_equals_blend_on_the_host(cfg):
    n = 4099
    pc, baked = _model(n, cfg), _baked(n, cfg)
    L = fdgs._lib.lib()
    state, where = baked.state_at(0.375, "linear")
    assert where == (1, 2, 0.5) == P.locate(TIMES, 0.375, "linear")
    fields = tuple(name for h, name in enumerate(P.FIELDS) if baked.head_on[h] and name != "rotations")
    a, b = _cpu_state(baked.frames[1]), _cpu_state(baked.frames[2])
    ref = host_blend(L, a, b, 0.5, fields=fields)
    got = _cpu_state(state)
    for k in (*fields, "rot"):
        assert not torch.equal(a[k], b[k]), k
        assert torch.equal(got[k], ref[k]), k                                    # bit for bit
    for h, name in enumerate(P.FIELDS):                                          # static arrays are passed as they are
        if not baked.head_on[h]:
            assert getattr(state, name) is getattr(baked.frames[0], name)
    # the frame: the rasterizer on the HOST-blended state
    cam, bg = _cam(1, 0.375), torch.zeros(3, device=_dev())
    got = baked.render(cam, syn.PipelineParams(), bg, interp="linear")
    full = dict(a, **ref)
    settings = fdgs.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5), bg=bg, scale_modifier=1.0,
        viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=pc.active_sh_degree, campos=cam.camera_center,
        prefiltered=False, debug=False)
    d = {k: v.to(_dev()) for k, v in full.items()}
    with torch.no_grad():
        image, radii, depth = fdgs.GaussianRasterizer(settings)(means3D=d["xyz"], means2D=torch.zeros_like(d["xyz"]), shs=d["shs"], opacities=d["opacity"],
                                                                scales=d["scales"], rotations=d["rot"])
    assert torch.equal(got["render"], image) and torch.equal(got["depth"], depth) and torch.equal(got["radii"], radii)
    at1, at2 = baked.render(_cam(1, 0.25), syn.PipelineParams(), bg), baked.render(_cam(1, 0.5), syn.PipelineParams(), bg)
    assert not torch.equal(got["render"], at1["render"]) and not torch.equal(got["render"], at2["render"])
    # nearest: the frame locate names (a tie: the lower index)
    i, j, w = P.locate(TIMES, 0.375, "nearest")
    assert (i, j, w) == (1, 1, 0.0)
    _same_frame(baked.render(cam, syn.PipelineParams(), bg, interp="nearest"), at1)
    # beyond the ends the time is clamped
    _same_frame(baked.render(_cam(1, 7.0), syn.PipelineParams(), bg), baked.render(_cam(1, 1.0), syn.PipelineParams(), bg))


def _timing_rows(fn):
    L = fdgs._lib.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    torch.cuda.synchronize()
    fdgs._lib.check(L.fdgs_timing_report(buf, len(buf), 1))
    L.fdgs_timing_enable(1)
    try:
        fn()
        fdgs._lib.check(L.fdgs_timing_report(buf, len(buf), 1))
    finally:
        L.fdgs_timing_enable(0)
    return {l.split()[0]: int(l.split()[1]) for l in buf.value.decode().strip().splitlines()}


def test_a_baked_frame_launches_no_deformation_and_a_blended_one_a_single_blend():
    pc, baked = _model(4099, "dynerf_default"), _baked(4099, "dynerf_default")
    bg = torch.zeros(3, device=_dev())
    rows = _timing_rows(lambda: _live(_cam(0, 0.25), pc))
    assert any(k.startswith("deform") for k in rows), rows
    rows = _timing_rows(lambda: baked.render(_cam(0, 0.25), syn.PipelineParams(), bg))
    assert not any(k.startswith("deform") or k == "state_blend" for k in rows), rows
    rows = _timing_rows(lambda: baked.render(_cam(0, 0.3), syn.PipelineParams(), bg, rgb8="round"))
    assert rows.get("state_blend") == 1 and rows.get("image_rgb8") == 1 and not any(k.startswith("deform") for k in rows), rows


def test_export_ply_sequence(tmp_path):
    n = 4099
    pc = _model(n, "dynerf_default")
    times = [0.0, 0.4, 1.0]
    paths = P.export_ply_sequence(pc, times, str(tmp_path / "gaussian_pertimestamp"))
    assert [p.split("/")[-1] for p in paths] == ["time_00000.ply", "time_00001.ply", "time_00002.ply"]
    names = fdgs.io.construct_list_of_attributes(pc)
    tables = []
    for path, t in zip(paths, times):
        with torch.no_grad():
            xyz, sc, rot, op, shs = fdgs.deformation.deform(pc._deformation, pc.get_xyz, pc._scaling, pc._rotation, pc._opacity,
                                                            shs_dc=pc._features_dc, shs_rest=pc._features_rest, time=t, activate=False)
        ref = torch.cat((xyz, torch.zeros_like(xyz), shs[:, :1].transpose(1, 2).flatten(start_dim=1), shs[:, 1:].transpose(1, 2).flatten(start_dim=1),
                         op, sc, rot), dim=1).cpu().numpy()
        v = fdgs.io.read_ply_vertices(path)
        assert list(v) == names and ref.shape == (n, 62)
        for c, name in enumerate(names):
            assert np.array_equal(v[name], ref[:, c]), (path, name)
        tables.append(ref)
    assert not np.array_equal(tables[0], tables[2])
    other = P.export_ply_sequence(pc, times[:1], str(tmp_path / "x"), pattern="frame{:03d}.ply")
    assert other == [str(tmp_path / "x" / "frame000.ply")]
    assert np.array_equal(fdgs.io.read_ply_vertices(other[0])["rot_3"], tables[0][:, 61])


@pytest.mark.parametrize("mode", ["trunc", "round"])
@pytest.mark.parametrize("shape", [(37, 23), (24, 36)], ids=["scalar_loads_and_tail", "vector_loads"])
def test_to_rgb8_equals_the_host_export(shape, mode):
    assert (shape[0] * shape[1]) % 4 == (3 if shape == (37, 23) else 0)
    x = boundary_image(*shape)
    got = P.to_rgb8(torch.from_numpy(x).to(_dev()), mode)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (*shape, 3) and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy(), host_rgb8(fdgs._lib.lib(), x, mode))


def test_baked_render_rgb8_is_to_rgb8_of_its_own_image():
    baked = _baked(4099, "dnerf_bouncingballs")
    bg = torch.tensor([1.0, 1.0, 1.0], device=_dev())
    out = baked.render(_cam(3, 1.0), syn.PipelineParams(), bg, rgb8="trunc")
    assert tuple(out["rgb8"].shape) == (H, W, 3) and torch.equal(out["rgb8"], P.to_rgb8(out["render"], "trunc"))
    assert np.array_equal(out["rgb8"].cpu().numpy(), host_rgb8(fdgs._lib.lib(), np.ascontiguousarray(out["render"].cpu().numpy()), "trunc"))
    assert "rgb8" not in baked.render(_cam(3, 1.0), syn.PipelineParams(), bg)
    assert len(torch.unique(out["rgb8"])) > 50


def test_no_graph_is_recorded():
    pc, baked = _model(4099, "dynerf_default"), _baked(4099, "dynerf_default")
    for p in pc.parameters():
        p.grad = None
    bg = torch.zeros(3, device=_dev())
    with torch.enable_grad():
        fresh = P.bake(pc, TIMES[:2])
        outs = [baked.render(_cam(0, 0.25), syn.PipelineParams(), bg), baked.render(_cam(0, 0.3), syn.PipelineParams(), bg, rgb8="trunc"),
                fresh.render(_cam(0, 0.1), syn.PipelineParams(), bg)]
        for out in outs:
            for k, v in out.items():
                if isinstance(v, torch.Tensor):
                    assert not v.requires_grad and v.grad_fn is None, k
        for f in fresh.frames:
            assert not any(a.requires_grad for a in f.arrays())
    assert all(p.grad is None for p in pc.parameters())
