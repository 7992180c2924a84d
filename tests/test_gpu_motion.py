"""Motion vectors and coverage on the device (csrc/motion.hip, render_motion of fdgs.playback / fdgs.compose).  Every comparison but the
last is EXACT: the two kernels run the functions their *_host twins run (csrc/motion_ops.h, compiled without contraction), the blend forward
has no atomics on its image path, and the extra blend pass walks the very lists a whole second frame would sort again.  The last test holds
the second blend against the C rasterizer oracle, with the bound tests/test_gpu_raster.py asserts for colours in [0, 1) scaled by the size of
the colours (the image is linear in them)."""
import ctypes
import importlib
import math

import numpy as np
import pytest
import torch

from oracle.raster_oracle import RasterOracle
from scenes import raster_scene
from test_gpu_playback import H, TIMES, W, _baked, _cam, _dev, _model
from test_gpu_sparse_playback import _sparse
from test_motion_host import SENTINEL, SIZES, bits, camera_matrices, host_resolve, host_rows, positions, resolve_image, with_culled_rows

pytestmark = pytest.mark.gpu
fdgs = importlib.import_module("4dgaussians_amd")
C, P, R, syn = fdgs.compose, fdgs.playback, fdgs.rasterizer, fdgs.synthetic
L = fdgs._lib
KEYS = ("render", "depth", "radii", "visibility_filter")
MOTION_KEYS = ("motion_raw", "motion", "alpha")


def _pipe():
    return syn.PipelineParams()


def _dev_t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


# ---- the kernels against their host twins ------------------------------------------------------------------------------------------------

def device_rows(at, to, view_at, proj_at, view_to, proj_to, stride, out_offset, w=W, h=H):
    """fdgs_motion_rows with xyz_* one row (12 bytes) into their allocations and `out` out_offset floats into its own -> ([n, stride], guard)."""
    n = at.shape[0]
    a = torch.full((n + 1, 3), 9.0, device=_dev()); a[1:] = _dev_t(at)
    b = torch.full((n + 1, 3), 9.0, device=_dev()); b[1:] = _dev_t(to)
    mats = [_dev_t(m) for m in (view_at, proj_at, view_to, proj_to)]
    out = torch.full((out_offset + n * stride + 4,), float(SENTINEL), device=_dev())
    assert out.data_ptr() % 16 == 0
    L.check(L.lib().fdgs_motion_rows(L.stream_ptr(), n, a.data_ptr() + 12, b.data_ptr() + 12, *[m.data_ptr() for m in mats], w, h,
                                     out.data_ptr() + 4 * out_offset, stride))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return o[out_offset:out_offset + n * stride].reshape(n, stride), np.concatenate([o[:out_offset], o[out_offset + n * stride:]])


@pytest.mark.parametrize("n", SIZES)
def test_device_rows_equal_the_host_twin(n):
    """Both strides; `out` on a 16-byte boundary (stride 4: one float4 per lane) and 12 bytes past one (scalar stores); rows behind either
    camera among them; nothing outside the n rows is written."""
    lib = L.lib()
    view_at, proj_at, c_at = camera_matrices(20.0)
    view_to, proj_to, c_to = camera_matrices(31.0)
    at, to = positions(n)
    at, to, *_ = with_culled_rows(at, to, c_at, c_to)
    for stride in (3, 4):
        want, _ = host_rows(lib, at, to, view_at, proj_at, view_to, proj_to, stride)
        for out_offset in (0, 3):
            got, guard = device_rows(at, to, view_at, proj_at, view_to, proj_to, stride, out_offset)
            assert np.array_equal(bits(got), bits(want)), (stride, out_offset)
            assert np.array_equal(bits(guard), bits(np.full_like(guard, SENTINEL))), (stride, out_offset)


@pytest.mark.parametrize("shape,offset", [((1, 1), 0), ((5, 7), 0), ((64, 96), 0), ((64, 96), 1)],
                         ids=["one_pixel", "odd_planes_and_tail", "vector", "unaligned_base"])
def test_device_resolve_equals_the_host_twin(shape, offset):
    h, w = shape
    for min_alpha in (0.0, 0.25):
        raw = resolve_image(h, w, min_alpha)
        want_motion, want_alpha = host_resolve(L.lib(), raw, min_alpha)
        src = torch.zeros(offset + 3 * h * w, device=_dev())
        src[offset:] = _dev_t(raw.reshape(-1))
        motion = torch.full((offset + 2 * h * w + 4,), float(SENTINEL), device=_dev())
        alpha = torch.full((offset + h * w + 4,), float(SENTINEL), device=_dev())
        L.check(L.lib().fdgs_motion_resolve(L.stream_ptr(), h, w, min_alpha, src.data_ptr() + 4 * offset, motion.data_ptr() + 4 * offset,
                                            alpha.data_ptr() + 4 * offset))
        torch.cuda.synchronize()
        m, a = motion.cpu().numpy(), alpha.cpu().numpy()
        assert np.array_equal(bits(m[offset:offset + 2 * h * w]), bits(want_motion.reshape(-1)))
        assert np.array_equal(bits(a[offset:offset + h * w]), bits(want_alpha.reshape(-1)))
        for buf, used in ((m, 2 * h * w), (a, h * w)):
            rest = np.concatenate([buf[:offset], buf[offset + used:]])
            assert np.array_equal(bits(rest), bits(np.full_like(rest, SENTINEL)))


# ---- one extra pass equals a whole second frame ------------------------------------------------------------------------------------------

def _placement():
    return C.Placement(rotation=(0.8, 0.0, 0.6, 0.0), translation=(0.4, -0.2, 0.3), scale=0.6)


def _scene():
    return C.compose([_baked(4099, "dynerf_default"), _baked(8200, "dnerf_bouncingballs")], [None, _placement()])


def _object(kind):
    if kind == "composite":
        return _scene()
    which, n, cfg = kind
    return _baked(n, cfg) if which == "baked" else _sparse(n, cfg, which)


def _frame_at(obj, t):
    st = obj.state_at(t)
    return st[0] if isinstance(st, tuple) else st


def _settings(cam, bg, sh_degree):
    return fdgs.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5), bg=bg, scale_modifier=1.0,
        viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=sh_degree, campos=cam.camera_center,
        prefiltered=False, debug=False)


def _flat(m):
    return np.ascontiguousarray(m.cpu().numpy().reshape(-1), dtype=np.float32)


def _same(a, b, keys):
    for k in keys:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


KINDS = [("baked", 4099, "dynerf_default"), ("baked", 8200, "dnerf_bouncingballs"), ("baked", 4099, "dnerf_bouncingballs"),
         ("baked", 8200, "dynerf_default"), ("all", 4099, "dynerf_default"), ("all", 8200, "dnerf_bouncingballs"),
         ("quantile", 4099, "dynerf_default"), ("quantile", 8200, "dnerf_bouncingballs"), "composite"]
# (frame camera, frame time, toward camera, toward time): the first frame of a test takes the exact binning path, the later ones the
# speculative capacity path; a frame time between two timestamps, a toward time between two others
FRAMES = [(0, 0.25, 1, 0.5), (1, 0.375, 2, 0.75), (2, 1.0, 0, 0.0)]


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k if isinstance(k, str) else "-".join(str(v) for v in k))
def test_one_extra_blend_pass_equals_a_whole_second_frame(kind):
    lib = L.lib()
    obj = _object(kind)
    bg, zero, pipe = torch.tensor([0.1, 0.2, 0.3], device=_dev()), torch.zeros(3, device=_dev()), _pipe()
    moved = 0.0
    for f, (k, t, k2, t2) in enumerate(FRAMES):
        cam, cam2 = _cam(k, t), _cam(k2, 0.123)                  # (the toward camera's own time is overridden)
        seen_before = dict(R._seen)
        got = obj.render_motion(cam, pipe, bg, toward=cam2, toward_time=t2, min_alpha=0.05)
        assert (len(seen_before) == 0) == (f == 0)               # frame 0: no history (exact path); later: a capacity is known
        # the reference: the host twin on CPU copies of the two position sets, then a WHOLE frame with those colours
        xyz_to = _frame_at(obj, t2).xyz.cpu().numpy().copy()
        st = _frame_at(obj, t)
        xyz_at = st.xyz.cpu().numpy().copy()
        colors, _ = host_rows(lib, xyz_at, xyz_to, _flat(cam.world_view_transform), _flat(cam.full_proj_transform),
                              _flat(cam2.world_view_transform), _flat(cam2.full_proj_transform), 3, offset_rows=0)
        with torch.no_grad():
            image, *_ = R.rasterize_forward(_settings(cam, zero, obj.active_sh_degree), st.xyz, None, _dev_t(colors), st.opacity, st.scales,
                                            st.rotations, None)
        assert torch.equal(got["motion_raw"], image)
        motion, alpha = host_resolve(lib, got["motion_raw"].cpu().numpy(), 0.05)
        assert np.array_equal(bits(got["motion"].cpu().numpy()), bits(motion)) and np.array_equal(bits(got["alpha"].cpu().numpy()), bits(alpha))
        want = obj.render(cam, pipe, bg)
        _same(got, want, KEYS)
        assert set(got) == set(want) | set(MOTION_KEYS) and got["viewspace_points"] is None
        moved = max(moved, float(got["motion"].abs().max()))
        assert float(got["alpha"].max()) > 0.5
    assert moved > 1.0                                           # (frames in which something moves by more than a pixel)


@pytest.mark.parametrize("n,cfg", [(4099, "dynerf_default"), (8200, "dnerf_bouncingballs")])
def test_sparse_with_every_row_dynamic_equals_dense(n, cfg):
    dense, sparse = _baked(n, cfg), _sparse(n, cfg, "all")
    bg, pipe = torch.tensor([0.3, 0.2, 0.1], device=_dev()), _pipe()
    for k, t, k2, t2 in FRAMES:
        a = dense.render_motion(_cam(k, t), pipe, bg, toward=_cam(k2, t2), rgb8="trunc")
        b = sparse.render_motion(_cam(k, t), pipe, bg, toward=_cam(k2, t2), rgb8="trunc")
        assert set(a) == set(b)
        _same(a, b, KEYS + MOTION_KEYS + ("rgb8",))


@pytest.mark.parametrize("kind", [("baked", 4099, "dynerf_default"), ("baked", 8200, "dnerf_bouncingballs"), ("quantile", 8200, "dnerf_bouncingballs"),
                                  "composite"], ids=lambda k: k if isinstance(k, str) else "-".join(str(v) for v in k))
def test_a_frame_toward_itself_has_zero_motion_and_its_alpha_is_the_blend_of_ones(kind):
    obj = _object(kind)
    zero, pipe = torch.zeros(3, device=_dev()), _pipe()
    for k, t in ((0, 0.25), (1, 0.6)):
        cam = _cam(k, t)
        got = obj.render_motion(cam, pipe, zero, toward=cam)
        assert not bool(got["motion"].any()) and not bool(got["motion_raw"][:2].any())
        ones = obj.render(cam, pipe, zero, override_color=torch.ones(obj.N, 3, device=_dev()))
        assert torch.equal(got["alpha"], ones["render"][:1]) and float(got["alpha"].max()) > 0.5
        again = obj.render_motion(cam, pipe, zero, toward_time=t)
        _same(got, again, KEYS + MOTION_KEYS)


def test_the_state_stays_truthful_after_a_motion_frame():
    bg, pipe = torch.tensor([0.1, 0.2, 0.3], device=_dev()), _pipe()
    n, cfg = 4099, "dynerf_default"
    fresh = {"baked": lambda: P.bake(_model(n, cfg), TIMES), "sparse": lambda: P.bake_sparse(_model(n, cfg), TIMES, 1e-3), "composite": _scene}
    for name, make in fresh.items():
        for t0, t1 in ((0.25, 0.6), (0.6, 0.5), (0.1, 0.1)):
            obj = make()
            obj.render_motion(_cam(0, t0), pipe, bg, toward_time=t1)
            got = obj.render(_cam(1, t1), pipe, bg)
            _same(got, make().render(_cam(1, t1), pipe, bg), KEYS)
            _same(obj.render(_cam(2, t0), pipe, bg), make().render(_cam(2, t0), pipe, bg), KEYS)


# ---- the second blend against the C rasterizer oracle --------------------------------------------------------------------------------------

def test_second_blend_of_motion_colours_against_the_oracle():
    """The scene of test_gpu_raster.py::test_colors_precomp_and_cov3d_precomp_paths.  The colours are the motion rows toward a displaced copy
    of the positions (same camera), evaluated in float64 and rounded to float32, max |colour| <= 8 pixels (checked here, on the CPU); they
    are put into recC of a finished SH frame and blended by a second fdgs_render_fwd.  Bound: mean |device - oracle| < 2e-6 max(1, max |colour|)."""
    dev = _dev()
    n, w, h = 2000, 160, 120
    sc = raster_scene(n, w, h, seed=4, scale_boost=3.0)
    xyz = sc["means3D"].astype(np.float64)
    to = xyz + np.random.default_rng(5).uniform(-0.06, 0.06, xyz.shape)
    view, proj = sc["viewmatrix"].astype(np.float64).reshape(-1), sc["projmatrix"].astype(np.float64).reshape(-1)

    def pix(p, S, k):
        hh = proj[k] * p[:, 0] + proj[4 + k] * p[:, 1] + proj[8 + k] * p[:, 2] + proj[12 + k]
        ww = proj[3] * p[:, 0] + proj[7] * p[:, 1] + proj[11] * p[:, 2] + proj[15]
        return ((hh / (ww + float(np.float32(1e-7))) + 1.0) * S - 1.0) * 0.5

    def zview(p):
        return view[2] * p[:, 0] + view[6] * p[:, 1] + view[10] * p[:, 2] + view[14]

    ok = (zview(xyz) > 0.2) & (zview(to) > 0.2)
    cols = np.stack([np.where(ok, pix(to, w, 0) - pix(xyz, w, 0), 0.0), np.where(ok, pix(to, h, 1) - pix(xyz, h, 1), 0.0), np.ones(n)], 1).astype(np.float32)
    biggest = float(np.abs(cols).max())
    assert 2.0 < biggest <= 8.0 and bool(ok.all())
    sc2 = {k: v for k, v in sc.items() if k != "shs"}
    sc2["bg"] = np.zeros(3, np.float32)
    o = RasterOracle(**sc2, colors_precomp=cols)
    t = {k: torch.tensor(sc[k], device=dev) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    settings = R.GaussianRasterizationSettings(
        image_height=h, image_width=w, tanfovx=sc["tanfovx"], tanfovy=sc["tanfovy"], bg=torch.tensor(sc["bg"], device=dev), scale_modifier=1.0,
        viewmatrix=torch.tensor(sc["viewmatrix"], device=dev), projmatrix=torch.tensor(sc["projmatrix"], device=dev), sh_degree=sc["sh_degree"],
        campos=torch.tensor(sc["campos"], device=dev), prefiltered=False, debug=False)
    with torch.no_grad():
        color, radii, depth, state = R.rasterize_forward(settings, t["means3D"], t["shs"], None, t["opacities"], t["scales"], t["rotations"], None)
    first = color.clone()
    rec = torch.zeros(n, 4, device=dev)
    rec[:, :3] = torch.tensor(cols, device=dev)
    recC = ctypes.c_void_p()
    L.check(L.lib().fdgs_geom_field(L.ptr(state.geom), n, 3, recC))
    torch.cuda.synchronize()
    hip = ctypes.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(recC, ctypes.c_void_p(rec.data_ptr()), ctypes.c_size_t(16 * n), ctypes.c_int(3)) == 0
    p2 = L.RasterParams.from_buffer_copy(state.params)
    zero = torch.zeros(3, device=dev)
    p2.bg, p2.acc_zero = L.ptr(zero), None
    raw, depth2 = torch.empty(3, h, w, device=dev), torch.empty(1, h, w, device=dev)
    L.check(L.lib().fdgs_render_fwd(L.stream_ptr(), p2, L.ptr(state.geom), L.ptr(state.binning), L.ptr(state.img), state.capacity, L.ptr(raw),
                                    L.ptr(depth2)))
    torch.cuda.synchronize()
    err = float(np.abs(raw.cpu().numpy() - o.color).mean())
    print(f"second blend vs oracle: mean |dC| = {err:.3e}, max |colour| = {biggest:.3f}, bound = {2e-6 * max(1.0, biggest):.3e}")
    assert err < 2e-6 * max(1.0, biggest)
    assert torch.equal(depth2, depth) and torch.equal(color, first)          # the depth again; the frame's own image untouched
    assert float(np.abs(o.color[:2]).max()) > 1.0 and float(o.color[2].max()) > 0.9
