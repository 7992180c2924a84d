"""The rasterizer forward's two newer shapes against the ones they replace, bit for bit (nothing here is toleranced but the gradients that
float atomics already reorder):

* knob bin_count = 1: the one-call frame (fdgs_raster_fwd_capacity) counts the tiles' pairs inside the projection kernel, turns the counts
  into ranges and the forward's tile order in one launch, and emits on the counters -- against bin_count = 0 (count launch, scan, cursors,
  order launch) and against the staged exact path (fdgs_preprocess_fwd -> fdgs_bin_prepare -> fdgs_bin_sort -> fdgs_render_fwd);
* knob blend_fwd_form = 1: render_fwd_kernel takes two list entries per trip, packed across the entries -- against form 0.
"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from conftest import set_knob
from scenes import raster_scene, rel_l2
from test_gpu_tile_sort import _KEYS, _copy, _mod, _settings

pytestmark = pytest.mark.gpu

TILE = 16
ALPHA_MIN, ALPHA_MAX, T_STOP = np.float32(1.0 / 255.0), np.float32(0.99), np.float32(1e-4)      # csrc/gs_math.h


def _dev():
    return torch.device("cuda:0")


def _img_field(st, which, n, dtype):
    q = ctypes.c_void_p()
    L = _mod()._lib.lib()
    assert L.fdgs_img_field(ctypes.c_void_p(st.img.data_ptr()), st.params.W, st.params.H, which, ctypes.byref(q)) == 0
    return _copy(q.value, n, dtype, st.img.device)


def _state_outputs(st, color, depth, radii):
    """Everything a forward leaves behind, as host arrays of raw words."""
    torch.cuda.synchronize()
    W, H = st.params.W, st.params.H
    ntiles = ((W + TILE - 1) // TILE) * ((H + TILE - 1) // TILE)
    L = _mod()._lib.lib()
    n = st.num_rendered
    out = dict(n=n, color=color.cpu().numpy().view(np.uint32), depth=depth.cpu().numpy().view(np.uint32), radii=radii.cpu().numpy())
    out["ranges"] = _img_field(st, 2, 2 * ntiles, torch.int32).view(np.uint32).reshape(ntiles, 2)
    out["final_T"] = _img_field(st, 0, W * H, torch.int32).view(np.uint32)
    out["ncontrib"] = _img_field(st, 1, W * H, torch.int32).view(np.uint32)
    out["todo"] = _img_field(st, 3, ntiles, torch.int32).view(np.uint32)
    held = min(n, st.capacity)
    q = ctypes.c_void_p()
    gid = np.zeros(0, np.uint32)
    if held:
        assert L.fdgs_binning_field(ctypes.c_void_p(st.binning.data_ptr()), st.capacity, W, H, 0, ctypes.byref(q)) == 0
        gid = _copy(q.value, held, torch.int32, st.binning.device).view(np.uint32)
    # the lists, tile by tile (what lies between two ranges is nobody's)
    out["lists"] = [gid[a:b] for a, b in out["ranges"].astype(np.int64)]
    return out


def _frame(sc, path, monkeypatch, **knobs):
    """One forward of `sc`.  path "staged": the four-call exact path; "onecall": fdgs_raster_fwd_capacity on a capacity that holds the frame
    (the pair-count history is set from a staged frame of the same scene, as a training loop's second frame finds it)."""
    R = _mod().rasterizer
    dev = _dev()
    for k, v in knobs.items():
        set_knob(k, v)
    t = [torch.tensor(sc[k], device=dev) for k in _KEYS]
    P, W, H = len(sc["means3D"]), sc["image_width"], sc["image_height"]
    key = (dev.index, W, H, P)
    if path == "onecall":
        assert key in R._seen, "a staged frame first"
        monkeypatch.setattr(R, "BINNING", "auto")
        before = R.capacity_reruns
    else:
        monkeypatch.setattr(R, "BINNING", "exact")
    color, radii, depth, st = R.rasterize_forward(_settings(sc, dev), t[0], t[1], None, t[2], t[3], t[4], None)
    if path == "onecall":
        assert R.capacity_reruns == before and st.capacity % 4096 == 0          # it was the one call, and no rerun
    return _state_outputs(st, color, depth, radii), st


def _same(a, b, what):
    assert a["n"] == b["n"], what
    for k in ("ranges", "ncontrib", "final_T", "color", "depth", "radii", "todo"):
        assert np.array_equal(a[k], b[k]), (what, k)
    for tl, (x, y) in enumerate(zip(a["lists"], b["lists"])):
        assert np.array_equal(x, y), (what, "list of tile", tl)


# ---------------------------------------------------------------------------------------------------------------- 1. chain equality
def _place(sc, view_xyz):
    """World positions of points given in the camera's frame (p_view = [p, 1] @ V, scenes.py stores V that way)."""
    V = np.asarray(sc["viewmatrix"], np.float64).reshape(4, 4)
    p = np.concatenate([np.asarray(view_xyz, np.float64), np.ones((len(view_xyz), 1))], 1) @ np.linalg.inv(V)
    return p[:, :3].astype(np.float32)


def _scene_small():
    return raster_scene(300, 40, 24, seed=31, scale_boost=2.0)            # 3 x 2 tiles, partial tiles on both edges


def _scene_mid():
    """272 x 272 = 17 x 17 tiles, 2 000 Gaussians; by construction: squares of more than 64 tiles (walked by the whole wave), one over all 289
    tiles (more than 256: never masked), Gaussians 512 .. 767 behind the camera (a whole projection workgroup with nothing on screen), one in
    front of the camera but so far to the side that its square is empty.  test_chain_equality asserts all four from the frame's geom."""
    sc = raster_scene(2000, 272, 272, seed=32, scale_boost=1.5)
    for k in _KEYS:
        sc[k] = sc[k].copy()
    z = 4.0
    sc["means3D"][0] = _place(sc, [[0.0, 0.0, z]])[0]
    sc["scales"][0] = 40.0
    sc["opacities"][0] = 0.05
    big = np.arange(1, 9)
    sc["means3D"][big] = _place(sc, [[0.15 * np.cos(i), 0.15 * np.sin(i), z + 0.01 * i] for i in big])
    sc["scales"][big] = (0.25 + 0.03 * big)[:, None].astype(np.float32)
    sc["opacities"][big] = 0.1
    sc["means3D"][512:768] = (2.0 * sc["campos"][None, :] - sc["means3D"][512:768]).astype(np.float32)
    sc["means3D"][9] = _place(sc, [[500.0, 0.0, z]])[0]
    sc["scales"][9] = 0.05
    return sc


def _scene_one():
    sc = raster_scene(400, 96, 80, seed=6, scale_boost=2.0)
    for k in _KEYS:
        sc[k] = sc[k][7:8]
    return sc


def _scene_all_culled():
    sc = raster_scene(400, 96, 80, seed=6, scale_boost=2.0)
    sc["means3D"] = (2.0 * sc["campos"][None, :] - sc["means3D"]).astype(np.float32)
    return sc


CHAIN_SCENES = {"40x24": _scene_small, "272x272": _scene_mid, "one": _scene_one, "all_culled": _scene_all_culled}


def _geom_u32(st, which, n):
    q = ctypes.c_void_p()
    assert _mod()._lib.lib().fdgs_geom_field(ctypes.c_void_p(st.geom.data_ptr()), st.params.P, which, ctypes.byref(q)) == 0
    return _copy(q.value, n, torch.int32, st.geom.device).view(np.uint32)


@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("name", list(CHAIN_SCENES))
def test_chain_equality(name, cull, monkeypatch):
    sc = CHAIN_SCENES[name]()
    P = len(sc["means3D"])
    off = dict(tile_cull=cull, bin_count=0, blend_fwd_form=0)
    want, st = _frame(sc, "staged", monkeypatch, **off)
    if name == "272x272":
        tiles = _geom_u32(st, 5, P)
        rect = _geom_u32(st, 7, 2 * P).reshape(P, 2).astype(np.int64)
        w, h = (rect[:, 1] & 0xFFFF) - (rect[:, 0] & 0xFFFF), (rect[:, 1] >> 16) - (rect[:, 0] >> 16)
        area = np.where(tiles > 0, w * h, 0)
        assert ((area > 64) & (area <= 256)).any() and (area == 289).any()
        assert not tiles[512:768].any() and tiles[:512].any()
        assert tiles[9] == 0 and want["radii"][9] == 0
        assert (want["ranges"][:, 1] > want["ranges"][:, 0]).all()
    elif name == "all_culled":
        assert want["n"] == 0 and not want["ranges"].any()
    else:
        assert want["n"] > 0
    _same(want, _frame(sc, "onecall", monkeypatch, **off)[0], "one call, count launch")
    for count in (1, 2):
        _same(want, _frame(sc, "onecall", monkeypatch, tile_cull=cull, bin_count=count, blend_fwd_form=0)[0], f"one call, bin_count {count}")
    _same(want, _frame(sc, "onecall", monkeypatch, tile_cull=cull, bin_count=1, blend_fwd_form=1)[0], "one call, both knobs on")
    _same(want, _frame(sc, "staged", monkeypatch, tile_cull=cull, bin_count=1, blend_fwd_form=0)[0], "staged, bin_count 1")


# ---------------------------------------------------------------------------------------------------------------- 2. overflow rerun
def test_exact_rerun_after_a_projection_that_counted(monkeypatch):
    """The default mode with a predictor that is far too low (the shape of test_gpu_tile_sort.test_overflow_of_a_predicted_capacity): the
    one-call frame counts in its projection and overflows, fdgs_bin_sort + fdgs_render_fwd finish it exactly on the same geom."""
    R = _mod().rasterizer
    dev = _dev()
    sc = _scene_mid()
    want, _ = _frame(sc, "staged", monkeypatch, bin_count=0, blend_fwd_form=0)
    assert want["n"] > 40000
    key = (dev.index, 272, 272, 2000)
    monkeypatch.setattr(R, "BINNING", "auto")
    set_knob("bin_count", 1)
    set_knob("blend_fwd_form", 1)
    t = [torch.tensor(sc[k], device=dev) for k in _KEYS]
    for too_low in (want["n"] // 4, 1):
        R._seen[key] = [too_low, 2000]
        before = R.capacity_reruns
        color, radii, depth, st = R.rasterize_forward(_settings(sc, dev), t[0], t[1], None, t[2], t[3], t[4], None)
        assert R.capacity_reruns == before + 1 and st.capacity == want["n"]
        _same(want, _state_outputs(st, color, depth, radii), f"predictor {too_low}")


# ---------------------------------------------------------------------------------------------------------------- 3. blend-loop equality
# The lists come from a real frame: N Gaussians at increasing depth, each over every tile, so every tile's list is 0, 1, .., N - 1.  Their
# RECORDS are then written by hand (fdgs_geom_field 1 .. 3: what the blending kernel reads, nothing else) and blended once per form with
# fdgs_render_fwd over the frame's own buffers.
def _records(N, W, H, seed):
    """recA (x, y, cxx, cxy), recB (cyy, opacity, depth, 0), recC (r, g, b, 0) by list position."""
    rng = np.random.default_rng(seed)
    A, B, C = np.zeros((N, 4), np.float32), np.zeros((N, 4), np.float32), np.zeros((N, 4), np.float32)
    A[:, 0], A[:, 1] = rng.uniform(0, W, N), rng.uniform(0, H, N)
    A[:, 2] = 0.001
    B[:, 0] = 0.001
    B[:, 1] = rng.uniform(0.015, 0.04, N)                 # faint and wide: T falls slowly, to about 1e-3 after a round and to 1e-4 in the second
    B[:, 2] = 1.0 + 0.01 * np.arange(N)
    C[:, :3] = rng.uniform(-1.0, 2.0, (N, 3))
    j = np.arange(N)
    saddle = (j % 7) == 3                                  # an indefinite form: power > 0 where dx dy > 0 (both parities of j)
    A[saddle, 2], A[saddle, 3], B[saddle, 0] = 0.01, -0.02, 0.01
    A[saddle, 0], A[saddle, 1] = W / 2 + rng.uniform(-3, 3, saddle.sum()), H / 2 + rng.uniform(-3, 3, saddle.sum())
    narrow = (j % 17) == 1                                 # dense and narrow: alpha 0.5 at its centre, below 1 / 255 four pixels away
    A[narrow, 2], A[narrow, 3], B[narrow, 0], B[narrow, 1] = 0.5, 0.0, 0.5, 0.5
    A[narrow, 0], A[narrow, 1] = np.floor(A[narrow, 0]), np.floor(A[narrow, 1])
    for pos, (x, y) in ((255, (3, 3)), (511, (3, 3)), (254, (11, 5)), (253, (5, 11)), (510, (11, 5)), (509, (5, 11))):
        if pos < N:                                        # stoppers at the end of a round and on either half of a pair
            A[pos] = (x, y, 0.5, 0.0)
            B[pos, 0], B[pos, 1] = 0.5, 0.995
            if pos % 256 == 255:                           # the end of a round: wider, and "opacity" 4 so that alpha is the 0.99 cap for 8 pixels around
                A[pos, 2], B[pos, 0], B[pos, 1] = 0.05, 0.05, 4.0
    return A, B, C


def _restate(A, B, W, H):
    """The forward's decisions in numpy float32, the kernel's operations in the kernel's order (its exp is the device's: an entry whose
    alpha or T comes within `margin` of a threshold makes its pixel `unsure` from there on).  -> per pixel and entry what happened."""
    f = np.float32
    py, px = np.meshgrid(np.arange(H, dtype=f), np.arange(W, dtype=f), indexing="ij")
    N = len(A)
    T = np.ones((H, W), f)
    live, sure = np.ones((H, W), bool), np.ones((H, W), bool)
    last = np.zeros((H, W), np.int64)
    what = np.zeros((N, H, W), np.int8)                    # 0 not reached, 1 power > 0, 2 alpha < 1/255, 3 stopped here, 4 blended
    margin = f(1e-3)
    for j in range(N):
        dx, dy = A[j, 0] - px, A[j, 1] - py
        u1, cx = dx * (dx * A[j, 2]), dx * A[j, 3]
        u2, c2 = dy * (dy * B[j, 0]), dy * cx
        power = f(-0.5) * (u1 + u2) - c2                   # (q * -0.5 is exact: the fused multiply-add rounds once, like this subtraction)
        alpha = np.minimum(ALPHA_MAX, B[j, 1] * np.exp(np.minimum(power, f(0)), dtype=f))
        test_T = T * (f(1) - alpha)
        pos, low = power > 0, alpha < ALPHA_MIN
        stop = ~pos & ~low & (test_T < T_STOP)
        sure &= ~(live & ~pos & ((np.abs(alpha - ALPHA_MIN) < margin * ALPHA_MIN) | (~low & (np.abs(test_T - T_STOP) < margin * T_STOP))))
        sure &= ~(live & (np.abs(power) < f(1e-6)))
        blend = live & ~pos & ~low & ~stop
        what[j] = np.where(~live, 0, np.where(pos, 1, np.where(low, 2, np.where(stop, 3, 4))))
        T = np.where(blend, test_T, T)
        last = np.where(blend, j + 1, last)
        live &= ~stop
    return what, last, sure


BLEND_IMAGES = [(16, 16), (24, 40)]
BLEND_LENGTHS = [0, 1, 2, 3, 255, 256, 257, 513]


def _records_view(st, which, P):
    q = ctypes.c_void_p()
    assert _mod()._lib.lib().fdgs_geom_field(ctypes.c_void_p(st.geom.data_ptr()), P, which, ctypes.byref(q)) == 0
    off = q.value - st.geom.data_ptr()
    assert 0 <= off and off + 16 * P <= st.geom.numel()
    return st.geom[off:off + 16 * P].view(torch.float32).view(P, 4)


@pytest.mark.parametrize("N", BLEND_LENGTHS)
@pytest.mark.parametrize("W,H", BLEND_IMAGES)
def test_blend_loop_forms_agree(W, H, N, monkeypatch):
    dev = _dev()
    Lm = _mod()._lib
    R = _mod().rasterizer
    P = max(N, 1)
    sc = raster_scene(P, W, H, seed=40, sh_degree=0)
    for k in _KEYS:
        sc[k] = sc[k].copy()
    sign = 1.0 if N else -1.0                                                   # (N = 0: one Gaussian, behind the camera)
    sc["means3D"] = _place(sc, [[0.0, 0.0, sign * (3.0 + 0.01 * i)] for i in range(P)])
    sc["scales"][:] = 3.0
    monkeypatch.setattr(R, "BINNING", "exact")
    set_knob("tile_cull", 0)
    t = [torch.tensor(sc[k], device=dev) for k in _KEYS]
    color, radii, depth, st = R.rasterize_forward(_settings(sc, dev), t[0], t[1], None, t[2], t[3], t[4], None)
    first = _state_outputs(st, color, depth, radii)
    for lst in first["lists"]:
        assert np.array_equal(lst, np.arange(N)), "every tile lists 0 .. N - 1"
    A, B, C = _records(P, W, H, seed=41 + N)
    for which, rec in ((1, A), (2, B), (3, C)):
        _records_view(st, which, P).copy_(torch.tensor(rec, device=dev))
    p2 = Lm.RasterParams.from_buffer_copy(st.params)
    p2.acc_zero = None
    outs = []
    for form in (0, 1):
        set_knob("blend_fwd_form", form)
        c2, d2 = torch.full((3, H, W), -7.0, device=dev), torch.full((1, H, W), -7.0, device=dev)
        Lm.check(Lm.lib().fdgs_render_fwd(Lm.stream_ptr(), p2, Lm.ptr(st.geom), Lm.ptr(st.binning) if N else None, Lm.ptr(st.img), st.capacity if N else 0,
                                          Lm.ptr(c2), Lm.ptr(d2)))
        outs.append(_state_outputs(st, c2, d2, radii))
    for k in ("color", "depth", "final_T", "ncontrib", "todo"):
        assert np.array_equal(outs[0][k], outs[1][k]), k
    if N == 0:
        assert not outs[1]["ncontrib"].any()
        return
    # the cases the constructed list has to contain, from the numpy restatement -- and the restatement is the kernel's: wherever no
    # decision came near a threshold it predicts n_contrib
    what, last, sure = _restate(A[:N], B[:N], W, H)
    got_last = outs[1]["ncontrib"].astype(np.int64).reshape(H, W)
    assert sure.mean() > 0.5 and np.array_equal(got_last[sure], last[sure])
    if N < 513:
        return
    even, odd = what[0:N - 1:2][:, sure], what[1:N:2][:, sure]                 # the two entries of every pair, at the pixels that are sure
    cases = {
        "power > 0 on the first entry only": ((even == 1) & (odd != 1) & (odd != 0)).any(),
        "power > 0 on the second entry only": ((odd == 1) & (even != 1)).any(),
        "alpha < 1/255 on the first entry only": ((even == 2) & (odd != 2) & (odd != 0)).any(),
        "alpha < 1/255 on the second entry only": ((odd == 2) & (even != 2)).any(),
        "stops on the first entry of a pair": ((even == 3) & (odd == 0)).any(),
        "stops on the second entry": (odd == 3).any(),
        "stops on the last entry of a round": (what[255][sure] == 3).any() or (what[511][sure] == 3).any(),
        "blends through a round boundary": ((what[255][sure] == 4) & (what[256][sure] != 0)).any(),
    }
    assert all(cases.values()), [k for k, v in cases.items() if not v]


# ---------------------------------------------------------------------------------------------------------------- 4. backward consistency
def test_backward_is_the_knobs_off_backward(monkeypatch):
    """render() forward and backward at 40 x 24, the new defaults against bin_count = 0 / blend_fwd_form = 0.  The forward is bit-equal, and
    so is everything the backward walks (test_chain_equality).  No gradient group is bit-reproducible even between two runs of ONE build:
    every one of them is summed by float atomics (the blending backward's per-Gaussian lines, the deformation backward's weight and plane
    gradients), whose order differs from run to run -- two knobs-off runs may agree on a group by chance and a third differ.  So every
    group is held to rel-L2 < 5e-6, the bound tests/test_gpu_raster.py applies to the same gradients between the binning paths and between
    the backward's forms (test_capacity_paths_equal_the_blocking_exact_path; tests/test_gpu_tile_sort.py compares no gradients), and what
    IS deterministic is compared exactly: a row of a gradient is all zero with the knobs on if and only if it is with them off."""
    fdgs = importlib.import_module("4dgaussians_amd")
    syn = fdgs.synthetic
    dev = _dev()
    cam = syn.make_camera(40, 24, theta_deg=25.0, time=0.3).to(dev)
    wimg = torch.tensor(np.random.default_rng(9).standard_normal((3, 24, 40)).astype(np.float32), device=dev)

    def run(**knobs):
        for k, v in knobs.items():
            set_knob(k, v)
        pc = syn.SynthModel(600, "dynerf_default", seed=3)
        with torch.no_grad():
            pc._scaling.add_(1.0)
        pc = pc.to(dev)
        res = fdgs.render(cam, pc, syn.PipelineParams(), torch.zeros(3, device=dev), stage="fine")
        (res["render"] * wimg).sum().backward()
        torch.cuda.synchronize()
        g = {k: v.grad.cpu().numpy() for k, v in pc.named_parameters() if v.grad is not None}
        g["viewspace"] = res["viewspace_points"].grad.cpu().numpy()
        return res["render"].detach().cpu().numpy(), res["depth"].detach().cpu().numpy(), g

    run(bin_count=0, blend_fwd_form=0)                                          # (the first frame of a shape takes the staged path)
    a1 = run(bin_count=0, blend_fwd_form=0)
    tune = importlib.import_module("4dgaussians_amd._lib")
    tune.lib().fdgs_tuning_reset()
    b = run()
    assert np.array_equal(a1[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a1[1].view(np.uint32), b[1].view(np.uint32))
    assert a1[2].keys() == b[2].keys() and len(b[2]) > 3
    for k in a1[2]:
        assert rel_l2(b[2][k], a1[2][k]) < 5e-6, (k, rel_l2(b[2][k], a1[2][k]))
        if a1[2][k].ndim > 1:
            rows = lambda g: (g.reshape(len(g), -1) != 0).any(axis=1)
            assert np.array_equal(rows(a1[2][k]), rows(b[2][k])), k
