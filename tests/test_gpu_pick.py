"""The pick pass on the device (csrc/render.hip: render_pick_kernel, fdgs_render_pick; render_pick of fdgs.playback / fdgs.compose).

Every comparison at the C level is EXACT, and the expected values come from the device's own forward blend: with a one-hot row in recC
(include/fdgs.h at fdgs_geom_field: recC may be rewritten between two fdgs_render_fwd calls of a forward-only frame) and a zero background
a colour plane of a second fdgs_render_fwd is the map of ONE Gaussian's blend weight w = alpha * T, bit for bit -- 1 * w is exact, 0 * w is
+0 and adding +0 is exact.  From those maps and the frame's own sorted lists numpy restates the pass: the first argmax of w over a tile's
list, the sequential float32 running sum of w in list order, the first entry at which that sum reaches alpha_cut.  The pick kernel evaluates
w with the forward's expressions and adds it without contraction, so ids compare with array_equal and weights and depths on their bits."""
import ctypes
import functools
import importlib
import types

import numpy as np
import pytest
import torch

from scenes import raster_scene
from test_gpu_motion import KEYS, KINDS, _frame_at, _object, _pipe, _same
from test_gpu_playback import _cam, _dev

pytestmark = pytest.mark.gpu
fdgs = importlib.import_module("4dgaussians_amd")
C, P, R, syn = fdgs.compose, fdgs.playback, fdgs.rasterizer, fdgs.synthetic
L = fdgs._lib
TILE = 16
GUARD = 64                       # sentinel words in front of and behind every output plane
SENTINEL = -123456789
PICK_KEYS = ("pick_id", "pick_weight", "surface_id", "surface_depth")
CUTS = (0.5, 1.0 / 255.0, 1.0)
# scene -> (Gaussians, W, H, seed, scale_boost, opacity scale).  (a): 3 x 3 tiles with partial tiles on both edges, splats small enough to
# leave pixels empty and pixels thinly covered.  (b): 3 x 2 tiles whose lists are longer than 256 and 512 entries; the opacities are
# scaled down so that a pixel's blend does not saturate after a few dozen entries and the WALK goes as far as the lists do: the staging
# pipeline runs two rounds in two of the tiles and three in the others.  _check_conditions asserts all of that about the device's own
# frame: a seed that misses a condition fails there instead of testing nothing.
SCENES = {"a": (48, 40, 36, 1, 0.4, 1.0), "b": (600, 33, 17, 1, 4.0, 0.12)}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _view(buf, ptr, count, dtype):
    """`count` elements of `dtype` at the device address `ptr` inside the uint8 tensor `buf`, as a tensor view (reads and writes go to the buffer)."""
    off = ptr.value - buf.data_ptr()
    nbytes = count * torch.empty(0, dtype=dtype).element_size()
    assert 0 <= off and off + nbytes <= buf.numel()
    return buf[off:off + nbytes].view(dtype)


def _geom(state, which, count, dtype):
    q = ctypes.c_void_p()
    L.check(L.lib().fdgs_geom_field(L.ptr(state.geom), state.params.P, which, q))
    return _view(state.geom, q, count, dtype)


def _img(state, which, count, dtype):
    q = ctypes.c_void_p()
    L.check(L.lib().fdgs_img_field(L.ptr(state.img), state.params.W, state.params.H, which, q))
    return _view(state.img, q, count, dtype)


def _pairs(state, which):
    q = ctypes.c_void_p()
    L.check(L.lib().fdgs_binning_field(L.ptr(state.binning), state.capacity, state.params.W, state.params.H, which, q))
    return _view(state.binning, q, max(state.capacity, 1), torch.int32)


def _blend_again(fr, bg):
    """fdgs_render_fwd once more over the frame's own buffers, background `bg` -> (colour, depth)."""
    st = fr.state
    p2 = L.RasterParams.from_buffer_copy(st.params)
    p2.bg, p2.acc_zero = L.ptr(bg), None
    color, depth = torch.empty(3, fr.h, fr.w, device=_dev()), torch.empty(1, fr.h, fr.w, device=_dev())
    L.check(L.lib().fdgs_render_fwd(L.stream_ptr(), p2, L.ptr(st.geom), L.ptr(st.binning), L.ptr(st.img), st.capacity, L.ptr(color), L.ptr(depth)))
    return color, depth


def _forward(name, n, w, h, seed, boost, opacity_scale):
    """The forward-only frame of a scene and what numpy needs of its lists."""
    dev = _dev()
    sc = raster_scene(n, w, h, seed=seed, scale_boost=boost)
    sc["opacities"] = (sc["opacities"] * np.float32(opacity_scale)).astype(np.float32)
    t = {k: torch.tensor(sc[k], device=dev) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    settings = R.GaussianRasterizationSettings(
        image_height=h, image_width=w, tanfovx=sc["tanfovx"], tanfovy=sc["tanfovy"], bg=torch.tensor(sc["bg"], device=dev), scale_modifier=1.0,
        viewmatrix=torch.tensor(sc["viewmatrix"], device=dev), projmatrix=torch.tensor(sc["projmatrix"], device=dev), sh_degree=sc["sh_degree"],
        campos=torch.tensor(sc["campos"], device=dev), prefiltered=False, debug=False)
    with torch.no_grad():
        color, radii, depth, state = R.rasterize_forward(settings, t["means3D"], t["shs"], None, t["opacities"], t["scales"], t["rotations"], None,
                                                         expect_backward=False)
    fr = types.SimpleNamespace(name=name, n=n, w=w, h=h, sc=sc, state=state, color=color, depth=depth, radii=radii, keep=(t, settings))
    fr.gx, fr.gy = (w + TILE - 1) // TILE, (h + TILE - 1) // TILE
    fr.bg = torch.tensor(sc["bg"], device=dev)
    torch.cuda.synchronize()
    fr.ranges = _img(state, 2, 2 * fr.gx * fr.gy, torch.int32).view(-1, 2).cpu().numpy().astype(np.int64)
    fr.n_contrib = _img(state, 1, h * w, torch.int32).view(h, w).cpu().numpy().astype(np.int64)
    fr.walk = _img(state, 3, fr.gx * fr.gy, torch.int32).cpu().numpy().astype(np.int64)
    fr.gid = _pairs(state, 0).cpu().numpy().astype(np.int64)
    fr.zdepth = _geom(state, 2, 4 * n, torch.float32).view(n, 4)[:, 2].cpu().numpy().copy()
    assert state.num_rendered <= state.capacity and int(fr.ranges.max()) == state.num_rendered
    return fr


@functools.lru_cache(maxsize=None)
def _frame(name):
    """The frame of SCENES[name] with the per-Gaussian w maps of its blend: computed once, shared by every test, never modified (the
    frame's recC is put back after the one-hot passes)."""
    fr = _forward(name, *SCENES[name])
    n, w, h, state, dev = fr.n, fr.w, fr.h, fr.state, _dev()
    recC = _geom(state, 3, 4 * n, torch.float32).view(n, 4)
    saved = recC.clone()
    zero = torch.zeros(3, device=dev)
    wmaps = torch.empty(n + 2, h, w, device=dev)
    lane = torch.arange(3, device=dev)
    for g0 in range(0, n, 3):                                    # one blend per three Gaussians: plane k is the w map of Gaussian g0 + k
        k = min(3, n - g0)
        recC.zero_()
        recC[g0 + lane[:k], lane[:k]] = 1.0
        wmaps[g0:g0 + 3] = _blend_again(fr, zero)[0]
    recC.copy_(saved)
    torch.cuda.synchronize()
    fr.wmaps = wmaps[:n].cpu().numpy()
    return fr


@functools.lru_cache(maxsize=None)
def _expected(name, cut):
    """(pick_id, pick_weight, surface_id, surface_depth, A) [h, w] restated in numpy from the w maps and the lists."""
    fr = _frame(name)
    cut = np.float32(cut)
    pick_id, surf_id = np.full((fr.h, fr.w), -1, np.int32), np.full((fr.h, fr.w), -1, np.int32)
    pick_w, surf_d, total = np.zeros((fr.h, fr.w), np.float32), np.zeros((fr.h, fr.w), np.float32), np.zeros((fr.h, fr.w), np.float32)
    for tile in range(fr.gx * fr.gy):
        lo, hi = fr.ranges[tile]
        y0, x0 = (tile // fr.gx) * TILE, (tile % fr.gx) * TILE
        ys, xs = slice(y0, min(y0 + TILE, fr.h)), slice(x0, min(x0 + TILE, fr.w))
        if hi == lo:
            continue
        ids = fr.gid[lo:hi]
        wl = fr.wmaps[ids][:, ys, xs]                            # [list, rows, cols] in list order
        assert wl.dtype == np.float32
        first = wl.argmax(axis=0)                                # numpy: the first of equal maxima
        best = np.take_along_axis(wl, first[None], 0)[0]
        hit = best > 0
        pick_id[ys, xs] = np.where(hit, ids[first], -1)
        pick_w[ys, xs] = np.where(hit, best, np.float32(0))
        run = np.add.accumulate(wl, axis=0, dtype=np.float32)    # sequential float32 sums in list order
        over = run >= cut
        at = over.argmax(axis=0)
        got = over.any(axis=0)
        surf_id[ys, xs] = np.where(got, ids[at], -1)
        surf_d[ys, xs] = np.where(got, fr.zdepth[ids[at]], np.float32(0))
        total[ys, xs] = run[-1]
    return pick_id, pick_w, surf_id, surf_d, total


def _pick(fr, cut, row_map=None, only=None):
    """fdgs_render_pick on the frame -> {name: [h, w] numpy} of the outputs asked for (`only`: one name, the others NULL); every output
    sits between GUARD sentinel words, which must survive."""
    dev, hw = _dev(), fr.h * fr.w
    names = PICK_KEYS if only is None else (only,)
    bufs = {k: torch.full((hw + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev) for k in names}
    out = L.PickOut()
    for k in names:
        setattr(out, k, bufs[k].data_ptr() + 4 * GUARD)
    st = fr.state
    L.check(L.lib().fdgs_render_pick(L.stream_ptr(), st.params, L.ptr(st.geom), L.ptr(st.binning), L.ptr(st.img), st.capacity, float(cut),
                                     L.ptr(row_map), out))
    torch.cuda.synchronize()
    res = {}
    for k in names:
        a = bufs[k].cpu().numpy()
        assert (a[:GUARD] == SENTINEL).all() and (a[GUARD + hw:] == SENTINEL).all(), k
        body = a[GUARD:GUARD + hw].reshape(fr.h, fr.w)
        res[k] = body if k.endswith("_id") else body.view(np.float32)
    return res


def _assert_matches(got, want, what):
    pick_id, pick_w, surf_id, surf_d, _ = want
    if "pick_id" in got:
        assert np.array_equal(got["pick_id"], pick_id), what
    if "pick_weight" in got:
        assert np.array_equal(bits(got["pick_weight"]), bits(pick_w)), what
    if "surface_id" in got:
        assert np.array_equal(got["surface_id"], surf_id), what
    if "surface_depth" in got:
        assert np.array_equal(bits(got["surface_depth"]), bits(surf_d)), what


def _check_conditions(fr):
    """What the scene must contain for the comparisons to mean something."""
    pick_id, _, surf_id, _, _ = _expected(fr.name, 0.5)
    lengths = fr.ranges[:, 1] - fr.ranges[:, 0]
    per_pixel = np.repeat(np.repeat(lengths.reshape(fr.gy, fr.gx), TILE, 0), TILE, 1)[:fr.h, :fr.w]
    stats = dict(nothing=int(((pick_id == -1) & (surf_id == -1)).sum()), thin=int(((pick_id >= 0) & (surf_id == -1)).sum()),
                 differ=int(((pick_id >= 0) & (surf_id >= 0) & (pick_id != surf_id)).sum()), longest=int(lengths.max()),
                 stopped_early=int((fr.n_contrib < per_pixel).sum()), visible=int((fr.radii > 0).sum()), lengths=lengths.tolist(),
                 walk=fr.walk.tolist())
    print(f"scene {fr.name}: {stats}")
    assert (pick_id == -1).sum() == ((pick_id == -1) & (surf_id == -1)).sum()       # no pick: no surface either
    assert stats["differ"] > 0 and stats["stopped_early"] > 0, stats
    assert np.array_equal(fr.walk, [fr.n_contrib[(t // fr.gx) * TILE:(t // fr.gx + 1) * TILE, (t % fr.gx) * TILE:(t % fr.gx + 1) * TILE].max()
                                    for t in range(fr.gx * fr.gy)])
    if fr.name == "b":       # lists of more than 512 entries, walked for three rounds; and a tile whose walk ends in its second round
        assert fr.gx == 3 and fr.gy == 2 and stats["longest"] > 512 and int(fr.walk.max()) > 512, stats
        assert bool(((fr.walk > 256) & (fr.walk <= 512)).any()), stats
    else:                    # partial tiles on both edges; empty pixels; pixels whose accumulated alpha stays below the cut
        assert fr.gx == 3 and fr.gy == 3 and fr.w % TILE and fr.h % TILE
        assert stats["nothing"] > 0 and stats["thin"] > 0, stats


@pytest.mark.parametrize("cut", CUTS, ids=["median", "first_contributor", "opaque"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_pick_equals_the_numpy_restatement_of_the_forward_blend(name, cut):
    fr = _frame(name)
    _check_conditions(fr)
    want = _expected(name, cut)
    got = _pick(fr, cut)
    _assert_matches(got, want, (name, cut))
    pick_id, pick_w, surf_id, surf_d, total = want
    assert (pick_id >= 0).sum() > 0 and np.array_equal(surf_id[pick_id == -1], np.full(int((pick_id == -1).sum()), -1))
    if cut == 1.0:                                               # no surface wherever the accumulated alpha stays below 1
        assert np.array_equal(got["surface_id"] == -1, total < np.float32(1.0))
    if cut == CUTS[1]:                                           # alpha >= 1/255 and T = 1: the first contributor is the surface
        assert np.array_equal(got["surface_id"] >= 0, got["pick_id"] >= 0)
    assert np.array_equal(bits(got["surface_depth"][got["surface_id"] == -1]), np.zeros(int((got["surface_id"] == -1).sum()), np.uint32))
    assert np.array_equal(bits(got["pick_weight"][got["pick_id"] == -1]), np.zeros(int((got["pick_id"] == -1).sum()), np.uint32))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_row_map_is_applied_to_the_ids_and_to_nothing_else(name):
    fr = _frame(name)
    plain = _pick(fr, 0.5)
    perm = np.random.default_rng(11).permutation(fr.n).astype(np.int32)
    mapped = _pick(fr, 0.5, row_map=torch.from_numpy(perm).to(_dev()))
    for k in ("pick_id", "surface_id"):
        assert np.array_equal(mapped[k], np.where(plain[k] >= 0, perm[np.maximum(plain[k], 0)], -1)), k
        assert (mapped[k] != plain[k]).any()
    for k in ("pick_weight", "surface_depth"):
        assert np.array_equal(bits(mapped[k]), bits(plain[k])), k


@pytest.mark.parametrize("name", sorted(SCENES))
def test_each_output_alone_equals_its_plane_of_the_full_call(name):
    fr = _frame(name)
    full = _pick(fr, 0.5)
    for k in PICK_KEYS:
        alone = _pick(fr, 0.5, only=k)
        assert list(alone) == [k] and np.array_equal(bits(alone[k]), bits(full[k])), k


@pytest.mark.parametrize("name", sorted(SCENES))
def test_nothing_of_the_frame_is_written(name):
    fr = _frame(name)
    st, n, hw, tiles = fr.state, fr.n, fr.h * fr.w, fr.gx * fr.gy
    per_xcd = ((((fr.gy + 1) // 2) + 7) // 8) * 2 * fr.gx
    fields = {"final_T": lambda: _img(st, 0, hw, torch.int32), "n_contrib": lambda: _img(st, 1, hw, torch.int32),
              "ranges": lambda: _img(st, 2, 2 * tiles, torch.int32), "walk": lambda: _img(st, 3, tiles, torch.int32),
              "order_f": lambda: _img(st, 4, 8 * per_xcd, torch.int32), "order_b": lambda: _img(st, 5, 8 * per_xcd, torch.int32),
              "recA": lambda: _geom(st, 1, 4 * n, torch.int32), "recB": lambda: _geom(st, 2, 4 * n, torch.int32),
              "recC": lambda: _geom(st, 3, 4 * n, torch.int32), "pair_gid": lambda: _pairs(st, 0), "pair_tile": lambda: _pairs(st, 1),
              "geom": lambda: st.geom, "binning": lambda: st.binning, "img": lambda: st.img}
    before = {k: f().clone() for k, f in fields.items()}
    torch.cuda.synchronize()
    for cut in CUTS:
        _pick(fr, cut)
    for k, f in fields.items():
        assert torch.equal(f(), before[k]), k
    color, depth = _blend_again(fr, fr.bg)                       # the frame's blend once more: the image and the depth it returned before
    assert torch.equal(color, fr.color) and torch.equal(depth, fr.depth)
    _assert_matches(_pick(fr, 0.5), _expected(name, 0.5), name)   # ... and a pick after that blend: still the same


def test_an_empty_frame_gets_minus_one_and_zero_everywhere():
    """P > 0 with num_rendered == 0 (every Gaussian behind the camera) and P == 0: one launch that reads nothing of the frame."""
    dev = _dev()
    sc = _frame("a").sc
    for n in (5, 0):
        xyz = torch.tensor(sc["campos"], device=dev).repeat(n, 1)                    # at the camera's centre: culled by the near plane
        t, settings = _frame("a").keep
        with torch.no_grad():
            *_, state = R.rasterize_forward(settings, xyz, t["shs"][:n], None, t["opacities"][:n], t["scales"][:n], t["rotations"][:n], None,
                                            expect_backward=False)
        assert state.num_rendered == 0 and state.capacity == 0
        fr = types.SimpleNamespace(h=sc["image_height"], w=sc["image_width"], state=state)
        got = _pick(fr, 0.5)
        assert (got["pick_id"] == -1).all() and (got["surface_id"] == -1).all()
        assert not bits(got["pick_weight"]).any() and not bits(got["surface_depth"]).any()


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------

def _row_depths(obj, t, cam):
    """View depth of every row of the state at time t, in the row order "radii" uses: the four-term float32 dot product in torch."""
    xyz = _frame_at(obj, t).xyz
    if obj._maps[1] is not None:
        xyz = obj._maps[1](xyz.contiguous())
    v = cam.world_view_transform.to(xyz.device).float()
    return xyz[:, 0] * v[0, 2] + xyz[:, 1] * v[1, 2] + xyz[:, 2] * v[2, 2] + v[3, 2]


def _expected_row_map(obj):
    if isinstance(obj, C.Composite):
        if all(m.perm is None for m in obj.models):
            return None
        return torch.cat([(torch.arange(m.N, device=_dev(), dtype=torch.int32) if m.perm is None else m.perm.to(torch.int32)) + o
                          for m, o in zip(obj.models, obj.offsets)])
    return None if obj.perm is None else obj.perm.to(torch.int32)


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k if isinstance(k, str) else "-".join(str(v) for v in k))
def test_render_pick_is_render_plus_what_is_under_every_pixel(kind):
    """One frame at a baked time and one in between.  surface_depth against the view depth of row surface_id within 1e-5 relative: the depth
    is a four-term float32 dot product, a few ulp (6e-8 each) between the kernel's and torch's evaluation, and 1e-5 leaves a factor of
    about 20 over that; a wrong row of these random scenes is off at the 1e-3 scale.  Pixels whose pick and surface rows lie closer than
    1e-5 relative in depth could hide a swap of the two and are counted and printed."""
    obj = _object(kind)
    bg, pipe = torch.tensor([0.1, 0.2, 0.3], device=_dev()), _pipe()
    for k, t in ((0, 0.25), (1, 0.375)):
        cam = _cam(k, t)
        before = obj.render(cam, pipe, bg, rgb8="trunc")
        got = obj.render_pick(cam, pipe, bg, rgb8="trunc")
        after = obj.render(cam, pipe, bg, rgb8="trunc")
        assert set(got) == set(before) | set(PICK_KEYS) and got["viewspace_points"] is None
        _same(got, before, KEYS + ("rgb8",))
        _same(after, before, KEYS + ("rgb8",))
        h, w = before["depth"].shape[1:]
        assert got["pick_id"].shape == got["surface_id"].shape == got["pick_weight"].shape == (h, w) and got["surface_depth"].shape == (1, h, w)
        assert got["pick_id"].dtype == got["surface_id"].dtype == torch.int32
        assert got["pick_weight"].dtype == got["surface_depth"].dtype == torch.float32
        want_map = _expected_row_map(obj)
        assert (obj._pick_row_map is None) == (want_map is None)
        if want_map is not None:
            assert obj._pick_row_map.dtype == torch.int32 and torch.equal(obj._pick_row_map, want_map)
        pick, surf = got["pick_id"].long(), got["surface_id"].long()
        assert int(pick.max()) < obj.N and int(surf.max()) < obj.N and int(pick.min()) >= -1 and int(surf.min()) >= -1
        assert int((pick >= 0).sum()) > 100 and int((surf >= 0).sum()) > 100          # (these scenes cover nearly every pixel)
        assert bool((got["radii"][pick[pick >= 0]] > 0).all()) and bool((got["radii"][surf[surf >= 0]] > 0).all())
        assert bool((surf[pick == -1] == -1).all()) and bool((got["pick_weight"][pick >= 0] > 0).all())
        assert not bool(got["pick_weight"][pick == -1].any()) and not bool(got["surface_depth"][0][surf == -1].any())
        z = _row_depths(obj, t, cam)
        on = surf >= 0
        zs, zd = z[surf[on]], got["surface_depth"][0][on]
        rel = float(((zd - zs).abs() / zs.abs()).max())
        both = on & (pick >= 0) & (pick != surf)
        close = int((((z[pick[both]] - z[surf[both]]).abs() / z[surf[both]].abs()) < 1e-5).sum())
        print(f"{kind} t={t}: max rel |surface_depth - depth of row surface_id| = {rel:.3e}; {int(both.sum())} pixels with two rows, "
              f"{close} of them closer than 1e-5 in depth")
        assert rel < 1e-5
        if isinstance(obj, C.Composite):
            for ids in (got["pick_id"], got["surface_id"]):
                model, row = obj.model_of_rows(ids)
                assert model.dtype == row.dtype == torch.int32 and model.shape == row.shape == ids.shape
                for m, sl in enumerate(obj.slices):
                    inside = (ids >= sl.start) & (ids < sl.stop)
                    assert torch.equal(model == m, inside) and torch.equal(row[inside], ids[inside] - sl.start)
                assert torch.equal(model == -1, ids == -1) and torch.equal(row == -1, ids == -1)
            print(f"composite t={t}: models picked {obj.model_of_rows(got['pick_id'])[0].unique().tolist()}, "
                  f"models at the surface {obj.model_of_rows(got['surface_id'])[0].unique().tolist()}")


def test_alpha_cut_moves_the_surface_and_not_the_pick():
    obj = _object(KINDS[1])
    bg, pipe, cam = torch.zeros(3, device=_dev()), _pipe(), _cam(0, 0.25)
    low, mid, high = (obj.render_pick(cam, pipe, bg, alpha_cut=c) for c in (1.0 / 255.0, 0.5, 1.0))
    for other in (low, high):
        assert torch.equal(other["pick_id"], mid["pick_id"]) and torch.equal(other["pick_weight"], mid["pick_weight"])
    assert torch.equal(low["surface_id"] >= 0, low["pick_id"] >= 0)
    on = mid["surface_id"] >= 0
    assert bool((low["surface_depth"][0][on] <= mid["surface_depth"][0][on]).all())          # lists are sorted by depth, front first
    assert int((high["surface_id"] >= 0).sum()) <= int(on.sum()) <= int((low["surface_id"] >= 0).sum())
    assert bool((low["surface_depth"][0][on] < mid["surface_depth"][0][on]).any())            # ... and the cut does move it


def test_unproject_returns_the_positions_of_the_visible_gaussians():
    """Scene (a): the projection kernel's pixel position (recA.xy) and view depth (recB.z) of every visible Gaussian, unprojected, against its
    position.  Float32 chain, u = 2**-24, |p_view| < 8 in this scene (asserted): the kernel's pixel carries ~4 roundings of a value <= 40
    pixels, i.e. <= 1e-5 pixel, which is 1e-5 * 2 * tan * z / W < 1e-6 in view space; the depth one rounding, u * z; unproject itself is
    ~10 operations on values <= |p_view| and a 4 x 4 inverse of an orthonormal matrix (entries exact to ~2 u): together below
    32 u * 8 = 1.5e-5 absolute.  A half-pixel slip in the convention would move a point by z * tan / W ~ 3e-2."""
    fr = _frame("a")
    cam = syn.make_camera(fr.w, fr.h, theta_deg=30.0, time=0.0)
    assert np.array_equal(np.asarray(cam.world_view_transform, np.float32), fr.sc["viewmatrix"])
    vis = (fr.radii > 0).cpu()
    recA = _geom(fr.state, 1, 4 * fr.n, torch.float32).view(fr.n, 4)
    recB = _geom(fr.state, 2, 4 * fr.n, torch.float32).view(fr.n, 4)
    xy, z = recA[:, :2][vis.to(_dev())], recB[:, 2][vis.to(_dev())]
    got = P.unproject(cam, xy, z)
    want = torch.tensor(fr.sc["means3D"])[vis].to(_dev())
    assert got.device == z.device and got.shape == want.shape and int(vis.sum()) >= 16
    assert float(z.max()) < 8.0 and float(want.abs().max()) < 8.0
    err = float((got - want).abs().max())
    print(f"unproject of {int(vis.sum())} visible Gaussians: max |dp| = {err:.3e}")
    assert err < 1.5e-5
