"""The contribution pass on the device (csrc/render.hip: render_contrib_kernel, fdgs_render_contrib; render_contrib of fdgs.playback /
fdgs.compose; Baked.select_rows).

At the C level the expected values come from the device's own forward blend, the per-Gaussian w maps of tests/test_gpu_pick.py (a one-hot
recC pass per three Gaussians: plane k is ONE Gaussian's blend weight w = alpha * T, bit for bit).  With v = float32(w * m) per pixel
(m = 1 without a pixel weight) and every !(v > 0) dropped: pixels = count_nonzero(v), weight_max = max(v), tiles = the 16 x 16 tiles with
any v > 0 -- all three EXACT, the maximum on its bits -- and weight_sum against the float64 sum of v.

The bound on weight_sum: any order of float32 additions of n non-negative terms errs by at most (n - 1) * 2**-24 relative to first order;
the tests allow (pixels_g + 1) * 2**-23, twice that.  A wrong or dropped term is off by at least one w >= (1/255) * 1e-4."""
import importlib

import numpy as np
import pytest
import torch

from test_gpu_motion import KEYS, KINDS, _frame_at, _object, _pipe, _same
from test_gpu_pick import SCENES, TILE, _expected_row_map, _frame, _geom, _img, _pairs, bits
from test_gpu_playback import _baked, _cam, _dev

pytestmark = pytest.mark.gpu
fdgs = importlib.import_module("4dgaussians_amd")
C, P, R, syn = fdgs.compose, fdgs.playback, fdgs.rasterizer, fdgs.synthetic
L = fdgs._lib
GUARD = 64                       # sentinel words (16 records) in front of and behind `rows`: the array stays 16-byte aligned
SENTINEL = -123456789
U23 = 2.0 ** -23


def _contrib_state(state, n, weight=None, row_map=None, passes=1, rows=None):
    """`passes` x fdgs_render_contrib over `state` into zeroed rows (or the int32 [n,4] numpy `rows`) -> dict of numpy columns; the
    sentinel words around the array must survive."""
    dev = _dev()
    buf = torch.full((4 * n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    body = buf[GUARD:GUARD + 4 * n]
    body.copy_(torch.zeros(4 * n, dtype=torch.int32) if rows is None else torch.from_numpy(rows.reshape(-1)))
    assert (buf.data_ptr() + 4 * GUARD) % 16 == 0
    for _ in range(passes):
        L.check(L.lib().fdgs_render_contrib(L.stream_ptr(), state.params, L.ptr(state.geom), L.ptr(state.binning), L.ptr(state.img),
                                            state.capacity, L.ptr(weight), L.ptr(row_map), buf.data_ptr() + 4 * GUARD))
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    assert (a[:GUARD] == SENTINEL).all() and (a[GUARD + 4 * n:] == SENTINEL).all()
    return _columns(a[GUARD:GUARD + 4 * n].reshape(n, 4))


def _columns(raw):
    raw = np.ascontiguousarray(raw)
    return dict(weight_sum=raw[:, 0].copy().view(np.float32), weight_max=raw[:, 1].copy().view(np.float32), pixels=raw[:, 2].copy(),
                tiles=raw[:, 3].copy(), raw=raw)


def _contrib(fr, weight=None, **kw):
    w = None if weight is None else torch.from_numpy(np.ascontiguousarray(weight, np.float32).reshape(-1)).to(_dev())
    return _contrib_state(fr.state, fr.n, weight=w, **kw)


def _expected(fr, weight=None):
    """The statistics restated from the w maps: v = float32(w * m), !(v > 0) dropped."""
    v = fr.wmaps if weight is None else fr.wmaps * np.asarray(weight, np.float32)[None]          # float32 x float32: ONE rounded product
    assert v.dtype == np.float32
    with np.errstate(invalid="ignore"):
        hit = v > 0                                                                                  # (False for NaN, zero, negative)
    v = np.where(hit, v, np.float32(0))
    n = fr.n
    pad = np.zeros((n, fr.gy * TILE, fr.gx * TILE), bool)
    pad[:, :fr.h, :fr.w] = hit
    per_tile = pad.reshape(n, fr.gy, TILE, fr.gx, TILE).any(axis=(2, 4))                             # [n, gy, gx]
    return dict(pixels=hit.reshape(n, -1).sum(1).astype(np.int32), weight_max=v.reshape(n, -1).max(1),
                tiles=per_tile.reshape(n, -1).sum(1).astype(np.int32), weight_sum=v.reshape(n, -1).astype(np.float64).sum(1), hit=hit)


def _assert_matches(got, want, what, times=1):
    assert np.array_equal(got["pixels"], times * want["pixels"]), what
    assert np.array_equal(got["tiles"], times * want["tiles"]), what
    assert np.array_equal(bits(got["weight_max"]), bits(want["weight_max"])), what
    exact = times * want["weight_sum"]
    err = np.abs(got["weight_sum"].astype(np.float64) - exact)
    bound = (times * want["pixels"] + 1) * U23 * exact
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: weight_sum worst error / bound = {worst:.3f}; rows with pixels: {int((want['pixels'] > 0).sum())}")
    assert (err <= bound).all(), what
    assert not bits(got["weight_sum"][want["pixels"] == 0]).any(), what                             # untouched records stay all-zero


def _check_conditions(fr, want):
    """What the scene must contain for the comparisons to mean something: a seed that misses a condition fails here."""
    assert int((want["tiles"] >= 2).sum()) > 0, "no row is blended in two or more tiles"
    assert int((want["pixels"] == 0).sum()) > 0 and int((want["pixels"] > 0).sum()) > 0
    assert fr.w % TILE and fr.h % TILE                                                               # partial tiles on both edges
    if fr.name == "b":       # an entry staged in the second or third round of its tile that was blended into a pixel of that tile
        late = 0
        for tile in range(fr.gx * fr.gy):
            lo, hi = fr.ranges[tile]
            y0, x0 = (tile // fr.gx) * TILE, (tile % fr.gx) * TILE
            for pos in range(256, int(hi - lo)):
                late += bool(want["hit"][fr.gid[lo + pos], y0:y0 + TILE, x0:x0 + TILE].any())
        lengths = fr.ranges[:, 1] - fr.ranges[:, 0]
        print(f"scene b: {late} (tile, entry) pairs of staging rounds 2 and 3 with pixels > 0; list lengths {lengths.tolist()}")
        assert late > 0 and int(lengths.max()) > 512 and int(fr.walk.max()) > 512


@pytest.mark.parametrize("name", sorted(SCENES))
def test_contrib_equals_the_statistics_of_the_forward_blend_weights(name):
    fr = _frame(name)
    want = _expected(fr)
    _check_conditions(fr, want)
    _assert_matches(_contrib(fr), want, name)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_two_passes_accumulate(name):
    """Two calls into the same rows: pixels and tiles double, weight_max stays, weight_sum is the sum of twice as many terms; rows that
    start from other values keep them under the sums and under a smaller maximum."""
    fr = _frame(name)
    want = _expected(fr)
    _assert_matches(_contrib(fr, passes=2), want, (name, "two passes"), times=2)
    start = np.zeros((fr.n, 4), np.int32)
    start[:, 2], start[:, 3] = 1000, 7
    old = np.float32(np.median(want["weight_max"][want["pixels"] > 0]))                               # an old maximum in the middle of the new ones
    start[:, 1] = old.view(np.int32)
    got = _contrib(fr, rows=start)
    assert np.array_equal(got["pixels"], want["pixels"] + 1000) and np.array_equal(got["tiles"], want["tiles"] + 7)
    assert np.array_equal(bits(got["weight_max"]), bits(np.maximum(want["weight_max"], old)))
    assert (want["weight_max"] > old).any() and (want["weight_max"] < old).any()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_row_map_chooses_the_record(name):
    fr = _frame(name)
    want = _expected(fr)
    perm = np.random.default_rng(11).permutation(fr.n).astype(np.int32)
    got = _contrib(fr, row_map=torch.from_numpy(perm).to(_dev()))
    inv = np.argsort(perm)                                                                           # record r holds Gaussian inv[r]
    _assert_matches(got, {k: v[inv] for k, v in want.items() if k != "hit"}, (name, "row map"))
    assert (got["pixels"] != want["pixels"]).any()
    # ids the map sends outside [0, P) are dropped: nothing but the records of the others is written (the sentinels are checked inside)
    holes = perm.copy()
    holes[::3], holes[1::3] = -1, fr.n
    got = _contrib(fr, row_map=torch.from_numpy(holes).to(_dev()))
    kept = np.zeros(fr.n, np.int32)
    kept[holes[2::3]] = want["pixels"][2::3]
    assert np.array_equal(got["pixels"], kept)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_a_mask_of_the_left_half_cuts_through_tiles(name):
    fr = _frame(name)
    cut = (fr.w + 1) // 2
    assert cut % TILE                                                                                # the edge lies inside a tile column
    mask = np.zeros((fr.h, fr.w), np.float32)
    mask[:, :cut] = 1.0
    want = _expected(fr, mask)
    full = _expected(fr)
    assert (want["pixels"] < full["pixels"]).any() and (want["tiles"] < full["tiles"]).any() and (want["pixels"] > 0).any()
    _assert_matches(_contrib(fr, mask), want, (name, "left half"))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_a_fractional_weight_with_zeros_a_negative_and_a_nan(name):
    fr = _frame(name)
    rng = np.random.default_rng(5)
    weight = rng.uniform(0.05, 1.5, (fr.h, fr.w)).astype(np.float32)
    weight[rng.uniform(size=weight.shape) < 0.2] = 0.0
    seen = np.argwhere(_expected(fr)["hit"].any(0))                                                  # pixels that blend something
    (ya, xa), (yb, xb), (yc, xc) = seen[len(seen) // 3], seen[len(seen) // 2], seen[2 * len(seen) // 3]
    weight[ya, xa], weight[yb, xb], weight[yc, xc] = -0.5, np.nan, -0.0
    want = _expected(fr, weight)
    assert (want["pixels"] > 0).any() and np.isfinite(want["weight_sum"]).all() and np.isfinite(want["weight_max"]).all()
    _assert_matches(_contrib(fr, weight), want, (name, "fractional"))


def test_an_empty_frame_leaves_rows_untouched():
    """P > 0 with num_rendered == 0 (every Gaussian behind the camera) and P == 0."""
    dev = _dev()
    sc = _frame("a").sc
    for n in (5, 0):
        xyz = torch.tensor(sc["campos"], device=dev).repeat(n, 1)                    # at the camera's centre: culled by the near plane
        t, settings = _frame("a").keep
        with torch.no_grad():
            *_, state = R.rasterize_forward(settings, xyz, t["shs"][:n], None, t["opacities"][:n], t["scales"][:n], t["rotations"][:n], None,
                                            expect_backward=False)
        assert state.num_rendered == 0 and state.capacity == 0
        start = np.arange(4 * 5, dtype=np.int32).reshape(5, 4) + 17
        got = _contrib_state(state, 5, rows=start)
        assert np.array_equal(got["raw"], start)


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
    _contrib(fr)
    _contrib(fr, np.full((fr.h, fr.w), 0.5, np.float32), row_map=torch.arange(n, dtype=torch.int32, device=_dev()))
    for k, f in fields.items():
        assert torch.equal(f(), before[k]), k


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------

def _state_of(obj, cam, bg, pipe):
    """The forward-only frame render_contrib makes, made by hand: (result dict, RasterState)."""
    with torch.no_grad():
        settings, t = fdgs.renderer._frame_settings(cam, None, bg, 1.0, obj.active_sh_degree, obj.device, pipe)
        return P._state_frame(_frame_at(obj, t), settings, *obj._maps, None, None)


def _close_sums(a, b, pixels, what):
    """Two float32 sums of the same `pixels` terms in two orders: each within (pixels + 1) * 2**-23 of the exact sum (the module docstring),
    so within twice that of each other."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    assert (np.abs(a - b) <= 2 * (pixels + 1) * U23 * np.maximum(a, b)).all(), what


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k if isinstance(k, str) else "-".join(str(v) for v in k))
def test_render_contrib_is_render_plus_the_rows_statistics(kind):
    """One frame at a baked time and one in between, accumulated into one Contribution; against the C call made by hand on the same state
    WITHOUT a row map, brought to model / scene order with the permutation in numpy."""
    obj = _object(kind)
    bg, pipe = torch.tensor([0.1, 0.2, 0.3], device=_dev()), _pipe()
    acc = None
    total = np.zeros((obj.N, 4), np.int64)
    sums = np.zeros(obj.N, np.float64)
    for k, t in ((0, 0.25), (1, 0.375)):
        cam = _cam(k, t)
        before = obj.render(cam, pipe, bg, rgb8="trunc")
        got = obj.render_contrib(cam, pipe, bg, into=acc, rgb8="trunc")
        after = obj.render(cam, pipe, bg, rgb8="trunc")
        assert set(got) == set(before) | {"contribution"} and got["viewspace_points"] is None
        _same(got, before, KEYS + ("rgb8",))
        _same(after, before, KEYS + ("rgb8",))                                                       # the state stays truthful
        acc = got["contribution"] if acc is None else acc
        assert got["contribution"] is acc and acc.frames == k + 1 and acc.N == obj.N and acc.rows.shape == (obj.N, 4)
        want_map = _expected_row_map(obj)
        assert (obj._pick_row_map is None) == (want_map is None)
        if want_map is not None:
            assert obj._pick_row_map.dtype == torch.int32 and torch.equal(obj._pick_row_map, want_map)
        out, state = _state_of(obj, cam, bg, pipe)
        _same(out, before, KEYS)
        stored = _contrib_state(state, obj.N)                                                        # stored order: no row map
        to_model = np.arange(obj.N) if want_map is None else want_map.cpu().numpy()
        one = {key: np.zeros_like(v) for key, v in stored.items() if key != "raw"}
        for key in one:
            one[key][to_model] = stored[key]
        one_acc = P.Contribution(obj.N, obj.device)
        frame = obj.render_contrib(cam, pipe, bg, into=one_acc)["contribution"]
        assert frame is one_acc and one_acc.frames == 1
        mine = _columns(one_acc.rows.cpu().numpy())
        assert np.array_equal(mine["pixels"], one["pixels"]) and np.array_equal(mine["tiles"], one["tiles"])
        assert np.array_equal(bits(mine["weight_max"]), bits(one["weight_max"]))
        _close_sums(mine["weight_sum"], one["weight_sum"], one["pixels"], (kind, t))
        radii = before["radii"].cpu().numpy()
        assert (radii[one["pixels"] > 0] > 0).all() and int((one["pixels"] > 0).sum()) > 100
        assert int(((radii > 0) & (one["pixels"] == 0)).sum()) > 0                                   # visible is not the same as blended
        assert (one["tiles"] <= one["pixels"]).all() and ((one["tiles"] > 0) == (one["pixels"] > 0)).all()
        assert (one["weight_max"] <= np.float32(0.99)).all() and (one["weight_sum"] >= one["weight_max"]).all()
        total[:, 2] += one["pixels"]
        total[:, 3] += one["tiles"]
        total[:, 1] = np.maximum(total[:, 1], bits(one["weight_max"]).astype(np.int64))
        sums += one["weight_sum"].astype(np.float64)
    both = _columns(acc.rows.cpu().numpy())
    assert np.array_equal(both["pixels"], total[:, 2]) and np.array_equal(both["tiles"], total[:, 3])
    assert np.array_equal(bits(both["weight_max"]).astype(np.int64), total[:, 1])
    _close_sums(both["weight_sum"], sums.astype(np.float32), total[:, 2], (kind, "two frames"))
    assert torch.equal(acc.keep_mask(), acc.pixels >= 1) and 0 < int(acc.keep_mask().sum()) < obj.N
    if isinstance(obj, C.Composite):                                                                 # scene rows: model m's at slices[m]
        model, row = obj.model_of_rows(torch.nonzero(acc.keep_mask()).reshape(-1).to(torch.int32))
        assert sorted(model.unique().tolist()) == [0, 1]
        for m, sl in enumerate(obj.slices):
            assert int((model == m).sum()) == int(acc.keep_mask()[sl].sum())


def test_a_pixel_weight_restricts_the_rows_to_a_region():
    obj = _object(KINDS[1])
    bg, pipe, cam = torch.zeros(3, device=_dev()), _pipe(), _cam(0, 0.25)
    h, w = 64, 96
    full = obj.render_contrib(cam, pipe, bg)["contribution"]
    lasso = torch.zeros(h, w, device=_dev())
    lasso[10:30, 20:50] = 1.0
    inside = obj.render_contrib(cam, pipe, bg, pixel_weight=lasso)["contribution"]
    outside = obj.render_contrib(cam, pipe, bg, pixel_weight=(1.0 - lasso).reshape(1, h, w))["contribution"]
    assert torch.equal(inside.pixels + outside.pixels, full.pixels) and 0 < int(inside.pixels.sum()) < int(full.pixels.sum())
    assert torch.equal(torch.maximum(inside.weight_max, outside.weight_max), full.weight_max)
    assert int((inside.pixels > 20 * 30).sum()) == 0
    pick = obj.render_pick(cam, pipe, bg)["pick_id"][10:30, 20:50]
    assert bool((inside.pixels[pick[pick >= 0].long()] > 0).all())                                   # what the pick shows there is among them
    for bad in (lasso[:, :-1], lasso.double(), lasso.cpu()):
        with pytest.raises(ValueError, match="pixel_weight"):
            obj.render_contrib(cam, pipe, bg, pixel_weight=bad)
    with pytest.raises(ValueError, match="into"):
        obj.render_contrib(cam, pipe, bg, into=P.Contribution(obj.N, torch.device("cpu")))


T_END = 0.01       # a pixel whose final transmittance is >= this was not ended early: the walk ends a pixel at the first entry with
#                    T * (1 - alpha) < 1e-4, and alpha <= 0.99, so the T it is left with is < 1e-4 / (1 - 0.99)


def _select_case(baked, cam, bg, pipe):
    """keep = the rows one view blends; the selection's frame of that view against the full bake's.  The entry that ENDS a saturated pixel
    (T * (1 - alpha) < 1e-4) is not blended, so a row that only ever ends pixels has pixels == 0, and without it those pixels go on to the
    next entry: bit-identity is asserted on the pixels the full frame did not end early, which is every pixel when `open_` is all True.
    -> (selection, its RasterState, open_ [H,W] bool)."""
    n = baked.N
    seen = P.contribution(baked, [cam], pipe, bg)
    keep = seen.keep_mask(min_pixels=1)
    assert seen.frames == 1 and 0 < int(keep.sum()) < n
    full, fstate = _state_of(baked, cam, bg, pipe)
    h, w = full["depth"].shape[1:]
    open_ = _img(fstate, 0, h * w, torch.float32).view(h, w).clone() >= T_END
    full = baked.render(cam, pipe, bg)
    small = baked.select_rows(keep)
    assert small.N == int(keep.sum()) and small.nbytes == P.bake_bytes(small.N, len(baked.times), baked.head_on) < baked.nbytes
    assert small.times == baked.times and small.head_on == baked.head_on and (small.perm is None) == (baked.perm is None)
    got = small.render(cam, pipe, bg)
    assert torch.equal(got["render"][:, open_], full["render"][:, open_]) and torch.equal(got["depth"][:, open_], full["depth"][:, open_])
    assert got["radii"].dtype == full["radii"].dtype and torch.equal(got["radii"], full["radii"][keep])
    assert bool((got["radii"] > 0).all()) and int(((full["radii"] > 0) & ~keep).sum()) > 0        # visible is not the same as blended
    print(f"select_rows: kept {small.N} of {n} rows, {baked.nbytes} -> {small.nbytes} bytes; pixels ended early in the full frame: "
          f"{int((~open_).sum())} of {h * w}; max |render difference| = {float((got['render'] - full['render']).abs().max()):.3e}")
    return small, _state_of(small, cam, bg, pipe)[1], open_, seen, keep


def test_dropping_the_rows_no_pixel_shows_leaves_the_view_bit_identical():
    """A dense bake of 600 rows of opacity ~0.12, so that no pixel of the view saturates (asserted: every final T >= 0.01); every seventh
    row is made transparent (opacity sigmoid(-12) < 1/255: projected, listed, never blended), so keep.sum() < N by construction.  The
    subset keeps the stored order and binning breaks depth ties by Gaussian index, so the view's lists hold the same blended entries in
    the same order: image and depth are torch.equal.  The guard asserts that this view has no depth tie among the kept rows at all."""
    n = 600
    pc = syn.SynthModel(n, "dynerf_default", seed=700).to(_dev())
    with torch.no_grad():
        pc._scaling.add_(0.5)
        pc._opacity.fill_(-2.0)
        pc._opacity[::7] = -12.0
    baked = P.bake(pc, [0.0, 0.25, 0.5, 1.0])
    assert baked.perm is None
    bg, pipe, cam = torch.tensor([0.1, 0.2, 0.3], device=_dev()), _pipe(), _cam(0, 0.25)
    small, state, open_, seen, keep = _select_case(baked, cam, bg, pipe)
    assert bool(open_.all())                                                                         # no pixel was ended early ...
    full, got = baked.render(cam, pipe, bg), small.render(cam, pipe, bg)
    assert torch.equal(got["render"], full["render"]) and torch.equal(got["depth"], full["depth"])  # ... so the whole frame is identical
    assert torch.equal(got["radii"], full["radii"][keep])
    assert not bool(keep[::7].any()) and int(keep.sum()) > 100
    again = P.contribution(small, [cam], pipe, bg)                                                   # every kept row is blended as before
    assert torch.equal(again.pixels, seen.pixels[keep]) and torch.equal(again.tiles, seen.tiles[keep])
    assert torch.equal(again.weight_max, seen.weight_max[keep])
    z = _geom(state, 2, 4 * small.N, torch.int32).view(small.N, 4)[:, 2].cpu().numpy()             # recB.z: the view depth the sort keys on
    assert len(np.unique(z)) == small.N
    mid = _cam(1, 0.375)                                                                             # a blended time: the snapshot holds every timestamp
    assert small.render(mid, pipe, bg)["render"].shape == baked.render(mid, pipe, bg)["render"].shape


def test_select_rows_of_a_bake_stored_through_the_permutation():
    """8200 opaque rows, stored in Hilbert order: the selection keeps that order and renumbers `perm`.  This view saturates, so the
    identity holds on the pixels that were not ended early (_select_case); the others and the depth ties, if any, are printed."""
    baked = _baked(8200, "dynerf_default")
    assert baked.perm is not None
    bg, pipe, cam = torch.tensor([0.1, 0.2, 0.3], device=_dev()), _pipe(), _cam(0, 0.25)
    small, state, open_, _, _ = _select_case(baked, cam, bg, pipe)
    assert sorted(small.perm.tolist()) == list(range(small.N))
    z = _geom(state, 2, 4 * small.N, torch.int32).view(small.N, 4)[:, 2].cpu().numpy()
    print(f"kept rows that share their depth bits with another: {small.N - len(np.unique(z))}")
