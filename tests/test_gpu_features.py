"""The feature pass on the device (csrc/render.hip: render_features_kernel, fdgs_render_features; render_features of fdgs.playback /
fdgs.compose).

Every comparison is EXACT, and the oracle is the device's own forward blend: three channels at a time are written into recC of a
forward-only frame (include/fdgs.h at fdgs_geom_field: recC may be rewritten between two fdgs_render_fwd calls of such a frame) and
fdgs_render_fwd runs again over the frame's own buffers with a zero background; recC is saved before and put back afterwards.  A channel's
sum does not depend on the two channels it shares a blend with, so plane c of that blend is what channel c must be, on its bits, whatever
C it is part of; the blend of a channel of ones is what `alpha` must be.  The frames are the two of tests/test_gpu_pick.py (shared with it,
never modified): (a) 48 Gaussians on 40 x 36 with partial tiles on both edges and empty pixels, (b) 600 Gaussians on 33 x 17 whose lists run
past 512 entries, three rounds of the staging pipeline."""
import functools
import importlib

import numpy as np
import pytest
import torch

from test_gpu_motion import KEYS, _object, _pipe, _same
from test_gpu_pick import GUARD, SCENES, TILE, _blend_again, _frame, _geom, bits
from test_gpu_playback import _cam, _dev

pytestmark = pytest.mark.gpu
fdgs = importlib.import_module("4dgaussians_amd")
R, L = fdgs.rasterizer, fdgs._lib
SENTINEL = -123456.0
CMAX = 33
# the kernel takes 16 channels per workgroup: partial chunks (1, 3, 8, 9), a full one (16: 16-byte loads), two (17) and three (33) chunks
CHANNELS = (1, 3, 8, 9, 16, 17, 33)


def _check_conditions():
    """What the two frames must contain for the comparisons to mean something, asserted about the device's own frames."""
    a, b = _frame("a"), _frame("b")
    assert int(b.n_contrib.max()) > 512 and int((b.n_contrib > 256).sum()) > 0                 # walks of two and of three rounds
    assert int((a.n_contrib == 0).sum()) > 0                                                    # pixels nothing is blended into
    for fr in (a, b):
        empty = int(((fr.ranges[:, 1] - fr.ranges[:, 0]) == 0).sum())
        assert empty > 0 or (fr.w % TILE and fr.h % TILE), fr.name                              # an empty tile, or tiles cut by both edges
    assert a.w % TILE and a.h % TILE and b.w % TILE and b.h % TILE


def _oracle(fr, vals):
    """[C,h,w] numpy: the frame's own blend of the [n, C] device tensor `vals`, three channels per fdgs_render_fwd, zero background."""
    n, c = vals.shape
    recC = _geom(fr.state, 3, 4 * n, torch.float32).view(n, 4)
    saved = recC.clone()
    zero = torch.zeros(3, device=_dev())
    planes = torch.empty(c + 2, fr.h, fr.w, device=_dev())
    try:
        for c0 in range(0, c, 3):
            k = min(3, c - c0)
            recC[:, :3] = 0.0
            recC[:, :k] = vals[:, c0:c0 + k]
            planes[c0:c0 + 3] = _blend_again(fr, zero)[0]
    finally:
        recC.copy_(saved)
        torch.cuda.synchronize()
    return planes[:c].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(values [n, CMAX] on the device, of both signs; the oracle of its channels [CMAX,h,w]; the oracle of a channel of ones [h,w]): computed
    once per frame, shared by every test, never modified."""
    fr = _frame(name)
    vals = torch.from_numpy(np.random.default_rng(5).standard_normal((fr.n, CMAX)).astype(np.float32)).to(_dev())
    want = _oracle(fr, vals)
    ones = _oracle(fr, torch.ones(fr.n, 1, device=_dev()))[0]
    assert (want < 0).any() and (want > 0).any() and (ones > 0).any()
    return vals, want, ones


def _features(state, h, w, values, c, stride, rows, row_map=None, min_alpha=-1.0, with_alpha=True, values_ptr=None):
    """fdgs_render_features over `state` -> (features [c,h,w], alpha [h,w] or None) as numpy; both outputs sit between GUARD sentinel words,
    which must survive.  `values` is the device tensor the pointer (values_ptr, default its own) points into."""
    dev, hw = _dev(), h * w
    feat = torch.full((c * hw + 2 * GUARD,), SENTINEL, device=dev)
    alpha = torch.full((hw + 2 * GUARD,), SENTINEL, device=dev)
    L.check(L.lib().fdgs_render_features(L.stream_ptr(), state.params, L.ptr(state.geom), L.ptr(state.binning), L.ptr(state.img), state.capacity,
                                         c, values.data_ptr() if values_ptr is None else values_ptr, stride, rows, L.ptr(row_map),
                                         float(min_alpha), feat.data_ptr() + 4 * GUARD, alpha.data_ptr() + 4 * GUARD if with_alpha else None))
    torch.cuda.synchronize()
    f, a = feat.cpu().numpy(), alpha.cpu().numpy()
    assert (f[:GUARD] == SENTINEL).all() and (f[GUARD + c * hw:] == SENTINEL).all()
    if not with_alpha:
        assert (a == SENTINEL).all()
        return f[GUARD:GUARD + c * hw].reshape(c, h, w), None
    assert (a[:GUARD] == SENTINEL).all() and (a[GUARD + hw:] == SENTINEL).all()
    return f[GUARD:GUARD + c * hw].reshape(c, h, w), a[GUARD:GUARD + hw].reshape(h, w)


def _run(fr, vals, **kw):
    vals = vals.contiguous()
    return _features(fr.state, fr.h, fr.w, vals, vals.shape[1], vals.shape[1], vals.shape[0], **kw)


@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_channel_has_the_bits_of_the_forward_blend(name, c):
    _check_conditions()
    fr = _frame(name)
    vals, want, ones = _reference(name)
    got, alpha = _run(fr, vals[:, :c])
    for k in range(c):
        assert np.array_equal(bits(got[k]), bits(want[k])), (name, c, k)
    assert np.array_equal(bits(alpha), bits(ones)), (name, c)
    assert not bits(got[:, fr.n_contrib == 0]).any() and not bits(alpha[fr.n_contrib == 0]).any()      # +0 where nothing is blended


@pytest.mark.parametrize("name", sorted(SCENES))
def test_row_map_picks_the_row_and_rows_outside_blend_as_zeros(name):
    fr = _frame(name)
    vals, want, ones = _reference(name)
    c = 9
    rng = np.random.default_rng(11)
    perm = rng.permutation(fr.n).astype(np.int32)
    perm_t = torch.from_numpy(perm).to(_dev())
    got, alpha = _run(fr, vals[:, :c], row_map=perm_t)
    permuted = _oracle(fr, vals[perm_t.long(), :c])                                   # Gaussian g takes row perm[g]
    assert np.array_equal(bits(got), bits(permuted)) and not np.array_equal(bits(got), bits(want[:c]))
    assert np.array_equal(bits(alpha), bits(ones))
    # some entries -1, and fewer rows than Gaussians: those Gaussians blend as zeros (and alpha does not change)
    rows = fr.n - fr.n // 4
    holes = perm.copy()
    holes[rng.choice(fr.n, fr.n // 5, replace=False)] = -1
    live = (holes >= 0) & (holes < rows)
    assert 0 < int(live.sum()) < int((holes >= 0).sum()) < fr.n
    masked = vals[perm_t.long(), :c] * torch.from_numpy(live.astype(np.float32)).to(_dev())[:, None]
    masked = torch.where(torch.from_numpy(live).to(_dev())[:, None], masked, torch.zeros_like(masked))      # (+0, not -0)
    short = vals[:rows, :c].contiguous()
    got2, alpha2 = _features(fr.state, fr.h, fr.w, short, c, c, rows, row_map=torch.from_numpy(holes).to(_dev()))
    assert np.array_equal(bits(got2), bits(_oracle(fr, masked))) and not np.array_equal(bits(got2), bits(got))
    assert np.array_equal(bits(alpha2), bits(ones))


@pytest.mark.parametrize("c", [3, 16, 17])      # (16 and a row stride of 19 floats: every fourth row allows the 16-byte loads)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_a_slice_of_a_wider_array_gives_the_bits_of_a_contiguous_copy(name, c):
    fr = _frame(name)
    vals, want, _ = _reference(name)
    wide = torch.full((fr.n, c + 3), 77.0, device=_dev())
    wide[:, 1:1 + c] = vals[:, :c]
    assert wide.data_ptr() % 16 == 0 and wide[:, 1:1 + c].data_ptr() == wide.data_ptr() + 4
    got, _ = _features(fr.state, fr.h, fr.w, wide, c, c + 3, fr.n, values_ptr=wide.data_ptr() + 4)
    copy, _ = _run(fr, wide[:, 1:1 + c])
    assert np.array_equal(bits(got), bits(copy)) and np.array_equal(bits(got), bits(want[:c]))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_normalized_features_are_the_float32_quotient_of_the_raw_outputs(name):
    fr = _frame(name)
    vals, _, _ = _reference(name)
    raw, a = _run(fr, vals[:, :9])
    got, a2 = _run(fr, vals[:, :9], min_alpha=1e-4)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = raw / a[None]
    assert q.dtype == np.float32
    want = np.where(a[None] > np.float32(1e-4), q, np.float32(0))
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(a2), bits(a))
    assert (a > np.float32(1e-4)).any() and (name != "a" or not (a > np.float32(1e-4)).all())      # (a) has pixels below the cut
    nan_cut, _ = _run(fr, vals[:, :9], min_alpha=float("nan"))                        # a NaN min_alpha: raw sums
    assert np.array_equal(bits(nan_cut), bits(raw))


def _training_frame(fr):
    t, settings = fr.keep
    with torch.no_grad():
        color, _, depth, state = R.rasterize_forward(settings, t["means3D"], t["shs"], None, t["opacities"], t["scales"], t["rotations"], None,
                                                     expect_backward=True)
    torch.cuda.synchronize()
    assert state.acc is not None and torch.equal(color, fr.color) and torch.equal(depth, fr.depth)
    return state


@pytest.mark.parametrize("name", sorted(SCENES))
def test_nothing_of_the_frame_is_written(name):
    """geom, binning and img keep every byte over a pass, on the forward-only frame and on a training frame (expect_backward=True) of the
    same scene; the training frame gives the forward-only frame's features."""
    fr = _frame(name)
    vals, want, ones = _reference(name)
    for state in (fr.state, _training_frame(fr)):
        before = [b.clone() for b in (state.geom, state.binning, state.img)]
        acc = None if state.acc is None else state.acc.clone()
        torch.cuda.synchronize()
        for c, cut in ((17, -1.0), (8, 1e-4)):
            got, alpha = _features(state, fr.h, fr.w, vals[:, :c].contiguous(), c, c, fr.n, min_alpha=cut)
            assert np.array_equal(bits(alpha), bits(ones))
            if cut < 0:
                assert np.array_equal(bits(got), bits(want[:c]))
        for b, was in zip((state.geom, state.binning, state.img), before):
            assert torch.equal(b, was)
        assert acc is None or torch.equal(state.acc, acc)
    color, depth = _blend_again(fr, fr.bg)                       # the frame's blend once more: the image and the depth it returned before
    assert torch.equal(color, fr.color) and torch.equal(depth, fr.depth)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_alpha_is_optional(name):
    fr = _frame(name)
    vals, want, _ = _reference(name)
    got, none = _run(fr, vals[:, :9], with_alpha=False)
    assert none is None and np.array_equal(bits(got), bits(want[:9]))


def test_an_empty_frame_gets_zeros_everywhere():
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
        vals = torch.ones(max(n, 1), 9, device=dev)
        for cut in (-1.0, 1e-4):
            got, alpha = _features(state, sc["image_height"], sc["image_width"], vals, 9, 9, n, min_alpha=cut)
            assert not bits(got).any() and not bits(alpha).any()


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------

HIGH = [("baked", 4099, "dynerf_default"), ("baked", 8200, "dnerf_bouncingballs"), ("quantile", 8200, "dnerf_bouncingballs"), "composite"]


def _values(n, c, seed=7):
    return torch.randn(n, c, generator=torch.Generator().manual_seed(seed)).to(_dev())


@pytest.mark.parametrize("kind", HIGH, ids=lambda k: k if isinstance(k, str) else "-".join(str(v) for v in k))
def test_render_features_is_render_plus_the_override_colour_blends(kind):
    """8200 rows are stored in another order than the model's (a row map is handed over), 4099 are not.  One frame at a baked time and one
    in between; C = 3 against one override_color blend over a zero background, C = 9 against three."""
    obj = _object(kind)
    bg, zero, pipe = torch.tensor([0.1, 0.2, 0.3], device=_dev()), torch.zeros(3, device=_dev()), _pipe()
    vals = _values(obj.N, 12)
    for k, t in ((0, 0.25), (1, 0.375)):
        cam = _cam(k, t)
        before = obj.render(cam, pipe, bg, rgb8="trunc")
        three = obj.render_features(cam, pipe, bg, vals[:, 1:4], rgb8="trunc")          # a slice: read in place, row stride 12
        nine = obj.render_features(cam, pipe, bg, vals[:, :9].contiguous(), rgb8="trunc")
        after = obj.render(cam, pipe, bg, rgb8="trunc")
        h, w = before["depth"].shape[1:]
        for got, c in ((three, 3), (nine, 9)):
            assert set(got) == set(before) | {"features", "alpha"} and got["viewspace_points"] is None
            _same(got, before, KEYS + ("rgb8",))
            assert got["features"].shape == (c, h, w) and got["alpha"].shape == (1, h, w)
            assert got["features"].dtype == got["alpha"].dtype == torch.float32
        _same(after, before, KEYS + ("rgb8",))
        assert (obj._pick_row_map is None) == (obj._maps[0] is None)
        assert torch.equal(three["features"], obj.render(cam, pipe, zero, override_color=vals[:, 1:4])["render"])
        for c0 in (0, 3, 6):
            assert torch.equal(nine["features"][c0:c0 + 3], obj.render(cam, pipe, zero, override_color=vals[:, c0:c0 + 3])["render"]), c0
        assert torch.equal(three["alpha"], nine["alpha"]) and int((nine["alpha"] > 0).sum()) > 100
        ones = obj.render(cam, pipe, zero, override_color=torch.ones(obj.N, 3, device=_dev()))["render"]
        assert torch.equal(nine["alpha"][0], ones[0])
        norm = obj.render_features(cam, pipe, bg, vals[:, :9].contiguous(), normalize=True)
        assert torch.equal(norm["alpha"], nine["alpha"])
        a, f = nine["alpha"].cpu(), nine["features"].cpu()                              # (the quotient on the host: IEEE division)
        assert torch.equal(norm["features"].cpu(), torch.where(a > 1e-4, f / a, torch.zeros_like(f)))


def _mattes():
    scene = _object("composite")
    assert len(scene.models) == 2 and any(m.perm is not None for m in scene.models)
    ind = scene.model_indicator()
    assert ind.shape == (scene.N, 2) and ind.dtype == torch.float32 and ind.device == scene.device
    for m, sl in enumerate(scene.slices):
        assert bool((ind[sl, m] == 1).all()) and float(ind[sl].sum()) == sl.stop - sl.start
    return scene, ind, _cam(0, 0.25)


def test_the_mattes_of_a_composite_have_the_bits_of_their_indicator_blends():
    scene, ind, cam = _mattes()
    zero = torch.zeros(3, device=_dev())
    out = scene.render_features(cam, _pipe(), torch.tensor([0.1, 0.2, 0.3], device=_dev()), ind)
    blend = scene.render(cam, _pipe(), zero, override_color=torch.cat([ind, torch.ones(scene.N, 1, device=_dev())], 1))["render"]
    assert torch.equal(out["features"], blend[:2]) and torch.equal(out["alpha"][0], blend[2])
    assert int((out["features"][0] > 0).sum()) > 100 and int((out["features"][1] > 0).sum()) > 100          # both models are in the picture


def test_the_mattes_of_a_composite_sum_to_alpha():
    """Every blend weight goes to exactly one matte, so in exact arithmetic the M mattes sum to alpha; in float32 the three running sums
    round differently, and the bound asserted is the stated one: |sum of the mattes - alpha| <= M * 2**-23 * alpha (the sum taken in
    float64)."""
    scene, ind, cam = _mattes()
    out = scene.render_features(cam, _pipe(), torch.zeros(3, device=_dev()), ind)
    total, alpha = out["features"].double().sum(0), out["alpha"][0].double()
    err, bound = (total - alpha).abs(), len(scene.models) * 2.0 ** -23 * alpha
    on = alpha > 0
    print(f"mattes: max |sum - alpha| / alpha = {float((err[on] / alpha[on]).max()):.3e} (bound {len(scene.models) * 2.0 ** -23:.3e}), "
          f"{int((err > bound).sum())} of {int(on.sum())} pixels above the bound")
    assert bool((err <= bound).all())
