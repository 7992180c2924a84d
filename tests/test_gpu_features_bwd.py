"""The feature pass's backward on the device (csrc/render_features_bwd.h: render_features_bwd_kernel, fdgs_render_features_bwd;
render_features(differentiable=True) of fdgs.playback / fdgs.compose).

At the C level the oracle is the device's own forward blend, the per-Gaussian w maps of tests/test_gpu_pick.py (a one-hot recC pass per
three Gaussians: plane k is ONE Gaussian's blend weight w = alpha * T, bit for bit): want[n, c] = sum over the pixels of w[n] * G[c] in
float64, with a standard-normal G of both signs.

The bound per element: (pixels_row + 2) * 2**-23 * sum over the pixels of |w * G|.  A float32 sum of n rounded products in ANY order
errs by at most (n - 1 + 1) * 2**-24 * sum |terms| to first order (one rounding per product, n - 1 additions; a fused multiply-add only
removes roundings); the tests allow twice that, the contribution test's rule, with one more term for the atomic that joins a tile's sum to
the row.  A wrong or dropped term is off by a whole w * G.

From Python the check is the adjoint identity <G, F(V2)> = <V2, dL/dV> for an independent V2, in float64, within the sum of the forward's
bound, (max n_contrib + 1) * 2**-23 * <|G|, F(|V2|)>, and the backward's bound above summed against |V2| -- whose pixel counts and sums of
w * |G| come from render_contrib, one pass per channel: the route that existed before this kernel."""
import functools
import importlib

import numpy as np
import pytest
import torch

from test_gpu_features import _features
from test_gpu_motion import KEYS, _object, _pipe, _same
from test_gpu_pick import SCENES, TILE, _frame, _img, bits
from test_gpu_playback import _cam, _dev

pytestmark = pytest.mark.gpu
fdgs = importlib.import_module("4dgaussians_amd")
C, P, R, syn = fdgs.compose, fdgs.playback, fdgs.rasterizer, fdgs.synthetic
L = fdgs._lib
GUARD = 64                       # sentinel words in front of and behind dvalues
SENTINEL = -123456.0
U23 = 2.0 ** -23
CMAX = 33
# the kernel takes 16 channels per workgroup: partial chunks (1, 3), a full one (16), two (17) and three (33) chunks
CHANNELS = (1, 3, 16, 17, 33)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(G [CMAX,h,w] float32 numpy of both signs, pixels [n]): computed once per frame, shared by every test, never modified."""
    fr = _frame(name)
    g = np.random.default_rng(17).standard_normal((CMAX, fr.h, fr.w)).astype(np.float32)
    assert (g < 0).any() and (g > 0).any() and np.isfinite(g).all()
    return g, (fr.wmaps > 0).reshape(fr.n, -1).sum(1)


def _oracle(fr, g):
    """(want [n,c], sum |w * G| [n,c]) in float64 from the frame's w maps."""
    w64 = fr.wmaps.astype(np.float64)
    return np.einsum("nhw,chw->nc", w64, g.astype(np.float64)), np.einsum("nhw,chw->nc", np.abs(w64), np.abs(g.astype(np.float64)))


@functools.lru_cache(maxsize=None)
def _expected(name):
    return _oracle(_frame(name), _reference(name)[0])


def _bwd(state, g, rows, row_map=None, alpha=None, min_alpha=-1.0, stride=None, passes=1, offset=0):
    """`passes` x fdgs_render_features_bwd over `state` with the gradient image g [c,h,w] (numpy) into zeroed [rows, c] columns of a
    [rows, stride] array that starts `offset` floats behind a 256-byte boundary -> [rows, stride] numpy; the spare columns and the GUARD
    words around the array hold sentinels, which must survive."""
    dev = _dev()
    c = g.shape[0]
    stride = c if stride is None else stride
    buf = torch.full((2 * GUARD + rows * stride,), SENTINEL, device=dev)
    assert buf.data_ptr() % 256 == 0
    first = GUARD + offset
    body = buf[first:first + rows * stride].view(rows, stride) if rows else None
    if rows:
        body[:, :c] = 0.0
    gt = torch.from_numpy(np.ascontiguousarray(g)).to(dev)
    at = None if alpha is None else torch.from_numpy(np.ascontiguousarray(alpha, np.float32)).to(dev)
    for _ in range(passes):
        L.check(L.lib().fdgs_render_features_bwd(L.stream_ptr(), state.params, L.ptr(state.geom), L.ptr(state.binning), L.ptr(state.img),
                                                 state.capacity, c, L.ptr(gt), L.ptr(at), float(min_alpha), L.ptr(row_map), rows,
                                                 buf.data_ptr() + 4 * first, stride))
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    assert (a[:first] == SENTINEL).all() and (a[first + rows * stride:] == SENTINEL).all()
    out = a[first:first + rows * stride].reshape(rows, stride)
    assert (out[:, c:] == SENTINEL).all()
    return out


def _assert_within(got, want, absum, pixels, what, times=1):
    err = np.abs(got.astype(np.float64) - times * want)
    bound = (times * pixels[:, None] + 2) * U23 * times * absum
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: worst error / bound = {worst:.3f}; rows with pixels: {int((pixels > 0).sum())} of {len(pixels)}")
    assert (err <= bound).all(), what
    assert not bits(got[pixels == 0]).any(), what                                    # rows with no pixel keep all-zero bits


@functools.lru_cache(maxsize=None)
def _check_conditions():
    """What the two frames must contain for the comparisons to mean something, asserted about the device's own frames (once: a failure is
    not cached, so every test that asks fails)."""
    a, b = _frame("a"), _frame("b")
    lengths = np.concatenate([fr.ranges[:, 1] - fr.ranges[:, 0] for fr in (a, b)])
    walks = np.concatenate([np.minimum(fr.walk, fr.ranges[:, 1] - fr.ranges[:, 0]) for fr in (a, b)])
    print(f"list lengths {lengths.tolist()}, walk lengths {walks.tolist()}")
    assert ((lengths % 16) != 0).any(), "no tile whose list length is not a multiple of 16"
    assert ((lengths > 0) & (lengths < 16)).any(), "no tile shorter than 16"
    assert a.w % TILE and a.h % TILE and b.w % TILE and b.h % TILE                    # tiles cut by both edges
    for fr in (a, b):
        pixels = _reference(fr.name)[1]
        assert int((pixels == 0).sum()) > 0 and int((pixels > 0).sum()) > 0, fr.name
    late = {2: 0, 3: 0}                 # (tile, entry) pairs staged in round 2 / round 3 of their tile that are blended into a pixel of it
    for tile in range(b.gx * b.gy):
        lo, hi = b.ranges[tile]
        y0, x0 = (tile // b.gx) * TILE, (tile % b.gx) * TILE
        for pos in range(256, int(hi - lo)):
            late[2 if pos < 512 else 3] += bool((b.wmaps[b.gid[lo + pos], y0:y0 + TILE, x0:x0 + TILE] > 0).any())
    print(f"scene b: (tile, entry) pairs with gradient in staging round 2: {late[2]}, round 3: {late[3]}")
    assert late[2] > 0 and late[3] > 0


@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_dvalues_is_the_sum_of_w_times_the_gradient_image(name, c):
    _check_conditions()
    fr = _frame(name)
    g, pixels = _reference(name)
    want, absum = _expected(name)
    got = _bwd(fr.state, g[:c], fr.n)
    _assert_within(got, want[:, :c], absum[:, :c], pixels, (name, c))
    assert (np.abs(want[pixels > 0, :c]) > 0).all()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_two_passes_accumulate(name):
    fr = _frame(name)
    g, pixels = _reference(name)
    want, absum = _expected(name)
    got = _bwd(fr.state, g[:17], fr.n, passes=2)
    _assert_within(got, want[:, :17], absum[:, :17], pixels, (name, "two passes"), times=2)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_row_map_chooses_the_row_and_rows_outside_are_dropped(name):
    fr = _frame(name)
    g, pixels = _reference(name)
    want, absum = _expected(name)
    c = 9
    rng = np.random.default_rng(11)
    perm = rng.permutation(fr.n).astype(np.int32)
    got = _bwd(fr.state, g[:c], fr.n, row_map=torch.from_numpy(perm).to(_dev()))
    inv = np.argsort(perm)                                                           # row r holds Gaussian inv[r]
    _assert_within(got, want[inv, :c], absum[inv, :c], pixels[inv], (name, "row map"))
    assert (pixels[inv] != pixels).any()
    # some entries -1, and fewer rows than Gaussians: those Gaussians are dropped (the sentinels behind the rows are checked inside)
    rows = fr.n - fr.n // 4
    holes = perm.copy()
    holes[rng.choice(fr.n, fr.n // 5, replace=False)] = -1
    live = (holes >= 0) & (holes < rows)
    assert 0 < int(live.sum()) < int((holes >= 0).sum()) < fr.n and int((pixels[~live] > 0).sum()) > 0
    got = _bwd(fr.state, g[:c], rows, row_map=torch.from_numpy(holes).to(_dev()))
    w2, a2, p2 = np.zeros((rows, c)), np.zeros((rows, c)), np.zeros(rows, np.int64)
    w2[holes[live]], a2[holes[live]], p2[holes[live]] = want[live, :c], absum[live, :c], pixels[live]
    _assert_within(got, w2, a2, p2, (name, "row map with holes"))


@pytest.mark.parametrize("c,stride,offset", [(3, 7, 1), (16, 19, 0), (16, 16, 3), (17, 32, 0)])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_a_wider_stride_keeps_its_spare_columns(name, c, stride, offset):
    """dvalues as a column slice of a wider array, at addresses that are 4-byte aligned only (offset) and with rows that are not 64-byte
    aligned: the spare columns and the words around the array keep their sentinels (checked in _bwd)."""
    fr = _frame(name)
    g, pixels = _reference(name)
    want, absum = _expected(name)
    got = _bwd(fr.state, g[:c], fr.n, stride=stride, offset=offset)
    _assert_within(got[:, :c], want[:, :c], absum[:, :c], pixels, (name, c, stride, offset))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_a_normalised_forward_scales_the_gradient_by_alpha(name):
    """min_alpha = 1e-4: the oracle fed with numpy's float32 G / A where A > min_alpha and 0 elsewhere, A the alpha image the forward wrote."""
    fr = _frame(name)
    g, pixels = _reference(name)
    c = 9
    _, a = _features(fr.state, fr.h, fr.w, torch.ones(fr.n, 1, device=_dev()), 1, 1, fr.n, min_alpha=1e-4)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = g[:c] / a[None]
    assert q.dtype == np.float32
    scaled = np.where(a[None] > np.float32(1e-4), q, np.float32(0))
    assert (a > np.float32(1e-4)).any() and (name != "a" or not (a > np.float32(1e-4)).all())      # (a) has pixels below the cut
    want, absum = _oracle(fr, scaled)
    got = _bwd(fr.state, g[:c], fr.n, alpha=a, min_alpha=1e-4)
    # a row all of whose pixels lie below the cut gets nothing: its "pixels" for the zero-bits check are those above it
    pixels_cut = ((fr.wmaps > 0) & (a[None] > np.float32(1e-4))).reshape(fr.n, -1).sum(1)
    err = np.abs(got.astype(np.float64) - want)
    bound = (pixels[:, None] + 2) * U23 * absum
    print(f"{name}: normalised, worst error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all() and not bits(got[pixels_cut == 0]).any()
    raw = _bwd(fr.state, g[:c], fr.n, alpha=a, min_alpha=float("nan"))               # a NaN min_alpha: the forward wrote raw sums
    _assert_within(raw, _expected(name)[0][:, :c], _expected(name)[1][:, :c], pixels, (name, "NaN min_alpha"))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_nothing_of_the_frame_is_written(name):
    fr = _frame(name)
    g, pixels = _reference(name)
    state = fr.state
    before = [b.clone() for b in (state.geom, state.binning, state.img)]
    torch.cuda.synchronize()
    _bwd(state, g[:17], fr.n)
    _bwd(state, g[:8], fr.n, alpha=np.ones((fr.h, fr.w), np.float32), min_alpha=0.0)
    for b, was in zip((state.geom, state.binning, state.img), before):
        assert torch.equal(b, was)


def test_an_empty_frame_touches_nothing():
    """P > 0 with num_rendered == 0 (every Gaussian behind the camera) and P == 0: success, and dvalues keeps the bits it had."""
    dev = _dev()
    fr = _frame("a")
    t, settings = fr.keep
    for n in (5, 0):
        xyz = torch.tensor(fr.sc["campos"], device=dev).repeat(n, 1)                 # at the camera's centre: culled by the near plane
        with torch.no_grad():
            *_, state = R.rasterize_forward(settings, xyz, t["shs"][:n], None, t["opacities"][:n], t["scales"][:n], t["rotations"][:n], None,
                                            expect_backward=False)
        assert state.num_rendered == 0 and state.capacity == 0
        g = torch.ones(9, fr.h, fr.w, device=dev)
        dv = torch.full((max(n, 1), 9), SENTINEL, device=dev)
        L.check(L.lib().fdgs_render_features_bwd(L.stream_ptr(), state.params, L.ptr(state.geom), L.ptr(state.binning), L.ptr(state.img),
                                                 state.capacity, 9, L.ptr(g), None, -1.0, None, n, L.ptr(dv), 9))
        torch.cuda.synchronize()
        assert bool((dv == SENTINEL).all())


# ---- the Python surface ------------------------------------------------------------------------------------------------------------------

HIGH = [("baked", 4099, "dynerf_default"), ("baked", 8200, "dnerf_bouncingballs"), ("quantile", 8200, "dnerf_bouncingballs"), "composite"]
_ids = dict(ids=lambda k: k if isinstance(k, str) else "-".join(str(v) for v in k))


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(_dev())


def _adjoint(obj, cam, c, normalize=False, one_d=False, between=None):
    """One differentiable frame of `obj`, its backward under a random G, and the adjoint identity against an independent V2 within the
    stated bounds.  `between`: called between the forward and the backward (another frame, say)."""
    bg, pipe, dev = torch.tensor([0.1, 0.2, 0.3], device=_dev()), _pipe(), _dev()
    n = obj.N
    v = _randn(n, seed=3) if one_d else _randn(n, c, seed=3)
    v.requires_grad_()
    plain = obj.render_features(cam, pipe, bg, v.detach(), normalize=normalize)
    out = obj.render_features(cam, pipe, bg, v, normalize=normalize, differentiable=True)
    _same(out, plain, KEYS)
    assert set(out) == set(plain) and out["viewspace_points"] is None
    assert torch.equal(out["features"], plain["features"]) and torch.equal(out["alpha"], plain["alpha"])     # the plain pass's bits
    assert out["features"].requires_grad and not out["alpha"].requires_grad and not out["render"].requires_grad
    h, w = out["alpha"].shape[1:]
    g = _randn(c, h, w, seed=5)
    state = out["features"].grad_fn.frame.rstate
    n_contrib = int(_img(state, 1, h * w, torch.int32).max())
    if between is not None:
        between()
    (out["features"] * g).sum().backward()
    grad = v.grad
    assert grad.shape == v.shape and grad.dtype == torch.float32 and bool(torch.isfinite(grad).all())
    grad = grad.reshape(n, c)
    # the effective gradient image: what the kernel forms on load for a normalised forward (IEEE division on the device)
    alpha = plain["alpha"]
    g_eff = torch.where(alpha > 1e-4, g / alpha, torch.zeros_like(g)) if normalize else g
    v2 = _randn(n, c, seed=9)
    with torch.no_grad():
        f2 = obj.render_features(cam, pipe, bg, v2)["features"].double()
        f2_abs = obj.render_features(cam, pipe, bg, v2.abs())["features"].double()
        lhs = float((g_eff.double() * f2).sum())
        rhs = float((v2.double() * grad.double()).sum())
        forward_bound = (n_contrib + 1) * U23 * float((g_eff.abs().double() * f2_abs).sum())
        pixels = obj.render_contrib(cam, pipe, bg)["contribution"].pixels.double()
        backward_bound = 0.0
        for k in range(c):          # sum over the pixels of w * |G[k]| per row: one contribution pass per channel
            s = obj.render_contrib(cam, pipe, bg, pixel_weight=g_eff[k].abs().contiguous())["contribution"].weight_sum.double()
            backward_bound += float(((pixels + 2) * U23 * s * (1 + 1e-4) * v2[:, k].abs().double()).sum())
    bound = forward_bound + backward_bound
    print(f"adjoint: <G, F(V2)> = {lhs:.9e}, <V2, dV> = {rhs:.9e}, |difference| / bound = {abs(lhs - rhs) / bound:.2e} "
          f"(forward {forward_bound:.3e}, backward {backward_bound:.3e}; max n_contrib {n_contrib}, rows with pixels {int((pixels > 0).sum())})")
    assert int((pixels > 0).sum()) > 100 and abs(lhs) > 0
    assert abs(lhs - rhs) <= bound
    assert not bool(grad[pixels == 0].any())                                         # a row no pixel shows gets +0
    return out, v, g


@pytest.mark.parametrize("kind", HIGH, **_ids)
def test_the_backward_is_the_adjoint_of_the_forward(kind):
    """8200 rows are stored in another order than the model's (a row map is handed over), 4099 are not.  One frame at a baked time (the
    exact binning path: the first frame of its size) and one in between (the speculative path)."""
    obj = _object(kind)
    _adjoint(obj, _cam(0, 0.25), 5)
    _adjoint(obj, _cam(1, 0.375), 17)


@pytest.mark.parametrize("kind", HIGH[1:3], **_ids)
def test_one_dimensional_values_and_a_normalised_forward(kind):
    obj = _object(kind)
    _adjoint(obj, _cam(1, 0.375), 1, one_d=True)
    _adjoint(obj, _cam(0, 0.25), 4, normalize=True)
    _adjoint(obj, _cam(2, 0.5), 1, normalize=True, one_d=True)


@pytest.mark.parametrize("kind", HIGH[2:], **_ids)
def test_a_backward_after_another_frame_reads_its_own_frame(kind):
    """The sparse and the composite kinds keep ONE working state that every state_at overwrites: a backward that ran after a frame at
    another time and view, and read the state through the pointers of its params, would see that other frame's Gaussians."""
    obj = _object(kind)
    bg = torch.zeros(3, device=_dev())
    out, v, g = _adjoint(obj, _cam(0, 0.25), 5, between=lambda: obj.render(_cam(2, 1.0), _pipe(), bg))
    # ... and a second backward of the same graph, after yet another frame, accumulates the same gradient once more
    first = v.grad.clone()
    out2 = obj.render_features(_cam(0, 0.25), _pipe(), bg, v, differentiable=True)
    v.grad = None
    loss = (out2["features"] * g).sum()
    loss.backward(retain_graph=True)
    once = v.grad.clone()
    obj.render(_cam(1, 0.75), _pipe(), bg)
    loss.backward()
    # (the same sums three times, their float32 additions in another order each time -- atomics --: the adjoint check above bounds the
    # gradient itself; here 1e-4 of the largest element only tells a second frame's gradient, or none, from the first one's)
    scale = float(first.abs().max())
    assert float((once - first).abs().max()) <= 1e-4 * scale and float((v.grad - 2 * once).abs().max()) <= 1e-4 * scale


def test_an_embedding_is_fitted_to_a_rendered_target():
    """20 Adam steps on a [N,16] embedding against the features of known values: the loss falls monotonically over the first steps."""
    obj = _object(HIGH[1])
    bg, pipe, cam = torch.zeros(3, device=_dev()), _pipe(), _cam(0, 0.25)
    known = _randn(obj.N, 16, seed=21)
    target = obj.render_features(cam, pipe, bg, known)["features"]
    emb = torch.zeros(obj.N, 16, device=_dev(), requires_grad=True)
    opt = torch.optim.Adam([emb], lr=0.02)
    losses = []
    for _ in range(20):
        opt.zero_grad(set_to_none=True)
        out = obj.render_features(cam, pipe, bg, emb, differentiable=True)
        loss = ((out["features"] - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("fit: loss per step " + " ".join(f"{v:.5f}" for v in losses))
    assert all(b < a for a, b in zip(losses[:8], losses[1:9])), losses
    assert losses[-1] < losses[0]
