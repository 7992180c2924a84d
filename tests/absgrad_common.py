"""The reference of the absolute screen-space gradients (fdgs_raster_bwd_abs), shared by tests/test_absgrad_reference.py (CPU) and
tests/test_gpu_absgrad.py.

The reference needs no oracle change.  Restricting the loss to ONE pixel p makes RasterOracle.backward return exactly that pixel's term of
every per-Gaussian sum, so

    abs_ref = sum over the pixels p of | RasterOracle(float64).backward(dL_dcolor 1_p, dL_ddepth 1_p)["means2D"] |.

Alpha's share goes through the twin scene S' of tests/test_gpu_alpha.py (unit red colours over black: its red channel is alpha), added per
pixel BEFORE the absolute value.  By linearity the per-pixel rows of the three image gradients are kept apart -- colour, depth, alpha, each
[H*W, P, 2] float64 -- and a loss that sees some of them sums those it sees; one sweep of H*W oracle backwards per part and scene, cached.
An antialiased frame's reference is the same on opacities premultiplied by antialias_common's float64 h.

Before anything is compared, per_pixel() asserts the identity the construction stands on: the signed sum of the per-pixel rows is the
oracle's full means2D (measured: 2e-15 relative)."""
import functools

import numpy as np

import antialias_common as AC
from oracle.raster_oracle import RasterOracle
from scenes import raster_scene

# the smallest shapes at which the kernels can still go wrong (40 x 24: 3 x 2 tiles, partial on both edges)
SCENES = {
    "S": dict(n=60, width=40, height=24, seed=3),      # longest list 56: one 64-entry round
    "L": dict(n=400, width=40, height=24, seed=5),     # longest list 296: several 64-, 128- and 256-entry rounds; 60 % of the pixels saturated
    "1": dict(n=1, width=40, height=24, seed=5),       # one row
}
PARTS = ("color", "depth", "alpha")
IDENTITY_BOUND = 1e-12     # signed sum of the per-pixel rows against the oracle's own means2D, relative (float64 sums of <= 960 terms)


@functools.lru_cache(maxsize=None)
def scene(name):
    return raster_scene(**SCENES[name])


@functools.lru_cache(maxsize=None)
def image_grads(name):
    """(dL_dcolor [3,H,W], dL_ddepth [1,H,W], dL_dalpha [1,H,W]) float32, drawn in this order from default_rng(0)."""
    sc = scene(name)
    H, W = sc["image_height"], sc["image_width"]
    rng = np.random.default_rng(0)
    return tuple(rng.standard_normal((c, H, W)).astype(np.float32) for c in (3, 1, 1))


def _twin(sc):
    """S' of tests/test_gpu_alpha.py: the geometry of S with unit red colours over black -- its red channel is alpha."""
    tw = {k: v for k, v in sc.items() if k != "shs"}
    tw["colors_precomp"] = np.tile(np.array([1.0, 0.0, 0.0], np.float64), (sc["means3D"].shape[0], 1))
    tw["bg"] = np.zeros(3, np.float64)
    return tw


@functools.lru_cache(maxsize=None)
def oracles(name, aa):
    """(float64 oracle of S, of its twin S'); aa: on opacity * h."""
    sc = scene(name)
    o = {k: (np.asarray(v, np.float64) if isinstance(v, np.ndarray) else v) for k, v in sc.items()}
    if aa:
        h = AC.h64(sc, 1.0)[0]
        o["opacities"] = (o["opacities"].reshape(-1) * h).reshape(o["opacities"].shape)
    return RasterOracle(**o, dtype=np.float64), RasterOracle(**_twin(o), dtype=np.float64)


@functools.lru_cache(maxsize=None)
def per_pixel(name, part, aa=False):
    """[H*W, P, 2] float64: row p is the means2D gradient (x, y) of the loss restricted to pixel p, for ONE of the three image gradients.
    Read-only.  Asserts that the rows add up to the oracle's full gradient of that part."""
    sc = scene(name)
    H, W, P = sc["image_height"], sc["image_width"], sc["means3D"].shape[0]
    dc, dd, ga = image_grads(name)
    o, ot = oracles(name, aa)
    zc, one = np.zeros((3, H, W)), np.zeros((H, W))
    if part == "color":
        run = lambda m: o.backward(dc * m, None)
    elif part == "depth":
        run = lambda m: o.backward(zc, dd[0] * m)
    else:
        run = lambda m: ot.backward(np.concatenate([ga * m, zc[:2]]), None)
    rows = np.zeros((H * W, P, 2))
    for p in range(H * W):
        one.flat[p] = 1.0
        rows[p] = run(one)["means2D"][:, :2]
        one.flat[p] = 0.0
    full = run(np.ones((H, W)))["means2D"][:, :2]
    err = np.linalg.norm(rows.sum(0) - full) / max(np.linalg.norm(full), 1e-300)
    assert err < IDENTITY_BOUND, (name, part, aa, err)
    rows.setflags(write=False)
    return rows


def parts_of(with_depth, with_alpha):
    return ("color",) + (("depth",) if with_depth else ()) + (("alpha",) if with_alpha else ())


@functools.lru_cache(maxsize=None)
def reference(name, with_depth=False, with_alpha=False, aa=False):
    """(abs_ref [P,2], signed_ref [P,2], blended [P] bool) float64 of the loss on colour (+ depth) (+ alpha): the absolute and the signed
    sums over the pixels, and which rows some pixel blended (a non-zero per-pixel row of ANY part: the blend weight itself is not zero
    there, and a normal draw is not zero)."""
    rows = sum(per_pixel(name, part, aa) for part in parts_of(with_depth, with_alpha))
    blended = np.zeros(rows.shape[1], bool)
    for part in PARTS:
        if part == "color" or (part == "depth" and with_depth) or (part == "alpha" and with_alpha):
            blended |= (per_pixel(name, part, aa) != 0.0).any(axis=(0, 2))
    return np.abs(rows).sum(0), rows.sum(0), blended


def longest_list(name, aa=False):
    """The largest n_contrib of the frame: how many list entries the longest walk of the blending backward takes."""
    return int(oracles(name, aa)[0].image_state()[1].max())


def saturated_share(name):
    fT = oracles(name, False)[0].image_state()[0]
    return float((fT < 1e-3).mean())


def cancellation(name, with_depth=False, with_alpha=False, aa=False):
    """(rows with a non-zero absolute sum, how many of them have abs >= 10 |signed| summed over x and y, the median ratio)."""
    a, s, _ = reference(name, with_depth, with_alpha, aa)
    a, s = a.sum(1), np.abs(s).sum(1)
    live = a > 0
    ratio = a[live] / np.maximum(s[live], 1e-300)
    return int(live.sum()), int((ratio >= 10.0).sum()), float(np.median(ratio))


def assert_scene_condition(name):
    """What makes S and L a test of the absolute sums, asserted from the reference: the signed sum cancels for a good share of the rows; L's
    longest list takes more than one 256-entry round.  A property of the scene, so it is asserted once, on the reference of the colour +
    depth loss.  Measured with the draws of image_grads: S 34 of 59 rows at 10 x and more (median ratio 10.7; colour alone 39 of 59, median
    12.4), L 111 of 371 (colour alone 92 of 371, 24.8 %: one row short of the quarter; colour + depth + alpha 106 of 371)."""
    live, big, med = cancellation(name, with_depth=True)
    print(f"scene {name}: {live} rows with a non-zero absolute sum, {big} of them with abs >= 10 |signed|, median ratio {med:.1f}, "
          f"longest list {longest_list(name)}, saturated pixels {saturated_share(name):.2f}")
    assert live > 0 and big >= 0.25 * live, (name, live, big)
    if name == "L":
        assert longest_list(name) > 256
