"""The rasterizer at the settings the other GPU tests never vary, against the CPU oracle in float32: SH degree 2 and below, fewer than 16
stored SH coefficients (the scalar-load forward and the per-thread dL_dsh store of csrc/preprocess.hip), scale_modifier != 1 with gradients,
a background whose channels differ, mixed precomputed inputs, images smaller than one tile.  Run with -m gpu on MI355X.

The forward is checked stage by stage, the backward with a colour gradient and a depth gradient together -- over the whole tensors and, with
the same bound, separately over the rows that take a branch of the per-Gaussian chain rule of their own:

  1. "frustum": the view-space centre is clamped in x or y (the xc / yc flags of project_bwd; computed here from the scene),
  2. "colour":  a channel of the SH colour was clamped at 0 (the mask sh_bwd applies; the oracle's "clamped" field),
  3. "plain":   every other row,

so that a wrong branch which touches a few dozen rows cannot hide in a sum over the whole tensor.

Scene S1 as drawn (800 splats four times their size on 72 x 40 pixels) saturates after a few dozen rows: at scale_modifier 0.6 only 48 rows
carry any gradient (43 frustum, 8 colour, 5 plain), at 1.7 only 16 (16 / 2 / 0), whatever offset the SH rows get.  S1 runs as drawn, with
the subset bound on whatever rows it has; "S1f" is the same scene with every opacity multiplied by 0.05, which lets the rows behind show
through, and there each of the three subsets must hold at least 20 rows with a non-zero oracle gradient in every case (asserted on the
oracle before the GPU runs; measured 49 .. 526 rows).  LIVE_ROWS pins the count of every subset of every case, so that a change of a scene
which empties a subset cannot go unnoticed.  The tests without the gpu mark need no GPU.

Measured on MI355X over the 46 cases: every gradient, whole tensors and subsets, within 6.3e-06 rel-L2 of the oracle (bound 1e-3).  What the
subsets are for, measured with a copy of the oracle whose backward ignores the x clamp flag: on S2 dL/dmeans3D moves by 1.3e-4 over the whole
tensor -- under the bound, the fault would pass -- and by 2.3e-2 over the 25 frustum rows; on S1 / S1f by 0.2 .. 0.7 either way.
"""
import functools
import importlib

import numpy as np
import pytest
import torch

from oracle.raster_oracle import RasterOracle
from scenes import SH_PAIRS, raster_scene, rel_l2
from test_gpu_raster import _geom, _mod, _radii_mismatches_sit_on_a_ceil_boundary, _settings

BG = (0.9, 0.1, 0.4)
SH_OFFSET = 0.6          # subtracted from shs[::5, 0, :] of S1 / S1f: drives colour channels below zero
FAINT = 0.05             # S1f: opacity factor
MIN_SUBSET_ROWS = 20
GRAD_BOUND = 1e-3        # the project's gradient bound (test_gpu_raster.py::test_backward_parity)

SCENES = {
    "S1": dict(n=800, width=72, height=40, seed=41, theta=25.0, extent=3.0, scale_boost=4.0),   # centres beyond 1.3 * tanfov whose splats reach the image
    "S2": dict(n=1500, width=97, height=65, seed=44, theta=200.0, scale_boost=1.5),             # unsaturated pixels: the background matters
    "S3": dict(n=300, width=13, height=9, seed=42, theta=-70.0, scale_boost=2.0),               # one partial tile
    "S4": dict(n=129, width=1, height=1, seed=43, theta=140.0, scale_boost=3.0),                # a 1 x 1 image
}

# (scene, M, degree, scale_modifier, mixed precomputed input or None)
CASES = [(s, M, d, 0.6, None) for s in ("S1", "S1f", "S2") for (M, d) in SH_PAIRS]
CASES += [(s, M, 2, 1.7, None) for s in ("S1", "S1f", "S2") for M in (16, 9)]
CASES += [(s, M, 2, mod, None) for s in ("S3", "S4", "S5_1", "S5_64", "S5_65") for (M, mod) in ((16, 0.6), (9, 0.6), (9, 1.7))]   # S5_n: S3 cut to n rows
CASES += [(s, 0, 2, 0.6, "colors") for s in ("S1", "S1f")] + [(s, 9, 2, 0.6, "cov3D") for s in ("S1", "S1f")]
SMALL_IMAGES = ("S3", "S4", "S5_1", "S5_64", "S5_65")     # too few pixels for a 0.9999 quantile

# rows with a non-zero oracle gradient in (frustum, colour, plain) per case: a property of the inputs, computed by the oracle alone
LIVE_ROWS = {
    "S1-M16-deg2-mod0.6": (43, 8, 5), "S1-M16-deg0-mod0.6": (43, 6, 5), "S1-M12-deg2-mod0.6": (43, 8, 5), "S1-M9-deg2-mod0.6": (43, 8, 5),
    "S1-M9-deg1-mod0.6": (43, 8, 5), "S1-M4-deg1-mod0.6": (43, 8, 5), "S1-M1-deg0-mod0.6": (43, 6, 5), "S1f-M16-deg2-mod0.6": (298, 62, 188),
    "S1f-M16-deg0-mod0.6": (298, 49, 192), "S1f-M12-deg2-mod0.6": (298, 62, 188), "S1f-M9-deg2-mod0.6": (298, 62, 188),
    "S1f-M9-deg1-mod0.6": (298, 56, 189), "S1f-M4-deg1-mod0.6": (298, 56, 189), "S1f-M1-deg0-mod0.6": (298, 49, 192),
    "S2-M16-deg2-mod0.6": (25, 55, 1233), "S2-M16-deg0-mod0.6": (25, 0, 1288), "S2-M12-deg2-mod0.6": (25, 55, 1233),
    "S2-M9-deg2-mod0.6": (25, 55, 1233), "S2-M9-deg1-mod0.6": (25, 31, 1257), "S2-M4-deg1-mod0.6": (25, 31, 1257),
    "S2-M1-deg0-mod0.6": (25, 0, 1288), "S1-M16-deg2-mod1.7": (16, 2, 0), "S1-M9-deg2-mod1.7": (16, 2, 0), "S1f-M16-deg2-mod1.7": (526, 83, 127),
    "S1f-M9-deg2-mod1.7": (526, 83, 127), "S2-M16-deg2-mod1.7": (31, 12, 296), "S2-M9-deg2-mod1.7": (31, 12, 296),
    "S3-M16-deg2-mod0.6": (22, 9, 258), "S3-M9-deg2-mod0.6": (22, 9, 258), "S3-M9-deg2-mod1.7": (5, 3, 60), "S4-M16-deg2-mod0.6": (0, 3, 12),
    "S4-M9-deg2-mod0.6": (0, 3, 12), "S4-M9-deg2-mod1.7": (0, 2, 10), "S5_1-M16-deg2-mod0.6": (0, 0, 1), "S5_1-M9-deg2-mod0.6": (0, 0, 1),
    "S5_1-M9-deg2-mod1.7": (0, 0, 1), "S5_64-M16-deg2-mod0.6": (3, 1, 58), "S5_64-M9-deg2-mod0.6": (3, 1, 58), "S5_64-M9-deg2-mod1.7": (5, 1, 58),
    "S5_65-M16-deg2-mod0.6": (3, 1, 59), "S5_65-M9-deg2-mod0.6": (3, 1, 59), "S5_65-M9-deg2-mod1.7": (5, 1, 59),
    "S1-M0-deg2-mod0.6-colors_precomp": (43, 0, 5), "S1f-M0-deg2-mod0.6-colors_precomp": (298, 0, 215),
    "S1-M9-deg2-mod0.6-cov3D_precomp": (26, 3, 1), "S1f-M9-deg2-mod0.6-cov3D_precomp": (458, 72, 189),
}


@functools.lru_cache(maxsize=None)
def _scene(sid):
    if sid.startswith("S5_"):
        sc = dict(_scene("S3"))
        for k in ("means3D", "shs", "opacities", "scales", "rotations"):
            sc[k] = np.ascontiguousarray(sc[k][:int(sid[3:])])
        return sc
    sc = raster_scene(**SCENES["S1" if sid == "S1f" else sid])
    sc["bg"] = np.array(BG, np.float32)
    if sid in ("S1", "S1f"):
        sc["shs"][::5, 0, :] -= np.float32(SH_OFFSET)
    if sid == "S1f":
        sc["opacities"] = sc["opacities"] * np.float32(FAINT)
    return sc


def _cov3d_of(sc):
    """Sigma = (R S)(R S)^T of the scene's scales and rotations WITHOUT a modifier, in float64 (utils/general_utils.py:84-116)."""
    rot, s = sc["rotations"].astype(np.float64), sc["scales"].astype(np.float64)
    r, x, y, z = rot.T
    Rm = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                   2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    Lm = Rm * s[:, None, :]
    S = Lm @ Lm.transpose(0, 2, 1)
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], -1).astype(np.float32)


def _inputs(sid, M, deg, mixed):
    """The oracle's keyword arguments of one case (numpy, float32): the scene with M coefficients per row, or with one precomputed input."""
    sc = dict(_scene(sid))
    sc["sh_degree"] = deg
    if mixed == "colors":
        del sc["shs"]
        sc["colors_precomp"] = np.random.default_rng(3).random((len(sc["means3D"]), 3)).astype(np.float32)
    else:
        sc["shs"] = np.ascontiguousarray(sc["shs"][:, :M])
    if mixed == "cov3D":
        sc["cov3D_precomp"] = _cov3d_of(sc)
        del sc["scales"], sc["rotations"]
    return sc


def _weights(o):
    """A random dL/dcolor and a random dL/ddepth (seeded), each scaled by the number of its pixels."""
    rng = np.random.default_rng(7)
    dc = rng.standard_normal(o.color.shape).astype(np.float32) / o.color.size
    dd = rng.standard_normal(o.depth.shape).astype(np.float32) / o.depth.size
    return dc, dd


def _subsets(sc, o):
    """{name: bool [P]} -- the three row subsets of the module docstring."""
    V = sc["viewmatrix"].reshape(4, 4).astype(np.float64)
    pv = sc["means3D"].astype(np.float64) @ V[:3, :3] + V[3, :3]
    tz = np.where(pv[:, 2] == 0, 1e-30, pv[:, 2])
    frustum = (np.abs(pv[:, 0] / tz) > 1.3 * sc["tanfovx"]) | (np.abs(pv[:, 1] / tz) > 1.3 * sc["tanfovy"])
    colour = o.field("clamped").reshape(len(frustum), 3).any(axis=1) if "shs" in sc else np.zeros_like(frustum)
    return {"frustum": frustum, "colour": colour, "plain": ~frustum & ~colour}


def _live_rows(g):
    """bool [P]: the oracle gives the row a non-zero gradient in some output."""
    P = g["means3D"].shape[0]
    live = np.zeros(P, bool)
    for v in g.values():
        if v is not None:
            live |= np.abs(v.reshape(P, -1)).sum(axis=1) > 0
    return live


@functools.lru_cache(maxsize=None)
def _reference(sid, M, deg, mod, mixed):
    """(inputs, oracle, dL/dcolor, dL/ddepth, oracle gradients, subsets, live rows per subset, float64 depths): computed once, shared, never changed."""
    sc = _inputs(sid, M, deg, mixed)
    o = RasterOracle(**sc, scale_modifier=mod)
    dc, dd = _weights(o)
    g = o.backward(dc, dd)
    subsets = _subsets(sc, o)
    live = _live_rows(g)
    o64 = RasterOracle(**sc, scale_modifier=mod, dtype=np.float64)      # (depth only, see test_settings_parity)
    depth64 = np.where(o64.radii > 0, o64.field("depth"), np.nan)
    return sc, o, dc, dd, g, subsets, {k: int((m & live).sum()) for k, m in subsets.items()}, depth64


def _oracle_grads(sid, mod=0.6, deg=2, bg=None, weights_of=None):
    sc = _inputs(sid, 16, deg, None)
    if bg is not None:
        sc["bg"] = np.array(bg, np.float32)
    o = RasterOracle(**sc, scale_modifier=mod)
    dc, dd = weights_of if weights_of is not None else _weights(o)
    return o.backward(dc, dd), (dc, dd)


def test_the_inputs_can_tell_the_settings_apart():
    """Oracle alone, no GPU: on S2 each setting this module varies moves the gradient it acts on by at least 1e-2 rel-L2, ten times the bound
    the GPU cases assert -- a kernel that ignored the setting would fail its case.  (S1 is too saturated for the background: 2e-4 there.)
    Measured: background channels swapped 1.6e-2 on the opacity gradient, degree 3 for 2 0.91 on shs, modifier 0.63 for 0.6 0.12 on scales."""
    base, w = _oracle_grads("S2")
    swapped, _ = _oracle_grads("S2", bg=BG[::-1], weights_of=w)
    deg3, _ = _oracle_grads("S2", deg=3, weights_of=w)
    mod63, _ = _oracle_grads("S2", mod=0.63, weights_of=w)
    moved = dict(background=rel_l2(swapped["opacities"], base["opacities"]), degree=rel_l2(deg3["shs"], base["shs"]),
                 modifier=rel_l2(mod63["scales"], base["scales"]))
    print("S2, oracle: rel-L2 moved by the setting: " + ", ".join(f"{k} {v:.3g}" for k, v in moved.items()))
    for k, v in moved.items():
        assert v >= 1e-2, (k, v)


def test_subsets_hold_the_rows_they_are_documented_to_hold():
    """Oracle alone, no GPU: every case has the LIVE_ROWS rows with a non-zero oracle gradient in its three subsets, and on S1f each subset has
    at least MIN_SUBSET_ROWS of them (the GPU cases assert both again before they touch the device)."""
    assert sorted(LIVE_ROWS) == sorted(_case_id(c) for c in CASES)
    for case in CASES:
        _check_live_rows(case, _reference(*case)[6])


def _check_live_rows(case, counts):
    assert (counts["frustum"], counts["colour"], counts["plain"]) == LIVE_ROWS[_case_id(case)], (case, counts)
    if case[0] == "S1f":     # (precomputed colours have no colour clamp)
        for k, n in counts.items():
            assert n >= MIN_SUBSET_ROWS or (k == "colour" and case[4] == "colors"), (case, k, n)


def _case_id(c):
    return f"{c[0]}-M{c[1]}-deg{c[2]}-mod{c[3]}" + (f"-{c[4]}_precomp" if c[4] else "")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_settings_parity(case):
    sid, M, deg, mod, mixed = case
    sc, o, dc, dd, gref, subsets, counts, depth64 = _reference(*case)
    _check_live_rows(case, counts)
    if mixed == "cov3D":    # the modifier scales S in Sigma = (R S)(R S)^T: a precomputed Sigma must not see it (the oracle agrees)
        assert np.array_equal(RasterOracle(**sc, scale_modifier=1.0).color, o.color)
    dev = torch.device("cuda:0")
    R, L = _mod().rasterizer, importlib.import_module("4dgaussians_amd._lib")
    P, W, H = len(sc["means3D"]), sc["image_width"], sc["image_height"]
    names = [k for k in ("means3D", "shs", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp") if k in sc]
    rs = _settings(sc, dev, scale_modifier=mod)

    # ---- forward, per-Gaussian stage: the reference's tile lists (no exact tile culling), so that tiles_touched is comparable
    t = {k: torch.tensor(sc[k], device=dev) for k in names}
    with L.tuning(tile_cull=0):
        _, radii0, _, st = R.rasterize_forward(rs, t["means3D"], t.get("shs"), t.get("colors_precomp"), t["opacities"], t.get("scales"),
                                               t.get("rotations"), t.get("cov3D_precomp"))
        torch.cuda.synchronize()
    radii0 = radii0.cpu().numpy()
    _radii_mismatches_sit_on_a_ceil_boundary(sc | dict(scale_modifier=mod), radii0, o)
    ok = (radii0 == o.radii) & (o.radii > 0)
    recA, recB, recC = (_geom(st, k, (P, 4), torch.float32, dev) for k in (1, 2, 3))
    cov = _geom(st, 4, (P, 6), torch.float32, dev)
    tiles = _geom(st, 5, (P,), torch.int32, dev)
    assert np.array_equal(tiles[ok], o.field("tiles_touched")[ok])
    assert np.array_equal(tiles[radii0 == 0], np.zeros(int((radii0 == 0).sum()), np.int32))
    if ok.any():
        np.testing.assert_allclose(recA[ok, :2], o.field("xy")[ok], rtol=0, atol=2e-3)
        co = o.field("conic_opacity")
        assert rel_l2(recA[ok, 2:4], co[ok, 0:2]) < 1e-5 and rel_l2(recB[ok, 0], co[ok, 2]) < 1e-5
        np.testing.assert_allclose(recB[ok, 1], co[ok, 3], rtol=0, atol=0)
        # depth: the project's rtol 1e-6, against the FLOAT64 oracle.  S1 has centres 0.21 in front of a camera 3 away from them: the sum
        # cancels, the float32 oracle itself is 5.8e-7 off float64 there and the kernel's fused evaluation 5.5e-7 to the other side (1.05e-6
        # apart, both correct to float32) -- a reference that uses up half the bound cannot carry it
        assert not np.isnan(depth64[ok]).any()       # (the float64 oracle culls none of these rows)
        np.testing.assert_allclose(recB[ok, 2], depth64[ok], rtol=1e-6)
        # ... and against the float32 oracle the project's 1e-6 too, but for S1 / S1f, where two float32 evaluations may be two such errors apart
        np.testing.assert_allclose(recB[ok, 2], o.field("depth")[ok], rtol=2e-6 if sid in ("S1", "S1f") else 1e-6)
        np.testing.assert_allclose(recC[ok, :3], o.field("rgb")[ok], rtol=0, atol=1e-5)
        ref_cov = o.field("cov3D")[ok]
        assert (np.abs(cov[ok] - ref_cov) / np.maximum(np.abs(ref_cov).max(axis=1, keepdims=True), 1e-30)).max() < 1e-5

    # ---- the module under autograd, default knobs
    t = {k: torch.tensor(sc[k], device=dev, requires_grad=True) for k in names}
    means2D = torch.zeros(P, 3, device=dev, requires_grad=True)
    color, radii, depth = R.GaussianRasterizer(rs)(means3D=t["means3D"], means2D=means2D, shs=t.get("shs"), colors_precomp=t.get("colors_precomp"),
                                                   opacities=t["opacities"], scales=t.get("scales"), rotations=t.get("rotations"),
                                                   cov3D_precomp=t.get("cov3D_precomp"))
    ((color * torch.tensor(dc, device=dev)).sum() + (depth * torch.tensor(dd, device=dev)).sum()).backward()
    torch.cuda.synchronize()
    radii = radii.cpu().numpy()
    assert np.array_equal(radii, radii0)
    color, depth = color.detach().cpu().numpy(), depth.detach().cpu().numpy()
    d, ddep = np.abs(color - o.color), np.abs(depth - o.depth)
    psnr = 10 * np.log10(1.0 / max(float(((color - o.color) ** 2).mean()), 1e-20))
    print(f"[{_case_id(case)}] image: mean|dC| {d.mean():.2e} max|dC| {d.max():.2e} psnr {psnr:.1f} dB; depth: mean {ddep.mean():.2e} max {ddep.max():.2e}")
    assert color.shape == (3, H, W) and depth.shape == (1, H, W)
    assert d.mean() < 2e-6 and psnr > 80.0 and ddep.mean() < 2e-5
    if sid in SMALL_IMAGES:
        assert d.max() < 5e-5 and ddep.max() < 5e-4
    else:
        assert np.quantile(d, 0.9999) < 5e-5 and np.quantile(ddep, 0.9999) < 5e-4

    # ---- backward: whole tensors, then the subsets
    ref_name = dict(colors_precomp="colors", cov3D_precomp="cov3D")
    grads = {k: (t[k].grad.cpu().numpy(), gref[ref_name.get(k, k)].reshape(sc[k].shape)) for k in names}
    grads["means2D"] = (means2D.grad.cpu().numpy(), gref["means2D"])
    for k in names:
        assert t[k].grad.shape == t[k].shape, k
    if "shs" in sc:
        assert t["shs"].grad.shape == (P, M, 3)
    errs = {k: rel_l2(a, b) for k, (a, b) in grads.items()}
    print(f"[{_case_id(case)}] grad rel-L2: " + ", ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < GRAD_BOUND, (k, v)
    for name, rows in subsets.items():
        if counts[name] == 0:
            print(f"[{_case_id(case)}] subset {name}: no row with a gradient")
            continue
        sub = {k: rel_l2(a[rows], b[rows]) for k, (a, b) in grads.items()}
        print(f"[{_case_id(case)}] subset {name}: {counts[name]} rows with a gradient of {int(rows.sum())}: " + ", ".join(f"{k}={v:.2e}" for k, v in sub.items()))
        for k, v in sub.items():
            assert v < GRAD_BOUND, (name, k, v)

    # ---- exact zeros: inactive SH bands (inside a short row and inside a 16-coefficient row), every row of a culled Gaussian
    if "shs" in sc:
        assert not np.any(grads["shs"][0][:, (deg + 1) ** 2:]), "an inactive SH band received a gradient"
    culled = radii == 0
    for k, (a, _) in grads.items():
        assert not np.any(a[culled]), f"{k}: a culled Gaussian received a gradient"
