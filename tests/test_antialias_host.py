"""The opacity compensation of csrc/gs_math.h executed WITHOUT a GPU: the three *_aa host twins (csrc/preprocess.hip) against the float64
restatement of tests/antialias_common.py.

  forward   every field fdgs_preprocess_host returns is returned bit for bit; opacity_eff is the float64 opacity * h within 4 float32 ulp,
            and a row at the floor gets exactly opacity * sqrt(2.5e-5), rounded.
  backward  against float64 autograd of raster_torch.project's outputs contracted with seeded sums, plus opacity * h contracted with the
            opacity sums: rel-L2 < 1e-3 per group over all rows, the clamped rows alone and the floor rows alone.  The float32 autograd of
            the same contraction against the float64 one is printed beside each figure: the reference's own share of the bound.
            With d_opacity = 0 every output is fdgs_preprocess_bwd_host's, bit for bit; on floor rows the geometry outputs are, whatever
            d_opacity is.
  camera    fdgs_camera_grad_host_aa against float64 autograd with respect to the three camera tensors, same bound.
"""
import numpy as np
import pytest
import torch

import antialias_common as AC
from scenes import rel_l2

CASES = [(P, kind, mod) for P in AC.SIZES for kind in AC.KINDS for mod in AC.MODS] + [(AC.WIDE[0], "sh16", 1.0, AC.WIDE[1], AC.WIDE[2])]


def _case(c):
    P, kind, mod = c[:3]
    size = c[3:] or (AC.W, AC.H)
    sc = AC.inputs(P, kind, *size)
    if kind == "cov3d":
        sc = AC.with_cov3d(sc, mod)
    return sc, mod


def _id(c):
    return "-".join(str(x) for x in c)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_twin_returns_the_plain_fields_and_the_compensated_opacity(case):
    sc, mod = _case(case)
    plain, _, _ = AC.twin_forward(sc, mod, aa=False)
    out, _, _ = AC.twin_forward(sc, mod, aa=True)
    for k in AC.FWD_KEYS:
        assert np.array_equal(out[k].view(np.uint32) if out[k].dtype == np.float32 else out[k],
                              plain[k].view(np.uint32) if plain[k].dtype == np.float32 else plain[k]), k
    h, r, cl, vis = AC.h64(sc, mod)
    seen = out["tiles"] > 0
    assert (seen != vis).mean() < 2e-3                      # (a radius on a ceil boundary may cull on one side only)
    assert not np.any(out["opacity_eff"][~seen]), "a culled row has an effective opacity"
    rows = seen & vis
    op = sc["opacities"].reshape(-1).astype(np.float64)
    want = op * h
    u = AC.ulps(out["opacity_eff"][rows], want[rows])
    floor = rows & (r <= AC.FLOOR)
    print(f"[{_id(case)}] opacity_eff vs float64 opacity * h: max {u.max():.2f} ulp over {int(rows.sum())} rows, {int(floor.sum())} at the floor, "
          f"h in [{h[rows].min():.4f}, {h[rows].max():.6f}]")
    assert u.max() <= 4.0, u.max()
    sure = floor & (r < 0.5 * AC.FLOOR)                      # (well below it: float32 and float64 agree on the side)
    exact = (sc["opacities"].reshape(-1)[sure] * np.sqrt(np.float32(AC.FLOOR))).astype(np.float32)
    assert np.array_equal(out["opacity_eff"][sure], exact)
    if case[0] >= 257:
        assert int(sure.sum()) >= 8


def _backward_case(case):
    sc, mod = _case(case)
    out, p, keep = AC.twin_forward(sc, mod, aa=True)
    h, r, cl, vis = AC.h64(sc, mod)
    mask = (vis & (out["tiles"] > 0)).astype(np.float64)
    w = AC.weights(sc, out["radii"])
    return sc, mod, out, p, keep, r, cl, mask, w


def _groups(sc):
    g = ["means2D", "means3D", "cov3D", "opacities"]
    if sc.get("shs") is not None:
        g.append("shs")
    if sc.get("scales") is not None:
        g += ["scales", "rotations"]
    return g


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_backward_twin_against_float64_autograd(case):
    sc, mod, out, p, keep, r, cl, mask, w = _backward_case(case)
    if mask.sum() == 0:
        pytest.fail("the scene has no visible row")
    share = AC.assert_h_path_is_material(sc, mod, w, mask)
    M = 0 if sc.get("shs") is None else sc["shs"].shape[1]
    subsets = {"all": np.ones(len(mask), bool)}
    if case[0] >= 257:
        subsets["clamped"], subsets["floor"] = cl, r <= AC.FLOOR
    print(f"[{_id(case)}] the compensation's share of the scales / covariance gradient: {share:.3f}")
    failures = []
    for name, rows in subsets.items():
        m = mask * rows
        if name != "all":
            assert int(m.sum()) >= 8, (name, int(m.sum()))
        ref, _ = AC.autograd(sc, mod, w, m)
        own, _ = AC.autograd(sc, mod, w, m, dtype=torch.float32)
        got = AC.twin_backward(p, out, AC.sums_f32(w, m), M)
        for k in _groups(sc):
            a = got[k][:, :M] if k == "shs" else got[k]
            assert np.isfinite(a).all(), (name, k)
            e, e32 = rel_l2(a, ref[k].reshape(a.shape)), rel_l2(own[k], ref[k])
            print(f"   {name:8s} {k:10s} twin vs float64 {e:.2e}   (float32 autograd vs float64 {e32:.2e})")
            if not e < AC.GRAD_BOUND:
                failures.append((name, k, e))
        if name == "floor":                # at the floor h is a constant: the opacity gets sqrt(2.5e-5) * g, the geometry nothing from it
            sure = (m > 0) & (r < 0.5 * AC.FLOOR)
            want = (np.sqrt(np.float32(AC.FLOOR)) * AC.sums_f32(w, m)["opacity"][sure]).astype(np.float32)
            assert np.array_equal(got["opacities"][sure], want)
    assert not failures, failures


@pytest.mark.parametrize("case", [c for c in CASES if c[0] >= 257 and c[2] == 1.0], ids=_id)
def test_backward_twin_without_an_opacity_sum_is_the_plain_twin_and_floor_rows_ignore_it(case):
    sc, mod, out, p, keep, r, cl, mask, w = _backward_case(case)
    M = 0 if sc.get("shs") is None else sc["shs"].shape[1]
    s = AC.sums_f32(w, mask)
    plain = AC.twin_backward(p, out, s, M, aa=False)
    zero = dict(s, opacity=np.zeros_like(s["opacity"]))
    got0 = AC.twin_backward(p, out, zero, M, aa=True)
    for k in AC.BWD_KEYS:
        assert np.array_equal(got0[k].view(np.uint32), plain[k].view(np.uint32)), k
    assert not np.any(got0["opacities"])
    got = AC.twin_backward(p, out, s, M, aa=True)
    floor = (mask > 0) & (r < 0.5 * AC.FLOOR)
    assert int(floor.sum()) >= 8
    changed = 0
    for k in AC.BWD_KEYS:
        assert np.array_equal(got[k][floor].view(np.uint32), plain[k][floor].view(np.uint32)), k
        changed += int(np.any(got[k][~floor] != plain[k][~floor]))
    assert changed >= 2, "the opacity sums reach no geometry gradient off the floor"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_camera_twin_against_float64_autograd(case):
    sc, mod, out, p, keep, r, cl, mask, w = _backward_case(case)
    _, ref = AC.autograd(sc, mod, w, mask)
    _, own = AC.autograd(sc, mod, w, mask, dtype=torch.float32)
    _, part = AC.autograd(sc, mod, w, mask, parts=("h",))
    got = AC.twin_camera(p, out, AC.sums_f32(w, mask))
    view = lambda v: v[:16].reshape(4, 4)[:, :3]
    proj = lambda v: v[16:32].reshape(4, 4)[:, (0, 1, 3)]
    share = np.linalg.norm(view(part)) / np.linalg.norm(view(ref))
    print(f"[{_id(case)}] the compensation's share of the view matrix' gradient: {share:.3f}")
    assert share > 1e-2, share
    assert not np.any(proj(part)) and not np.any(part[32:35]), "the compensation reaches the view matrix only"
    groups = {"view": view, "proj": proj}
    if sc.get("shs") is not None:
        groups["campos"] = lambda v: v[32:35]
    for k, f in groups.items():
        e, e32 = rel_l2(f(got), f(ref)), rel_l2(f(own), f(ref))
        print(f"   {k:6s} twin vs float64 {e:.2e}   (float32 autograd vs float64 {e32:.2e})")
        assert e < AC.GRAD_BOUND, (k, e)
    assert not np.any(got[:16].reshape(4, 4)[:, 3]) and not np.any(got[16:32].reshape(4, 4)[:, 2]) and not np.any(got[35:])
    plain = AC.twin_camera(p, out, dict(AC.sums_f32(w, mask), opacity=np.zeros(len(mask), np.float32)))
    assert np.array_equal(plain, AC.twin_camera(p, out, AC.sums_f32(w, mask), aa=False))
