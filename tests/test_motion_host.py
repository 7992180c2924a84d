"""Motion vectors in the C-ABI, host side (no GPU): the *_host twins of fdgs_motion_rows / fdgs_motion_resolve run the very functions the
device kernels compile (csrc/motion_ops.h), over host arrays.

Every float32 operation of motion_ops.h is ONE IEEE operation in the written order, and numpy's float32 + - * / are single IEEE operations
too: the numpy restatements below equal the library bit for bit.  The one inexact comparison is against the float64 evaluation of the same
formula, with a bound that is derived, not measured (u = 2**-24; S the image extent; Sh, Sw the sums of the absolute terms of h and w;
d = w + 1e-7; x = h / d):
    h: three products and three sums, |dh| <= 4 u Sh;  w the same, then d = w + eps one more, r = 1 / d one more, x = h * r one more:
       |dx| <= u [4 Sh / |d| + |x| (4 Sw / |d| + 3)]
    pix = ((x + 1) S - 1) / 2: three more roundings on values <= (|x| + 2) S (the halving is exact):
       B(pix) = u (S / 2) [4 Sh / |d| + |x| (4 Sw / |d| + 3) + 3 (|x| + 2)]
    motion = pix_to - pix_at, one rounding:  |motion - ref| <= 2 (B_to + B_at + u |ref|), the factor 2 for the second-order terms."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

fdgs = importlib.import_module("4dgaussians_amd")
syn = fdgs.synthetic
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
W, H = 96, 64
NEW = ("fdgs_motion_rows", "fdgs_motion_rows_host", "fdgs_motion_resolve", "fdgs_motion_resolve_host")
SIZES = [0, 1, 255, 256, 257, 4099]
F = np.float32
EPS = F(1e-7)
NEAR = F(0.2)
SENTINEL = F(-77.25)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(fdgs._lib.LIB_PATH):
        importlib.import_module("4dgaussians_amd.build").build()
    return fdgs._lib.lib()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def camera_matrices(theta, time=0.0, w=W, h=H):
    """(view [16], proj [16]) float32, in the layout the rasterizer reads: element m[4 * j + i]."""
    cam = syn.make_camera(w, h, theta_deg=theta, time=time)
    return (np.ascontiguousarray(cam.world_view_transform.numpy().reshape(-1), dtype=np.float32),
            np.ascontiguousarray(cam.full_proj_transform.numpy().reshape(-1), dtype=np.float32), cam.camera_center.numpy().astype(np.float32))


def positions(n, seed=7):
    """(xyz_at, xyz_to) [n,3] float32: make_gaussians' positions and a displaced copy; where there are rows enough, rows 1, 2 sit at the AT
    camera's centre in the at set (culled there only), rows 3, 4 at the TOWARD camera's centre in the toward set, rows 5, 6 both."""
    at = syn.make_gaussians(max(n, 1), seed=seed)["xyz"].numpy().astype(np.float32)[:n].copy()
    rng = np.random.default_rng(seed)
    to = (at + rng.normal(0.0, 0.05, at.shape).astype(np.float32)).astype(np.float32)
    return at, to


def with_culled_rows(at, to, centre_at, centre_to):
    at, to = at.copy(), to.copy()
    n = at.shape[0]
    one_at, one_to, both = [r for r in (1, 2) if r < n], [r for r in (3, 4) if r < n], [r for r in (5, 6) if r < n]
    for r in one_at + both:
        at[r] = centre_at + F(0.01) * F(r)
    for r in one_to + both:
        to[r] = centre_to - F(0.01) * F(r)
    return at, to, one_at, one_to, both


def np_zview(v, p):
    z = v[2] * p[:, 0]
    z = z + v[6] * p[:, 1]
    z = z + v[10] * p[:, 2]
    return z + v[14]


def np_pix(m, p, S, k):
    """motion_pix of csrc/motion_ops.h, operation by operation in np.float32."""
    h = m[k] * p[:, 0]
    h = h + m[4 + k] * p[:, 1]
    h = h + m[8 + k] * p[:, 2]
    h = h + m[12 + k]
    w = m[3] * p[:, 0]
    w = w + m[7] * p[:, 1]
    w = w + m[11] * p[:, 2]
    w = w + m[15]
    d = w + EPS
    r = F(1.0) / d
    x = h * r
    t = x + F(1.0)
    t = t * F(S)
    t = t - F(1.0)
    return t * F(0.5)


def np_rows(view_at, proj_at, at, view_to, proj_to, to, w=W, h=H):
    with np.errstate(all="ignore"):
        ok = (np_zview(view_at, at) > NEAR) & (np_zview(view_to, to) > NEAR)
        dx = np_pix(proj_to, to, w, 0) - np_pix(proj_at, at, w, 0)
        dy = np_pix(proj_to, to, h, 1) - np_pix(proj_at, at, h, 1)
    out = np.stack([np.where(ok, dx, F(0)), np.where(ok, dy, F(0)), np.ones_like(dx)], axis=1).astype(np.float32)
    assert out.dtype == np.float32 and dx.dtype == np.float32
    return out, ok


def host_rows(lib, at, to, view_at, proj_at, view_to, proj_to, stride, w=W, h=H, offset_rows=1):
    """fdgs_motion_rows_host with every base pointer `offset_rows` rows (12 bytes each) into its allocation -> ([n, stride] result, the
    guard floats in front of and behind it)."""
    n = at.shape[0]
    pad = 3 * offset_rows
    a = np.full((n + offset_rows, 3), 9.0, np.float32); a[offset_rows:] = at
    b = np.full((n + offset_rows, 3), 9.0, np.float32); b[offset_rows:] = to
    out = np.full(pad + n * stride + 4, SENTINEL, np.float32)
    rc = lib.fdgs_motion_rows_host(n, a.ctypes.data + 4 * pad, b.ctypes.data + 4 * pad, view_at.ctypes.data, proj_at.ctypes.data,
                                   view_to.ctypes.data, proj_to.ctypes.data, w, h, out.ctypes.data + 4 * pad, stride)
    assert rc == 0, lib.fdgs_last_error()
    return out[pad:pad + n * stride].reshape(n, stride).copy(), np.concatenate([out[:pad], out[pad + n * stride:]])


def host_resolve(lib, raw, min_alpha):
    _, h, w = raw.shape
    raw = np.ascontiguousarray(raw, dtype=np.float32)
    motion, alpha = np.full((2, h, w), SENTINEL, np.float32), np.full((1, h, w), SENTINEL, np.float32)
    rc = lib.fdgs_motion_resolve_host(h, w, float(min_alpha), raw.ctypes.data, motion.ctypes.data, alpha.ctypes.data)
    assert rc == 0, lib.fdgs_last_error()
    return motion, alpha


def resolve_image(h, w, min_alpha, seed=3):
    """raw [3,h,w] float32 whose third plane holds, among values in [0, 1), an exact 0, min_alpha itself, the float just above it and a NaN
    (as far as there are pixels)."""
    rng = np.random.default_rng(seed)
    raw = rng.normal(0.0, 3.0, (3, h, w)).astype(np.float32)
    a = rng.random(h * w).astype(np.float32)
    special = [F(0.0), F(min_alpha), np.nextafter(F(min_alpha), F(np.inf)), F(np.nan), F(-0.0)]
    if h * w == 1:
        a[0] = special[2]
    else:
        for k, v in enumerate(special[:h * w]):
            a[(k * 7) % (h * w)] = v
    raw[2] = a.reshape(h, w)
    return raw


def np_resolve(raw, min_alpha):
    a = raw[2]
    with np.errstate(all="ignore"):
        ok = a > F(min_alpha)
        motion = np.stack([np.where(ok, raw[0] / a, F(0)), np.where(ok, raw[1] / a, F(0))]).astype(np.float32)
    return motion, a[None].copy()


# ---- tests -----------------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_four_functions_and_lib_binds_them(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fdgs.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in fdgs._lib.SYMBOLS and hasattr(lib, name), name
    assert lib.fdgs_abi_version() == 6 and fdgs._lib.ABI_VERSION == 6
    assert "motion.hip" in importlib.import_module("4dgaussians_amd.build").SOURCES
    assert len(fdgs._lib.SYMBOLS["fdgs_motion_rows"][1]) == len(fdgs._lib.SYMBOLS["fdgs_motion_rows_host"][1]) + 1 == 12
    assert len(fdgs._lib.SYMBOLS["fdgs_motion_resolve"][1]) == len(fdgs._lib.SYMBOLS["fdgs_motion_resolve_host"][1]) + 1 == 7


@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("n", SIZES)
def test_rows_host_equals_the_numpy_restatement_bit_for_bit(lib, n, stride):
    view_at, proj_at, c_at = camera_matrices(20.0)
    view_to, proj_to, c_to = camera_matrices(31.0)
    at, to = positions(n)
    at, to, one_at, one_to, both = with_culled_rows(at, to, c_at, c_to)
    got, guard = host_rows(lib, at, to, view_at, proj_at, view_to, proj_to, stride)
    ref, ok = np_rows(view_at, proj_at, at, view_to, proj_to, to)
    assert np.array_equal(bits(got[:, :3]), bits(ref))
    assert np.array_equal(bits(guard), bits(np.full_like(guard, SENTINEL)))           # nothing outside the n rows is written
    if stride == 4:
        assert np.array_equal(bits(got[:, 3]), np.zeros(n, np.uint32))               # +0
    # the near cull, in either view: exactly (+0, +0, 1)
    z_at, z_to = np_zview(view_at, at), np_zview(view_to, to)
    assert all(z_at[r] <= NEAR and z_to[r] > NEAR for r in one_at) and all(z_to[r] <= NEAR and z_at[r] > NEAR for r in one_to)
    assert all(z_at[r] <= NEAR and z_to[r] <= NEAR for r in both)
    culled = one_at + one_to + both
    assert sorted(np.flatnonzero(~ok).tolist()) == sorted(culled)
    for r in culled:
        assert bits(got[r, :3]).tolist() == bits(np.array([0.0, 0.0, 1.0])).tolist()
    if n >= 255:
        assert len(culled) == 6 and float(np.abs(got[:, :2]).max()) > 1.0             # (and the others do move)
    assert np.array_equal(bits(got[:, 2]), bits(np.ones(n)))


def test_rows_host_of_a_frame_toward_itself_is_exactly_zero(lib):
    view, proj, centre = camera_matrices(-75.0)
    at, _ = positions(4099)
    at[5] = centre                                                                   # (one culled row among them)
    for stride in (3, 4):
        got, _ = host_rows(lib, at, at, view, proj, view, proj, stride)
        want = np.zeros((4099, stride), np.float32)
        want[:, 2] = 1.0
        assert np.array_equal(bits(got), bits(want))                                 # (+0, +0, 1 [, +0])


def _pix64(m, p, S, k):
    """(pix, B(pix)) in float64 on the float32 inputs: the same formula and the bound of the module docstring."""
    m, p = m.astype(np.float64), p.astype(np.float64)
    terms_h = [m[k] * p[:, 0], m[4 + k] * p[:, 1], m[8 + k] * p[:, 2], np.full(p.shape[0], m[12 + k])]
    terms_w = [m[3] * p[:, 0], m[7] * p[:, 1], m[11] * p[:, 2], np.full(p.shape[0], m[15])]
    h, w = sum(terms_h), sum(terms_w)
    Sh, Sw = sum(np.abs(t) for t in terms_h), sum(np.abs(t) for t in terms_w)
    d = w + float(EPS)
    x = h / d
    pix = ((x + 1.0) * S - 1.0) * 0.5
    B = U * (S / 2.0) * (4.0 * Sh / np.abs(d) + np.abs(x) * (4.0 * Sw / np.abs(d) + 3.0) + 3.0 * (np.abs(x) + 2.0))
    return pix, B


@pytest.mark.parametrize("n", [257, 4099])
def test_rows_host_against_float64_within_the_derived_bound(lib, n):
    view_at, proj_at, _ = camera_matrices(20.0)
    view_to, proj_to, _ = camera_matrices(31.0)
    at, to = positions(n, seed=11)
    got, _ = host_rows(lib, at, to, view_at, proj_at, view_to, proj_to, 3)
    assert bool((np_zview(view_at, at) > 1.0).all() and (np_zview(view_to, to) > 1.0).all())      # nothing near the cull
    for k, S in ((0, W), (1, H)):
        p_to, B_to = _pix64(proj_to, to, S, k)
        p_at, B_at = _pix64(proj_at, at, S, k)
        ref = p_to - p_at
        bound = 2.0 * (B_to + B_at + U * np.abs(ref))
        err = np.abs(got[:, k].astype(np.float64) - ref)
        print(f"n={n} k={k}: max |motion - float64| = {err.max():.3e}, min bound = {bound.min():.3e}, max err / bound = {(err / bound).max():.3f}")
        assert bool((err <= bound).all())
        assert float(np.abs(ref).max()) > 1.0 and float(bound.max()) < 1e-3           # (a bound that says something)


@pytest.mark.parametrize("min_alpha", [0.0, 0.25])
@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (64, 96)])
def test_resolve_host_equals_the_float32_division_bit_for_bit(lib, shape, min_alpha):
    raw = resolve_image(*shape, min_alpha)
    motion, alpha = host_resolve(lib, raw, min_alpha)
    ref_motion, ref_alpha = np_resolve(raw, min_alpha)
    assert np.array_equal(bits(motion), bits(ref_motion))
    assert np.array_equal(bits(alpha), bits(ref_alpha)) and np.array_equal(bits(alpha[0]), bits(raw[2]))       # a copy of plane 2, NaN included
    a = raw[2]
    off = ~(a > F(min_alpha))                                                        # a == 0, a == min_alpha, NaN: exactly +0
    assert np.array_equal(bits(motion[:, off]), np.zeros((2, int(off.sum())), np.uint32))
    if shape != (1, 1):
        assert bool(np.isnan(a).any()) and bool((a == F(min_alpha)).any()) and bool((a == np.nextafter(F(min_alpha), F(np.inf))).any())
        just_above = a == np.nextafter(F(min_alpha), F(np.inf))
        assert bool((motion[0][just_above] != 0).all())
    else:
        assert bool((motion != 0).all())


def test_bad_arguments_are_refused_with_a_message(lib):
    view, proj, _ = camera_matrices(0.0)
    at, to = positions(8)
    out = np.zeros((8, 4), np.float32)
    good = dict(N=8, at=at.ctypes.data, to=to.ctypes.data, va=view.ctypes.data, pa=proj.ctypes.data, vt=view.ctypes.data, pt=proj.ctypes.data,
                W=W, H=H, out=out.ctypes.data, stride=4)
    assert lib.fdgs_motion_rows_host(*good.values()) == 0
    bad = [dict(N=-1), dict(stride=2), dict(stride=5), dict(W=0), dict(H=0), dict(H=-3)] + [{k: None} for k in ("at", "to", "va", "pa", "vt", "pt", "out")]
    for change in bad:
        before = out.copy()
        assert lib.fdgs_motion_rows_host(*{**good, **change}.values()) == -1, change      # FDGS_E_INVALID
        assert lib.fdgs_last_error(), change
        assert np.array_equal(out, before)
    raw, motion, alpha = np.ones((3, 4, 5), np.float32), np.zeros((2, 4, 5), np.float32), np.zeros((1, 4, 5), np.float32)
    good = dict(H=4, W=5, min_alpha=0.0, raw=raw.ctypes.data, motion=motion.ctypes.data, alpha=alpha.ctypes.data)
    assert lib.fdgs_motion_resolve_host(*good.values()) == 0
    for change in [dict(H=0), dict(W=0), dict(W=-1), dict(raw=None), dict(motion=None), dict(alpha=None)]:
        assert lib.fdgs_motion_resolve_host(*{**good, **change}.values()) == -1, change
        assert lib.fdgs_last_error(), change
