"""Scene composition, host side (no GPU): fdgs_state_place_host runs the very functions the device kernel compiles (csrc/compose_ops.h)
over host arrays; the pure-Python part of fdgs.compose; the placement convention through the float64 rasterizer oracle.

Bounds (u = 2**-24, the float32 unit roundoff; none of them is measured).  A sum of n products evaluated left to right has, on every
term, one rounding for the product and at most one per addition it passes through; with k the largest number of roundings on one term,
|out - ref| <= k u sum|terms| to first order, the reference being the float64 evaluation with the float32-ROUNDED placement parameters:
  positions       s p (1), the product with R (1), two additions, the shift (1): 5, taken as k = 6; terms |R_ij| |s p_j| and |d_i|
  quaternions     a product and three additions: 4, taken as k = 5; terms the four |qR_i| |q_j| of a component
  SH band l       a product and 2 l + 1 additions (the first one to +0 is exact): k = 2 l + 2; terms |in_j| |M_l[j][k]|
  output norms    each component is off by at most 4 u sum|terms| <= 4 u, the inputs' norms are within 2 u of 1: |norm - 1| <= 8 u
Scales are one rounding of np.float32(s) * x: exact against numpy's float32 product.  Opacity, everything mode POINTS copies, the zeroed
bands, the identity placement, the fused blend and the field masks are exact."""
import importlib
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from test_playback_host import WEIGHTS, _state, host_blend

fdgs = importlib.import_module("4dgaussians_amd")
C, P = fdgs.compose, fdgs.playback
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
KEYS = ("xyz", "scales", "rot", "opacity", "shs")            # test_playback_host's names, in the order of playback.FIELDS
ALL = 31


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(fdgs._lib.LIB_PATH):
        importlib.import_module("4dgaussians_amd.build").build()
    return fdgs._lib.lib()


def axis_angle(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def script_rotation(theta, phi):
    Rz = np.array([[math.cos(theta), -math.sin(theta), 0], [math.sin(theta), math.cos(theta), 0], [0, 0, 1.0]])
    Rx = np.array([[1.0, 0, 0], [0, math.cos(phi), -math.sin(phi)], [0, math.sin(phi), math.cos(phi)]])
    return Rz @ Rx


R_GENERAL = axis_angle((0.3, -1.0, 0.5), 1.1)
D_GENERAL = (0.4, -0.3, 0.25)


def general_placement(mode="rigid", **kw):
    return C.Placement(rotation=R_GENERAL, translation=D_GENERAL, scale=1.7, mode=mode, **kw)


def host_place(lib, pstruct, a, b=None, w=0.0, mask=ALL, out=None):
    """fdgs_state_place_host on test_playback_host-style dicts of CPU tensors -> dict of CPU tensors (NaN where nothing was written)."""
    n = a["rot"].shape[0]
    if out is None:
        out = {k: torch.full_like(a[k], float("nan")) for k in KEYS}
    sa, sb, so = fdgs._lib.StateArrays(), fdgs._lib.StateArrays(), fdgs._lib.StateArrays()
    for h, (k, name) in enumerate(zip(KEYS, P.FIELDS)):
        if mask >> h & 1:
            assert a[k].is_contiguous() and a[k].dtype == torch.float32 and out[k].is_contiguous()
            setattr(sa, name, a[k].data_ptr())
            setattr(so, name, out[k].data_ptr())
            if b is not None:
                setattr(sb, name, b[k].data_ptr())
    rc = lib.fdgs_state_place_host(pstruct, n, mask, sa, sb if b is not None else None, w, so)
    assert rc == 0, lib.fdgs_last_error()
    return out


def hamilton(a, b):
    """a [4] (x) b [n,4], (r, x, y, z); returns the products' values and the sum of their magnitudes per component."""
    idx = (((0, 0, 1), (1, 1, -1), (2, 2, -1), (3, 3, -1)), ((0, 1, 1), (1, 0, 1), (2, 3, 1), (3, 2, -1)),
           ((0, 2, 1), (1, 3, -1), (2, 0, 1), (3, 1, 1)), ((0, 3, 1), (1, 2, 1), (2, 1, -1), (3, 0, 1)))
    val = np.stack([sum(s * a[i] * b[:, j] for i, j, s in comp) for comp in idx], axis=1)
    mag = np.stack([sum(abs(a[i] * b[:, j]) for i, j, s in comp) for comp in idx], axis=1)
    return val, mag


def sh_block(pl):
    """blockdiag(1, M1, M2, M3) [16,16] of the float32 matrices the placement passes, in float64."""
    B = np.zeros((16, 16))
    B[0, 0] = 1.0
    for l, M in zip((1, 2, 3), pl.sh):
        B[l * l:(l + 1) ** 2, l * l:(l + 1) ** 2] = M.astype(np.float64)
    return B


def check_against_float64(got, src, pl, deg):
    """`got` = place(src) with placement pl and SH degree deg, against the float64 formulas within the docstring's bounds."""
    s, R, d = float(pl.scale), pl.rotation.astype(np.float64), pl.translation.astype(np.float64)
    p = src["xyz"].double().numpy()
    ref = (s * p) @ R.T + d
    bound = 6 * U * (np.abs(s * p) @ np.abs(R).T + np.abs(d))
    assert (np.abs(got["xyz"].double().numpy() - ref) <= bound).all()
    assert np.array_equal(got["scales"].numpy(), pl.scale * src["scales"].numpy())                       # one float32 product
    assert torch.equal(got["opacity"], src["opacity"])
    shs, out = src["shs"].double().numpy(), got["shs"].double().numpy()
    assert np.array_equal(got["shs"][:, 0].numpy(), src["shs"][:, 0].numpy())                            # band 0: a copy
    nlive = (deg + 1) ** 2
    assert (got["shs"][:, nlive:] == 0).all() and not np.signbit(got["shs"][:, nlive:].numpy()).any()    # +0.0 exactly
    if pl.mode == "points":
        assert torch.equal(got["rot"], src["rot"])
        assert torch.equal(got["shs"][:, :nlive], src["shs"][:, :nlive])
        return
    val, mag = hamilton(pl.quat.astype(np.float64), src["rot"].double().numpy())
    assert (np.abs(got["rot"].double().numpy() - val) <= 5 * U * mag).all()
    assert float(np.abs(np.linalg.norm(got["rot"].double().numpy(), axis=1) - 1).max()) <= 8 * U
    B = sh_block(pl)
    for l in range(1, deg + 1):
        lo, hi = l * l, (l + 1) ** 2
        ref = np.einsum("njc,jk->nkc", shs[:, lo:hi], B[lo:hi, lo:hi])
        bound = (2 * l + 2) * U * np.einsum("njc,jk->nkc", np.abs(shs[:, lo:hi]), np.abs(B[lo:hi, lo:hi]))
        assert (np.abs(out[:, lo:hi] - ref) <= bound).all(), l
        assert not np.array_equal(out[:, lo:hi], shs[:, lo:hi])


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------

def test_header_declares_the_placement_abi_and_lib_binds_it(lib):
    text = open(os.path.join(ROOT, "include", "fdgs.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("fdgs_state_place", "fdgs_state_place_host"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in fdgs._lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"#define\s+FDGS_PLACE_POINTS\s+0\b", src) and re.search(r"#define\s+FDGS_PLACE_RIGID\s+1\b", src)
    assert fdgs._lib.PLACE_MODES == {"points": 0, "rigid": 1}

    def fields(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
        return [re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*(\[[^\]]*\])?\s*$", part.strip()).group(1)
                for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert fields("fdgs_placement") == [f[0] for f in fdgs._lib.Placement._fields_]
    assert fields("fdgs_state_arrays") == [f[0] for f in fdgs._lib.StateArrays._fields_] == list(P.FIELDS)
    import ctypes
    assert ctypes.sizeof(fdgs._lib.Placement) == 4 * (1 + 9 + 4 + 3 + 9 + 25 + 49 + 2)
    assert "compose.hip" in importlib.import_module("4dgaussians_amd.build").SOURCES
    assert lib.fdgs_abi_version() == 6
    assert "compose" in fdgs.__all__ and "compose" in fdgs.__doc__ and "stale" in C.Composite.__doc__


# ---- sh_rotation --------------------------------------------------------------------------------------------------------------------

ROTATIONS = {"identity": np.eye(3), "script": script_rotation(0.7, -0.4), "general": R_GENERAL}


@pytest.mark.parametrize("name", list(ROTATIONS))
def test_sh_rotation(name):
    R = ROTATIONS[name]
    Ms = C.sh_rotation(R)
    assert [M.shape for M in Ms] == [(3, 3), (5, 5), (7, 7)] and all(M.dtype == np.float64 for M in Ms)
    for M in Ms:
        assert np.abs(M @ M.T - np.eye(len(M))).max() <= 1e-12
    if name == "identity":
        for M in Ms:
            assert np.array_equal(M.astype(np.float32), np.eye(len(M), dtype=np.float32))
    g = np.random.default_rng(11)
    dirs = g.normal(size=(100, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    c = g.normal(size=(100, 3, 16))
    B = np.zeros((16, 16))
    B[0, 0] = 1
    for l, M in zip((1, 2, 3), Ms):
        B[l * l:(l + 1) ** 2, l * l:(l + 1) ** 2] = M
    lhs = fdgs.sh.eval_sh(3, torch.from_numpy(c @ B), torch.from_numpy(dirs))
    rhs = fdgs.sh.eval_sh(3, torch.from_numpy(c), torch.from_numpy(dirs @ R))               # (R^T dir as a row vector)
    assert float((lhs - rhs).abs().max()) <= 1e-12 * max(1.0, float(rhs.abs().max()))
    if name != "identity":
        assert float((lhs - fdgs.sh.eval_sh(3, torch.from_numpy(c), torch.from_numpy(dirs))).abs().max()) > 0.1


def test_sh_rotation_of_a_product():
    """Turning by R2, then by R1, is turning by R1 R2: c @ M(R2) @ M(R1) == c @ M(R1 R2)."""
    R1, R2 = ROTATIONS["script"], ROTATIONS["general"]
    for M1, M2, M12 in zip(C.sh_rotation(R1), C.sh_rotation(R2), C.sh_rotation(R1 @ R2)):
        assert np.abs(M2 @ M1 - M12).max() <= 1e-12
        assert np.abs(M1 @ M2 - M12).max() > 1e-3           # (the order matters)


# ---- the host twin ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("deg", [0, 1, 2, 3])
@pytest.mark.parametrize("mode", ["points", "rigid"])
@pytest.mark.parametrize("n", [4099, 1])
def test_host_place_against_float64(lib, n, mode, deg):
    a, _ = _state(n, seed=31 + n)
    pl = general_placement(mode)
    got = host_place(lib, pl.struct(deg), a)
    check_against_float64(got, a, pl, deg)


def test_identity_placement_reproduces_its_input(lib):
    a, _ = _state(4099, seed=2)
    got = host_place(lib, C.Placement().struct(3), a)
    for k in KEYS:
        assert torch.equal(got[k], a[k]), k
    pl = C.Placement()
    assert pl.mode == "rigid" and np.array_equal(pl.rotation, np.eye(3, dtype=np.float32)) and np.array_equal(pl.quat, np.float32([1, 0, 0, 0]))


@pytest.mark.parametrize("w", WEIGHTS)
@pytest.mark.parametrize("mode", ["points", "rigid"])
def test_fused_blend_is_blend_then_place(lib, mode, w):
    a, b = _state(4099, seed=23)
    ps = general_placement(mode).struct(3)
    fused = host_place(lib, ps, a, b, w)
    two = host_place(lib, ps, host_blend(lib, a, b, w))
    for k in KEYS:
        assert torch.equal(fused[k], two[k]), k
    if w == 0.0:
        # w = 0 with b given is the state a: bit for bit in the lerped fields (a + 0 * (b - a)); fdgs_state_blend renormalises the
        # quaternion also at w = 0 (out = a / |a|, test_playback_host allows it 16 u), so the rotations agree to that bound, not in bits
        plain = host_place(lib, ps, a)
        for k in KEYS:
            if k != "rot":
                assert torch.equal(fused[k], plain[k]), k
        assert float((fused["rot"].double() - plain["rot"].double()).abs().max()) <= 16 * U
    else:
        assert not torch.equal(fused["xyz"], host_place(lib, ps, a)["xyz"])


def test_field_mask(lib):
    a, b = _state(37, seed=3)
    ps = general_placement().struct(3)
    full = host_place(lib, ps, a, b, 0.25)
    assert not any(bool(torch.isnan(full[k]).any()) for k in KEYS)
    for mask in range(ALL):
        part = host_place(lib, ps, a, b, 0.25, mask=mask)
        for h, k in enumerate(KEYS):
            if mask >> h & 1:
                assert torch.equal(part[k], full[k]), (mask, k)
            else:
                assert bool(torch.isnan(part[k]).all()), (mask, k)


def test_bad_arguments(lib):
    a, b = _state(5, seed=1)
    L = fdgs._lib
    good = general_placement().struct(3)
    out = {k: torch.empty_like(a[k]) for k in KEYS}

    def arrays(state, skip=None):
        s = L.StateArrays()
        for k, name in zip(KEYS, P.FIELDS):
            if name != skip:
                setattr(s, name, state[k].data_ptr())
        return s

    def variant(**kw):
        p = general_placement().struct(3)
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    sa, sb, so = arrays(a), arrays(b), arrays(out)
    cases = [((good, -1, ALL, sa, None, 0.0, so), b"N"), ((good, 5, ALL, arrays(a, "scales"), None, 0.0, so), b"NULL"),
             ((good, 5, ALL, sa, None, 0.0, arrays(out, "shs")), b"NULL"), ((good, 5, ALL, sa, arrays(b, "xyz"), 0.5, so), b"NULL"),
             ((good, 5, ALL, None, None, 0.0, so), b"NULL"),
             ((variant(mode=2), 5, ALL, sa, None, 0.0, so), b"mode"), ((good, 5, ALL, sa, sb, 1.5, so), b"w"),
             ((good, 5, ALL, sa, sb, -0.1, so), b"w"), ((good, 5, ALL, sa, sb, float("nan"), so), b"w"),
             ((good, 5, ALL, sa, None, 0.5, so), b"w"),
             ((variant(scale=0.0), 5, ALL, sa, None, 0.0, so), b"scale"), ((variant(scale=-1.0), 5, ALL, sa, None, 0.0, so), b"scale"),
             ((variant(scale=float("inf")), 5, ALL, sa, None, 0.0, so), b"scale"), ((variant(scale=float("nan")), 5, ALL, sa, None, 0.0, so), b"scale"),
             ((variant(sh_degree=4), 5, ALL, sa, None, 0.0, so), b"sh_degree"), ((variant(sh_degree=-1), 5, ALL, sa, None, 0.0, so), b"sh_degree"),
             ((good, 5, 32, sa, None, 0.0, so), b"field_mask")]
    for args, word in cases:
        assert lib.fdgs_state_place_host(*args) == -1, word
        assert word in lib.fdgs_last_error(), (word, lib.fdgs_last_error())
        assert lib.fdgs_state_place(None, *args) == -1 and word in lib.fdgs_last_error(), word       # checked before a device is touched
    # a field that is not selected may be NULL
    assert lib.fdgs_state_place_host(good, 5, ALL & ~2, arrays(a, "scales"), None, 0.0, arrays(out, "scales")) == 0
    # nothing to do: no launch, on the device entry point too
    assert lib.fdgs_state_place_host(good, 0, ALL, None, None, 0.0, None) == 0 and lib.fdgs_state_place(None, good, 0, ALL, None, None, 0.0, None) == 0
    assert lib.fdgs_state_place_host(good, 5, 0, None, None, 0.0, None) == 0 and lib.fdgs_state_place(None, good, 5, 0, None, None, 0.0, None) == 0
    # the device entry point checks the alignment of the baked arrays before it touches a device
    odd = arrays(a)
    odd.shs = a["shs"].data_ptr() + 4
    assert lib.fdgs_state_place(None, good, 1, 16, odd, None, 0.0, so) == -1 and b"aligned" in lib.fdgs_last_error()


# ---- Placement, map_time, compose_bytes ------------------------------------------------------------------------------------------------

def test_placement_from_reference(lib):
    n = 4099
    a, _ = _state(n, seed=8)
    theta, phi, s, d = 0.7, -0.4, 1.3, (0.5, -1.25, 2.0)
    pl = C.Placement.from_reference(motion_bias=torch.tensor(d), rotation_bias=torch.tensor([theta, phi]), scales_bias=s)
    assert pl.mode == "points" and pl.scale == np.float32(s) and np.array_equal(pl.translation, np.float32(d))
    assert np.abs(pl.rotation.astype(np.float64) - script_rotation(theta, phi)).max() <= U
    got = host_place(lib, pl.struct(3), a)
    check_against_float64(got, a, pl, 3)                             # the rounded parameters: the bounds of the docstring
    # ... and the script's own float64 formula with the unrounded ones: the parameters' rounding adds at most u to each factor
    p = a["xyz"].double().numpy()
    Rm = script_rotation(theta, phi)
    ref = (p * s) @ Rm.T + np.array(d)
    bound = 9 * U * (np.abs(p * s) @ np.abs(Rm).T + np.abs(d))
    assert (np.abs(got["xyz"].double().numpy() - ref) <= bound).all()
    assert (np.abs(got["scales"].double().numpy() - s * a["scales"].double().numpy()) <= 2 * U * s * a["scales"].double().numpy()).all()
    assert torch.equal(got["rot"], a["rot"]) and torch.equal(got["shs"], a["shs"]) and torch.equal(got["opacity"], a["opacity"])


def test_placement_validation_and_rounding():
    R = R_GENERAL
    pl = C.Placement(rotation=R, translation=(0.1, 0.2, 0.3), scale=0.1)
    assert pl.rotation.dtype == pl.quat.dtype == pl.translation.dtype == np.float32 and isinstance(pl.scale, np.float32)
    assert np.array_equal(pl.rotation, R.astype(np.float32)) and pl.scale == np.float32(0.1) and float(pl.scale) != 0.1
    assert all(M.dtype == np.float32 for M in pl.sh) and [M.shape for M in pl.sh] == [(3, 3), (5, 5), (7, 7)]
    q = pl.quat.astype(np.float64)
    assert abs(np.linalg.norm(q) - 1) <= 2 * U and np.abs(C._quat_to_matrix(q) - R).max() <= 8 * U
    # a quaternion names the same placement as its matrix; a torch tensor is accepted
    same = C.Placement(rotation=C._matrix_to_quat(R))
    assert np.abs(same.rotation.astype(np.float64) - R).max() <= 2 * U and np.array_equal(same.quat, pl.quat)
    assert np.array_equal(C.Placement(rotation=torch.from_numpy(R)).rotation, pl.rotation)
    for axis, ang in (((1, 0, 0), math.pi), ((0, 1, 0), 3.0), ((0, 0, 1), -3.1), ((1, 1, 1), 2.5)):        # every branch of the conversion
        Rk = axis_angle(axis, ang)
        assert np.abs(C._quat_to_matrix(C._matrix_to_quat(Rk)) - Rk).max() <= 1e-14
    for bad in (dict(rotation=2 * R), dict(rotation=R * np.array([1, 1, -1.0])), dict(rotation=R + 1e-4), dict(rotation=(1, 0, 0)),
                dict(rotation=(0.6, 0.8, 0.1, 0)), dict(rotation=np.full((3, 3), np.nan)), dict(scale=0), dict(scale=-2.0),
                dict(scale=float("inf")), dict(scale=float("nan")), dict(scale=1e-60), dict(mode="affine"), dict(wrap="bounce"),
                dict(translation=(1, 2)), dict(translation=(0, float("nan"), 0)), dict(time_scale=float("inf"))):
        with pytest.raises(ValueError):
            C.Placement(**bad)


def test_map_time():
    ts = [0.25, 0.5, 1.25]
    mk = lambda **kw: C.Placement(**kw)
    for wrap in C.WRAPS:
        pl = mk(wrap=wrap)
        for t in (0.25, 0.3, 0.5, 1.25):                                   # inside, both ends included: unchanged, exactly
            assert C.map_time(ts, t, pl) == t
        assert C.map_time([0.7], 3.0, pl) == 0.7 and C.map_time((0.7,), -3.0, mk(wrap=wrap, time_scale=2.0, time_offset=1.0)) == 0.7
    assert C.map_time(ts, 2.0, mk()) == 1.25 and C.map_time(ts, -1.0, mk()) == 0.25
    assert C.map_time(ts, 0.25, mk(time_scale=2.0, time_offset=0.25)) == 0.75                           # t' = 2 t + 0.25
    loop = mk(wrap="loop")
    assert C.map_time(ts, 1.5, loop) == 0.5 and C.map_time(ts, 2.5, loop) == 0.5 and C.map_time(ts, 0.0, loop) == 1.0
    assert C.map_time(ts, -0.75, loop) == 0.25                                                          # a whole span below the start
    pp = mk(wrap="pingpong")
    assert C.map_time(ts, 1.5, pp) == 1.0 and C.map_time(ts, 2.25, pp) == 0.25 and C.map_time(ts, 2.5, pp) == 0.5
    assert C.map_time(ts, 0.0, pp) == 0.5 and C.map_time(ts, -0.75, pp) == 1.25
    for wrap in C.WRAPS:                                                   # always inside the range
        pl = mk(wrap=wrap, time_scale=-3.7, time_offset=0.123)
        for t in np.linspace(-5, 5, 41):
            assert ts[0] <= C.map_time(ts, float(t), pl) <= ts[-1]
    assert C.map_time(torch.tensor(ts), 1.5, loop) == 0.5


def _stub(n, device="cpu", head_on=(1, 1, 1, 0, 0)):
    return types.SimpleNamespace(N=n, device=torch.device(device), head_on=head_on, times=(0.0, 1.0), active_sh_degree=3, perm=None, frames=[])


def test_compose_bytes_and_refusals_come_before_any_device():
    pad = lambda floats: (floats + P.SLOT_ALIGN_FLOATS - 1) // P.SLOT_ALIGN_FLOATS * P.SLOT_ALIGN_FLOATS
    for Ns in ((4099, 8200), (1,), (300_000, 300_000), (0, 7, 64)):
        total = sum(Ns)
        assert C.compose_bytes(Ns) == 4 * (2 * pad(3 * total) + pad(4 * total) + pad(total) + pad(48 * total))
        assert 236 * total <= C.compose_bytes(Ns) < 236 * total + 5 * 4 * P.SLOT_ALIGN_FLOATS
    assert C.compose_bytes([64, 64]) == 236 * 128 and C.compose_bytes([300_000] * 2) == P.bake_bytes(600_000, 1, [1] * 5)
    for bad in ([], [5, -1]):
        with pytest.raises(ValueError):
            C.compose_bytes(bad)
    models = [_stub(4099), _stub(8200)]
    need = C.compose_bytes([4099, 8200])
    with pytest.raises(MemoryError):
        C.compose(models, max_bytes=need - 1)
    with pytest.raises(fdgs._lib.FdgsError):                 # enough memory allowed: the next thing it needs is a device (there is no CPU path)
        C.compose(models, max_bytes=need)
    with pytest.raises(ValueError):
        C.compose([_stub(5), _stub(5, device="meta")])
    with pytest.raises(ValueError):
        C.compose([])
    with pytest.raises(ValueError):
        C.compose(models, [None])
    with pytest.raises(ValueError):
        C.compose(models, [None, "rigid"])


# ---- the convention, through the float64 rasterizer oracle -----------------------------------------------------------------------------

def _psnr(a, b):
    mse = float(((a - b) ** 2).mean())
    return math.inf if mse == 0.0 else 10.0 * math.log10(1.0 / mse)


def oracle_scene(n=400, seed=6):
    """Activated float64 arrays of a synthetic model, the SH rest coefficients x 3 (so that the colour depends on the direction)."""
    g = fdgs.synthetic.make_gaussians(n, seed=seed)
    rot = g["rotation"].double()
    return dict(xyz=g["xyz"].double(), scales=g["scaling"].double().exp(), rot=rot / rot.norm(dim=1, keepdim=True),
                opacity=torch.sigmoid(g["opacity"].double()), shs=torch.cat((g["features_dc"], 3.0 * g["features_rest"]), 1).double())


def oracle_render(st, V, F, campos, cam, W=96, H=64):
    from oracle.raster_torch import rasterize
    return rasterize(means3D=st["xyz"], opacities=st["opacity"], viewmatrix=V, projmatrix=F, campos=campos, bg=torch.zeros(3, dtype=torch.float64),
                     image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5), sh_degree=3,
                     shs=st["shs"], scales=st["scales"], rotations=st["rot"])


def moved_camera(cam, R, d):
    """The camera from which the UNPLACED model looks like the model placed by (R, d) seen from `cam`: V' = A V, F' = A F,
    c' = (c - d) R with A = [[R^T, 0], [d, 1]] (row-vector convention: [p, 1] A = R p + d)."""
    A = torch.eye(4, dtype=torch.float64)
    A[:3, :3] = torch.from_numpy(R).T
    A[3, :3] = torch.tensor(d, dtype=torch.float64)
    return A @ cam.world_view_transform.double(), A @ cam.full_proj_transform.double(), (cam.camera_center.double() - A[3, :3]) @ torch.from_numpy(R)


def place_float64(st, R, d, turn_rot=True, turn_sh=True):
    qR = torch.from_numpy(C._matrix_to_quat(R))
    out = dict(st, xyz=st["xyz"] @ torch.from_numpy(R).T + torch.tensor(d, dtype=torch.float64))
    if turn_rot:
        out["rot"] = torch.from_numpy(hamilton(qR.numpy(), st["rot"].numpy())[0])
    if turn_sh:
        B = np.zeros((16, 16))
        B[0, 0] = 1
        for l, M in zip((1, 2, 3), C.sh_rotation(R)):
            B[l * l:(l + 1) ** 2, l * l:(l + 1) ** 2] = M
        out["shs"] = torch.einsum("njc,jk->nkc", st["shs"], torch.from_numpy(B))
    return out


def test_a_placed_model_is_the_model_seen_from_the_moved_camera():
    st = oracle_scene()
    cam = fdgs.synthetic.make_camera(96, 64, theta_deg=-73)
    R, d = R_GENERAL, D_GENERAL
    V, F, c = cam.world_view_transform.double(), cam.full_proj_transform.double(), cam.camera_center.double()
    want, _, want_radii = oracle_render(st, *moved_camera(cam, R, d), cam)
    got, _, radii = oracle_render(place_float64(st, R, d), V, F, c, cam)
    assert _psnr(got, want) > 200.0 and torch.equal(radii, want_radii) and int((radii > 0).sum()) > 300
    assert float(want.max()) > 0.3
    # the reference script's semantics, and the half measure: splats or colours that keep pointing the old way
    points, _, _ = oracle_render(place_float64(st, R, d, turn_rot=False, turn_sh=False), V, F, c, cam)
    no_sh, _, _ = oracle_render(place_float64(st, R, d, turn_sh=False), V, F, c, cam)
    assert _psnr(points, want) < 40.0 and _psnr(no_sh, want) < 40.0
