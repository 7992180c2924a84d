"""Playback in the C-ABI, host side (no GPU): the *_host twins of fdgs_state_blend / fdgs_pack_ply_rows / fdgs_image_rgb8 run the very
functions the device kernels compile (csrc/playback_ops.h), over host arrays; the pure-Python helpers of fdgs.playback.

Bounds (u = 2**-24, the float32 unit roundoff; none of them is measured):
  lerped fields   out = a + w * (b - a) is three roundings: |out - ref| <= 4 u (|a| + |b|) against the float64 evaluation
  quaternions     about ten roundings on values <= 1 and a norm >= 0.707 once the signs are aligned: |out - ref| <= 16 u absolute
  output norms    within 4 u of 1
Everything else (w = 0, the sign symmetry, the PLY table, both rgb8 modes) is exact."""
import ctypes
import importlib
import os
import re
import types

import numpy as np
import pytest
import torch

fdgs = importlib.import_module("4dgaussians_amd")
P = fdgs.playback
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
NEW = ("fdgs_state_blend", "fdgs_state_blend_host", "fdgs_pack_ply_rows", "fdgs_pack_ply_rows_host", "fdgs_image_rgb8", "fdgs_image_rgb8_host")
WEIGHTS = [0.0, 0.25, 0.5, 1.0, float(np.nextafter(np.float32(1), np.float32(0)))]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(fdgs._lib.LIB_PATH):
        importlib.import_module("4dgaussians_amd.build").build()
    return fdgs._lib.lib()


def test_header_declares_the_six_functions_and_lib_binds_them(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fdgs.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in fdgs._lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"#define\s+FDGS_RGB8_TRUNC\s+0\b", src) and re.search(r"#define\s+FDGS_RGB8_ROUND\s+1\b", src)
    assert re.search(r"#define\s+FDGS_MAX_BLEND_STREAMS\s+4\b", src) and fdgs._lib.MAX_BLEND_STREAMS == 4
    body = re.search(r"typedef struct fdgs_blend_stream \{(.*?)\} fdgs_blend_stream;", src, flags=re.S).group(1)
    assert [d.split()[-1].lstrip("*") for d in body.split(";") if d.strip()] == [f[0] for f in fdgs._lib.BlendStream._fields_]
    assert lib.fdgs_abi_version() == 6
    assert "playback.hip" in importlib.import_module("4dgaussians_amd.build").SOURCES
    assert "NaN" in open(os.path.join(ROOT, "include", "fdgs.h")).read().split("fdgs_image_rgb8")[0].rsplit("/*", 1)[1]


# ---- blend ---------------------------------------------------------------------------------------------------------------------------

def _state(n, seed):
    """(a, b): per state xyz [n,3], scales [n,3], opacity [n,1], shs [n,16,3] and unit quaternions [n,4]; every second quaternion of b is
    negated; the first rows (when there are enough) are pairs whose dot product is exactly zero."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(2):
        q = torch.randn(n, 4, generator=g, dtype=torch.float64)
        q = (q / q.norm(dim=1, keepdim=True)).float()
        out.append(dict(xyz=torch.randn(n, 3, generator=g) * 1.3, scales=torch.rand(n, 3, generator=g) * 0.1 + 1e-3,
                        opacity=torch.rand(n, 1, generator=g), shs=torch.randn(n, 16, 3, generator=g), rot=q))
    a, b = out
    b["rot"][1::2] *= -1
    if n >= 8:
        a["rot"][0], b["rot"][0] = torch.tensor([1.0, 0, 0, 0]), torch.tensor([0, 1.0, 0, 0])
        a["rot"][1], b["rot"][1] = torch.tensor([0, 0, 1.0, 0]), torch.tensor([0, 0, 0, -1.0])
        a["rot"][2], b["rot"][2] = torch.tensor([0.6, 0.8, 0, 0]), torch.tensor([0, 0, 0.8, 0.6])
        a["rot"][3], b["rot"][3] = torch.tensor([0.6, 0, -0.8, 0]), torch.tensor([0, -0.6, 0, 0.8])
    return a, b


def host_blend(lib, a, b, w, fields=("xyz", "scales", "opacity", "shs"), rot=True):
    """fdgs_state_blend_host on dicts of CPU tensors -> dict of CPU tensors."""
    n = a["rot"].shape[0]
    out = {k: torch.full_like(a[k], float("nan")) for k in (*fields, *(["rot"] if rot else []))}
    streams = (fdgs._lib.BlendStream * max(len(fields), 1))()
    for s, k in zip(streams, fields):
        assert a[k].is_contiguous() and b[k].is_contiguous() and a[k].dtype == torch.float32
        s.a, s.b, s.out, s.n_floats = a[k].data_ptr(), b[k].data_ptr(), out[k].data_ptr(), a[k].numel()
    r = [a["rot"].data_ptr(), b["rot"].data_ptr(), out["rot"].data_ptr()] if rot and n else [None] * 3
    rc = lib.fdgs_state_blend_host(w, len(fields), streams, n, *r)
    assert rc == 0, lib.fdgs_last_error()
    return out


def _ref_quat(a, b, w32):
    a, b = a.double(), b.double()
    dot = (a * b).sum(1, keepdim=True)
    s = torch.where(dot < 0, -1.0, 1.0)
    q = a + w32 * (s * b - a)
    return q / q.norm(dim=1, keepdim=True).clamp_min(1e-12), dot


@pytest.mark.parametrize("w", WEIGHTS)
@pytest.mark.parametrize("n", [4099, 1])
def test_host_blend_against_float64(lib, n, w):
    assert (3 * n) % 4 != 0
    a, b = _state(n, seed=17 + n)
    got = host_blend(lib, a, b, w)
    w32 = float(np.float32(w))
    for k in ("xyz", "scales", "opacity", "shs"):
        ref = a[k].double() + w32 * (b[k].double() - a[k].double())
        bound = 4 * U * (a[k].double().abs() + b[k].double().abs())
        assert bool(((got[k].double() - ref).abs() <= bound).all()), k
        if w == 0.0:
            assert torch.equal(got[k], a[k]), k                   # bit for bit
    ref, dot = _ref_quat(a["rot"], b["rot"], w32)
    if n >= 8:
        assert bool((dot[:4] == 0).all())                         # exact zeros: s = +1
        assert float(dot[4:].abs().min()) > 1e-6                  # everywhere else the sign is not a rounding question
    assert float((got["rot"].double() - ref).abs().max()) <= 16 * U
    assert float((got["rot"].double().norm(dim=1) - 1).abs().max()) <= 4 * U


@pytest.mark.parametrize("w", WEIGHTS)
def test_host_blend_of_a_negated_quaternion_is_the_same_quaternion(lib, w):
    """q and -q are one rotation: blend(a, b) == blend(a, -b) bit for bit -- wherever dot(a, b) != 0; at dot == 0 exactly the stated rule
    (s = dot < 0 ? -1 : 1) takes s = +1 for b and for -b alike, which are then two different, equally short, paths."""
    a, b = _state(4099, seed=5)
    nb = dict(b, rot=-b["rot"])
    x = host_blend(lib, a, b, w, fields=())["rot"]
    y = host_blend(lib, a, nb, w, fields=())["rot"]
    dot = (a["rot"].double() * b["rot"].double()).sum(1)
    assert int((dot == 0).sum()) == 4 and int((dot < 0).sum()) > 1000 and int((dot > 0).sum()) > 1000
    assert torch.equal(x[dot != 0], y[dot != 0])
    w32 = float(np.float32(w))
    for got, bb in ((x, b["rot"]), (y, nb["rot"])):               # the dot == 0 rows: s = +1 whatever the sign of the zero
        q = a["rot"][:4].double() + w32 * (bb[:4].double() - a["rot"][:4].double())
        assert float((got[:4].double() - q / q.norm(dim=1, keepdim=True)).abs().max()) <= 16 * U


def test_host_blend_subsets_empty_sets_and_bad_arguments(lib):
    a, b = _state(37, seed=3)
    full = host_blend(lib, a, b, 0.25)
    part = host_blend(lib, a, b, 0.25, fields=("xyz", "shs"), rot=False)       # any subset of the streams, no rotations
    assert set(part) == {"xyz", "shs"} and torch.equal(part["xyz"], full["xyz"]) and torch.equal(part["shs"], full["shs"])
    assert torch.equal(host_blend(lib, a, b, 0.25, fields=())["rot"], full["rot"])
    assert lib.fdgs_state_blend_host(0.5, 0, None, 0, None, None, None) == 0    # N = 0: a no-op
    assert lib.fdgs_state_blend(None, 0.5, 0, None, 0, None, None, None) == 0   # ... on the device entry point too: nothing is launched
    streams = (fdgs._lib.BlendStream * 5)()
    x = np.zeros(8, np.float32)
    for args, word in (((1.5, 0, None, 0, None, None, None), b"w"), ((-0.1, 0, None, 0, None, None, None), b"w"),
                       ((float("nan"), 0, None, 0, None, None, None), b"w"), ((0.5, 5, streams, 0, None, None, None), b"nstreams"),
                       ((0.5, 0, None, -1, None, None, None), b"N"), ((0.5, 1, None, 0, None, None, None), b"NULL"),
                       ((0.5, 0, None, 2, x.ctypes.data, None, x.ctypes.data), b"NULL")):
        assert lib.fdgs_state_blend_host(*args) == -1, args
        assert word in lib.fdgs_last_error(), (args, lib.fdgs_last_error())
    streams[0].n_floats = 4                                                     # a stream with floats but no pointers
    assert lib.fdgs_state_blend_host(0.5, 1, streams, 0, None, None, None) == -1 and b"NULL" in lib.fdgs_last_error()
    # the device entry point checks alignment before it touches a device
    buf = np.zeros(16, np.float32)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    streams[0].a, streams[0].b, streams[0].out = base + 4, base, base
    assert lib.fdgs_state_blend(None, 0.5, 1, streams, 0, None, None, None) == -1 and b"aligned" in lib.fdgs_last_error()


# ---- PLY pack ------------------------------------------------------------------------------------------------------------------------

def _raw_model(n, seed):
    g = torch.Generator().manual_seed(seed)
    return types.SimpleNamespace(_xyz=torch.randn(n, 3, generator=g), _scaling=torch.randn(n, 3, generator=g), _rotation=torch.randn(n, 4, generator=g),
                                 _opacity=torch.randn(n, 1, generator=g), _features_dc=torch.randn(n, 1, 3, generator=g),
                                 _features_rest=torch.randn(n, 15, 3, generator=g))


def host_pack(lib, xyz, scales, rot, op, shs):
    n = xyz.shape[0]
    arrs = [np.ascontiguousarray(t.numpy(), dtype=np.float32) for t in (xyz, scales, rot, op, shs)]
    out = np.full((n, 62), np.nan, np.float32)
    rc = lib.fdgs_pack_ply_rows_host(n, *[x.ctypes.data for x in arrs], out.ctypes.data)
    assert rc == 0, lib.fdgs_last_error()
    return out


@pytest.mark.parametrize("n", [4099, 1])
def test_host_ply_rows_equal_save_ply(lib, n, tmp_path):
    pc = _raw_model(n, seed=n)
    shs = torch.cat((pc._features_dc, pc._features_rest), dim=1).contiguous()
    got = host_pack(lib, pc._xyz, pc._scaling, pc._rotation, pc._opacity, shs)
    # the expression of io.save_ply (GaussianModel.save_ply)
    f_dc = pc._features_dc.transpose(1, 2).flatten(start_dim=1).contiguous().numpy()
    f_rest = pc._features_rest.transpose(1, 2).flatten(start_dim=1).contiguous().numpy()
    xyz = pc._xyz.numpy()
    ref = np.concatenate((xyz, np.zeros_like(xyz), f_dc, f_rest, pc._opacity.numpy(), pc._scaling.numpy(), pc._rotation.numpy()), axis=1)
    assert got.shape == ref.shape == (n, 62) and np.array_equal(got, ref)
    # through the writer export_ply_sequence uses: the file is byte for byte io.save_ply's and reads back with the same values
    names = fdgs.io.construct_list_of_attributes(pc)
    assert len(names) == 62
    fdgs.io.write_ply_vertices(str(tmp_path / "packed.ply"), names, got)
    fdgs.io.save_ply(pc, str(tmp_path / "saved.ply"))
    assert (tmp_path / "packed.ply").read_bytes() == (tmp_path / "saved.ply").read_bytes()
    v = fdgs.io.read_ply_vertices(str(tmp_path / "packed.ply"))
    assert list(v) == names
    for c, name in enumerate(names):
        assert np.array_equal(v[name], ref[:, c]), name
    assert np.array_equal(v["f_rest_17"], shs[:, 1 + 2, 1].numpy())            # f_rest_{c * 15 + k} = shs[n, 1 + k, c]


def test_host_ply_rows_bad_arguments(lib):
    assert lib.fdgs_pack_ply_rows_host(0, None, None, None, None, None, None) == 0
    assert lib.fdgs_pack_ply_rows(None, 0, None, None, None, None, None, None) == 0
    x = np.zeros(64, np.float32)
    assert lib.fdgs_pack_ply_rows_host(-1, *[x.ctypes.data] * 6) == -1 and b"N" in lib.fdgs_last_error()
    assert lib.fdgs_pack_ply_rows_host(1, x.ctypes.data, None, *[x.ctypes.data] * 4) == -1 and b"NULL" in lib.fdgs_last_error()


# ---- rgb8 ----------------------------------------------------------------------------------------------------------------------------

def boundary_image(h, w, seed=9):
    """float32 [3,h,w]: every k / 255 and every (k + 0.5) / 255 with their float32 neighbours on both sides, the special values, noise."""
    f = np.float32
    k = np.arange(256, dtype=np.float32)
    vals = []
    for centre in (k / f(255), (k + f(0.5)) / f(255)):
        centre = centre.astype(np.float32)
        vals += [centre, np.nextafter(centre, f(-np.inf)), np.nextafter(centre, f(np.inf))]
    vals.append(np.array([-1.0, -0.0, 0.0, 1.0, np.nextafter(f(1), f(2)), 7.5], np.float32))
    vals = np.concatenate(vals)
    total = 3 * h * w
    assert vals.size == 6 * 256 + 6 <= total
    noise = np.random.default_rng(seed).normal(0.5, 0.5, total - vals.size).astype(np.float32)
    x = np.concatenate((vals, noise))
    np.random.default_rng(seed + 1).shuffle(x)
    return np.ascontiguousarray(x.reshape(3, h, w))


def host_rgb8(lib, x, mode):
    out = np.full((x.shape[1], x.shape[2], 3), 77, np.uint8)
    rc = lib.fdgs_image_rgb8_host(x.shape[1], x.shape[2], fdgs._lib.RGB8_MODES[mode], x.ctypes.data, out.ctypes.data)
    assert rc == 0, lib.fdgs_last_error()
    return out


def rgb8_reference(x, mode):
    if mode == "trunc":       # render.py's to8b
        return np.ascontiguousarray((255 * np.clip(x, 0, 1)).astype(np.uint8).transpose(1, 2, 0))
    return torch.from_numpy(x.copy()).mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).numpy()      # save_image


@pytest.mark.parametrize("mode", ["trunc", "round"])
def test_host_rgb8_is_exact(lib, mode):
    x = boundary_image(23, 37)
    got, ref = host_rgb8(lib, x, mode), rgb8_reference(x, mode)
    assert got.shape == ref.shape == (23, 37, 3) and got.dtype == np.uint8
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]
    assert len(np.unique(got)) == 256


def test_host_rgb8_modes_differ_and_bad_arguments(lib):
    x = boundary_image(23, 37)
    assert not np.array_equal(host_rgb8(lib, x, "trunc"), host_rgb8(lib, x, "round"))
    out = np.zeros(3, np.uint8)
    assert lib.fdgs_image_rgb8_host(0, 5, 0, None, None) == 0 and lib.fdgs_image_rgb8(None, 0, 0, 1, None, None) == 0
    assert lib.fdgs_image_rgb8_host(1, 1, 2, x.ctypes.data, out.ctypes.data) == -1 and b"mode" in lib.fdgs_last_error()
    assert lib.fdgs_image_rgb8_host(-1, 1, 0, x.ctypes.data, out.ctypes.data) == -1 and b"size" in lib.fdgs_last_error()
    assert lib.fdgs_image_rgb8_host(1, 1, 0, None, out.ctypes.data) == -1 and b"NULL" in lib.fdgs_last_error()
    with pytest.raises(ValueError):
        P.to_rgb8(torch.zeros(3, 2, 2), "nearest")
    with pytest.raises(ValueError):
        P.to_rgb8(torch.zeros(2, 2), "trunc")


# ---- Python helpers ------------------------------------------------------------------------------------------------------------------

def test_locate():
    ts = [0.0, 0.25, 0.5, 1.0]
    assert P.locate(ts, 0.375) == (1, 2, 0.5) and P.locate(ts, 0.75, "linear") == (2, 3, 0.5)
    i, j, w = P.locate(ts, 0.3)
    assert (i, j) == (1, 2) and w == (0.3 - 0.25) / (0.5 - 0.25)
    for k, t in enumerate(ts):                                                  # exact hits, both modes
        assert P.locate(ts, t) == (k, k, 0.0) and P.locate(ts, t, "nearest") == (k, k, 0.0)
    assert P.locate(ts, -3.0) == (0, 0, 0.0) and P.locate(ts, 1.5) == (3, 3, 0.0)          # clamping
    assert P.locate(ts, float("inf"), "nearest") == (3, 3, 0.0)
    assert P.locate(ts, 0.375, "nearest") == (1, 1, 0.0)                        # a tie goes to the lower index
    assert P.locate(ts, 0.75, "nearest") == (2, 2, 0.0)
    assert P.locate(ts, 0.38, "nearest") == (2, 2, 0.0) and P.locate(ts, 0.37, "nearest") == (1, 1, 0.0)
    assert P.locate(ts, np.nextafter(0.25, 1.0)) == (1, 2, (np.nextafter(0.25, 1.0) - 0.25) / 0.25)
    assert P.locate([0.5], 0.1) == (0, 0, 0.0) and P.locate((0.5,), 0.9, "nearest") == (0, 0, 0.0)
    assert P.locate(torch.tensor(ts), 0.375) == (1, 2, 0.5)                     # any sequence of numbers
    for bad in ([0.0, 0.5, 0.5], [0.0, 0.5, 0.25], [1.0, 0.0], [], [0.0, float("nan")]):
        with pytest.raises(ValueError):
            P.locate(bad, 0.1)
    with pytest.raises(ValueError):
        P.locate(ts, 0.1, "cubic")


def test_bake_bytes():
    syn = fdgs.synthetic
    on = {name: fdgs.deformation._head_on(syn.deform_args(name)) for name in ("dynerf_default", "dnerf_bouncingballs", "hypernerf_default")}
    assert on["dynerf_default"] == [1, 1, 1, 1, 1] and on["dnerf_bouncingballs"] == on["hypernerf_default"] == [1, 1, 1, 0, 0]
    pad = lambda floats: (floats + P.SLOT_ALIGN_FLOATS - 1) // P.SLOT_ALIGN_FLOATS * P.SLOT_ALIGN_FLOATS
    assert (P.SLOT_ALIGN_FLOATS * 4) % 16 == 0
    for N, T in ((4099, 4), (1, 1), (300_000, 300), (8200, 7)):
        slot = {w: pad(N * w) for w in (3, 4, 1, 48)}
        # dynerf_default: 59 floats per Gaussian and timestamp, each of the five slots padded
        full = P.bake_bytes(N, T, on["dynerf_default"])
        assert full == 4 * T * (2 * slot[3] + slot[4] + slot[1] + slot[48])
        assert 4 * 59 * N * T <= full < 4 * T * (59 * N + 5 * P.SLOT_ALIGN_FLOATS)
        # dnerf_bouncingballs: 10 floats per timestamp, 49 once
        part = P.bake_bytes(N, T, on["dnerf_bouncingballs"])
        assert part == 4 * (T * (2 * slot[3] + slot[4]) + slot[1] + slot[48])
        assert 4 * N * (10 * T + 49) <= part < 4 * (N * (10 * T + 49) + (3 * T + 2) * P.SLOT_ALIGN_FLOATS)
    assert P.bake_bytes(64 * 1000, 300, [1] * 5) == 236 * 64_000 * 300                     # no padding when every slot is a multiple already
    assert P.bake_bytes(64 * 1000, 300, [1, 1, 1, 0, 0]) == 64_000 * (40 * 300 + 196)
    assert P.bake_bytes(300_000, 300, [1] * 5) < 22 * 10 ** 9                              # "300 timestamps of 300 k Gaussians: 21 GB"
    with pytest.raises(ValueError):
        P.bake_bytes(10, 0, [1] * 5)
    with pytest.raises(ValueError):
        P.bake_bytes(10, 1, [1] * 4)


def test_bake_validates_before_it_touches_the_model_or_the_device():
    pc = fdgs.synthetic.SynthModel(100, "dnerf_bouncingballs", seed=2)
    with pytest.raises(ValueError):
        P.bake(pc, [0.0, 0.5, 0.5])
    with pytest.raises(ValueError):
        P.bake(pc, [])
    need = P.bake_bytes(100, 3, [1, 1, 1, 0, 0])
    with pytest.raises(MemoryError):
        P.bake(pc, [0.0, 0.5, 1.0], max_bytes=need - 1)
    with pytest.raises(fdgs._lib.FdgsError):              # enough memory allowed: the next thing it needs is a device (there is no CPU path)
        P.bake(pc, [0.0, 0.5, 1.0], max_bytes=need)
    assert "playback" in fdgs.__all__ and "playback" in fdgs.__doc__
    assert "stale" in P.Baked.__doc__
