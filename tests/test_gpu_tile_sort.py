"""Binning form 1 (csrc/binning.hip: per-tile count, scan, emit, one LDS sort per tile; tuning knob bin_form = 1) against form 0 (depth
sort + pair expansion + global tile sort): the lists, the ranges and everything blended from them are compared with array_equal, nothing
is toleranced.  A tile's list is ordered by the float bits of the view depth, ties by Gaussian index."""
import ctypes
import importlib
import warnings

import numpy as np
import pytest
import torch

from conftest import set_knob
from scenes import raster_scene

pytestmark = pytest.mark.gpu

_KEYS = ("means3D", "shs", "opacities", "scales", "rotations")


def _mod():
    return importlib.import_module("4dgaussians_amd")


def _settings(sc, dev):
    R = _mod().rasterizer
    return R.GaussianRasterizationSettings(
        image_height=sc["image_height"], image_width=sc["image_width"], tanfovx=sc["tanfovx"], tanfovy=sc["tanfovy"],
        bg=torch.tensor(sc["bg"], device=dev), scale_modifier=1.0, viewmatrix=torch.tensor(sc["viewmatrix"], device=dev),
        projmatrix=torch.tensor(sc["projmatrix"], device=dev), sh_degree=sc["sh_degree"],
        campos=torch.tensor(sc["campos"], device=dev), prefiltered=False, debug=False)


def _copy(ptr, n, dtype, dev):
    t = torch.empty(max(n, 1), dtype=dtype, device=dev)
    if n:
        assert ctypes.CDLL("libamdhip64.so").hipMemcpy(ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(ptr), ctypes.c_size_t(n * t.element_size()), ctypes.c_int(3)) == 0
    return t[:n].cpu().numpy()


def _frame(sc, dev, **knobs):
    """One forward of `sc` with the knobs set -> everything the binning stage and the blending pass leave behind (host copies)."""
    L = _mod()._lib.lib()
    R = _mod().rasterizer
    for k, v in knobs.items():
        set_knob(k, v)
    t = [torch.tensor(sc[k], device=dev) for k in _KEYS]
    color, radii, depth, st = R.rasterize_forward(_settings(sc, dev), t[0], t[1], None, t[2], t[3], t[4], None)
    torch.cuda.synchronize()
    W, H, P = sc["image_width"], sc["image_height"], st.params.P
    ntiles = ((W + 15) // 16) * ((H + 15) // 16)
    n = st.num_rendered
    held = min(n, st.capacity)                    # (an overflowing capacity frame holds fewer pairs than it counted)
    q = ctypes.c_void_p()
    out = dict(n=n, capacity=st.capacity, color=color.cpu().numpy(), depth=depth.cpu().numpy(), radii=radii.cpu().numpy())
    for name, which in (("gid", 0), ("tile", 1)):
        if held:
            assert L.fdgs_binning_field(ctypes.c_void_p(st.binning.data_ptr()), st.capacity, W, H, which, ctypes.byref(q)) == 0
            out[name] = _copy(q.value, held, torch.int32, dev).view(np.uint32)
        else:
            out[name] = np.zeros(0, np.uint32)
    assert L.fdgs_img_field(ctypes.c_void_p(st.img.data_ptr()), W, H, 2, ctypes.byref(q)) == 0
    out["ranges"] = _copy(q.value, 2 * ntiles, torch.int32, dev).view(np.uint32).reshape(ntiles, 2)
    assert L.fdgs_img_field(ctypes.c_void_p(st.img.data_ptr()), W, H, 1, ctypes.byref(q)) == 0
    out["ncontrib"] = _copy(q.value, W * H, torch.int32, dev)
    if P:
        assert L.fdgs_geom_field(ctypes.c_void_p(st.geom.data_ptr()), P, 0, ctypes.byref(q)) == 0
        out["depth_bits"] = _copy(q.value, P, torch.float32, dev).view(np.uint32)
    return out


def _same(a, b, what=""):
    assert a["n"] == b["n"], what
    for k in ("gid", "tile", "ranges", "ncontrib", "color", "depth", "radii"):
        assert np.array_equal(a[k], b[k]), (what, k)


def _lists_are_in_key_order(f):
    """Independent of form 0: the list equals the pair set sorted by (tile, depth bits, Gaussian index)."""
    gid, tile = f["gid"].astype(np.int64), f["tile"].astype(np.int64)
    order = np.lexsort((gid, f["depth_bits"][gid].astype(np.int64), tile))
    assert np.array_equal(gid[order], gid) and np.array_equal(tile[order], tile)
    lens = np.bincount(tile, minlength=len(f["ranges"]))
    r = f["ranges"].astype(np.int64)
    assert np.array_equal(r[:, 1] - r[:, 0], lens)
    assert np.array_equal(r[lens > 0, 0], (np.cumsum(lens) - lens)[lens > 0]) and not r[lens == 0].any()


@pytest.fixture(autouse=True)
def _exact_binning(monkeypatch):
    monkeypatch.setattr(_mod().rasterizer, "BINNING", "exact")


SCENES = [
    dict(n=500, width=64, height=48, seed=2, theta=170.0, sh_degree=1, scale_boost=10.0),       # every splat on every tile
    dict(n=3000, width=201, height=77, seed=1, theta=-100.0, scale_boost=4.0),                  # ragged edge, lists of about 2 600
    dict(n=5000, width=320, height=240, seed=3, theta=0.0, sh_degree=0, extent=3.0),            # many culled, empty tiles
    dict(n=20000, width=400, height=400, seed=0, theta=30.0),
]


@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("case", range(len(SCENES)))
def test_forms_agree(case, cull):
    dev = torch.device("cuda:0")
    sc = raster_scene(**SCENES[case])
    a = _frame(sc, dev, tile_cull=cull, bin_form=0)
    b = _frame(sc, dev, tile_cull=cull, bin_form=1)
    assert a["n"] > 0
    _same(a, b)
    _lists_are_in_key_order(b)


def test_lists_below_at_and_above_the_threshold_in_one_frame():
    """tile_sort_cap = one tile's list length: that tile sorts in LDS, longer lists take the chunk-and-merge path."""
    dev = torch.device("cuda:0")
    sc = raster_scene(**SCENES[1])
    a = _frame(sc, dev, bin_form=0)
    lens = (a["ranges"][:, 1] - a["ranges"][:, 0]).astype(np.int64)
    lens = lens[lens > 0]
    cap = int(np.sort(lens)[len(lens) // 2])
    assert (lens < cap).any() and (lens == cap).any() and (lens > cap).any()
    _same(a, _frame(sc, dev, bin_form=1, tile_sort_cap=cap), "cap = median list")
    assert lens.max() > 20 * 64
    _same(a, _frame(sc, dev, bin_form=1, tile_sort_cap=64), "cap = 64")


def test_lists_far_longer_than_the_lds_capacity():
    dev = torch.device("cuda:0")
    sc = raster_scene(60000, 64, 48, seed=4, theta=170.0, sh_degree=0, scale_boost=10.0)
    a = _frame(sc, dev, bin_form=0)
    lens = (a["ranges"][:, 1] - a["ranges"][:, 0]).astype(np.int64)
    assert lens.min() > 2 * 4096
    b = _frame(sc, dev, bin_form=1)
    _same(a, b)
    _lists_are_in_key_order(b)


def test_equal_depths_come_out_in_index_order_and_the_same_every_time():
    dev = torch.device("cuda:0")
    sc = raster_scene(2000, 160, 120, seed=5, scale_boost=3.0)
    idx = np.random.default_rng(8).permutation(np.repeat(np.arange(2000), 4))        # every row four times, at scattered indices
    for k in _KEYS:
        sc[k] = np.ascontiguousarray(sc[k][idx])
    a = _frame(sc, dev, bin_form=0)
    runs = [_frame(sc, dev, bin_form=1) for _ in range(3)]
    bits = a["depth_bits"][a["gid"].astype(np.int64)]
    tie = (a["tile"][1:] == a["tile"][:-1]) & (bits[1:] == bits[:-1])
    assert tie.sum() >= a["n"] // 2                                                  # (three of every four neighbours are ties)
    assert (a["gid"][1:][tie] > a["gid"][:-1][tie]).all()
    for b in runs:
        _same(a, b)
    _lists_are_in_key_order(runs[0])


def test_degenerate_frames():
    dev = torch.device("cuda:0")
    sc = raster_scene(400, 96, 80, seed=6, scale_boost=2.0)
    # no Gaussians
    empty = dict(sc)
    for k in _KEYS:
        empty[k] = sc[k][:0]
    a, b = _frame(empty, dev, bin_form=0), _frame(empty, dev, bin_form=1)
    assert b["n"] == 0 and not b["ranges"].any()
    _same(a, b, "P = 0")
    # all of them behind the camera: mirrored through its centre
    behind = dict(sc)
    behind["means3D"] = (2.0 * sc["campos"][None, :] - sc["means3D"]).astype(np.float32)
    a, b = _frame(behind, dev, bin_form=0), _frame(behind, dev, bin_form=1)
    assert b["n"] == 0 and not b["radii"].any() and not b["ranges"].any()
    _same(a, b, "R = 0")
    # one Gaussian
    one = dict(sc)
    for k in _KEYS:
        one[k] = sc[k][7:8]
    a, b = _frame(one, dev, bin_form=0), _frame(one, dev, bin_form=1)
    assert b["n"] > 0
    _same(a, b, "P = 1")


def test_an_image_of_16384_tiles():
    dev = torch.device("cuda:0")
    sc = raster_scene(20000, 2048, 2048, seed=7)
    a = _frame(sc, dev, bin_form=0)
    b = _frame(sc, dev, bin_form=1)
    assert len(b["ranges"]) == 16384 and b["n"] > 0
    _same(a, b)


def test_overflow_of_a_predicted_capacity(monkeypatch):
    """A predictor that is far too low: the default mode still returns the exact lists; the opt-in capacity mode keeps whole tiles, in image
    order, while they fit -- every tile with a non-empty range holds exactly its exact list, the non-empty tiles are a prefix."""
    dev = torch.device("cuda:0")
    R = _mod().rasterizer
    sc = raster_scene(20000, 416, 304, seed=22, scale_boost=2.0)
    key = (dev.index, 416, 304, 20000)
    want = _frame(sc, dev, bin_form=0)
    assert want["n"] > 40000
    wr = want["ranges"].astype(np.int64)
    monkeypatch.setattr(R, "BINNING", "auto")
    for too_low in (want["n"] // 4, 1):
        R._seen[key] = [too_low, 20000]
        before = R.capacity_reruns
        got = _frame(sc, dev, bin_form=1)
        assert R.capacity_reruns == before + 1
        _same(want, got, f"auto, predictor {too_low}")
    monkeypatch.setattr(R, "BINNING", "capacity")
    R._seen[key] = [want["n"] // 4, 20000]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = _frame(sc, dev, bin_form=1)
    cap = got["capacity"]
    assert cap < want["n"] == got["n"]
    gr = got["ranges"].astype(np.int64)
    assert gr[:, 1].max() <= cap
    kept = gr[:, 1] > gr[:, 0]
    listed = wr[:, 1] > wr[:, 0]
    assert kept.any() and (listed & ~kept).any()
    first_dropped = int(np.nonzero(listed & ~kept)[0][0])
    assert not kept[first_dropped:].any() and np.array_equal(kept[:first_dropped], listed[:first_dropped])       # a prefix in image order
    assert wr[first_dropped, 1] > cap                                                                          # ... that ends where the lists stop fitting
    for tl in np.nonzero(kept)[0]:
        assert np.array_equal(gr[tl], wr[tl])
        assert np.array_equal(got["gid"][gr[tl, 0]:gr[tl, 1]], want["gid"][wr[tl, 0]:wr[tl, 1]])
        assert (got["tile"][gr[tl, 0]:gr[tl, 1]] == tl).all()
