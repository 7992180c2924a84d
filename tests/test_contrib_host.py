"""The contribution pass in the C-ABI and its Python helpers, host side (no GPU): fdgs_render_contrib refuses every bad argument with
FDGS_E_INVALID and a message BEFORE anything is launched and leaves `rows` as it stood -- the library loads and validates without a device,
as the pick entry point does --; Baked.select_rows and Contribution.keep_mask are checked on CPU tensors against values written by hand."""
import ctypes
import importlib
import os
import re
import types

import numpy as np
import pytest
import torch

fdgs = importlib.import_module("4dgaussians_amd")
P, L = fdgs.playback, fdgs._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 40, 36, 48
FIELDS = ("weight_sum", "weight_max", "pixels", "tiles")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        importlib.import_module("4dgaussians_amd.build").build()
    return L.lib()


def test_header_declares_the_entry_point_and_the_struct_and_lib_binds_it(lib):
    text = open(os.path.join(ROOT, "include", "fdgs.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+fdgs_render_contrib\s*\(", src)
    assert "fdgs_render_contrib" in L.SYMBOLS and hasattr(lib, "fdgs_render_contrib")
    assert lib.fdgs_abi_version() == 6 and L.ABI_VERSION == 6                        # an addition to ABI 6
    body = re.search(r"typedef struct fdgs_contrib_row \{(.*?)\} fdgs_contrib_row;", src, flags=re.S).group(1)
    decls = [d.split() for d in body.split(";") if d.strip()]
    assert decls == [["float", "weight_sum"], ["float", "weight_max"], ["uint32_t", "pixels"], ["uint32_t", "tiles"]]
    assert [f[0] for f in L.ContribRow._fields_] == list(FIELDS) and ctypes.sizeof(L.ContribRow) == 16
    assert [L.ContribRow._fields_[k][1] for k in range(4)] == [ctypes.c_float, ctypes.c_float, ctypes.c_uint32, ctypes.c_uint32]
    restype, argtypes = L.SYMBOLS["fdgs_render_contrib"]
    assert restype is ctypes.c_int and len(argtypes) == 9
    decl = re.search(r"\bint\s+fdgs_render_contrib\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
    assert len(decl.split(",")) == 9 and decl.split(",")[-1].split() == ["fdgs_contrib_row*", "rows"]


def _good():
    """A call that is valid up to the launch (never made here: there is no device), as keyword -> value; host arrays stand in for the
    buffers.  `rows` lies on a 16-byte boundary inside `store`, with a record of sentinels in front of it and one behind."""
    store = np.full(4 * (N + 2) + 4, -7, np.int32)
    skip = (-store.ctypes.data // 4) % 4                                             # words up to the next 16-byte boundary
    bufs = types.SimpleNamespace(geom=np.zeros(64, np.uint8), binning=np.zeros(64, np.uint8), img=np.zeros(64, np.uint8),
                                 row_map=np.arange(N, dtype=np.int32), weight=np.ones(H * W + 1, np.float32), store=store)
    rows = store.ctypes.data + 4 * (skip + 4)
    assert rows % 16 == 0
    p = L.RasterParams()
    p.P, p.W, p.H = N, W, H
    good = dict(stream=None, p=p, geom=bufs.geom.ctypes.data, binning=bufs.binning.ctypes.data, img=bufs.img.ctypes.data, R=100,
                pixel_weight=bufs.weight.ctypes.data, row_map=bufs.row_map.ctypes.data, rows=rows)
    return good, bufs


def _refused(lib, args, bufs, what):
    before = bufs.store.copy()
    assert lib.fdgs_render_contrib(*args.values()) == -1, what                       # FDGS_E_INVALID
    msg = lib.fdgs_last_error()
    assert msg, what
    assert np.array_equal(bufs.store, before), what
    return msg


def test_null_pointers_are_refused(lib):
    for name in ("p", "geom", "binning", "img", "rows"):
        good, bufs = _good()
        assert b"NULL" in _refused(lib, {**good, name: None}, bufs, name)


@pytest.mark.parametrize("field,value", [("W", 0), ("H", 0), ("H", -3), ("W", -1), ("P", -1), ("P", -2 ** 31)])
def test_bad_sizes_are_refused(lib, field, value):
    good, bufs = _good()
    setattr(good["p"], field, value)
    _refused(lib, good, bufs, (field, value))


@pytest.mark.parametrize("which,shifts", [("rows", (1, 2, 3, 4, 8, 12)), ("pixel_weight", (1, 2, 3)), ("row_map", (1, 2, 3))])
def test_misaligned_arrays_are_refused(lib, which, shifts):
    for shift in shifts:
        good, bufs = _good()
        good[which] += shift
        assert b"aligned" in _refused(lib, good, bufs, (which, shift))


def test_an_empty_frame_succeeds_without_a_device_and_without_touching_rows(lib):
    """P == 0 or num_rendered == 0: FDGS_OK before anything is launched (this process has no device), rows as they stood; the optional
    arrays may be NULL."""
    for change in (dict(R=0), dict(P=0), dict(R=0, pixel_weight=None, row_map=None)):
        good, bufs = _good()
        if "P" in change:
            good["p"].P = change.pop("P")
        before = bufs.store.copy()
        assert lib.fdgs_render_contrib(*{**good, **change}.values()) == 0, change
        assert np.array_equal(bufs.store, before), change


# ---- Contribution ------------------------------------------------------------------------------------------------------------------------

def test_contribution_views_and_keep_mask_against_hand_written_values():
    c = P.Contribution(5, torch.device("cpu"))
    assert c.N == 5 and c.frames == 0 and c.rows.shape == (5, 4) and c.rows.dtype == torch.int32 and not c.rows.any()
    assert c.weight_sum.dtype == c.weight_max.dtype == torch.float32 and c.pixels.dtype == c.tiles.dtype == torch.int32
    assert c.weight_sum.shape == c.weight_max.shape == c.pixels.shape == c.tiles.shape == (5,)
    #                 weight_sum  weight_max  pixels  tiles
    table = [(0.0, 0.0, 0, 0), (0.75, 0.5, 3, 1), (4.0, 0.25, 40, 2), (0.125, 0.125, 1, 1), (9.0, 0.99, 300, 4)]
    for r, (s, m, px, tl) in enumerate(table):
        c.weight_sum[r], c.weight_max[r], c.pixels[r], c.tiles[r] = s, m, px, tl                  # the views write through to `rows`
    raw = c.rows.numpy()
    assert np.array_equal(raw[:, 0].copy().view(np.float32), np.float32([t[0] for t in table]))
    assert np.array_equal(raw[:, 1].copy().view(np.float32), np.float32([t[1] for t in table]))
    assert raw[:, 2].tolist() == [0, 3, 40, 1, 300] and raw[:, 3].tolist() == [0, 1, 2, 1, 4]
    assert c.keep_mask().dtype == torch.bool
    assert c.keep_mask().tolist() == [False, True, True, True, True]                               # min_pixels = 1
    assert c.keep_mask(min_pixels=0).tolist() == [True] * 5
    assert c.keep_mask(min_pixels=3).tolist() == [False, True, True, False, True]
    assert c.keep_mask(min_pixels=4).tolist() == [False, False, True, False, True]
    assert c.keep_mask(min_weight_max=0.25).tolist() == [False, True, True, False, True]
    assert c.keep_mask(min_pixels=0, min_weight_sum=0.75).tolist() == [False, True, True, False, True]
    assert c.keep_mask(min_pixels=2, min_weight_max=0.3, min_weight_sum=1.0).tolist() == [False, False, False, False, True]
    c.frames = 3
    c.reset()
    assert c.frames == 0 and not c.rows.any()
    with pytest.raises(ValueError):
        P.Contribution(-1, torch.device("cpu"))


# ---- Baked.select_rows on a hand-made bake -----------------------------------------------------------------------------------------------

N7, T3 = 7, 3
HEAD_ON = (True, True, False, True, True)                      # rotations do not move: their array is stored once
TIMES = (0.0, 0.5, 1.0)


def _hand_made(perm):
    """A Baked of 7 rows and 3 timestamps in the layout of `bake`, every float distinct: value = 1000 * field + 100 * timestamp + stored row
    + column / 64 (exact in float32)."""
    copies = [T3 if on else 1 for on in HEAD_ON]
    storage = torch.full((P.bake_bytes(N7, T3, HEAD_ON) // 4,), -1.0)
    views = P._carve(P._field_slots(N7, copies), storage)[1]
    for h, per_time in enumerate(views):
        for k, v in enumerate(per_time):
            cols = v[0].numel()
            v.copy_((1000.0 * h + 100.0 * k + torch.arange(N7).reshape(-1, 1) + torch.arange(cols).reshape(1, -1) / 64.0).reshape(v.shape))
    slots = [v if on else v * T3 for v, on in zip(views, HEAD_ON)]
    frames = [P.BakedFrame([slots[h][k] for h in range(5)]) for k in range(T3)]
    return P.Baked(TIMES, frames, HEAD_ON, perm, storage, 2)


def _check_selection(full, keep, kept_model_rows):
    """`kept_model_rows`: the kept rows of the model, ascending, written by hand."""
    sel = full.select_rows(keep)
    n = len(kept_model_rows)
    stored_to_model = list(range(N7)) if full.perm is None else full.perm.tolist()
    kept_stored = [i for i in range(N7) if stored_to_model[i] in kept_model_rows]                 # stored order is preserved
    assert sel.N == n and sel.times == full.times and sel.head_on == full.head_on and sel.active_sh_degree == 2
    assert sel.nbytes == P.bake_bytes(n, T3, HEAD_ON) and sel._storage.numel() * 4 == sel.nbytes
    assert sel._storage.data_ptr() != full._storage.data_ptr() or n == 0                          # a snapshot
    for k in range(T3):
        for h, name in enumerate(P.FIELDS):
            got, src = getattr(sel.frames[k], name), getattr(full.frames[k], name)
            assert got.shape == (n, *P.FIELD_SHAPE[h]) and got.dtype == torch.float32
            assert torch.equal(got, src[kept_stored]), (k, name)
            if not HEAD_ON[h]:
                assert got.data_ptr() == getattr(sel.frames[0], name).data_ptr()                  # stored once
            elif k and n:
                assert got.data_ptr() != getattr(sel.frames[0], name).data_ptr()
    if full.perm is None:
        assert sel.perm is None and sel._maps == (None, None)
    else:
        rank = {m: r for r, m in enumerate(sorted(kept_model_rows))}
        assert sel.perm.dtype == full.perm.dtype and sel.perm.tolist() == [rank[stored_to_model[i]] for i in kept_stored]
        assert sorted(sel.perm.tolist()) == list(range(n))
    return sel


@pytest.mark.parametrize("perm", [None, [3, 0, 6, 1, 5, 2, 4]], ids=["model_order", "permuted"])
def test_select_rows_on_a_hand_made_bake(perm):
    full = _hand_made(None if perm is None else torch.tensor(perm, dtype=torch.int32))
    assert full.N == N7 and full.nbytes == P.bake_bytes(N7, T3, HEAD_ON)
    before = full._storage.clone()
    mask = torch.tensor([True, False, False, True, True, False, True])
    sel = _check_selection(full, mask, [0, 3, 4, 6])
    if perm is not None:                       # stored rows 0 (model 3), 1 (0), 2 (6), 6 (4) stay, in that order; ranks of 3, 0, 6, 4 among {0,3,4,6}
        assert sel.perm.tolist() == [1, 0, 3, 2]
        assert sel.frames[1].xyz[:, 0].tolist() == [100.0, 101.0, 102.0, 106.0]
    else:
        assert sel.frames[1].xyz[:, 0].tolist() == [100.0, 103.0, 104.0, 106.0]
    _check_selection(full, torch.tensor([6, 0, 4, 3, 0]), [0, 3, 4, 6])                            # an index tensor, any order, repeats
    _check_selection(full, torch.tensor([5], dtype=torch.int32), [5])
    _check_selection(full, torch.ones(N7, dtype=torch.bool), list(range(N7)))                      # every row
    empty = _check_selection(full, torch.zeros(N7, dtype=torch.bool), [])                          # no row
    assert empty.N == 0 and empty.nbytes == P.bake_bytes(0, T3, HEAD_ON)
    _check_selection(full, torch.zeros(0, dtype=torch.int64), [])
    assert torch.equal(full._storage, before)                                                      # the source is not written
    for bad in (torch.ones(N7 - 1, dtype=torch.bool), torch.ones(N7 + 1, dtype=torch.bool), torch.ones(N7, 1, dtype=torch.bool)):
        with pytest.raises(ValueError):
            full.select_rows(bad)
    for bad in (torch.tensor([7]), torch.tensor([-1]), torch.tensor([0.0, 1.0]), torch.tensor([[0, 1]])):
        with pytest.raises(ValueError):
            full.select_rows(bad)


def test_a_selection_of_a_selection_composes():
    full = _hand_made(torch.tensor([3, 0, 6, 1, 5, 2, 4], dtype=torch.int32))
    first = full.select_rows(torch.tensor([True, True, False, True, True, False, True]))           # model rows 0 1 3 4 6
    second = first.select_rows(torch.tensor([False, True, True, False, True]))                      # of those: 1 3 6
    direct = full.select_rows(torch.tensor([1, 3, 6]))
    assert second.N == direct.N == 3 and second.perm.tolist() == direct.perm.tolist()
    for k in range(T3):                                        # (the padding between the slots is never written: compare the arrays)
        for a, b in zip(second.frames[k].arrays(), direct.frames[k].arrays()):
            assert torch.equal(a, b)
