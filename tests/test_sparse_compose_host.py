"""Composites of sparse bakes, host side (no GPU): fdgs_state_place_rows_host against fdgs_state_place_host, and what fdgs.compose does
with allow_sparse before it needs a device.

Everything here is EXACT: the new twin calls the functions of csrc/compose_ops.h that fdgs_state_place_host calls, on compact row r, and
writes the result to row rows[r]; the expected array is therefore the placed compact state, its rows moved by numpy."""
import importlib
import itertools
import os
import re

import numpy as np
import pytest
import torch

from test_compose_host import general_placement
from test_sparse_playback_host import ALL, CANARY, WIDTH, arrays, bits, blend_states, canary, random_state

fdgs = importlib.import_module("4dgaussians_amd")
C, P = fdgs.compose, fdgs.playback
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fdgs_state_place_rows", "fdgs_state_place_rows_host")
NEAR_ONE = float(np.nextafter(np.float32(1), np.float32(0)))
BLENDS = [(False, 0.0), (True, 0.0), (True, 0.25), (True, NEAR_ONE)]
PLACE_MASKS = (ALL, 0b10101, 0b01011)
SIZES = (1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(fdgs._lib.LIB_PATH):
        importlib.import_module("4dgaussians_amd.build").build()
    return fdgs._lib.lib()


def row_lists(D, N):
    """Strictly ascending lists of exactly D rows of N: all, every other, random; for one row the first and the last as well."""
    if N == D:
        return {"all": np.arange(D, dtype=np.int32)}
    g = np.random.default_rng(D)
    out = {"every_other": np.arange(0, 2 * D, 2, dtype=np.int32), "random": np.sort(g.choice(N, size=D, replace=False)).astype(np.int32)}
    if D == 1:
        out.update(first=np.array([0], np.int32), last=np.array([N - 1], np.int32))
    return out


def placed_compact(lib, ps, D, a, b, w):
    """fdgs_state_place_host over the D compact rows, all fields -> {field: float32 [D, width]}."""
    tmp = {k: canary(D, wd).copy() for k, wd in WIDTH.items()}
    rc = lib.fdgs_state_place_host(ps, D, ALL, arrays(a, ALL), arrays(b, ALL), w, arrays(tmp, ALL))
    assert rc == 0, lib.fdgs_last_error()
    return tmp


def test_header_declares_the_two_functions_and_lib_binds_them(lib):
    text = open(os.path.join(ROOT, "include", "fdgs.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in fdgs._lib.SYMBOLS and hasattr(lib, name), name
    assert lib.fdgs_abi_version() == 6
    contract = text.split("Placing a SPARSE bake")[1].split("Sparse baked playback")[0]
    for word in ("STRICTLY ASCENDING", "16-byte aligned", "FDGS_E_INVALID", "unsigned", "without a launch", "state_place_rows", "bit for bit"):
        assert word in contract, word
    assert "stale" in C.Composite.__doc__ and "allow_sparse" in C.compose.__doc__


@pytest.mark.parametrize("D", SIZES)
def test_host_place_rows_is_host_place_moved_to_the_listed_rows(lib, D):
    a, b, _, _, _ = blend_states(D, seed=300 + D)
    keep_a, keep_b = ({k: v.copy() for k, v in s.items()} for s in (a, b))
    ref = {}
    for N in (D, 2 * D + 3):
        for (name, rows), mode, deg, (blend, w), mask in itertools.product(row_lists(D, N).items(), ("points", "rigid"), (0, 3), BLENDS, PLACE_MASKS):
            assert len(rows) == D and (np.diff(rows) > 0).all() and 0 <= rows[0] and rows[-1] < N
            ps = general_placement(mode).struct(deg)
            key = (mode, deg, blend, w)
            if key not in ref:
                ref[key] = placed_compact(lib, ps, D, a, b if blend else None, w)
            out = {k: canary(N, wd).copy() for k, wd in WIDTH.items()}
            rc = lib.fdgs_state_place_rows_host(ps, D, rows.ctypes.data, N, mask, arrays(a, mask), arrays(b if blend else None, mask), w,
                                                arrays(out, mask))
            assert rc == 0, lib.fdgs_last_error()
            listed = np.zeros(N, bool)
            listed[rows] = True
            for h, k in enumerate(P.FIELDS):
                if mask >> h & 1:
                    assert np.array_equal(bits(out[k][rows]), bits(ref[key][k])), (N, name, key, mask, k)         # bit for bit
                    assert (bits(out[k][~listed]) == CANARY).all(), (N, name, key, mask, k)
                else:
                    assert (bits(out[k]) == CANARY).all(), (N, name, key, mask, k)
    # the placement does something, and the blend too
    assert not np.array_equal(ref["rigid", 3, False, 0.0]["shs"], a["shs"]) and not np.array_equal(ref["rigid", 3, True, 0.25]["xyz"], ref["rigid", 3, False, 0.0]["xyz"])
    for k in P.FIELDS:
        assert np.array_equal(bits(a[k]), bits(keep_a[k])) and np.array_equal(bits(b[k]), bits(keep_b[k])), k


def test_bad_arguments(lib):
    N, D = 9, 3
    a, b = random_state(D, 2), random_state(D, 3)
    out = {k: canary(N, w).copy() for k, w in WIDTH.items()}
    rows = np.array([1, 4, 8], np.int32)
    R = rows.ctypes.data
    A = lambda s, mask=ALL: arrays(s, mask)
    good = general_placement().struct(3)

    def variant(**kw):
        p = general_placement().struct(3)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def refused(args, word):
        for rc in (lib.fdgs_state_place_rows_host(*args), lib.fdgs_state_place_rows(None, *args)):      # checked before a device is touched
            assert rc == -1 and word in lib.fdgs_last_error(), (rc, word, lib.fdgs_last_error())
            assert all((bits(v) == CANARY).all() for v in out.values())

    # nothing to do succeeds with NULL arrays, on the device entry point too
    for args in ((good, 0, None, N, ALL, None, None, 0.0, None), (good, 0, None, 0, ALL, None, None, 0.0, None),
                 (good, D, R, N, 0, None, None, 0.0, None), (good, D, None, N, 0, None, None, 0.0, None)):
        assert lib.fdgs_state_place_rows_host(*args) == 0 and lib.fdgs_state_place_rows(None, *args) == 0
    # sizes and the mask
    for d, n in ((-1, N), (D, -1), (N + 1, N), (1, 0)):
        refused((good, d, R, n, ALL, A(a), None, 0.0, A(out)), b"bad")
    refused((good, D, R, N, 32, A(a), None, 0.0, A(out)), b"field_mask")
    # the weight
    for w in (1.5, -0.1, float("nan")):
        refused((good, D, R, N, ALL, A(a), A(b), w, A(out)), b"bad w")
    refused((good, D, R, N, ALL, A(a), None, 0.5, A(out)), b"bad w")
    # NULL pointers: the placement, the list, a whole state, one selected field of any state
    refused((None, D, R, N, ALL, A(a), None, 0.0, A(out)), b"NULL")
    refused((good, D, None, N, ALL, A(a), None, 0.0, A(out)), b"NULL")
    refused((good, D, R, N, ALL, None, None, 0.0, A(out)), b"NULL")
    refused((good, D, R, N, ALL, A(a), None, 0.0, None), b"NULL")
    for h in range(5):
        part = ALL & ~(1 << h)
        refused((good, D, R, N, ALL, A(a, part), None, 0.0, A(out)), b"NULL")
        refused((good, D, R, N, ALL, A(a), A(b, part), 0.5, A(out)), b"NULL")
        refused((good, D, R, N, ALL, A(a), None, 0.0, A(out, part)), b"NULL")
    # the placement
    refused((variant(mode=2), D, R, N, ALL, A(a), None, 0.0, A(out)), b"mode")
    for deg in (-1, 4):
        refused((variant(sh_degree=deg), D, R, N, ALL, A(a), None, 0.0, A(out)), b"sh_degree")
    for s in (0.0, -1.0, float("inf"), float("nan")):
        refused((variant(scale=s), D, R, N, ALL, A(a), None, 0.0, A(out)), b"scale")
    # bad lists: the twin reads them, and writes nothing
    for bad, word in (([1, 4, 9], b"outside"), ([-1, 4, 8], b"outside"), ([1, 4, 4], b"ascending"), ([4, 1, 8], b"ascending"),
                      ([8, 4, 1], b"ascending")):
        lst = np.array(bad, np.int32)
        for sb, w in ((None, 0.0), (A(b), 0.5)):
            assert lib.fdgs_state_place_rows_host(good, D, lst.ctypes.data, N, ALL, A(a), sb, w, A(out)) == -1
            assert word in lib.fdgs_last_error() and all((bits(v) == CANARY).all() for v in out.values()), bad
    # the device entry point checks alignment before it touches a device: the list on 4 bytes, the rotations and SH of a and b on 16
    buf = np.zeros(N * 48 + 16, np.float32)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    for h in (2, 4):
        ok, odd = fdgs._lib.StateArrays(), fdgs._lib.StateArrays()
        setattr(ok, P.FIELDS[h], base)
        setattr(odd, P.FIELDS[h], base + 4)
        assert lib.fdgs_state_place_rows(None, good, D, R, N, 1 << h, odd, None, 0.0, ok) == -1 and b"aligned" in lib.fdgs_last_error()
        assert lib.fdgs_state_place_rows(None, good, D, R, N, 1 << h, ok, odd, 0.5, ok) == -1 and b"aligned" in lib.fdgs_last_error()
    assert lib.fdgs_state_place_rows(None, good, D, R + 2, N, ALL, A(a), None, 0.0, A(out)) == -1 and b"aligned" in lib.fdgs_last_error()
    # a field that is not selected may be NULL, and the twin takes any alignment
    odd_a = {k: np.zeros(D * w + 1, np.float32)[1:].reshape(D, w) for k, w in WIDTH.items()}
    part = ALL & ~2
    assert lib.fdgs_state_place_rows_host(good, D, R, N, part, A(odd_a, part), None, 0.0, A(out, part)) == 0
    assert (bits(out["scales"]) == CANARY).all() and not (bits(out["xyz"][rows]) == CANARY).any()


def _sparse_stub(n, device="cpu"):
    sb = object.__new__(P.SparseBaked)
    sb.N, sb.D, sb.head_on, sb.times, sb.active_sh_degree, sb.perm = n, n // 4, (1, 1, 1, 0, 0), (0.0, 1.0), 3, None
    sb._working = torch.empty(0, device=device)
    return sb


def test_compose_with_sparse_models_refuses_in_the_order_compose_does():
    models = [_sparse_stub(4099), _sparse_stub(8200)]
    need = C.compose_bytes([4099, 8200])
    with pytest.raises(MemoryError):
        C.compose(models, max_bytes=need - 1, allow_sparse=True)
    with pytest.raises(fdgs._lib.FdgsError):                 # enough memory allowed: the next thing it needs is a device (there is no CPU path)
        C.compose(models, max_bytes=need, allow_sparse=True)
    for kw in ({}, {"allow_sparse": False}):
        with pytest.raises(TypeError, match="Baked"):
            C.compose(models, max_bytes=need, **kw)
    with pytest.raises(TypeError, match="allow_sparse=True"):
        C.compose(models[:1])
    with pytest.raises(TypeError):                           # the flag opens the door to sparse bakes, not to anything
        C.compose([object()], allow_sparse=True)
    with pytest.raises(ValueError):
        C.compose([_sparse_stub(5), _sparse_stub(5, device="meta")], allow_sparse=True)
