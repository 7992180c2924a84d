"""Sparse baked playback in the C-ABI, host side (no GPU): the *_host twins of fdgs_state_extent / fdgs_state_gather / fdgs_state_scatter run
the very functions the device kernels compile (csrc/playback_ops.h), over host arrays; the pure-Python parts of fdgs.playback's sparse bake.

Everything here is EXACT.  The extent is one float32 subtraction, one fabsf and a maximum per component, which numpy's float32
`np.abs(cur - ref).max(-1)` evaluates with the same roundings; gather and copy-scatter move bits; a blended scatter is, row for row, what
fdgs_state_blend_host (test_playback_host.host_blend) writes."""
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

from test_playback_host import WEIGHTS, _state, host_blend

fdgs = importlib.import_module("4dgaussians_amd")
P = fdgs.playback
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fdgs_state_extent", "fdgs_state_extent_host", "fdgs_state_gather", "fdgs_state_gather_host", "fdgs_state_scatter",
       "fdgs_state_scatter_host")
WIDTH = dict(zip(P.FIELDS, P.FIELD_WIDTH))
ALL = 31
MASKS = [1, 2, 4, 8, 16, ALL]
CANARY = np.uint32(0xCAFEF00D)          # as a float32: a negative normal number no test data holds


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(fdgs._lib.LIB_PATH):
        importlib.import_module("4dgaussians_amd.build").build()
    return fdgs._lib.lib()


def canary(n, width):
    return np.full((n, width), CANARY, np.uint32).view(np.float32)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def random_state(n, seed, payloads=True):
    """{field: float32 [n, width]}; with `payloads` a few entries are NaNs with a payload, infinities and negative zeros: bit copies keep
    them."""
    g = np.random.default_rng(seed)
    st = {k: g.normal(0.0, 1.3, (n, w)).astype(np.float32) for k, w in WIDTH.items()}
    if payloads:
        for k in st:
            flat = bits(st[k]).reshape(-1)
            where = g.integers(0, flat.size, 4)
            flat[where] = np.array([0x7FA00001, 0xFFC12345, 0x7F800000, 0x80000000], np.uint32)[:where.size]
    return st


def arrays(state, mask):
    """fdgs_state_arrays over a {field: numpy array} (or None): the pointers of the fields `mask` selects, NULL elsewhere."""
    if state is None:
        return None
    s = fdgs._lib.StateArrays()
    for h, k in enumerate(P.FIELDS):
        if mask >> h & 1:
            setattr(s, k, state[k].ctypes.data)
    return s


def row_lists(N, seed=0):
    g = np.random.default_rng(seed + N)
    lists = {"all": np.arange(N), "every_other": np.arange(0, N, 2), "first": np.array([0]), "last": np.array([N - 1]),
             "random": np.sort(g.choice(N, size=max(1, N // 3), replace=False))}
    return {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in lists.items()}


def test_header_declares_the_six_functions_and_lib_binds_them(lib):
    text = open(os.path.join(ROOT, "include", "fdgs.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in fdgs._lib.SYMBOLS and hasattr(lib, name), name
    assert lib.fdgs_abi_version() == 6
    contract = text.split("Sparse baked playback")[1]
    for word in ("STRICTLY ASCENDING", "16-byte aligned", "FDGS_E_INVALID", "unsigned", "overlaps neither", "without a launch"):
        assert word in contract, word
    for name in ("motion_extent", "bake_sparse", "SparseBaked", "sparse_bake_bytes"):
        assert hasattr(P, name), name
    for n in ("1.", "2.", "3.", "4."):
        assert n in P.SparseBaked.__doc__


# ---- extent ----------------------------------------------------------------------------------------------------------------------------

def host_extent(lib, n, mask, ref, cur, ext):
    rc = lib.fdgs_state_extent_host(n, mask, arrays(ref, mask), arrays(cur, mask), ext.ctypes.data)
    assert rc == 0, lib.fdgs_last_error()


def fresh_extent(n, mask):
    """[n,5]: zeros in the selected columns, the canary in the others."""
    ext = canary(n, 5).copy()
    for h in range(5):
        if mask >> h & 1:
            ext[:, h] = 0.0
    return ext


def check_extent_columns(ext, mask, expected):
    for h, k in enumerate(P.FIELDS):
        if mask >> h & 1:
            assert np.array_equal(bits(ext[:, h]), bits(expected[k])), k          # exact, the sign of a zero included
        else:
            assert (bits(ext[:, h]) == CANARY).all(), k


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("n", [1, 4099])
def test_host_extent_is_numpy_float32(lib, n, mask):
    ref, cur, cur2 = (random_state(n, seed, payloads=False) for seed in (n, n + 1, n + 2))
    for k in cur2:
        cur2[k] = (ref[k] + np.float32(0.5) * (cur2[k] - ref[k])).astype(np.float32)    # nearer to ref: some rows keep the first maximum
    ext = fresh_extent(n, mask)
    host_extent(lib, n, mask, ref, cur, ext)
    first = {k: np.abs(cur[k] - ref[k]).max(axis=-1) for k in P.FIELDS}
    assert all(v.dtype == np.float32 for v in first.values())
    check_extent_columns(ext, mask, first)
    host_extent(lib, n, mask, ref, cur2, ext)                                            # a second call keeps the running maximum
    second = {k: np.maximum(first[k], np.abs(cur2[k] - ref[k]).max(axis=-1)) for k in P.FIELDS}
    check_extent_columns(ext, mask, second)
    if n > 1:
        assert any((second[k] != first[k]).any() and (second[k] == first[k]).any() for k in P.FIELDS)
    host_extent(lib, n, mask, ref, ref, ext)                                             # no motion: nothing changes
    check_extent_columns(ext, mask, second)


def test_host_extent_of_a_nan_difference_is_infinite(lib):
    n = 6
    ref, cur = random_state(n, 1, payloads=False), random_state(n, 2, payloads=False)
    for k, w in WIDTH.items():
        cur[k][0, w - 1] = np.nan                                   # a NaN component, the last of the row
        ref[k][1, 0] = np.nan                                       # ... on the other side, the first of the row
        ref[k][2, 0] = cur[k][2, 0] = np.inf                        # inf - inf
        cur[k][3, 0] = -np.inf                                      # an honest infinity
    ext = fresh_extent(n, ALL)
    host_extent(lib, n, ALL, ref, cur, ext)
    assert np.isposinf(ext[:4]).all() and np.isfinite(ext[4:]).all() and not np.isnan(ext).any()
    host_extent(lib, n, ALL, ref, ref, ext)                         # rows 0 .. 2 again (NaN - NaN, inf - inf), rows 3 .. 5 at rest
    assert np.isposinf(ext[:4]).all() and np.isfinite(ext[4:]).all()
    for h, k in enumerate(P.FIELDS):
        assert np.array_equal(ext[4:, h], np.abs(cur[k][4:] - ref[k][4:]).max(axis=-1)), k


# ---- gather and scatter ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("N", [1, 4099])
def test_host_gather_then_copy_scatter_restores_the_listed_rows(lib, N, mask):
    full = random_state(N, 40 + N)
    for name, rows in row_lists(N).items():
        D = len(rows)
        compact = {k: canary(D, w).copy() for k, w in WIDTH.items()}
        rc = lib.fdgs_state_gather_host(D, rows.ctypes.data, N, mask, arrays(full, mask), arrays(compact, mask))
        assert rc == 0, lib.fdgs_last_error()
        out = {k: canary(N, w).copy() for k, w in WIDTH.items()}
        rc = lib.fdgs_state_scatter_host(D, rows.ctypes.data, N, mask, arrays(compact, mask), None, 0.0, arrays(out, mask))
        assert rc == 0, lib.fdgs_last_error()
        listed = np.zeros(N, bool)
        listed[rows] = True
        for h, k in enumerate(P.FIELDS):
            if mask >> h & 1:
                assert np.array_equal(bits(compact[k]), bits(full[k][rows])), (name, k)
                assert np.array_equal(bits(out[k][listed]), bits(full[k][listed])), (name, k)
                assert (bits(out[k][~listed]) == CANARY).all(), (name, k)
            else:
                assert (bits(compact[k]) == CANARY).all() and (bits(out[k]) == CANARY).all(), (name, k)


def blend_states(D, seed):
    """(a, b) of test_playback_host._state as {field: numpy [D, width]} plus the torch dicts host_blend takes."""
    ta, tb = _state(D, seed)
    key = dict(xyz="xyz", scales="scales", rotations="rot", opacity="opacity", shs="shs")
    to_np = lambda t: {k: np.ascontiguousarray(t[key[k]].numpy().reshape(D, WIDTH[k])) for k in P.FIELDS}
    return to_np(ta), to_np(tb), ta, tb, key


@pytest.mark.parametrize("w", WEIGHTS)
@pytest.mark.parametrize("N", [1, 4099])
def test_host_blended_scatter_is_state_blend_on_the_listed_rows(lib, N, w):
    for name, rows in row_lists(N).items():
        D = len(rows)
        a, b, ta, tb, key = blend_states(D, seed=7 + D)
        ref = host_blend(lib, ta, tb, w)
        for mask in (MASKS if name == "random" else [ALL]):
            out = {k: canary(N, wd).copy() for k, wd in WIDTH.items()}
            rc = lib.fdgs_state_scatter_host(D, rows.ctypes.data, N, mask, arrays(a, mask), arrays(b, mask), w, arrays(out, mask))
            assert rc == 0, lib.fdgs_last_error()
            listed = np.zeros(N, bool)
            listed[rows] = True
            for h, k in enumerate(P.FIELDS):
                if mask >> h & 1:
                    assert np.array_equal(bits(out[k][listed]), bits(ref[key[k]].numpy().reshape(D, WIDTH[k]))), (name, mask, k)
                    assert (bits(out[k][~listed]) == CANARY).all(), (name, mask, k)
                else:
                    assert (bits(out[k]) == CANARY).all(), (name, mask, k)


def test_host_bad_arguments(lib):
    N, D = 9, 3
    full, a, b = random_state(N, 1), random_state(D, 2), random_state(D, 3)
    out = {k: canary(N, w).copy() for k, w in WIDTH.items()}
    compact = {k: canary(D, w).copy() for k, w in WIDTH.items()}
    ext, calm = fresh_extent(N, ALL), random_state(N, 4, payloads=False)
    rows = np.array([1, 4, 8], np.int32)
    R = rows.ctypes.data
    A = lambda s, mask=ALL: arrays(s, mask)
    untouched = lambda: all((bits(v) == CANARY).all() for v in (*out.values(), *compact.values()))

    def refused(rc, word):
        assert rc == -1 and word in lib.fdgs_last_error(), (rc, word, lib.fdgs_last_error())
        assert untouched()

    # nothing to do succeeds, on the device entry points too (nothing is launched, no device is touched)
    for args in ((0, None, N, ALL, None, None), (0, None, 0, ALL, None, None), (D, R, N, 0, None, None)):
        assert lib.fdgs_state_gather_host(*args) == 0 and lib.fdgs_state_gather(None, *args) == 0
        assert lib.fdgs_state_scatter_host(*args[:5], None, 0.0, args[5]) == 0 and lib.fdgs_state_scatter(None, *args[:5], None, 0.0, args[5]) == 0
    for args in ((0, ALL, None, None, None), (N, 0, None, None, None)):
        assert lib.fdgs_state_extent_host(*args) == 0 and lib.fdgs_state_extent(None, *args) == 0
    # sizes
    for d, n in ((-1, N), (D, -1), (N + 1, N)):
        refused(lib.fdgs_state_gather_host(d, R, n, ALL, A(full), A(compact)), b"bad")
        refused(lib.fdgs_state_scatter_host(d, R, n, ALL, A(a), None, 0.0, A(out)), b"bad")
        refused(lib.fdgs_state_gather(None, d, R, n, ALL, A(full), A(compact)), b"bad")
        refused(lib.fdgs_state_scatter(None, d, R, n, ALL, A(a), None, 0.0, A(out)), b"bad")
    refused(lib.fdgs_state_extent_host(-1, ALL, A(full), A(full), ext.ctypes.data), b"N")
    refused(lib.fdgs_state_extent(None, -1, ALL, A(full), A(full), ext.ctypes.data), b"N")
    refused(lib.fdgs_state_gather_host(D, R, N, 32, A(full), A(compact)), b"field_mask")
    refused(lib.fdgs_state_scatter_host(D, R, N, 32, A(a), None, 0.0, A(out)), b"field_mask")
    refused(lib.fdgs_state_extent_host(N, 32, A(full), A(full), ext.ctypes.data), b"field_mask")
    # the weight
    for w in (1.5, -0.1, float("nan")):
        refused(lib.fdgs_state_scatter_host(D, R, N, ALL, A(a), A(b), w, A(out)), b"bad w")
        refused(lib.fdgs_state_scatter(None, D, R, N, ALL, A(a), A(b), w, A(out)), b"bad w")
    refused(lib.fdgs_state_scatter_host(D, R, N, ALL, A(a), None, 0.5, A(out)), b"bad w")
    refused(lib.fdgs_state_scatter(None, D, R, N, ALL, A(a), None, 0.5, A(out)), b"bad w")
    # NULL pointers: the list, a whole state, one selected field of any state
    refused(lib.fdgs_state_gather_host(D, None, N, ALL, A(full), A(compact)), b"NULL")
    refused(lib.fdgs_state_scatter_host(D, None, N, ALL, A(a), None, 0.0, A(out)), b"NULL")
    refused(lib.fdgs_state_gather_host(D, R, N, ALL, None, A(compact)), b"NULL")
    refused(lib.fdgs_state_gather_host(D, R, N, ALL, A(full), None), b"NULL")
    refused(lib.fdgs_state_scatter_host(D, R, N, ALL, None, None, 0.0, A(out)), b"NULL")
    refused(lib.fdgs_state_scatter_host(D, R, N, ALL, A(a), None, 0.0, None), b"NULL")
    refused(lib.fdgs_state_extent_host(N, ALL, None, A(full), ext.ctypes.data), b"NULL")
    refused(lib.fdgs_state_extent_host(N, ALL, A(full), None, ext.ctypes.data), b"NULL")
    refused(lib.fdgs_state_extent_host(N, ALL, A(full), A(full), None), b"NULL")
    for h in range(5):
        part = ALL & ~(1 << h)
        refused(lib.fdgs_state_gather_host(D, R, N, ALL, A(full, part), A(compact)), b"NULL")
        refused(lib.fdgs_state_gather_host(D, R, N, ALL, A(full), A(compact, part)), b"NULL")
        refused(lib.fdgs_state_scatter_host(D, R, N, ALL, A(a, part), None, 0.0, A(out)), b"NULL")
        refused(lib.fdgs_state_scatter_host(D, R, N, ALL, A(a), A(b, part), 0.5, A(out)), b"NULL")
        refused(lib.fdgs_state_scatter_host(D, R, N, ALL, A(a), None, 0.0, A(out, part)), b"NULL")
        refused(lib.fdgs_state_extent_host(N, ALL, A(full, part), A(full), ext.ctypes.data), b"NULL")
        refused(lib.fdgs_state_extent_host(N, ALL, A(full), A(full, part), ext.ctypes.data), b"NULL")
        # ... and an unselected field may be NULL
        assert lib.fdgs_state_extent_host(N, part, A(calm, part), A(calm, part), ext.ctypes.data) == 0
    assert (ext == 0).all()
    # bad lists: the twins read them
    for bad, word in (([1, 4, 9], b"outside"), ([-1, 4, 8], b"outside"), ([1, 4, 4], b"ascending"), ([4, 1, 8], b"ascending"),
                      ([8, 4, 1], b"ascending")):
        lst = np.array(bad, np.int32)
        refused(lib.fdgs_state_gather_host(D, lst.ctypes.data, N, ALL, A(full), A(compact)), word)
        refused(lib.fdgs_state_scatter_host(D, lst.ctypes.data, N, ALL, A(a), None, 0.0, A(out)), word)
        refused(lib.fdgs_state_scatter_host(D, lst.ctypes.data, N, ALL, A(a), A(b), 0.5, A(out)), word)
    # the device entry points check alignment before they touch a device: rotations and SH on 16 bytes
    buf = np.zeros(N * 48 + 16, np.float32)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    for h in (2, 4):
        good, odd = fdgs._lib.StateArrays(), fdgs._lib.StateArrays()
        setattr(good, P.FIELDS[h], base)
        setattr(odd, P.FIELDS[h], base + 4)
        for x, y in ((odd, good), (good, odd)):
            refused(lib.fdgs_state_gather(None, D, R, N, 1 << h, x, y), b"aligned")
            refused(lib.fdgs_state_scatter(None, D, R, N, 1 << h, x, None, 0.0, y), b"aligned")
            refused(lib.fdgs_state_extent(None, N, 1 << h, x, y, ext.ctypes.data), b"aligned")
        refused(lib.fdgs_state_scatter(None, D, R, N, 1 << h, good, odd, 0.5, good), b"aligned")
    # (the twins take any alignment)
    odd_state = {k: np.zeros(N * w + 1, np.float32)[1:].reshape(N, w) for k, w in WIDTH.items()}
    assert lib.fdgs_state_extent_host(N, ALL, A(odd_state), A(odd_state), ext.ctypes.data) == 0


# ---- Python helpers --------------------------------------------------------------------------------------------------------------------

def test_sparse_bake_bytes():
    pad = lambda floats: (floats + P.SLOT_ALIGN_FLOATS - 1) // P.SLOT_ALIGN_FLOATS * P.SLOT_ALIGN_FLOATS
    for N in (4099, 1, 8200):
        full = pad(3 * N) * 2 + pad(4 * N) + pad(N) + pad(48 * N)
        for T in (1, 4):
            for D in (0, 1, N):
                assert P.sparse_bake_bytes(N, D, T, (1, 1, 1, 1, 1)) == 4 * (full + T * (2 * pad(3 * D) + pad(4 * D) + pad(D) + pad(48 * D)) + pad(D))
                assert P.sparse_bake_bytes(N, D, T, (1, 1, 1, 0, 0)) == 4 * (full + T * (2 * pad(3 * D) + pad(4 * D)) + pad(D))
            for on in ((1, 1, 1, 1, 1), (1, 1, 1, 0, 0)):
                assert P.sparse_bake_bytes(N, 0, T, on) == 4 * full                      # the D = 0 figure: the full state alone
                # D == N: the dense bake, one more state of the fields that are on (the working state), and the row list
                assert P.sparse_bake_bytes(N, N, T, on) == (P.bake_bytes(N, T, on) + 4 * sum(pad(N * w) for w, o in zip(P.FIELD_WIDTH, on) if o)
                                                             + 4 * pad(N))
    on = (1, 1, 1, 1, 1)
    sizes = [P.sparse_bake_bytes(4099, D, 4, on) for D in range(0, 4100, 97)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]                                # monotone in D ...
    sizes = [P.sparse_bake_bytes(4099, 410, T, on) for T in range(1, 9)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)                       # ... and in T
    assert P.sparse_bake_bytes(300_000, 30_000, 300, on) < P.bake_bytes(300_000, 300, on) // 9
    for bad in ((10, 11, 1, on), (10, -1, 1, on), (-1, 0, 1, on), (10, 5, 0, on), (10, 5, 1, (1, 1, 1, 1))):
        with pytest.raises(ValueError):
            P.sparse_bake_bytes(*bad)


def test_bake_sparse_and_motion_extent_validate_before_they_touch_the_model_or_the_device():
    pc = fdgs.synthetic.SynthModel(100, "dnerf_bouncingballs", seed=2)
    for bad in ([0.0, 0.5, 0.5], [], [0.0, float("nan")]):
        with pytest.raises(ValueError):
            P.bake_sparse(pc, bad, 0.1)
        with pytest.raises(ValueError):
            P.motion_extent(pc, bad)
    for bad in (float("nan"), (0.1, 0.1, float("nan"), 0.1, 0.1), (0.1, 0.1), (0.1,) * 6):
        with pytest.raises(ValueError):
            P.bake_sparse(pc, [0.0, 0.5, 1.0], bad)
    stranger = type("Stranger", (), {"_deformation": object(), "_xyz": torch.zeros(3, 3)})()
    with pytest.raises(TypeError):
        P.bake_sparse(stranger, [0.0, 1.0], 0.1)
    with pytest.raises(TypeError):
        P.motion_extent(stranger, [0.0, 1.0])
    need = P.sparse_bake_bytes(100, 0, 3, [1, 1, 1, 0, 0])
    with pytest.raises(MemoryError):
        P.bake_sparse(pc, [0.0, 0.5, 1.0], 0.1, max_bytes=need - 1)
    with pytest.raises(fdgs._lib.FdgsError):              # enough memory allowed: the next thing it needs is a device (there is no CPU path)
        P.bake_sparse(pc, [0.0, 0.5, 1.0], (0.1, 0.1, 0.1, math.inf, -1.0), max_bytes=need)
    with pytest.raises(fdgs._lib.FdgsError):
        P.motion_extent(pc, [0.0, 0.5, 1.0])
    assert "stale" in P.Baked.__doc__ and "SNAPSHOT" in P.SparseBaked.__doc__


def test_compose_refuses_a_sparse_bake():
    sparse = object.__new__(P.SparseBaked)
    with pytest.raises(TypeError, match="Baked"):
        fdgs.compose.compose([sparse])
