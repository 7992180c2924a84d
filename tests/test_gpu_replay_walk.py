"""The edges of the replay walk (csrc/blend_replay.h) that the four passes' own files do not meet, for all four passes at once:
render_pick_kernel, render_features_kernel, render_features_bwd_kernel, render_contrib_kernel.

What the passes' own files meet (tests/test_gpu_pick.py, test_gpu_features.py, test_gpu_features_bwd.py, test_gpu_contrib.py; all four run
on the pick file's frames (a) 40 x 36 and (b) 33 x 17):

    edge                                                    pick   features   features_bwd   contrib
    list > 512 entries with n_contrib past 512 (3 rounds)   (b)    (b)        (b)            (b)
    width and height no multiples of 16                     (a,b)  (a,b)      (a,b)          (a,b)
    P = 0, and P > 0 without pairs                          yes    yes        yes            yes
    tile order on (the knob's default; 3 x 2 tiles: kept)   yes    yes        yes            yes
    tile order OFF                                          --     --         --             --
    a list of exactly 256 entries, one of exactly 257       --     --         --             --

The last two rows are this file: one frame whose six tiles are built entry by entry, every pass over it with the tile order on and off.
The scene: 40 x 24 pixels = 3 x 2 tiles with a partial column and a partial row; every Gaussian is a small isotropic splat (radius 4
pixels) next to the centre of ONE tile, so a tile's list is exactly the Gaussians placed there, at low opacity so that the centre pixels
blend every entry of their list:

    tile 0: 600 entries (three rounds, n_contrib past 512)      tile 1: 256 entries (one full round, nothing staged behind it)
    tile 2: 257 entries (one entry in a second round; partial)  tile 3: 300 entries (partial row)
    tile 4: 5 entries (shorter than one 16-entry block)          tile 5: none (cut by both edges)

The list lengths and the largest n_contrib are asserted twice: on the CPU with the float32 oracle alone (no device), and about the
device's own frame before any comparison.  The expected values and the comparisons are the four files' own (imported, not copied):
bitwise for the pick and the feature pass and for the contribution pass's counts and maximum, their files' documented bounds for the
two results that atomics sum in any order (weight_sum, dvalues)."""
import contextlib
import functools
import importlib
from unittest import mock

import numpy as np
import pytest
import torch

import test_gpu_contrib as contrib
import test_gpu_features as feat
import test_gpu_features_bwd as fbwd
import test_gpu_pick as pick
from conftest import set_knob
from oracle.raster_oracle import RasterOracle
from scenes import raster_scene
from test_gpu_pick import TILE, bits
from test_gpu_playback import _dev

fdgs = importlib.import_module("4dgaussians_amd")
P, syn = fdgs.playback, fdgs.synthetic
W, H = 40, 24
# (tile, entries), and the pixel the tile's splats lie around: the centre of a whole tile; in the partial column and row a pixel that is
# inside the image and more than a splat's radius (4 pixels) plus the jitter away from the neighbouring tile
STACKS = ((0, 600), (1, 256), (2, 257), (3, 300), (4, 5), (5, 0))
CENTRES = {0: (8.0, 8.0), 1: (24.0, 8.0), 2: (38.0, 8.0), 3: (8.0, 21.0), 4: (24.0, 21.0), 5: (38.0, 21.0)}
LENGTHS = [n for _, n in STACKS]
N = sum(LENGTHS)
SIGMA_PIX, JITTER, OPACITY = 0.8, 0.4, 0.008


def _walk_scene(n=N, width=W, height=H, seed=0, scale_boost=1.0):
    """raster_scene's dict (its camera, its SH rows) with the Gaussians of STACKS: centres unprojected from pixels next to their tile's
    centre, each at a view depth of its own (shuffled over the indices: the lists really get sorted), one scale in pixels for all."""
    assert (n, width, height) == (N, W, H)
    sc = raster_scene(n, width, height, seed=seed, scale_boost=scale_boost)
    cam = syn.make_camera(width, height, theta_deg=30.0, time=0.0)
    assert np.array_equal(np.asarray(cam.world_view_transform, np.float32), sc["viewmatrix"])
    rng = np.random.default_rng(seed)
    xy = np.concatenate([np.asarray(CENTRES[t], np.float32) + rng.uniform(-JITTER, JITTER, (k, 2)).astype(np.float32) for t, k in STACKS])
    z = (4.0 + 0.001 * np.arange(n)).astype(np.float32)
    rng.shuffle(z)
    sc["means3D"] = np.ascontiguousarray(P.unproject(cam, torch.from_numpy(xy), torch.from_numpy(z)).numpy().astype(np.float32))
    focal = width / (2.0 * sc["tanfovx"])
    sc["scales"] = np.ascontiguousarray(np.repeat((SIGMA_PIX * z / focal).astype(np.float32)[:, None], 3, 1))
    sc["rotations"] = np.ascontiguousarray(np.tile(np.asarray([1.0, 0.0, 0.0, 0.0], np.float32), (n, 1)))
    sc["opacities"] = np.full((n, 1), OPACITY, np.float32)
    return sc


def _assert_edges(lengths, n_contrib, what):
    """The list lengths are STACKS' and the centre pixels walk their whole lists: three rounds in tile 0, exactly one in tile 1, a second
    round of one entry in tile 2."""
    assert list(lengths) == LENGTHS, (what, list(lengths))
    pad = np.zeros((2 * TILE, 3 * TILE), np.int64)
    pad[:H, :W] = n_contrib
    walk = pad.reshape(2, TILE, 3, TILE).max(axis=(1, 3)).reshape(-1)
    print(f"{what}: list lengths {list(lengths)}, largest n_contrib per tile {walk.tolist()}")
    assert int(n_contrib.max()) > 512 and walk[0] > 512, (what, walk)
    assert walk[1] == 256 and walk[2] == 257, (what, walk)
    assert 256 < walk[3] <= 300 and 0 < walk[4] <= 5 and walk[5] == 0, (what, walk)
    assert W % TILE and H % TILE
    return walk


def test_the_scene_reaches_every_edge_on_the_cpu_oracle():
    sc = _walk_scene()
    o = RasterOracle(**{k: sc[k] for k in ("means3D", "opacities", "viewmatrix", "projmatrix", "campos", "bg", "image_height", "image_width",
                                           "tanfovx", "tanfovy", "sh_degree", "shs", "scales", "rotations")})
    try:
        tiles, gid = o.pairs()
        _, nc = o.image_state()
        assert int((o.radii > 0).sum()) == N
        assert np.array_equal(np.sort(gid), np.arange(N))       # every Gaussian is in exactly one list
        _assert_edges(np.bincount(tiles, minlength=6), nc.astype(np.int64), "oracle")
    finally:
        o.close()


@contextlib.contextmanager
def _as_pick_scene(fr=None):
    """test_gpu_pick's frame builders take a scene by its name in SCENES and build it with raster_scene: inside this block the name "walk"
    is this file's scene (and, given `fr`, _frame returns it), so that _forward, _frame and _expected run as they are."""
    with mock.patch.dict(pick.SCENES, {"walk": (N, W, H, 0, 1.0, 1.0)}), mock.patch.object(pick, "raster_scene", _walk_scene):
        if fr is None:
            yield
        else:
            with mock.patch.object(pick, "_frame", lambda name: fr):
                yield


@functools.lru_cache(maxsize=None)
def _frame():
    """The device's frame of the scene with its per-Gaussian w maps (test_gpu_pick._frame, uncached there): computed once, never modified."""
    with _as_pick_scene():
        fr = pick._frame.__wrapped__("walk")
    walk = _assert_edges(fr.ranges[:, 1] - fr.ranges[:, 0], fr.n_contrib, "device")
    assert np.array_equal(fr.walk, walk)
    return fr


@functools.lru_cache(maxsize=None)
def _pick_expected(cut):
    fr = _frame()
    with _as_pick_scene(fr):
        return pick._expected.__wrapped__("walk", cut)


@functools.lru_cache(maxsize=None)
def _feature_reference():
    fr = _frame()
    vals = torch.from_numpy(np.random.default_rng(5).standard_normal((fr.n, 17)).astype(np.float32)).to(_dev())
    return vals, feat._oracle(fr, vals), feat._oracle(fr, torch.ones(fr.n, 1, device=_dev()))[0]


@functools.lru_cache(maxsize=None)
def _gradient_reference():
    fr = _frame()
    g = np.random.default_rng(17).standard_normal((17, fr.h, fr.w)).astype(np.float32)
    return (g, (fr.wmaps > 0).reshape(fr.n, -1).sum(1)) + fbwd._oracle(fr, g)


ORDER = pytest.mark.parametrize("tile_order", [1, 0], ids=["tile_order_on", "tile_order_off"])


@pytest.mark.gpu
@ORDER
def test_pick_over_lists_of_256_and_257_entries(tile_order):
    fr = _frame()
    set_knob("tile_order", tile_order)
    for cut in (0.5, 1.0):
        want = _pick_expected(cut)
        pick._assert_matches(pick._pick(fr, cut), want, ("walk", cut, tile_order))
    assert (want[0] >= 0).any() and (want[0] == -1).any()


@pytest.mark.gpu
@ORDER
def test_features_over_lists_of_256_and_257_entries(tile_order):
    fr = _frame()
    vals, want, ones = _feature_reference()
    set_knob("tile_order", tile_order)
    for c in (3, 17):                                            # a partial chunk; a full one and a second
        got, alpha = feat._run(fr, vals[:, :c])
        assert np.array_equal(bits(got), bits(want[:c])), (c, tile_order)
        assert np.array_equal(bits(alpha), bits(ones)), (c, tile_order)


@pytest.mark.gpu
@ORDER
def test_features_bwd_over_lists_of_256_and_257_entries(tile_order):
    fr = _frame()
    g, pixels, want, absum = _gradient_reference()
    set_knob("tile_order", tile_order)
    for c in (3, 17):
        got = fbwd._bwd(fr.state, g[:c], fr.n)
        fbwd._assert_within(got, want[:, :c], absum[:, :c], pixels, ("walk", c, tile_order))
    assert int((pixels > 0).sum()) > 1000                        # (nearly every entry of every list is blended somewhere)


@pytest.mark.gpu
@ORDER
def test_contrib_over_lists_of_256_and_257_entries(tile_order):
    fr = _frame()
    want = contrib._expected(fr)
    set_knob("tile_order", tile_order)
    contrib._assert_matches(contrib._contrib(fr), want, ("walk", tile_order))
    last = {t: int(fr.gid[fr.ranges[t, 1] - 1]) for t in (1, 2)}  # the last entry of the 256-list and the lone entry of a second round
    assert want["pixels"][last[1]] > 0 and want["pixels"][last[2]] > 0
