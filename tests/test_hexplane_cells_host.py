"""CPU tests of the HexPlane index arithmetic (csrc/hexplane_ops.h) through its host twin fdgs_hexplane_cells_host: bit equality with the
fixture tests/golden/hexplane_cells.npz (torch float32 elementwise ops, validated against F.grid_sample when it was generated), the same
validation repeated live where the reference checkout is present, and agreement with the float32 path of the pinned CPU oracle."""
import importlib
import os

import numpy as np
import pytest
import torch

import hexplane_fixture as HF
from oracle import deform_oracle as DO


@pytest.fixture(scope="module")
def fx():
    _lib = importlib.import_module("4dgaussians_amd._lib")
    if not os.path.exists(_lib.LIB_PATH):
        importlib.import_module("4dgaussians_amd.build").build()
    return HF.load()


def test_fixture_is_one_that_can_fail(fx):
    """What the generator asserted when it wrote the file: the fused normalisation (one rounding instead of two) picks another cell on at
    least 100 entries, at least 50 weights are exactly zero and at least 50 entries clamp."""
    assert len(fx["x"]) > 60000
    assert int((HF.fused_i0(fx) != fx["i0"]).sum()) >= 100
    assert int((fx["w1"] == 0).sum()) >= 50 and int((fx["dscale"] == 0).sum()) >= 50


@pytest.mark.parametrize("time_size", [150, 75])
def test_host_twin_equals_fixture_bit_for_bit(fx, time_size):
    """Every entry, zipped into xyz / time rows with L = 3 levels (res = 64 * {1, 2, 4}): cells, w1, dscale and q of the twin equal the
    fixture bit for bit.  Nothing is left out: every spatial entry and every time entry of this time resolution is placed and compared."""
    seen = np.zeros(len(fx["x"]), bool)
    for aabb_id, aabb in enumerate(HF.AABBS):
        xyz, t, ent = HF.zip_rows(fx, aabb_id, time_size)
        cells, w1, ds, q = HF.cells_host(xyz, t, aabb, time_size)
        r, l, a, e = HF.entry_view(fx, ent)
        assert np.array_equal(cells[r, l, a, 0], fx["i0"][e].astype(np.int32))
        assert np.array_equal(cells[r, l, a, 1], fx["i1"][e].astype(np.int32))
        assert np.array_equal(w1[r, l, a].view(np.uint32), fx["w1bits"][e])
        assert np.array_equal(ds[r, l, a].view(np.uint32), fx["dscale"][e].view(np.uint32))
        assert np.array_equal(q[r, a].view(np.uint32), fx["qbits"][e])
        seen[e] = True
    want = (fx["axis"] < 3) | (fx["size"] == time_size)
    assert np.array_equal(seen, want)


def test_scalar_time_and_per_gaussian_time_agree(fx):
    xyz, t, _ = HF.zip_rows(fx, 0, 150)
    xyz, t = xyz[:257], t[:257]
    per = HF.cells_host(xyz, np.full(257, t[5], np.float32), HF.AABBS[0], 150)
    one = HF.cells_host(xyz, float(t[5]), HF.AABBS[0], 150)
    for a, b in zip(per, one):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_fixture_against_grid_sample_live(fx):
    """The generator's validation, repeated: d(sum of samples) / d(planes) of the reference's grid_sample_wrapper on one-row planes is w0 at i0,
    w1 at i1 and zero elsewhere, bit for bit, for every entry (needs the reference checkout)."""
    if not os.path.isdir("/root/reference/scene"):
        pytest.skip("the reference checkout is not present")
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    gen = importlib.import_module("make_hexplane_cells_golden")
    sampler, normalize_aabb = gen.reference_sampler()
    q, i0, i1, w0, w1, dscale = gen.expected(fx["x"], fx["axis"], fx["size"], fx["aabb0"], fx["aabb1"], normalize_aabb)
    assert np.array_equal(i0.numpy(), fx["i0"]) and np.array_equal(i1.numpy(), fx["i1"])
    assert np.array_equal(w1.numpy().view(np.uint32), fx["w1bits"]) and np.array_equal(dscale.numpy(), fx["dscale"])
    assert np.array_equal(q.numpy().view(np.uint32), fx["qbits"])
    assert gen.validate_against_grid_sample(q, fx["size"], i0, i1, w0, w1, sampler) == len(fx["x"])


def test_host_twin_and_pinned_oracle_are_the_same_function(fx):
    """oracle/deform_oracle.py::_bilinear_border in float32 on the fixture's coordinates: d(sample) / d(plane) of a ones-upstream lookup is the
    oracle's (cell, weight) pair per axis; it equals what the twin reports (the other axis sits on texel 0 with weight exactly 1)."""
    for aabb_id, aabb in enumerate(HF.AABBS):
        xyz, t, ent = HF.zip_rows(fx, aabb_id, 150)
        cells, w1, ds, q = HF.cells_host(xyz, t, aabb, 150)
        r, l, a, e = HF.entry_view(fx, ent)
        n = len(r)
        for s in np.unique(fx["size"][e]):
            m = np.nonzero(fx["size"][e] == s)[0]
            for c0 in range(0, len(m), 8192):
                mm = m[c0:c0 + 8192]
                qq = torch.from_numpy(q[r[mm], a[mm]].copy())
                # one [1, k, 1, size] plane whose channel c is private to coordinate c: the gradient row of channel c is that coordinate's weights
                k = len(mm)
                plane = torch.zeros(1, k, 1, int(s), requires_grad=True)
                v = DO._bilinear_border(plane, qq, torch.full((k,), -1.0))
                g, = torch.autograd.grad(v.diagonal().sum(), plane)
                g = g[0, :, 0, :]
                want = torch.zeros(k, int(s))
                i0 = torch.from_numpy(cells[r[mm], l[mm], a[mm], 0].astype(np.int64))
                i1 = torch.from_numpy(cells[r[mm], l[mm], a[mm], 1].astype(np.int64))
                ww1 = torch.from_numpy(w1[r[mm], l[mm], a[mm]].copy())
                rows = torch.arange(k)
                want[rows, i0] = 1.0 - ww1
                want[rows, i1] += ww1          # (i1 == i0 on the last texel: the sum)
                assert torch.equal(g, want), (aabb_id, int(s))
        assert n > 20000
