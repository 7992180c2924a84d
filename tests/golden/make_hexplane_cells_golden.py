"""Generates tests/golden/hexplane_cells.npz: HexPlane texel cells and weights of float32 coordinates on and around every texel
boundary, computed with torch float32 elementwise ops (the REFERENCE's normalize_aabb, then grid_sample's un-normalisation) and
validated entry by entry against ATen's own grid_sample kernel before anything is written.  Run in the build container only (it imports
scene/hexplane.py from the reference checkout):
    python tests/golden/make_hexplane_cells_golden.py

Every entry is one-dimensional: (xbits, axis, aabb_id, aabb0, aabb1, size) -> (i0, i1, w1bits, dscale).  axis 0..2 = x, y, z (normalised by the
aabb), axis 3 = time (never normalised: xbits is the grid coordinate itself, aabb0 = aabb1 = 0).
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import deform_oracle as DO  # noqa: E402
import hexplane_fixture as HF  # noqa: E402

SPATIAL_SIZES, TIME_SIZES, ULPS, N_RANDOM = (64, 128, 256), (75, 150), 8, 20000


def neighbours(x32, ulps=ULPS):
    """x and its `ulps` float32 neighbours on each side: [len(x) * (2 * ulps + 1)]"""
    out = [x32]
    lo, hi = x32.copy(), x32.copy()
    for _ in range(ulps):
        lo = np.nextafter(lo, np.float32(-np.inf)).astype(np.float32)
        hi = np.nextafter(hi, np.float32(np.inf)).astype(np.float32)
        out += [lo.copy(), hi.copy()]
    return np.concatenate(out)


def entries():
    rng = np.random.default_rng(20240)
    x, axis, aid, size = [], [], [], []

    def add(xs, a, i, s):
        xs = np.asarray(xs, np.float32).ravel()
        x.append(xs); axis.append(np.full(len(xs), a, np.int8)); aid.append(np.full(len(xs), i, np.int8)); size.append(np.full(len(xs), s, np.int16))

    for i, (amax, amin) in enumerate(HF.AABBS):
        for a in range(3):
            a0, a1 = np.float32(amax[a]), np.float32(amin[a])
            span = float(a1) - float(a0)
            for s in SPATIAL_SIZES:
                k = np.arange(s, dtype=np.float64)
                add(neighbours((float(a0) + span * k / (s - 1)).astype(np.float32)), a, i, s)          # every boundary, +-8 ulps
                # beyond texel 0 and texel size-1 from outside the box (border clamp, dscale = 0)
                beyond = np.array([1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 0.1, 0.5, 2.0]) * abs(span)
                add(np.concatenate([float(a0) - np.sign(span) * beyond, float(a1) + np.sign(span) * beyond]), a, i, s)
                add([a0, a1], a, i, s)                                                                    # both corner values exactly
    for s in TIME_SIZES:
        k = np.arange(s, dtype=np.float64)
        add(neighbours((2.0 * k / (s - 1) - 1.0).astype(np.float32)), 3, 0, s)
        add([-1.0000001, -1.001, -1.5, -3.0, 1.0000001, 1.001, 1.2, 1.5, 3.0, 0.0, 0.5], 3, 0, s)
    # seeded uniform coordinates, a little beyond the box / beyond [-1, 1]; a quarter of them are times
    ra, ri, u = rng.integers(0, 4, N_RANDOM), rng.integers(0, 2, N_RANDOM), rng.random(N_RANDOM)
    for a in range(4):
        sizes = TIME_SIZES if a == 3 else SPATIAL_SIZES
        for i in range(1 if a == 3 else 2):
            m = np.nonzero((ra == a) & ((ri == i) | (a == 3)))[0]
            rs = rng.integers(0, len(sizes), len(m))
            if a == 3:
                vals = 2.1 * u[m] - 1.05
            else:
                amax, amin = HF.AABBS[i]
                vals = 1.05 * (amin[a] + (amax[a] - amin[a]) * u[m])
            for j, s in enumerate(sizes):
                add(vals[rs == j], a, i, s)
    x, axis, aid, size = (np.concatenate(v) for v in (x, axis, aid, size))
    a0 = np.zeros(len(x), np.float32)
    a1 = np.zeros(len(x), np.float32)
    for i, (amax, amin) in enumerate(HF.AABBS):
        for a in range(3):
            m = (axis == a) & (aid == i)
            a0[m], a1[m] = amax[a], amin[a]
    return x, axis, aid, size, a0, a1


def expected(x, axis, size, a0, a1, normalize_aabb):
    """torch float32 elementwise: normalize_aabb (reference), ((q + 1) / 2) * (size - 1), clip, floor"""
    xt, sp = torch.from_numpy(x), torch.from_numpy(axis < 3)
    a0t, a1t = torch.from_numpy(a0), torch.from_numpy(a1)
    a1safe = torch.where(sp, a1t, torch.ones_like(a1t))         # (time entries: any non-degenerate box; their q is the time itself)
    q = torch.where(sp, normalize_aabb(xt, (a0t, a1safe)), xt)
    assert q.dtype == torch.float32
    hi = torch.from_numpy(size.astype(np.float32)) - 1.0
    p = ((q + 1.0) / 2.0) * hi
    inside = (p > 0) & (p < hi)
    dscale = torch.where(inside, 0.5 * hi, torch.zeros_like(hi))
    pc = torch.minimum(torch.maximum(p, torch.zeros_like(p)), hi)
    f = torch.floor(pc)
    i0 = f.to(torch.int64)
    i1 = torch.minimum(i0 + 1, torch.from_numpy(size.astype(np.int64)) - 1)
    w1 = pc - f
    w0 = 1.0 - w1
    return q, i0, i1, w0, w1, dscale


def validate_against_grid_sample(q, size, i0, i1, w0, w1, sampler, chunk=4096):
    """d(sum of samples) / d(planes) of a batch of [1, 1, size] planes, one per coordinate (the other grid coordinate fixed at -1: row 0 of
    a one-row plane, weight exactly 1): row r must be w0 at i0, w1 at i1 (their sum where i1 == i0) and zero elsewhere, bit for bit."""
    checked = 0
    for s in np.unique(size):
        idx = np.nonzero(size == s)[0]
        for c0 in range(0, len(idx), chunk):
            ix = torch.from_numpy(idx[c0:c0 + chunk])
            n = len(ix)
            planes = torch.zeros(n, 1, 1, int(s), requires_grad=True)
            coords = torch.stack([q[ix], torch.full((n,), -1.0)], dim=-1).reshape(n, 1, 2)
            out = sampler(planes, coords)
            g, = torch.autograd.grad(out.sum(), planes)
            g = g.reshape(n, int(s))
            want = torch.zeros(n, int(s))
            r = torch.arange(n)
            same = i0[ix] == i1[ix]
            want[r, i0[ix]] = torch.where(same, w0[ix] + w1[ix], w0[ix])
            want[r[~same], i1[ix][~same]] = w1[ix][~same]
            bad = (g.view(torch.int32) != want.view(torch.int32)) & ~((g == 0) & (want == 0))
            if bool(bad.any()):
                rr = int(torch.nonzero(bad.any(dim=1))[0])
                raise SystemExit(f"grid_sample disagrees at entry {int(ix[rr])} (size {s}): got {g[rr].nonzero().ravel().tolist()} "
                                 f"{g[rr][g[rr] != 0].tolist()}, expected i0 {int(i0[ix][rr])} i1 {int(i1[ix][rr])} w0 {float(w0[ix][rr])!r} w1 {float(w1[ix][rr])!r}")
            checked += n
    return checked


def reference_sampler():
    try:
        DO.import_reference_deform_network()
        from scene.hexplane import grid_sample_wrapper, normalize_aabb
        return (lambda planes, coords: grid_sample_wrapper(planes, coords)), normalize_aabb
    except Exception as e:      # noqa: BLE001
        raise SystemExit(f"the reference's scene/hexplane.py is needed for normalize_aabb: {e}")


def fallback_sampler(planes, coords):
    return F.grid_sample(planes, coords.view(coords.shape[0], 1, -1, 2), align_corners=True, mode="bilinear", padding_mode="border")


def main():
    sampler, normalize_aabb = reference_sampler()
    x, axis, aid, size, a0, a1 = entries()
    q, i0, i1, w0, w1, dscale = expected(x, axis, size, a0, a1, normalize_aabb)
    try:
        checked = validate_against_grid_sample(q, size, i0, i1, w0, w1, sampler)
    except (RuntimeError, TypeError):
        checked = validate_against_grid_sample(q, size, i0, i1, w0, w1, fallback_sampler)
    assert checked == len(x)
    fx = dict(xbits=x.view(np.uint32), axis=axis, aabb_id=aid, aabb0=a0, aabb1=a1, size=size, i0=i0.numpy().astype(np.int16),
              i1=i1.numpy().astype(np.int16), w1bits=w1.numpy().view(np.uint32), dscale=dscale.numpy(), qbits=q.numpy().view(np.uint32))
    view = dict(fx, x=x, w1=w1.numpy())
    flips = int((HF.fused_i0(view) != i0.numpy()).sum())
    zero_w = int((w1.numpy() == 0).sum())
    clamped = int((dscale.numpy() == 0).sum())
    print(f"{len(x)} entries, all validated against grid_sample; fused-normalisation flips {flips}, exact-zero w1 {zero_w}, clamped {clamped}")
    assert flips >= 100 and zero_w >= 50 and clamped >= 50
    path = os.path.join(HERE, "hexplane_cells.npz")
    np.savez_compressed(path, **fx)
    print(f"{path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
