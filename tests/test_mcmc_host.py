"""CPU: the host twins of MCMC densification (fdgs_mcmc_*_host: the inline functions of csrc/mcmc_ops.h over host arrays) against numpy /
float64 restatements of the definitions in include/fdgs.h (tests/mcmc_common.py).  Integer parts (Philox, weights -> scan -> draw) must
agree exactly; the relocation values and the noise step are held to bounds derived from float32 rounding, with the worst ratio printed."""
import math

import numpy as np
import pytest

import mcmc_common as MC

MIN_OP = 0.005


@pytest.fixture(scope="module")
def L():
    return MC.lib()


def test_philox_words_equal_the_numpy_restatement(L):
    g = np.random.default_rng(1)
    ctr = g.integers(0, 2 ** 32, (1000, 4), dtype=np.uint64).astype(np.uint32)
    ctr[:8] = [[0, 0, 0, 0], [1, 0, 0, 0], [0xFFFFFFFF] * 4, [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [2, 3, 0, 0], [0xFFFFFFFF, 0, 0, 0]]
    for k0, k1 in ((0, 0), (0xFFFFFFFF, 0xFFFFFFFF), (0xA4093822, 0x299F31D0), (7, MC.TAGS["noise"])):
        out = np.zeros((1000, 4), np.uint32)
        MC.ok(L.fdgs_mcmc_philox_host(1000, MC.p(ctr), k0, k1, MC.p(out)))
        assert np.array_equal(out, MC.philox(ctr, k0, k1))
    # the known-answer vectors of the generator's authors (Random123, kat_vectors: philox4x32 10)
    kat = np.zeros((3, 4), np.uint32)
    MC.ok(L.fdgs_mcmc_philox_host(1, MC.p(np.zeros((1, 4), np.uint32)), 0, 0, MC.p(kat[0:1])))
    MC.ok(L.fdgs_mcmc_philox_host(1, MC.p(np.full((1, 4), 0xFFFFFFFF, np.uint32)), 0xFFFFFFFF, 0xFFFFFFFF, MC.p(kat[1:2])))
    MC.ok(L.fdgs_mcmc_philox_host(1, MC.p(np.array([[0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344]], np.uint32)), 0xA4093822, 0x299F31D0, MC.p(kat[2:3])))
    assert kat.tolist() == [[0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8], [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD],
                            [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]]


def _twin_sample(L, scan, n, seed, tag):
    src = np.zeros(n, np.int32)
    cnt = np.zeros(scan.shape[0], np.uint32)
    MC.ok(L.fdgs_mcmc_sample_host(scan.shape[0], MC.p(scan), n, seed, tag, MC.p(src), MC.p(cnt)))
    return src, cnt


def test_weights_and_scan(L):
    x = np.concatenate([np.random.default_rng(2).uniform(-12, 18, 4000), [-200.0, -5.2933, -5.2932, 0.0, 17.0, 30.0, 200.0, np.nan]]).astype(np.float32)
    w, scan = np.zeros(x.shape[0], np.uint32), np.zeros(x.shape[0], np.uint64)
    MC.ok(L.fdgs_mcmc_weights_host(x.shape[0], MC.p(x), MIN_OP, MC.p(w), MC.p(scan)))
    with np.errstate(over="ignore", invalid="ignore"):
        o32 = MC.sigmoid32(x)
    dead = ~(o32 > np.float32(MIN_OP))
    safe = np.abs(o32 - np.float32(MIN_OP)) > 1e-6                   # (an opacity within rounding of the threshold may fall either way)
    assert np.array_equal((w == 0)[safe], dead[safe]) and dead[-1] and w[-1] == 0          # the NaN row is dead
    live = (w != 0) & ~np.isnan(x)
    want = np.clip(MC.weights64(x[live]), 1, 2 ** 32 - 1)
    assert np.abs(w[live].astype(np.float64) - want).max() <= 2 ** 9
    assert w[-2] == 2 ** 32 - 1 and w[-3] == 2 ** 32 - 1             # sigmoid = 1.0f: clamped below 2^32
    assert np.array_equal(scan, np.cumsum(w.astype(np.uint64), dtype=np.uint64))


def test_sources_equal_the_numpy_restatement(L):
    g = np.random.default_rng(3)
    for N, n, seed in ((1, 5, 1), (2, 64, 2), (257, 300, 3), (5000, 4097, 4)):
        w = g.integers(1, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)
        w[g.random(N) < 0.3] = 0
        w[N // 2] = 0xFFFFFFFF
        scan = np.cumsum(w.astype(np.uint64), dtype=np.uint64)
        for tag in (MC.TAGS["relocate"], MC.TAGS["grow"]):
            src, cnt = _twin_sample(L, scan, n, seed, tag)
            ref, ref_cnt = MC.sample(w, n, seed, tag)
            assert np.array_equal(src, ref) and np.array_equal(cnt, ref_cnt)
            assert (w[src] != 0).all()
    a, _ = _twin_sample(L, scan, 4097, 4, MC.TAGS["relocate"])
    b, _ = _twin_sample(L, scan, 4097, 4, MC.TAGS["grow"])
    c, _ = _twin_sample(L, scan, 4097, 5, MC.TAGS["relocate"])
    assert not np.array_equal(a, b) and not np.array_equal(a, c)     # the tag and the seed both key the draws


def test_frequencies_zero_weights_and_single_live_row(L):
    w = np.array([1, 2 ** 31, 0, 3 * 2 ** 28, 2 ** 32 - 1, 2 ** 20, 0, 2 ** 30, 5 * 2 ** 27, 2 ** 29, 2 ** 31 + 12345, 7 * 2 ** 26, 2 ** 25, 0, 2 ** 30 + 1,
                  2 ** 28], np.uint32)
    scan = np.cumsum(w.astype(np.uint64), dtype=np.uint64)
    n = 200_000
    src, cnt = _twin_sample(L, scan, n, 12345, MC.TAGS["relocate"])
    prob = w.astype(np.float64) / float(scan[-1])
    sd = np.sqrt(n * prob * (1 - prob))
    dev = np.abs(cnt - n * prob)
    print("sampling: worst deviation / standard deviation =", float((dev[sd > 0] / sd[sd > 0]).max()))
    assert (dev <= 5 * sd).all()                       # (zero-weight rows: sd = 0, count 0; the weight-1 row: n p = 1e-5, count 0)
    assert cnt[w == 0].sum() == 0 and int(cnt.sum()) == n
    one = np.zeros(100, np.uint32)
    one[37] = 1
    src, cnt = _twin_sample(L, np.cumsum(one.astype(np.uint64), dtype=np.uint64), 1000, 9, MC.TAGS["grow"])
    assert (src == 37).all() and cnt[37] == 1000


GRID_O = [0.006, 0.1, 0.5, 0.9, 0.999, None]          # None: sigmoid(20)
GRID_R = [1, 2, 3, 10, 51]
GRID_S = [1e-4, 1e-3, 0.03, 0.7, 10.0]


def _relocation_grid():
    xo, xs, cnt = [], [], []
    for o in GRID_O:
        x = 20.0 if o is None else math.log(o / (1 - o))
        for r in GRID_R:
            for k in range(len(GRID_S)):
                xo.append(x)
                xs.append([math.log(GRID_S[k]), math.log(GRID_S[(k + 1) % len(GRID_S)]), math.log(GRID_S[(k + 2) % len(GRID_S)])])
                cnt.append(r - 1)
    return np.array(xo, np.float32), np.array(xs, np.float32), np.array(cnt, np.uint32)


def _twin_relocation(L, xo, xs, cnt, min_op=MIN_OP):
    o_out, s_out = np.zeros_like(xo), np.zeros_like(xs)
    MC.ok(L.fdgs_mcmc_relocation_host(xo.shape[0], MC.p(xo), MC.p(xs), MC.p(cnt), min_op, MC.p(o_out), MC.p(s_out)))
    return o_out, s_out


def test_relocation_values_against_float64(L):
    """|sigmoid(x_o') - o'| <= o' (|x_o'| + 2) 2^-23 and |exp(x_s') - s'| <= s' (|x_s'| + 2) 2^-23: one float32 rounding of a double result
    (half a unit of x: at most |x| 2^-24), seen through the inverse activation (d o = o (1 - o) d x, d s = s d x), with a margin of two
    units for the double chain and the activations of the comparison.  Where the lower clamp acts x_o' is rounded up by up to 1.75 units on
    purpose (csrc/mcmc_ops.h); near logit(0.005) = -5.29 a unit is 2^-21, so that may use 7 of the bound's 7.29 x 2^-23.
    Measured worst ratios to the bound: opacity 0.46 (a row at the lower clamp; 0.14 elsewhere), scale 0.34."""
    xo, xs, cnt = _relocation_grid()
    o_out, s_out = _twin_relocation(L, xo, xs, cnt)
    worst_o = worst_o_unclamped = worst_s = 0.0
    for i in range(xo.shape[0]):
        o_new, s_new, o_raw = MC.relocation64(xo[i], xs[i], cnt[i], MIN_OP)
        got_o, got_s = float(MC.sigmoid64(o_out[i])), np.exp(s_out[i].astype(np.float64))
        ro = abs(got_o - o_new) / (o_new * (abs(float(o_out[i])) + 2) * 2.0 ** -23)
        rs = float((np.abs(got_s - s_new) / (s_new * (np.abs(s_out[i].astype(np.float64)) + 2) * 2.0 ** -23)).max())
        worst_o, worst_s = max(worst_o, ro), max(worst_s, rs)
        if o_raw >= MIN_OP:
            worst_o_unclamped = max(worst_o_unclamped, ro)
        assert ro <= 1.0, (i, xo[i], cnt[i], got_o, o_new, ro)
        assert rs <= 1.0, (i, xo[i], cnt[i], got_s, s_new, rs)
        assert got_o >= float(np.float32(MIN_OP))                                    # o' never below min_opacity ...
        assert float(MC.sigmoid32(o_out[i:i + 1])[0]) > np.float32(MIN_OP)           # ... and not dead by the float32 test either
    print(f"relocation values: worst ratio to the bound: opacity {worst_o:.3f} (rows the lower clamp leaves alone: {worst_o_unclamped:.3f}), scale {worst_s:.3f}")


def test_relocation_identity_and_ratio_clamp(L):
    xo, xs, cnt = _relocation_grid()
    one = cnt == 0
    o_out, s_out = _twin_relocation(L, xo[one], xs[one], cnt[one])
    inside = xo[one] < 15.9                       # (sigmoid(20) lies above the upper clamp 1 - 2^-23 = sigmoid(15.94): its opacity is clamped)
    assert inside.sum() == 25 and np.array_equal(o_out[inside], xo[one][inside]) and np.array_equal(s_out, xs[one])   # r = 1: the identity, bit for bit
    assert np.allclose(o_out[~inside], math.log((1 - 2.0 ** -23) / 2.0 ** -23), rtol=1e-6)
    x1, s1 = np.full(5, 1.5, np.float32), np.tile(np.array([[-3.0, -2.0, -1.0]], np.float32), (5, 1))
    o_out, s_out = _twin_relocation(L, x1, s1, np.array([49, 50, 51, 79, 2 ** 32 - 1], np.uint32))
    assert (o_out[1:] == o_out[1]).all() and (s_out[1:] == s_out[1]).all()           # counts above 50: ratio 51
    assert o_out[0] != o_out[1]
    # a barely live source drawn often: o' = 0.006 / 11 would be dead -- clamped, and the clamp holds for other thresholds too
    for min_op in (0.005, 0.02, 0.001):
        x = np.array([math.log(1.2 * min_op / (1 - 1.2 * min_op))] * 3, np.float32)
        o_out, _ = _twin_relocation(L, x, s1[:3], np.array([1, 10, 200], np.uint32), min_op)
        assert (MC.sigmoid64(o_out) >= float(np.float32(min_op))).all() and (MC.sigmoid32(o_out) > np.float32(min_op)).all()
        assert (MC.sigmoid64(o_out) <= float(np.float32(min_op)) * (1 + 4e-6)).all()
    # the upper clamp: x_o = 40 is o = 1 to float32; r = 1 keeps x_o' finite at logit(1 - 2^-23)
    o_out, _ = _twin_relocation(L, np.array([40.0], np.float32), s1[:1], np.array([0], np.uint32))
    assert abs(float(o_out[0]) - math.log((1 - 2.0 ** -23) / 2.0 ** -23)) < 1e-5


def test_the_formula_preserves_the_central_alpha_and_the_covered_area():
    """The method's invariant, on the float64 restatement: r Gaussians (o', s') stacked at one place blend to the central alpha of the one
    (o, s) they replace -- 1 - (1 - o')^r = o within 1e-9 -- and (what fixes s') to the same integral of the blended alpha along a line
    through the centre, int 1 - (1 - o' exp(-x^2 / 2 s'^2))^r dx = o s sqrt(2 pi).  This pins the formula itself."""
    for o in (0.006, 0.1, 0.5, 0.9, 0.999):
        for r in (2, 3, 10, 51):
            x_o, x_s = np.float32(math.log(o / (1 - o))), np.array([math.log(0.03)] * 3, np.float32)
            o_new, s_new, o_raw = MC.relocation64(x_o, x_s, r - 1, 0.0)
            o64 = float(MC.sigmoid64(x_o))
            assert abs((1 - (1 - o_raw) ** r) - o64) <= 1e-9
            s = float(np.exp(np.float64(x_s[0])))
            xs = np.linspace(-12 * s, 12 * s, 200001)
            blended = 1 - (1 - o_raw * np.exp(-xs ** 2 / (2 * s_new[0] ** 2))) ** r
            area = float(np.sum(blended[:-1] + blended[1:]) * 0.5 * (xs[1] - xs[0]))          # trapezoid: exponentially convergent here
            assert abs(area - o64 * s * math.sqrt(2 * math.pi)) <= 1e-9 * s, (o, r, area, o64 * s * math.sqrt(2 * math.pi))


def _noise_inputs(n, seed):
    rows, _ = MC.random_rows(n, seed, dead_frac=0.5)
    rows["opacity"][:n // 2] = np.random.default_rng(seed).uniform(-7.0, -3.5, (n // 2, 1)).astype(np.float32)   # around the gate: g from ~1 to ~0.1
    xi = np.random.default_rng(seed + 1).normal(0, 1, (n, 3)).astype(np.float32)
    return rows, xi


def test_noise_twin_against_float64(L):
    """Per component |dx - dx64| <= 64 * 2^-23 * (sum_j |M_ij| |xi_j|) g lr + 2^-23 |xyz_i|: the first term allows about thirty float32
    operations of quaternion normalisation, rotation, products and the gate, the second the final add.  Scales spread over e^4 per Gaussian.
    A float32 evaluation of the step MISSES this bound on such rows (measured over ten seeds: worst ratios 0.6 .. 3.1 -- the entries of a
    float32 rotation matrix carry an absolute error of 2^-24, which the largest s^2 multiplies, while the bound is relative to |M_ij|); the
    step is therefore evaluated in double and rounded by the final add.  Measured worst ratio: 0.48 (the add's half unit)."""
    n, lr = 4000, 5e5 * 1.6e-4
    rows, xi = _noise_inputs(n, 5)
    xyz = rows["xyz"].copy()
    MC.ok(L.fdgs_mcmc_noise_host(n, MC.p(xyz), MC.p(rows["scaling"]), MC.p(rows["rotation"]), MC.p(rows["opacity"]), lr, 100.0, MIN_OP, 0, 0, MC.p(xi)))
    dx64, bound = MC.noise64(rows["xyz"], rows["scaling"], rows["rotation"], rows["opacity"], xi, lr, 100.0, MIN_OP)
    dx = xyz.astype(np.float64) - rows["xyz"].astype(np.float64)
    ratio = np.abs(dx - dx64) / bound
    print("noise twin: worst ratio to the bound =", float(ratio.max()))
    assert (ratio <= 1.0).all()
    assert (np.abs(dx64).max(1) > 1e-3).sum() > n // 8                                # the test moves something


def test_noise_gate(L):
    """A dead row (o far below min_opacity) receives the full noise, a row with o = 0.5 at most exp(-49) of it."""
    rows, xi = _noise_inputs(64, 6)
    lr = 80.0
    rows["opacity"][:32], rows["opacity"][32:] = -20.0, 0.0
    rows["xyz"][:] = 0.0
    xyz = rows["xyz"].copy()
    MC.ok(L.fdgs_mcmc_noise_host(64, MC.p(xyz), MC.p(rows["scaling"]), MC.p(rows["rotation"]), MC.p(rows["opacity"]), lr, 100.0, MIN_OP, 0, 0, MC.p(xi)))
    full, _ = MC.noise64(rows["xyz"], rows["scaling"], rows["rotation"], np.full((64, 1), -1e4), xi, lr, 0.0, MIN_OP)    # k_gate 0: g = 1/2
    full = 2 * full
    gate_dead = 1 / (1 + math.exp(100 * (-MIN_OP)))                                   # o -> 0: g = 0.622, the most a row can get
    assert np.allclose(xyz[:32], gate_dead * full[:32], rtol=1e-4, atol=0)
    assert (np.abs(xyz[32:]) <= math.exp(-49.0) * np.abs(full[32:]) + 1e-45).all()


def test_normals_of_the_twin(L):
    n = 65536
    z = np.zeros((n, 3), np.float32)
    MC.ok(L.fdgs_mcmc_normals_host(n, 77, 3, MC.p(z)))
    assert np.isfinite(z).all()
    v = z.astype(np.float64).reshape(-1)
    m = v.shape[0]
    print("normals: mean", v.mean(), "variance", v.var(), "max |z|", np.abs(v).max())
    assert abs(v.mean()) <= 5 / math.sqrt(m) and abs(v.var() - 1) <= 5 * math.sqrt(2 / m)
    for c in range(3):
        assert abs(z[:, c].astype(np.float64).mean()) <= 5 / math.sqrt(n) and abs(z[:, c].astype(np.float64).var() - 1) <= 5 * math.sqrt(2 / n)
    assert abs(np.corrcoef(z.T.astype(np.float64))[np.triu_indices(3, 1)]).max() <= 5 / math.sqrt(n)
    assert np.abs(v).max() <= math.sqrt(64 * math.log(2)) * (1 + 1e-6)
    z2 = np.zeros((n, 3), np.float32)
    MC.ok(L.fdgs_mcmc_normals_host(n, 77, 4, MC.p(z2)))
    assert not np.array_equal(z, z2)                                                   # another iteration: other normals
    # a word of 0 must not reach log(0): u1 = (w0 + 1) 2^-32 -- restated from the Philox words, radius included
    ctr = np.zeros((n, 4), np.uint32)
    ctr[:, 0], ctr[:, 1] = np.arange(n), 3
    w = MC.philox(ctr, 77, MC.TAGS["noise"]).astype(np.float64)
    u1, u2 = (w[:, 0] + 1) * 2.0 ** -32, np.floor(w[:, 1] / 256) * 2.0 ** -24
    ref0 = np.sqrt(-2 * np.log(u1)) * np.cos(2 * math.pi * u2)
    assert np.abs(z[:, 0] - ref0).max() <= 8e-6
    assert math.isfinite(math.sqrt(-2 * math.log((0 + 1) * 2.0 ** -32)))
