"""Restatements of MCMC densification's definitions (include/fdgs.h, "MCMC densification") in numpy / float64, shared by the CPU tests of the
host entry points (test_mcmc_abi.py, test_mcmc_host.py).  Test infrastructure: nothing here is imported by the
product."""
import ctypes
import importlib
import math
import os

import numpy as np

_lib = importlib.import_module("4dgaussians_amd._lib")
TAGS = _lib.MCMC_TAGS
U64 = np.uint64
MASK = U64(0xFFFFFFFF)


def lib():
    if not os.path.exists(_lib.LIB_PATH):
        importlib.import_module("4dgaussians_amd.build").build()
    return _lib.lib()


def p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def ok(rc):
    assert rc == 0, lib().fdgs_last_error().decode()


# ---- Philox4x32-10 (Salmon et al., SC'11) -----------------------------------------------------------------------------------------------
def philox(counters, k0, k1):
    """words [n,4] uint32 of counters [n,4] under the key (k0, k1)."""
    c0, c1, c2, c3 = (np.ascontiguousarray(counters[:, i]).astype(U64) for i in range(4))
    k0, k1 = U64(k0), U64(k1)
    for _ in range(10):
        p0, p1 = U64(0xD2511F53) * c0, U64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> U64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> U64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + U64(0x9E3779B9)) & MASK, (k1 + U64(0xBB67AE85)) & MASK
    return np.stack([c0, c1, c2, c3], 1).astype(np.uint32)


# ---- sampling ---------------------------------------------------------------------------------------------------------------------------
def sample(weights, n, seed, tag):
    """(sources int32[n], counts) of n draws over uint32 weights: uint64 scan, 64-bit Philox word, mulhi64, first row whose sum exceeds it."""
    scan = np.cumsum(weights.astype(U64), dtype=U64)
    total = int(scan[-1])
    ctr = np.zeros((n, 4), np.uint32)
    ctr[:, 0] = np.arange(n, dtype=np.uint32)
    w = philox(ctr, seed, tag)
    u = (w[:, 1].astype(U64) << U64(32)) | w[:, 0].astype(U64)
    r = np.array([(int(x) * total) >> 64 for x in u], dtype=U64)
    src = np.searchsorted(scan, r, side="right").astype(np.int32)
    return src, np.bincount(src, minlength=weights.shape[0]).astype(np.uint32)


def weights64(x):
    """floor(sigmoid64(x) * 2^32) as float64: what a weight is compared against (to 2^9 units: a float32 sigmoid scaled by 2^32)."""
    return np.floor(4294967296.0 / (1.0 + np.exp(-x.astype(np.float64))))


def sigmoid32(x):
    """The float32 expression of the dead test, 1 / (1 + expf(-x))."""
    x = x.astype(np.float32)
    return (np.float32(1) / (np.float32(1) + np.exp(-x))).astype(np.float32)


# ---- relocation values ------------------------------------------------------------------------------------------------------------------
MAX_RATIO = 51


def ratio(count):
    return min(int(count) + 1, MAX_RATIO)


def relocation64(x_o, x_s, count, min_opacity):
    """(o' after the clamp, s'[3], o' before the clamp) in float64 from the float32 raw parameters: the definition as written, the double sum
    over exact integer binomials added up by math.fsum.  1 - o is never formed from o: log(1 - o) = -log(1 + e^x)."""
    r = ratio(count)
    x = float(x_o)
    log_1mo = -float(np.logaddexp(0.0, x))
    o = math.exp(-float(np.logaddexp(0.0, -x)))
    on = -math.expm1(log_1mo / r)
    terms = [math.comb(i - 1, k) * (-1.0) ** k * on ** (k + 1) / math.sqrt(k + 1) for i in range(1, r + 1) for k in range(i)]
    D = math.fsum(terms)
    s_new = np.exp(np.asarray(x_s, np.float64)) * o / D
    return min(max(on, float(np.float32(min_opacity))), 1.0 - 2.0 ** -23), s_new, on


def sigmoid64(x):
    x = np.asarray(x, np.float64)
    return np.exp(-np.logaddexp(0.0, -x))


# ---- noise ------------------------------------------------------------------------------------------------------------------------------
def noise64(xyz, scaling, rotation, opacity, xi, lr, k_gate, min_opacity):
    """(dx [N,3], bound [N,3]) in float64 from float32 inputs: dx = (R diag(s^2) R^T) xi g lr and the bound of the float32 evaluation,
    64 * 2^-23 * (sum_j |M_ij| |xi_j|) g lr + 2^-23 |xyz_i|."""
    f = lambda a: np.asarray(a, np.float64)
    xyz, scaling, q, xo, xi = f(xyz), f(scaling), f(rotation), f(opacity).reshape(-1), f(xi)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    r, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    M = np.einsum("nik,nk,njk->nij", R, np.exp(scaling) ** 2, R)
    o = sigmoid64(xo)
    g = np.exp(-np.logaddexp(0.0, float(k_gate) * (o - float(np.float32(min_opacity)))))
    dx = np.einsum("nij,nj->ni", M, xi) * (g * lr)[:, None]
    bound = 64 * 2.0 ** -23 * np.einsum("nij,nj->ni", np.abs(M), np.abs(xi)) * (g * lr)[:, None] + 2.0 ** -23 * np.abs(xyz)
    return dx, bound


def random_rows(n, seed, dead_frac=0.3, sh_rest=15):
    """Raw parameters of n Gaussians (float32 numpy): about dead_frac of the opacities far below the dead threshold, the rest well above."""
    g = np.random.default_rng(seed)
    dead = g.random(n) < dead_frac if 0 < dead_frac < 1 else np.full(n, dead_frac >= 1)
    op = np.where(dead, g.uniform(-12.0, -7.0, n), g.uniform(-4.0, 6.0, n)).astype(np.float32).reshape(n, 1)
    return {"xyz": g.normal(0, 1, (n, 3)).astype(np.float32), "f_dc": g.normal(0, 1, (n, 1, 3)).astype(np.float32),
            "f_rest": g.normal(0, 1, (n, sh_rest, 3)).astype(np.float32), "opacity": op,
            "scaling": g.uniform(-5.0, -1.0, (n, 3)).astype(np.float32), "rotation": g.normal(0, 1, (n, 4)).astype(np.float32)}, dead
