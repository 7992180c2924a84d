"""The yardstick of the sparse Adam tests (test_sparse_adam_host.py, test_gpu_sparse_adam.py): cases, references and the error measure.

One step of the float32 reference is torch.optim.Adam on the CPU over a copy (bias_correction=False: the same formulas written out in torch
float32, step_size = lr and sqrt(1 - beta2^t) = 1); afterwards the invisible rows of p, exp_avg and exp_avg_sq are put back from before the
step.  A float64 evaluation of the same formulas is the ground truth of the per-element bound

    |x - x64| <= c * 2^-23 * (|x64| + |dx64|),      dx64 = the step's change of that element in float64,

for x in (p, exp_avg, exp_avg_sq).  c is not a constant of this file: `reference()` measures the worst ratio torch's own float32 CPU Adam
reaches against float64 on a case's inputs, and `bound_c()` allows twice the worst of those over every case, not less than 1 (two correct
float32 evaluations differ by contraction and ordering).  Measured figures are in the docstring of test_sparse_adam_host.py.

A case is (N, first mask kind, bias_correction, poison): the ten tensors of test_gpu_optim.py::_make at N rows (row lengths 3, 3, 45, 1,
3, 4; the dense `bias` (7), `one` (1) and the channels_last `plane`; `unused` without gradient), six steps with "lr" rewritten per step and
gradient scales 10^(it-3), the mask kind advancing by one every step.  `poison` plants NaN and inf in the gradients of invisible rows.
References are computed once per case and shared (functools.lru_cache); nothing may write to them.
"""
import functools

import numpy as np
import torch

ROW_GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
NS = (1, 33, 1001)
MASK_KINDS = ("none", "all", "first", "last", "alternate", "run32", "random12")
STEPS = 6
BETAS, EPS = (0.9, 0.999), 1e-15
ULP = 2.0 ** -23


def shapes(N):
    return {"xyz": (N, 3), "f_dc": (N, 1, 3), "f_rest": (N, 15, 3), "opacity": (N, 1), "scaling": (N, 3), "rotation": (N, 4),
            "bias": (7,), "one": (1,), "plane": (1, 16, 9, 11), "unused": (5,)}


def make_mask(kind, N, seed=0):
    m = torch.zeros(N, dtype=torch.bool)
    if kind == "all":
        m[:] = True
    elif kind == "first":
        m[0] = True
    elif kind == "last":
        m[N - 1] = True
    elif kind == "alternate":
        m[::2] = True
    elif kind == "run32":
        m[45:45 + 32] = True                  # (empty where N <= 45)
    elif kind == "random12":
        m = torch.rand(N, generator=torch.Generator().manual_seed(1234 + seed)) < 0.12
    else:
        assert kind == "none", kind
    return m


def lr_of(it, gi):
    return 1e-3 / (1 + it) * (1 + gi)


@functools.lru_cache(maxsize=None)
def inputs(N, first, poison=False):
    """(initial parameters {name: tensor}, per step: ({name: gradient}, {name: lr}, mask [N] bool)) -- CPU float32, read-only."""
    gen = torch.Generator().manual_seed(100 * N + first)
    sh = shapes(N)
    p0 = {k: torch.randn(*s, generator=gen) for k, s in sh.items()}
    steps = []
    for it in range(STEPS):
        mask = make_mask(MASK_KINDS[(first + it) % len(MASK_KINDS)], N, seed=it)
        g = {k: torch.randn(*s, generator=gen) * 10.0 ** (it - 3) for k, s in sh.items() if k != "unused"}
        if poison:
            for k in ROW_GROUPS:
                bad = g[k].view(N, -1)
                bad[~mask] = torch.tensor([float("nan"), float("inf"), -float("inf")])[torch.arange(int((~mask).sum())) % 3].unsqueeze(1)
        lrs = {k: lr_of(it, gi) for gi, k in enumerate(sh)}
        steps.append((g, lrs, mask))
    return p0, steps


def _rows(k, mask):
    """Which elements of tensor `k` a step with `mask` touches: its rows for a row group, everything otherwise (None)."""
    return mask if k in ROW_GROUPS else None


def f64_step(p, m, v, g, lr, t, rows, bias_correction):
    """One Adam step in float64 from float32 state: (p, m, v) as float64 arrays, rows outside `rows` (bool [N] or None) unchanged."""
    p, m, v, g = (x.detach().cpu().double() for x in (p, m, v, g))
    b1, b2 = BETAS
    m1 = m + (g - m) * (1.0 - b1)
    v1 = b2 * v + (1.0 - b2) * g * g
    step_size, sqrt_bc2 = (lr / (1.0 - b1 ** t), (1.0 - b2 ** t) ** 0.5) if bias_correction else (lr, 1.0)
    p1 = p - step_size * (m1 / (v1.sqrt() / sqrt_bc2 + EPS))
    if rows is not None:
        keep = ~rows
        for new, old in ((p1, p), (m1, m), (v1, v)):
            new.view(rows.numel(), -1)[keep] = old.view(rows.numel(), -1)[keep]
    return p1, m1, v1


def ratio(x, x64, x_old, rows=None):
    """Worst |x - x64| / (2^-23 (|x64| + |x64 - x_old|)) over the stepped elements; inf where a non-finite value or a difference at a zero
    denominator shows."""
    x, x_old = x.detach().cpu().double(), x_old.detach().cpu().double()
    if rows is not None:
        x, x64, x_old = (a.view(rows.numel(), -1)[rows] for a in (x, x64, x_old))
    if x.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(x).all()):
        return float("inf")
    err, den = (x - x64).abs(), ULP * (x64.abs() + (x64 - x_old).abs())
    r = torch.where(den > 0, err / den.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


def same_bits(a, b):
    return torch.equal(a.detach().cpu().contiguous().view(torch.int32), b.detach().cpu().contiguous().view(torch.int32))


def _torch_f32_step(p, m, v, g, lr):
    """bias_correction=False in torch float32: torch's single-tensor Adam with step_size = lr and bias_correction2_sqrt = 1."""
    b1, b2 = BETAS
    m.lerp_(g, 1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    p.addcdiv_(m, v.sqrt().add_(EPS), value=-lr)


@functools.lru_cache(maxsize=None)
def reference(N, first, bias_correction=True, poison=False):
    """The float32 yardstick chain over the case's six steps.  Returns (final {name: (p, m, v)}, torch's worst ratio against float64 per
    quantity {"p": r, "m": r, "v": r})."""
    p0, steps = inputs(N, first, poison)
    names = [k for k in p0 if k != "unused"]
    P = {k: torch.nn.Parameter(p0[k].clone()) for k in p0}
    opt = torch.optim.Adam([{"params": [P[k]], "lr": 0.0, "name": k} for k in p0], lr=0.0, eps=EPS, betas=BETAS) if bias_correction else None
    M = {k: torch.zeros_like(p0[k]) for k in names}
    V = {k: torch.zeros_like(p0[k]) for k in names}
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for it, (g, lrs, mask) in enumerate(steps):
        if opt is not None and it > 0:
            M, V = ({k: opt.state[P[k]][key] for k in names} for key in ("exp_avg", "exp_avg_sq"))
        before = {k: (P[k].detach().clone(), M[k].clone(), V[k].clone()) for k in names}
        if opt is not None:
            for group in opt.param_groups:
                group["lr"] = lrs[group["name"]]
            for k in names:
                P[k].grad = g[k].clone()
            opt.step()
            M, V = ({k: opt.state[P[k]][key] for k in names} for key in ("exp_avg", "exp_avg_sq"))
        else:
            with torch.no_grad():
                for k in names:
                    _torch_f32_step(P[k], M[k], V[k], g[k], lrs[k])
        with torch.no_grad():
            for k in names:
                rows = _rows(k, mask)
                if rows is not None:        # the invisible rows are put back from before the step
                    for new, old in zip((P[k], M[k], V[k]), before[k]):
                        new.view(N, -1)[~rows] = old.view(N, -1)[~rows]
                x64 = f64_step(*before[k], g[k], lrs[k], it + 1, rows, bias_correction)
                for q, new, ref, old in zip("pmv", (P[k], M[k], V[k]), x64, before[k]):
                    worst[q] = max(worst[q], ratio(new, ref, old, rows))
    return {k: (P[k].detach(), M[k], V[k]) for k in names}, worst


def cases():
    """Every (N, first mask kind index): each kind is the first mask of one run at every N, and every kind is met at every step index."""
    return [(N, first) for N in NS for first in range(len(MASK_KINDS))]


@functools.lru_cache(maxsize=None)
def torch_ratios(bias_correction=True):
    """torch's float32 CPU Adam against float64 over every case: the worst ratio per quantity."""
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for N, first in cases():
        _, w = reference(N, first, bias_correction)
        worst = {q: max(worst[q], w[q]) for q in worst}
    return worst


def bound_c(bias_correction=True):
    return max(1.0, 2.0 * max(torch_ratios(bias_correction).values()))


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    d = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / d) if d > 0 else float(np.linalg.norm(a))


class Chain:
    """The ten tensors of a case on `dev` with both moments, laid out as the product lays them out (`plane` channels_last), and the
    checks of one step: invisible rows bit-identical, stepped elements within the bound of float64 from this chain's own state."""

    def __init__(self, N, first, dev, poison=False):
        self.N, self.first, self.dev, self.poison = N, first, dev, poison
        p0, self.steps = inputs(N, first, poison)
        self.names = [k for k in p0 if k != "unused"]
        self.p = {k: p0[k].clone().to(dev) for k in p0}
        self.p["plane"] = self.p["plane"].contiguous(memory_format=torch.channels_last)
        self.m = {k: torch.zeros_like(self.p[k], memory_format=torch.preserve_format) for k in self.names}
        self.v = {k: torch.zeros_like(self.p[k], memory_format=torch.preserve_format) for k in self.names}
        self.worst = {"p": 0.0, "m": 0.0, "v": 0.0}

    def grads(self, it):
        g = {k: self.steps[it][0][k].to(self.dev) for k in self.names}
        g["plane"] = g["plane"].contiguous(memory_format=torch.channels_last)
        return g

    def snapshot(self):
        return {k: tuple(x.detach().cpu().clone() for x in (self.p[k], self.m[k], self.v[k])) for k in self.names}

    def check_step(self, it, before, bias_correction, c):
        g, lrs, mask = self.steps[it]
        after = self.snapshot()
        for k in self.names:
            rows = _rows(k, mask)
            x64 = f64_step(*before[k], g[k], lrs[k], it + 1, rows, bias_correction)
            for q, new, ref, old in zip("pmv", after[k], x64, before[k]):
                if rows is not None:
                    assert same_bits(new.view(self.N, -1)[~rows], old.view(self.N, -1)[~rows]), (k, q, it, "an invisible row changed")
                r = ratio(new, ref, old, rows)
                self.worst[q] = max(self.worst[q], r)
                assert r <= c, (k, q, it, r, c)

    def check_against_reference(self, bias_correction):
        ref, _ = reference(self.N, self.first, bias_correction, self.poison)
        for k in self.names:
            for new, want in zip((self.p[k], self.m[k], self.v[k]), ref[k]):
                assert rel_l2(new.detach().cpu().numpy(), want.numpy()) < 1e-6, k
