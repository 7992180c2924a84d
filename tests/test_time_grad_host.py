"""fdgs_deform_time_grad_host -- the host twin of the time-gradient kernels (csrc/deform_time_grad.h) -- against the float64 autograd of
oracle.deform_oracle.hexplane_features with respect to t, on a random dL/dfeat.  CPU only.

The twin sums in double; what separates it from the float64 oracle is the float32 index arithmetic it shares with the kernels: a query
coordinate is off by ~2^-24 of the axis, i.e. by res * 2^-24 ~ 8e-6 of a texel at 128 texels, and the bilinear weights with it.
Bounds: per row rel-L2 <= 1e-5.  Summed over the rows (where the rows cancel: |sum| is ~ 1/20 of the rows' norm times sqrt(N)) the oracle's
OWN float32 evaluation is further than 1e-5 from its float64 one, so the sum's bound is that measured figure x 2 = 3.44e-5.
Measured on the CPU, per case (dnerf, hypernerf, dynerf, dynerf with multires [1, 2, 4]):
    twin vs float64 oracle            rows 6.11e-6, 8.88e-6, 5.36e-6, 8.88e-6     sum 1.09e-5, 1.63e-5, 9.52e-7, 1.63e-5
    oracle float32 vs float64         rows 6.18e-6, 8.89e-6, 5.38e-6, 8.89e-6     sum 1.09e-5, 1.72e-5, 1.16e-6, 1.72e-5"""
import numpy as np
import pytest
import torch

import time_grad_common as TC

CASES = [("dnerf_bouncingballs", None), ("hypernerf_default", None), ("dynerf_default", None), ("dynerf_default", dict(multires=[1, 2, 4]))]
N = 300
ROW_BOUND = 1e-5
SUM_BOUND = 2 * 1.72e-5        # (the oracle's float32 evaluation against its float64 one, summed, x 2: see above)


def _case(cfg, overrides, scalar_time=None):
    args, net, ins = TC.safe_inputs(cfg, N, overrides=overrides, relu=False)
    xyz, t = ins[0], ins[5]
    if scalar_time is not None:
        t = torch.full_like(t, scalar_time)
    F = net.deformation_net.grid.feat_dim
    dfeat = torch.randn(N, F, generator=torch.Generator().manual_seed(7)).numpy()
    return net, xyz, t, dfeat


@pytest.mark.parametrize("cfg,overrides", CASES)
def test_host_twin_against_float64_autograd_of_the_oracle(cfg, overrides):
    net, xyz, t, dfeat = _case(cfg, overrides)
    assert int((TC.time_row_distance(t, net) >= 1e-4).sum()) >= N - TC.N_PLANTED        # (the filter left random times, not only clamped rows)
    p, keep = TC.host_params(net, xyz, t)
    rows, tot, arows, atot = TC.host_twin(p, dfeat, np.ones(N, np.uint8))
    ref = TC.oracle_dt(net, xyz, t, dfeat)
    ref32 = TC.oracle_dt(net, xyz, t, dfeat, torch.float32)
    # the time planes are ones + 0.1 randn: the reference gradient is not ~ 0 (on identity time planes it is exactly 0, and a twin that
    # returned zeros would pass)
    assert np.linalg.norm(ref) > 1e-3 * np.linalg.norm(arows) > 0.0
    e_rows, e_sum = TC.rel_l2(rows, ref), abs(tot - ref.sum()) / abs(ref.sum())
    print(f"[{cfg} {overrides}] twin vs float64 oracle: rows {e_rows:.2e}, sum {e_sum:.2e}; oracle float32 vs float64: rows {TC.rel_l2(ref32, ref):.2e}, sum {abs(ref32.sum() - ref.sum()) / abs(ref.sum()):.2e}; "
          f"|ref| {np.linalg.norm(ref):.3e}, |sum abs| {np.linalg.norm(arows):.3e}")
    assert e_rows <= ROW_BOUND and e_sum <= SUM_BOUND
    assert tot == pytest.approx(rows.sum(), rel=1e-12) and atot == pytest.approx(arows.sum(), rel=1e-12)
    assert np.all(arows >= np.abs(rows) * (1 - 1e-12))
    # clamped times (t = 1.0 on the last time row, t = 1.2 beyond it): exactly 0, in the oracle too
    cl = TC.clamped(t).numpy()
    assert cl.sum() >= 2 and np.all(rows[cl] == 0.0) and np.all(arows[cl] == 0.0) and np.all(ref[cl] == 0.0)
    assert np.count_nonzero(rows[~cl]) == (~cl).sum()


@pytest.mark.parametrize("cfg,overrides", [CASES[0], CASES[3]])
def test_host_twin_with_one_frame_time(cfg, overrides):
    net, xyz, t, dfeat = _case(cfg, overrides, scalar_time=0.37)
    p, keep = TC.host_params(net, xyz, 0.37)
    rows, tot, arows, atot = TC.host_twin(p, dfeat, np.ones(N, np.uint8))
    ref = TC.oracle_dt(net, xyz, t, dfeat)
    assert np.linalg.norm(ref) > 1e-3 * np.linalg.norm(arows) > 0.0
    assert TC.rel_l2(rows, ref) <= ROW_BOUND and abs(tot - ref.sum()) / abs(ref.sum()) <= SUM_BOUND
    for t_clamped in (1.0, 1.2):
        p, keep = TC.host_params(net, xyz, t_clamped)
        rows, tot, arows, atot = TC.host_twin(p, dfeat, np.ones(N, np.uint8))
        assert tot == 0.0 and atot == 0.0 and not rows.any()


def test_dead_rows_contribute_nothing_even_when_their_dfeat_is_nan():
    net, xyz, t, dfeat = _case("dynerf_default", None)
    p, keep = TC.host_params(net, xyz, t)
    live = (np.arange(N) % 3 != 0).astype(np.uint8)
    rows, tot, arows, atot = TC.host_twin(p, dfeat, np.ones(N, np.uint8))
    bad = dfeat.copy()
    bad[live == 0] = np.nan
    rows2, tot2, arows2, atot2 = TC.host_twin(p, bad, live)
    assert np.all(rows2[live == 0] == 0.0) and np.all(arows2[live == 0] == 0.0) and np.isfinite(tot2) and np.isfinite(atot2)
    assert np.array_equal(rows2[live == 1], rows[live == 1]) and tot2 == pytest.approx(rows[live == 1].sum(), rel=1e-12)


def test_host_twin_validates_its_arguments():
    net, xyz, t, dfeat = _case("dynerf_default", None)
    p, keep = TC.host_params(net, xyz, t)
    L = TC._lib.lib()
    assert L.fdgs_deform_time_grad_host(p, None, None, None, None, None, None) != 0
    p.planes[1][4] = None
    live = np.ones(N, np.uint8)
    assert L.fdgs_deform_time_grad_host(p, dfeat.ctypes.data, live.ctypes.data, None, None, None, None) != 0
    assert b"plane" in L.fdgs_last_error()


def test_the_row_filters_of_the_gpu_tests_yield_their_row_counts():
    """tests/test_gpu_time_grad.py compares with the float64 oracle on rows that are safe in ReLU, spatial cell and time row, the planted
    clamped rows among them: the candidates it draws suffice (checked here, without a GPU)."""
    for cfg, n in TC.ORACLE_CASES:
        args, net, ins = TC.safe_inputs(cfg, n)
        t = ins[5].reshape(-1)
        assert ins[0].shape[0] == n and int((t == 1.0).sum()) >= 1 and int((t == 1.2).sum()) >= 1
        assert bool(((TC.time_row_distance(t, net) >= 1e-4) | TC.clamped(t)).all())
    for cfg, n, t in TC.ORACLE_SCALAR_CASES:
        assert TC.safe_inputs_one_time(cfg, n, t)[2][0].shape[0] == n
