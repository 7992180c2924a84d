"""The yardstick of tests/test_gpu_absgrad.py, tested where no GPU is present (CPU): the per-pixel construction of tests/absgrad_common.py
adds up to the oracle's own gradient, the scenes have the property that makes them a test of the absolute sums, and the reference has the
structure the device result is held to."""
import numpy as np
import pytest

import absgrad_common as AG


@pytest.mark.parametrize("name", ["S", "L"])
def test_scene_conditions(name):
    AG.assert_scene_condition(name)
    sc = AG.scene(name)
    assert (sc["image_width"], sc["image_height"]) == (40, 24)            # 3 x 2 tiles, partial on both edges
    if name == "S":
        assert AG.longest_list("S") <= 64                                  # one 64-entry round
    else:
        assert AG.saturated_share("L") >= 0.4


@pytest.mark.parametrize("part", AG.PARTS)
def test_the_per_pixel_rows_add_up_to_the_oracles_gradient(part):
    rows = AG.per_pixel("S", part)                                         # (asserts the identity itself)
    assert rows.shape == (40 * 24, 60, 2) and np.abs(rows).sum() > 0


@pytest.mark.parametrize("aa", [False, True])
def test_the_reference_has_the_structure_the_device_is_held_to(aa):
    a, s, blended = AG.reference("S", True, True, aa)
    assert a.shape == (60, 2) and (a >= 0).all()
    assert (np.abs(s) <= a * (1 + 1e-12)).all()                            # the triangle inequality, row by row
    assert blended.any() and not a[~blended].any() and (a[blended].sum(1) > 0).all()
    # alpha's share enters before the absolute value: the reference of the mixed loss is not the sum of the parts' references
    a_c = AG.reference("S", False, False, aa)[0]
    rows_a = np.abs(AG.per_pixel("S", "alpha", aa)).sum(0)
    rows_d = np.abs(AG.per_pixel("S", "depth", aa)).sum(0)
    assert (a <= (a_c + rows_a + rows_d) * (1 + 1e-12)).all() and not np.allclose(a, a_c + rows_a + rows_d, rtol=1e-3)


def test_the_antialiased_reference_is_another_one():
    a0, a1 = AG.reference("S")[0], AG.reference("S", aa=True)[0]
    assert np.linalg.norm(a0 - a1) > 1e-3 * np.linalg.norm(a0)


def test_one_row():
    a, s, blended = AG.reference("1")
    assert a.shape == (1, 2) and blended[0] and a[0].min() > 0
