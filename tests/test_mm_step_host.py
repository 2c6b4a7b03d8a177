"""The 2x2 step solve every 3MG solver shares (surfh_amd/csrc/mm_step.h: mm_step2, on the host and in the plane kernels), through
the host-only C-ABI hook surfh_mm_step2 -- no GPU -- against numpy.linalg.solve on the unscaled system
[[dBd, dBm], [dBm, mBm]] s = [dg, mg] in float64, and its three guards."""
import ctypes

import numpy as np
import pytest


def step(dBd, dBm, mBm, dg, mg):
    from surfh_amd import _lib
    out = (ctypes.c_double * 2)()
    assert _lib.load().surfh_mm_step2(dBd, dBm, mBm, dg, mg, out) == 0
    return out[0], out[1]


def test_well_conditioned_system():
    """cond([[3, 0.5], [0.5, 2]]) = 1.9: the scaled and the unscaled solve both carry a few ulp, far inside 1e-12"""
    dBd, dBm, mBm, dg, mg = 3.0, 0.5, 2.0, 1.25, -0.75
    ref = np.linalg.solve(np.array([[dBd, dBm], [dBm, mBm]]), np.array([dg, mg]))
    s = np.array(step(dBd, dBm, mBm, dg, mg))
    assert np.all(np.abs(s - ref) <= 1e-12 * np.abs(ref))


def test_no_memory_direction():
    assert step(3.0, 0.5, 0.0, 1.25, -0.75) == (1.25 / 3.0, 0.0)


def test_collinear_pair_takes_the_one_direction_step():
    dBd, mBm, dg, mg = 3.0, 2.0, 1.25, -0.75
    dBm = np.sqrt(dBd * mBm * (1.0 - 1e-13))                # det of the scaled system = 1e-13 <= 1e-12
    assert step(dBd, dBm, mBm, dg, mg) == (dg / dBd, 0.0)


@pytest.mark.parametrize("dBd", [0.0, -1.0, float("nan")])
def test_no_curvature_keeps_still(dBd):
    assert step(dBd, 0.5, 2.0, 1.25, -0.75) == (0.0, 0.0)
