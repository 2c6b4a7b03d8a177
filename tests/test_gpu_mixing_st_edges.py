"""``MixingST`` (mixing_st.hip) at the edges the golden shape 20 x 18, T = 3 does not reach (needs an MI355X): a pixel count one
below, equal to and several times a 256-thread block, one and MAXT = 8 templates, one and 37 wavelengths, and voxel lists that
hold every voxel, a random 30 % with 50 voxels listed twice, one single voxel, and one pixel whose wavelengths come in descending
order.  ``forward``, ``adjoint``, ``fwadj`` and the precomputed TST (read through ``fwadj`` on unit maps) against
``MixingSTOracle`` on every local measure at the 1e-6 of test_gpu_variants.test_masked_mixing_model_vs_reference."""
import numpy as np
import pytest

from oracle import surfh_oracle as orc
from test_gpu_local_parity import check_local
from test_gpu_parity import note

pytestmark = pytest.mark.gpu

TOL_ST = 1e-6
SHAPES = [(17, 15), (16, 16), (23, 45)]                       # npix = 255, 256, 1035
CUBE_AXES = dict(plane=0, alpha=1, beta=2)
MAP_AXES = dict(template=0, alpha=1, beta=2)
LISTS = ("every_voxel", "random_30_percent_50_twice", "single_voxel", "one_pixel_descending")


def voxel_list(kind, L, na, nb, rng):
    if kind == "every_voxel":
        return np.array(np.where(np.ones((L, na, nb), dtype=bool))).T
    if kind == "random_30_percent_50_twice":
        v = np.array(np.where(rng.random((L, na, nb)) < 0.3)).T
        return np.concatenate([v, v[rng.integers(0, len(v), 50)]])
    if kind == "single_voxel":
        return np.array([[L - 1, na - 1, nb - 1]])
    i, j = na // 2, nb - 1
    return np.array([[l, i, j] for l in range(L - 1, -1, -1)])


def make(kind, shape, T, L, seed):
    from surfh_amd.mixing import MixingST
    na, nb = shape
    rng = np.random.default_rng(seed)
    tpl = rng.random((T, L)) + 0.25
    fast = voxel_list(kind, L, na, nb, rng)
    listed = np.zeros((L, na, nb), dtype=bool)
    listed[tuple(fast.T)] = True
    sel = np.where(~listed)                                    # the mask S is one on the listed voxels
    m = MixingST(tpl, np.arange(na, dtype=float), np.arange(nb, dtype=float), np.arange(L, dtype=float), sel, fast)
    return m, orc.MixingSTOracle(tpl, shape, sel, fast), fast, rng


@pytest.mark.parametrize("L", [1, 37])
@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=["npix255", "npix256", "npix1035"])
def test_against_oracle(shape, T, L):
    na, nb = shape
    for n, kind in enumerate(LISTS):
        m, o, fast, rng = make(kind, shape, T, L, 1000 * na + 10 * T + L + n)
        try:
            maps, cube = rng.random((T, na, nb)), rng.standard_normal((L, na, nb))
            tags = dict(shape=list(shape), T=T, L=L, voxels=kind)
            f = m.forward(maps)
            check_local("mixing_st_forward", f, o.forward(maps), CUBE_AXES, tol=TOL_ST, **tags)
            off = np.ones((L, na, nb), dtype=bool)
            off[tuple(fast.T)] = False
            assert not f[off].any()                            # nothing outside the list
            check_local("mixing_st_adjoint", m.adjoint(cube), o.adjoint(cube), MAP_AXES, tol=TOL_ST, **tags)
            check_local("mixing_st_fwadj", m.fwadj(maps), o.fwadj(maps), MAP_AXES, tol=TOL_ST, **tags)
            tst = np.empty((T, T, na, nb))
            for mp in range(T):
                unit = np.zeros((T, na, nb))
                unit[mp] = 1.0
                tst[:, mp] = m.fwadj(unit)
            check_local("mixing_st_tst", tst, o.TST, dict(block=(0, 1), alpha=2, beta=3), tol=TOL_ST, **tags)
        finally:
            m.close()


@pytest.mark.parametrize("shape", SHAPES, ids=["npix255", "npix256", "npix1035"])
def test_dot_test(shape):
    """<A x, y> = <x, A^T y> with float64 sums over the listed voxels (A x is zero elsewhere), 1e-6 as
    test_gpu_lambda_trim.test_dot_test: normalised for zero-mean vectors, the strict ratio for non-negative ones."""
    na, nb = shape
    T, L = 8, 37
    m, _, fast, rng = make("random_30_percent_50_twice", shape, T, L, 77 + na)
    idx = tuple(np.unique(fast, axis=0).T)
    try:
        x, y = rng.standard_normal((T, na, nb)), rng.standard_normal((L, na, nb))
        ax = m.forward(x).astype(np.float64)
        l, r = float(np.vdot(ax[idx], y[idx])), float(np.vdot(x, m.adjoint(y).astype(np.float64)))
        ngap = abs(l - r) / (np.linalg.norm(y[idx]) * np.linalg.norm(ax[idx]))
        x, y = rng.random((T, na, nb)), rng.random((L, na, nb))
        l, r = float(np.vdot(m.forward(x).astype(np.float64)[idx], y[idx])), float(np.vdot(x, m.adjoint(y).astype(np.float64)))
        pgap = abs(l - r) / abs(r)
    finally:
        m.close()
    note("mixing_st_dot_test", shape=list(shape), zero_mean=ngap, non_negative=pgap)
    print(f"MixingST {shape}: dot test, zero-mean (normalised) {ngap:.2e}, non-negative {pgap:.2e}")
    assert ngap < 1e-6 and pgap < 1e-6


def test_nine_templates_are_refused():
    from surfh_amd.mixing import MixingST
    L, na, nb = 5, 4, 3
    fast = np.array([[0, 0, 0]])
    with pytest.raises(ValueError, match="templates"):
        MixingST(np.ones((9, L)), np.arange(na, dtype=float), np.arange(nb, dtype=float), np.arange(L, dtype=float), None, fast)
