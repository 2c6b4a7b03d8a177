"""Host side of the template extraction (surfh_amd.templates): sklearn's random init, input validation before any
library call, the helpers, and the files as scripts/main_fusion.py loads them.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from surfh_amd import _lib, synth
from surfh_amd import templates as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("k,seed", [(1, 0), (4, 0), (6, 42)])
def test_random_init_is_sklearns(dtype, k, seed):
    nmf = pytest.importorskip("sklearn.decomposition._nmf")
    X = np.abs(np.random.default_rng(1).standard_normal((37, 53))).astype(dtype)
    W, H = T.init_random(X, k, seed)
    Wr, Hr = nmf._initialize_nmf(X, k, init="random", random_state=seed)
    assert W.dtype == Wr.dtype == dtype and H.dtype == Hr.dtype
    assert np.array_equal(W, Wr) and np.array_equal(H, Hr)


def test_templates_module_does_not_import_sklearn():
    code = ("import sys; sys.modules['sklearn'] = None\n"
            "import numpy as np\n"
            "from surfh_amd import templates as T\n"
            "W, H = T.init_random(np.ones((3, 4)), 2, 0)\n"
            "T.NMF(2, random_state=0)\n"
            "print(W.shape, H.shape)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "(3, 2) (2, 4)" in r.stdout, r.stderr


@pytest.fixture
def no_library(monkeypatch):
    """Any library call fails the test: validation must come first."""
    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", boom)


@pytest.mark.parametrize("bad", [np.array([[1.0, -1e-3], [2.0, 3.0]]), np.array([[1.0, np.nan], [2.0, 3.0]]),
                                 np.array([[1.0, np.inf], [2.0, 3.0]]), np.ones(4), np.zeros((0, 3))])
def test_invalid_X_raises_before_library(no_library, bad):
    with pytest.raises(ValueError):
        T.NMF(2, random_state=0).fit(bad)
    with pytest.raises(ValueError):
        T.nmf_sweep(bad, range(1, 3))


@pytest.mark.parametrize("kw", [dict(solver="mu"), dict(beta_loss="kullback-leibler"), dict(alpha_W=0.1),
                                dict(alpha_H=0.1), dict(init="nndsvd"), dict(init="nndsvda"), dict(shuffle=True)])
def test_unsupported_options_raise(no_library, kw):
    with pytest.raises(NotImplementedError):
        T.NMF(2, **kw)


def test_bad_parameters_raise(no_library):
    X = np.ones((4, 5))
    for kw in (dict(n_components=0), dict(n_components=2, max_iter=0), dict(n_components=2, tol=-1.0)):
        with pytest.raises(ValueError):
            T.NMF(**kw)
    with pytest.raises(ValueError):
        T.NMF(2, init="custom").fit(X)                       # custom without W, H
    with pytest.raises(ValueError):
        T.NMF(2, init="custom").fit(X, W=np.ones((4, 3)), H=np.ones((3, 5)))
    with pytest.raises(ValueError):
        T.NMF(2, init="custom").fit(X, W=-np.ones((4, 2)), H=np.ones((2, 5)))
    for kw in (dict(size=0), dict(size=64), dict(size=3, mode="wrap"), dict(size=3, mode="constant")):
        with pytest.raises(ValueError):
            T.median_filter_spectral(np.ones((5, 2)), **kw)
    with pytest.raises(ValueError):
        T.median_filter_spectral(np.float32(1.0), 3)


def test_cube_to_matrix_and_subsample():
    cube = np.arange(5 * 4 * 3, dtype=np.float32).reshape(5, 4, 3)
    X = T.cube_to_matrix(cube)
    assert X.shape == (12, 5) and np.array_equal(X[7], cube[:, 2, 1])
    Xb = T.cube_to_matrix(cube, box=(1, 3, 0, 2))
    assert Xb.shape == (4, 5) and np.array_equal(Xb[3], cube[:, 2, 1])
    comp, wl = T.subsample_templates(np.arange(2 * 10).reshape(2, 10), np.arange(10.0), 4)
    assert comp.shape == (2, 3) and np.array_equal(wl, [0.0, 4.0, 8.0]) and np.array_equal(comp[1], [10, 14, 18])
    with pytest.raises(ValueError):
        T.subsample_templates(np.ones((2, 10)), np.ones(9))


def test_synthetic_template_cube():
    d = synth.synthetic_template_cube(n_lambda=64, ny=5, nx=6, n_templates=6, nan_fraction=0.2, seed=3)
    c = d["cube"]
    assert c.shape == (64, 5, 6) and c.dtype == np.float32
    nan = np.isnan(c)
    assert nan.any() and np.array_equal(nan, np.broadcast_to(nan[0], c.shape))
    assert np.all(c[~nan] >= 0) and d["templates"].shape == (6, 64) and d["abundances"].shape == (6, 5, 6)
    exact = np.einsum("kl,kyx->lyx", d["templates"], d["abundances"])
    assert np.allclose(c[~nan], exact[~nan], rtol=1e-6)
    assert np.array_equal(d["templates"][:4], synth.templates(64))


@pytest.mark.parametrize("nt", [4, 6])
def test_written_files_load_in_main_fusion(tmp_path, nt):
    L, step = 42, 4
    comp = np.random.default_rng(nt).random((nt, L))
    wavel = np.linspace(5.0, 28.0, L)
    p_t, p_w = T.write_templates(tmp_path / "Templates", comp, wavel, step=step)
    assert os.path.basename(p_t) == f"nmf_orion_1ABC_2ABC_3ABC_4ABC_{nt}_templates_SS4.npy"
    assert os.path.basename(p_w) == f"wavel_axis_orion_1ABC_2ABC_3ABC_4ABC_{nt}_templates_SS4.npy"
    n_w = len(wavel[::step])
    os.makedirs(tmp_path / "PSF")
    np.save(tmp_path / "PSF" / "psfs_pixscale0.025_npix_501_fov12.525_chan_1ABC_2ABC_3ABC_4ABC_SS4.npy",
            np.ones((n_w, 3, 3)))
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import main_fusion                                   # noqa: PLC0415
    paths, s, sa = main_fusion.initialize_parameters(str(tmp_path))
    _, _, wl, tpl, sotf = main_fusion.load_simulation_data(paths, s, sa, 8, nt)
    assert tpl.shape == (nt, n_w) and wl.shape == (n_w,)
    assert np.allclose(tpl, comp[:, ::step] / 10e3) and np.array_equal(wl, wavel[::step])
    assert sotf.shape[0] == n_w
