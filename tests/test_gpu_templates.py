"""The GPU template extraction (surfh_spectral_median, surfh_nmf_cd, surfh_amd.templates) against scipy's median filter
and sklearn's coordinate-descent NMF (tests/golden/templates.npz), batching and determinism, recovery of synthetic
templates, the driver script, and one size run that reports the speed."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from surfh_amd import synth
from surfh_amd import templates as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "templates.npz")
GOLDEN_EDGES = os.path.join(ROOT, "tests", "golden", "templates_edges.npz")


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN)


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def test_median_matches_scipy_bit_for_bit(z):
    n = int(z["med_count"])
    sizes = set()
    for i in range(n):
        a, ref = z[f"med{i}_in"], z[f"med{i}_out"]
        s, mode = int(z[f"med{i}_size"]), str(z[f"med{i}_mode"])
        out = T.median_filter_spectral(a, s, mode)
        assert out.dtype == np.float32 and out.shape == ref.shape
        assert np.array_equal(out, ref), (i, a.shape, s, mode)
        sizes.add((s, a.shape[0] < s))
    assert {1, 3, 4, 11, 15} <= {s for s, _ in sizes} and any(short for _, short in sizes)


def test_median_large_sizes_and_float64():
    rng = np.random.default_rng(3)
    a = rng.standard_normal((300, 5, 4))
    for s in (17, 32, 33, 63):
        out = T.median_filter_spectral(a, s)
        assert out.dtype == np.float64
        from scipy import ndimage                   # noqa: PLC0415
        assert np.array_equal(out, ndimage.median_filter(a.astype(np.float32), size=s, axes=[0])), s


@pytest.mark.parametrize("n", [1, 5, 30])
def test_nmf_fixed_iterations_match_sklearn(z, n):
    m = T.NMF(4, init="random", random_state=0, tol=0.0, max_iter=n)
    W = m.fit_transform(z["X"])
    assert W.dtype == np.float32 and m.n_iter_ == n
    tol = {1: 1e-5, 5: 1e-4, 30: 1e-3}[n]
    assert _rel(W, z[f"it{n}_W"]) < tol
    assert _rel(m.components_, z[f"it{n}_H"]) < tol
    assert abs(m.reconstruction_err_ - z[f"it{n}_err"]) / z[f"it{n}_err"] < tol


def test_nmf_default_run_matches_sklearn(z):
    m = T.NMF(4, init="random", random_state=0).fit(z["X"])
    n_ref, ratio = int(z["full_n_iter"]), z["full_ratio"]
    near = np.abs(ratio[max(n_ref - 2, 0):n_ref] - 1e-4).min() < 1e-6
    assert m.n_iter_ == n_ref or (near and abs(m.n_iter_ - n_ref) == 1), (m.n_iter_, n_ref)
    assert abs(m.reconstruction_err_ - z["full_err"]) / z["full_err"] < 1e-4
    assert m.components_.shape == (4, z["X"].shape[1]) and m.n_components_ == 4
    # the violation trace stops where sklearn's test does
    v = m.violation_
    assert len(v) == m.n_iter_ and v[-1] / v[0] <= 1e-4 and np.all(v[1:-1] / v[0] > 1e-4)


def test_nmf_float64_input_and_custom_init(z):
    X = z["X"].astype(np.float64)
    W0, H0 = T.init_random(X, 3, 7)
    m = T.NMF(3, init="custom", tol=0.0, max_iter=4)
    W = m.fit_transform(X, W=W0, H=H0)
    assert W.dtype == np.float64 and m.components_.dtype == np.float64
    m32 = T.NMF(3, init="random", random_state=7, tol=0.0, max_iter=4)
    W32 = m32.fit_transform(X.astype(np.float32))
    assert np.allclose(W, W32, rtol=1e-5, atol=1e-6)


def test_sweep_is_batch_independent_and_deterministic(z):
    X = z["X"]
    models, info = T.nmf_sweep(X, range(1, 7), random_state=0, max_iter=200, tol=1e-4)
    _, info2 = T.nmf_sweep(X, range(1, 7), random_state=0, max_iter=200, tol=1e-4)
    models2, _ = T.nmf_sweep(X, range(1, 7), random_state=0, max_iter=200, tol=1e-4)
    for a, b in zip(models, models2):
        assert np.array_equal(a.components_, b.components_) and np.array_equal(a._W, b._W)
    assert np.array_equal(info["error"], info2["error"]) and np.array_equal(info["n_iter"], info2["n_iter"])
    for k, m in zip(range(1, 7), models):
        one = T.NMF(k, init="random", random_state=0)
        W = one.fit_transform(X)
        assert one.n_iter_ == m.n_iter_, k
        assert np.array_equal(W, m._W) and np.array_equal(one.components_, m.components_), k
        assert one.reconstruction_err_ == m.reconstruction_err_, k
    # against sklearn's sweep: same errors (the runs that stop early stop where sklearn does, within a few iterations)
    assert np.allclose(info["error"], z["sweep_err"], rtol=2e-3)
    # the notebook's MRE
    for m, mre in zip(models, info["mre"]):
        R = X.astype(np.float64) - m._W.astype(np.float64) @ m.components_.astype(np.float64)
        ref = np.mean(np.divide(R, X, out=np.zeros_like(R), where=X != 0))
        assert abs(mre - ref) <= 1e-6 * max(1.0, abs(ref))


def test_sweep_across_a_tile_column_is_batch_independent(z):
    """K = 1..11 holds 66 components: the GEMMs (k_gemm_nt, k_gemm_tn) run a second tile column of 64 and the K = 11 model
    straddles it (components 55..65).  Every model equals its single-model run bit for bit, as templates.hip promises."""
    X = z["X"]
    ks = range(1, 12)
    assert sum(ks) == 66 and sum(range(1, 11)) < 64 < sum(ks)
    models, info = T.nmf_sweep(X, ks, random_state=0, max_iter=30, tol=0.0)
    for k, m, err, nit in zip(ks, models, info["error"], info["n_iter"]):
        one = T.NMF(k, init="random", random_state=0, max_iter=30, tol=0.0)
        W = one.fit_transform(X)
        assert one.n_iter_ == m.n_iter_ == nit == 30, k
        assert np.array_equal(W, m._W) and np.array_equal(one.components_, m.components_), k
        assert one.reconstruction_err_ == m.reconstruction_err_ == err, k


def test_sweep_across_a_tile_column_matches_sklearn(z):
    """The default sweep with 66 components in the batch against sklearn's errors: K = 1..6 of templates.npz and K = 7..11 of
    templates_edges.npz, at the rtol of test_sweep_is_batch_independent_and_deterministic."""
    from test_gpu_parity import note
    ze = np.load(GOLDEN_EDGES)
    ref = np.concatenate([z["sweep_err"], ze["sweep_err"]])
    assert list(z["sweep_k"]) + list(ze["sweep_k"]) == list(range(1, 12))
    _, info = T.nmf_sweep(z["X"], range(1, 12), random_state=0, max_iter=200, tol=1e-4)
    e = np.abs(info["error"] - ref) / ref
    note("nmf_sweep_66_components", worst=float(e.max()), at_k=int(np.argmax(e)) + 1, n_iter=[int(v) for v in info["n_iter"]])
    print("NMF sweep K = 1..11 against sklearn:", e, "n_iter", info["n_iter"], "sklearn", list(z["sweep_n_iter"]) + list(ze["sweep_n_iter"]))
    assert np.allclose(info["error"], ref, rtol=2e-3), e


@pytest.mark.parametrize("n", [1, 5])
def test_nmf_ragged_reduction_length_matches_sklearn(n):
    """97 x 650 with K = 5: 650 = 512 + 138 and 138 % 16 = 10, so the last K step of the reduction over the wavelengths is
    ragged (the ``k < k1`` guards), and 97 rows leave a ragged last step of the reduction over the pixels."""
    from test_gpu_parity import note
    ze = np.load(GOLDEN_EDGES)
    X = ze["Xr"]
    assert X.shape == (97, 650) and X.shape[1] % 16 == 10 and X.shape[0] % 16 == 1
    m = T.NMF(5, init="random", random_state=0, tol=0.0, max_iter=n)
    W = m.fit_transform(X)
    assert W.dtype == np.float32 and m.n_iter_ == n
    tol = {1: 1e-5, 5: 1e-4}[n]
    e = dict(W=_rel(W, ze[f"r_it{n}_W"]), H=_rel(m.components_, ze[f"r_it{n}_H"]),
             err=float(abs(m.reconstruction_err_ - ze[f"r_it{n}_err"]) / ze[f"r_it{n}_err"]))
    note("nmf_ragged", iterations=n, **e)
    print(f"NMF 97 x 650, K = 5, {n} iterations against sklearn:", e)
    assert max(e.values()) < tol, e


def test_recovers_exact_rank4_templates():
    d = synth.synthetic_template_cube(n_lambda=256, ny=23, nx=30, n_templates=4)
    X = T.cube_to_matrix(d["cube"])
    m = T.NMF(4, init="random", random_state=0, max_iter=1000, tol=1e-6)
    W = m.fit_transform(X)
    err = np.linalg.norm(X - W @ m.components_) / np.linalg.norm(X)
    assert err < 1e-3, err
    assert abs(m.reconstruction_err_ / np.linalg.norm(X.astype(np.float64)) - err) < 1e-5


@pytest.mark.parametrize("nt", [4, 6])
def test_make_templates_script_feeds_main_fusion(tmp_path, nt):
    out = tmp_path / "fusion"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "make_templates.py"), "--synthetic", "-o", str(out),
                        "-nt", str(nt), "--sweep", "1", "6", "--max_iter", "300"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import main_fusion                                   # noqa: PLC0415
    L = 256
    os.makedirs(out / "PSF", exist_ok=True)
    np.save(out / "PSF" / "psfs_pixscale0.025_npix_501_fov12.525_chan_1ABC_2ABC_3ABC_4ABC_SS4.npy",
            np.ones((L // 4, 3, 3)))
    paths, step, step_angle = main_fusion.initialize_parameters(str(out))
    _, _, wavel, tpl, _ = main_fusion.load_simulation_data(paths, step, step_angle, 8, nt)
    assert tpl.shape == (nt, L // 4) and wavel.shape == (L // 4,)
    sw = np.load(out / "Templates" / "sweep.npz")
    assert list(sw["n_components"]) == list(range(1, 7)) and np.all(np.isfinite(sw["error"]))


@pytest.mark.parametrize("P", [690, 4096])
def test_size_sweep_speed(P):
    L = 16384
    rng = np.random.default_rng(P)
    X = (rng.gamma(2.0, 1.0, (P, 6)) @ (1.0 + rng.random((6, L)))).astype(np.float32)
    t0 = time.perf_counter()
    models, info = T.nmf_sweep(X, range(1, 12), random_state=0, max_iter=200, tol=0.0)
    wall = time.perf_counter() - t0
    ms = info["ms_per_iter"]
    n_k = sum(range(1, 12))
    # per iteration: X is read by X Hcat^T and by Wcat^T X
    gbs = 2 * X.nbytes / (ms * 1e-3) / 1e9
    print(f"\nNMF sweep K=1..11, P={P}, L={L}: {ms:.3f} ms per iteration ({n_k} components), "
          f"{gbs:.0f} GB/s effective over X, wall {wall:.2f} s for 200 iterations")
    assert np.all(info["n_iter"] == 200) and np.all(np.isfinite(info["error"]))
