"""Host restatements of the exponential modified-Shepard kernel (surfh/ToolsDir/shepard_interpolation.pyx:78-141) for the
tests of surfh_amd.preprocessing: a NumPy float32 replica of the reference's pair test (which samples each query point
uses, bit for bit) and a float64 checker of the weighted mean over a given neighbour set."""
from __future__ import annotations

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shepard.npz")
f32, f64 = np.float32, np.float64


def inv_res(res):
    return f32(1.0 / f64(f32(res)))


def pair_distance(a, l, qa, ql, alpha_res, lambda_res, epsilon=1e-6):
    """[n_query, n_samples] distances as the reference forms them: float32 differences, products, squares, sum and
    sqrt, then + epsilon as a double (both are Python floats there)."""
    a, l = np.asarray(a, f32).ravel(), np.asarray(l, f32).ravel()
    qa, ql = np.asarray(qa, f32).ravel(), np.asarray(ql, f32).ravel()
    ia, il = inv_res(alpha_res), inv_res(lambda_res)
    with np.errstate(invalid="ignore", over="ignore"):       # non-finite coordinates give inf or NaN: no neighbour
        d1 = (a[None, :] - qa[:, None]) * ia
        d2 = (l[None, :] - ql[:, None]) * il
        d = np.sqrt(d1 * d1 + d2 * d2)
        return d.astype(f64) + f64(f32(epsilon))


def neighbour_mask(a, l, qa, ql, alpha_res, lambda_res, pixel_cutoff, epsilon=1e-6):
    """[n_query, n_samples] bool: the samples the reference uses for each query point."""
    return pair_distance(a, l, qa, ql, alpha_res, lambda_res, epsilon) <= f64(f32(pixel_cutoff))


def replica(a, l, v, qa, ql, p, pixel_cutoff, alpha_res, lambda_res, alpha=2.0, epsilon=1e-6):
    """float32 replica: (out [n_query] float64 sums of the float32 weights, neighbour counts)."""
    dist = pair_distance(a, l, qa, ql, alpha_res, lambda_res, epsilon)
    m = dist <= f64(f32(pixel_cutoff))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        df = dist.astype(f32).astype(f64)
        value = (-f64(f32(alpha)) * np.exp(f64(f32(p)) * np.log(df))).astype(f32)
        w = np.where(m, np.exp(value.astype(f64)).astype(f32).astype(f64), 0.0)
        num = _masked_sum(w, v, m)
        den = w.sum(axis=1)
        out = np.where(den != 0, num / np.where(den != 0, den, 1.0), 0.0)
    return out, m.sum(axis=1)


def _masked_sum(w, v, m):
    """sum over the neighbours only: a NaN or infinite value outside the cutoff takes no part, as in the reference
    (0 * NaN inside a matrix product would spread it to every query point)."""
    return np.where(m, w * np.asarray(v, f32).astype(f64).ravel()[None, :], 0.0).sum(axis=1)


def checker(a, l, v, qa, ql, mask, p, pixel_cutoff, alpha_res, lambda_res, alpha=2.0, epsilon=1e-6):
    """float64 brute force over the neighbour set ``mask`` (from ``neighbour_mask``): sum w v / sum w, w = exp(-alpha d^p)."""
    a, l, qa, ql = (np.asarray(x, f32).astype(f64).ravel() for x in (a, l, qa, ql))
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.hypot((a[None, :] - qa[:, None]) / f64(f32(alpha_res)),
                     (l[None, :] - ql[:, None]) / f64(f32(lambda_res))) + epsilon
        w = np.where(mask, np.exp(-alpha * d ** p), 0.0)
        den = w.sum(axis=1)
        num = _masked_sum(w, v, mask)
        return np.where(den != 0, num / np.where(den != 0, den, 1.0), 0.0)


def kernel_cases(z):
    """The direct kernel cases of the fixture: dicts with a, l, v, ga, gl (2-D meshes), p, cutoff, ares, lres, out."""
    cases = []
    for i in range(int(z["n_kernel_cases"])):
        p, cut, ares, lres = (float(x) for x in z[f"k{i}_par"])
        cases.append(dict(a=z[f"k{i}_a"], l=z[f"k{i}_l"], v=z[f"k{i}_v"], ga=z[f"k{i}_ga"], gl=z[f"k{i}_gl"], p=p,
                          cutoff=cut, ares=ares, lres=lres, out=z[f"k{i}_out"]))
    return cases


class ChannelShape:
    """Stand-in for a model channel: the correction only reads ``oshape``."""

    def __init__(self, oshape):
        self.oshape = tuple(int(s) for s in oshape)
