"""Generate tests/golden/shepard_edges.npz: the REAL reference's ``exponential_modified_shepard`` on the edge cases of
tests/shepard_cases.py (``fixture_cases``: non-finite samples and query points, parameters outside shepard.npz's,
lattice distances against cutoffs one ulp apart, samples on cell edges, sparse clusters, dense cells).

Run only in the build container:   python tests/golden/make_golden_shepard_edges.py
The reference's kernel is compiled as in make_golden_shepard.py (into the git-ignored oracle/_ref/, gcc -O3).  Only
arrays are written: per case ``<name>__a, l, v, ga, gl`` (float32 inputs), ``<name>__par`` (p, alpha, cutoff, epsilon,
alpha_res, lambda_res) and ``<name>__out`` (the reference's output), plus ``names`` and ``raised`` (the cases on which
the reference raised, left to the replica; none did)."""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import make_golden_shepard as mg  # noqa: E402
import shepard_cases as sc  # noqa: E402
import shepard_oracle as so  # noqa: E402


def main():
    _, shep, _ = mg.load_reference()
    out = {"meta": json.dumps(dict(mg.META, functions=mg.META["functions"][:1]))}
    names, raised = [], []
    for name, c in sc.fixture_cases(np.load(so.GOLDEN)).items():
        try:
            with np.errstate(all="ignore"):
                r = shep.exponential_modified_shepard(c["a"], c["l"], c["v"], c["ga"], c["gl"], p=c["p"],
                                                      alpha=c["alpha"], pixel_cutoff=c["cutoff"], alpha_res=c["ares"],
                                                      lambda_res=c["lres"], epsilon=c["eps"])
        except Exception as e:  # noqa: BLE001   the case is then left to the replica
            print(f"{name}: the reference raised {e!r}")
            raised.append(name)
            continue
        names.append(name)
        out.update({f"{name}__{k}": c[k] for k in ("a", "l", "v", "ga", "gl")})
        out[f"{name}__par"] = np.array([c[k] for k in sc.PAR])
        out[f"{name}__out"] = np.asarray(r, dtype=np.float32)
    out["names"], out["raised"] = np.array(names), np.array(raised, dtype="U1")
    np.savez_compressed(sc.GOLDEN_EDGES, **out)
    print(sc.GOLDEN_EDGES, os.path.getsize(sc.GOLDEN_EDGES), "bytes,", len(names), "cases")


if __name__ == "__main__":
    main()
