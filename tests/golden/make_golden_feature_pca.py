"""Writes tests/golden/feature_pca.npz: what the reference's own apply_pca_to_features (tools/visualize_features_pca.py, scikit-learn's
PCA) gives on the seeded feature matrices of tests/feature_pca_cases.py.  Run on the CPU:

    python tests/golden/make_golden_feature_pca.py <path of the reference tree>

Per case: the SHA-256 and the first 8 rows of the inputs (the matrices are drawn again from their seeds by the tests: they would not
fit the size limit of a committed file), the reference's colours (fp32), components and explained-variance ratio, and the distance of
the numpy restatement (feature_pca_cases.restated) to the reference.  Only data is written; no reference source.

It refuses to write unless, in every case, the first four eigenvalues are a relative 2 % apart and the restatement's colours are within
2e-4 of the reference's: the reference alone is then far inside the 1 / 510 the device result is allowed."""
import contextlib
import hashlib
import importlib.util
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import feature_pca_cases as fc  # noqa: E402


def load_reference(ref):
    spec = importlib.util.spec_from_file_location("ref_visualize_features_pca", os.path.join(ref, "tools", "visualize_features_pca.py"))
    mod = importlib.util.module_from_spec(spec)
    with contextlib.redirect_stdout(io.StringIO()):
        spec.loader.exec_module(mod)
    assert mod.HAS_SKLEARN, "scikit-learn is needed to run the reference"
    return mod


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = load_reference(sys.argv[1])
    out = {}
    for case, spec in fc.CASES.items():
        x = fc.features(case)
        with contextlib.redirect_stdout(io.StringIO()):
            r = ref.apply_pca_to_features(x, n_components=spec["k"])
        mine = fc.restated(x, spec["k"])
        ev = mine["eigenvalues"][:4]
        gap = float(np.min((ev[:-1] - ev[1:]) / ev[:-1]))
        d_col = float(np.abs(mine["colors"] - r["colors"]).max())
        d_comp = float(np.abs(mine["components"] - r["pca_model"].components_).max())
        d_ratio = float(np.abs(mine["explained_variance_ratio"] / r["explained_variance"] - 1.0).max())
        mean_over_spread = float(np.linalg.norm(mine["mean"]) / np.sqrt(mine["eigenvalues"].sum()))
        print(f"{case}: {x.shape} {x.dtype} k = {spec['k']}, eigenvalue gap {gap:.3g}, |mean| / spread {mean_over_spread:.3g}, restatement "
              f"vs reference: colours {d_col:.3g}, components {d_comp:.3g}, ratio (relative) {d_ratio:.3g}")
        assert gap >= fc.MIN_EIGEN_GAP, (case, gap)
        assert d_col <= fc.MAX_RESTATEMENT_DISTANCE, (case, d_col)
        if spec["common"]:
            assert mean_over_spread >= spec["common"] * 0.9, (case, mean_over_spread)
        out.update({f"{case}.sha256": hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest(), f"{case}.head": x[:8],
                    f"{case}.colors": r["colors"].astype(np.float32), f"{case}.components": np.asarray(r["pca_model"].components_, np.float64),
                    f"{case}.ratio": np.asarray(r["explained_variance"], np.float64),
                    f"{case}.restatement_distance": np.array([d_col, d_comp, d_ratio])})
    np.savez_compressed(fc.GOLDEN, **out)
    size = os.path.getsize(fc.GOLDEN)
    print(f"{fc.GOLDEN}: {size} bytes")
    assert size < 1 << 20


if __name__ == "__main__":
    main()
