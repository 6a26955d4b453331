"""Seeded feature matrices for the PCA-colour tests and the numpy fp64 restatement of DESIGN.md 8r (steps 1-6).  No scikit-learn here:
what the reference's apply_pca_to_features gave on these inputs is recorded in tests/golden/feature_pca.npz.

The inputs themselves are not in the golden file (8000 x 96 fp32 alone is 3 MB): they are drawn again from the seeds below with
numpy's frozen RandomState streams and elementwise arithmetic only (no reduction whose order a BLAS or a SIMD width could change), and
the golden file holds their SHA-256, which `features` checks."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "feature_pca.npz")

CENTRES = 6
WEIGHTS = (0.30, 0.24, 0.18, 0.13, 0.09, 0.06)       # unequal clusters: the between-cluster eigenvalues are apart
NOISE = 0.35                                          # length of the noise added to a unit centre, before the row is normalised
# common: length of a vector added to every row before the normalisation, in units of the spread (sqrt(trace C)) of the plain rows
CASES = {
    "f32": dict(n=8000, d=96, k=3, dtype="float32", seed=11, common=0.0),
    "f16": dict(n=8000, d=96, k=3, dtype="float16", seed=12, common=0.0),
    "k1": dict(n=3000, d=64, k=1, dtype="float32", seed=13, common=0.0),
    "k2": dict(n=3000, d=64, k=2, dtype="float32", seed=14, common=0.0),
    "mean10": dict(n=4000, d=96, k=3, dtype="float32", seed=15, common=10.0),
}
MIN_EIGEN_GAP = 0.02          # relative, between the first four eigenvalues
MAX_RESTATEMENT_DISTANCE = 2e-4


def _unit_rows(v):
    sq = np.zeros(v.shape[0])
    for j in range(v.shape[1]):                       # column by column: the order of the sum is fixed
        sq += v[:, j] * v[:, j]
    return v / np.sqrt(sq)[:, None]


def clustered(n, d, seed, common=0.0):
    """(n, d) fp64: six unit centres, a centre per row by WEIGHTS, Gaussian noise of length ~NOISE, [a common vector,] unit rows"""
    g = np.random.RandomState(seed)
    centres = _unit_rows(g.randn(CENTRES, d))
    lab = np.searchsorted(np.cumsum(WEIGHTS)[:-1], g.rand(n))
    v = _unit_rows(centres[lab] + (NOISE / np.sqrt(d)) * g.randn(n, d))
    if common:
        u = _unit_rows(g.randn(1, d))[0]
        spread = np.sqrt(1.0 - 1.0 / CENTRES)         # a nominal spread of unit rows around their mean; fixed, not measured
        v = _unit_rows(v + common * spread * u)
    return v


def features(case, digest=None):
    """the case's feature matrix in its dtype; digest: the recorded SHA-256 (hex) it must reproduce"""
    spec = CASES[case]
    x = clustered(spec["n"], spec["d"], spec["seed"], spec["common"]).astype(spec["dtype"])
    if digest is not None:
        got = hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()
        assert got == str(digest), f"{case}: the seeded inputs are not the recorded ones ({got} != {digest})"
    return x


def sign_fixed(components):
    """in each row the entry of largest magnitude is made positive; equal magnitudes: the lowest index decides"""
    out = np.array(components, dtype=np.float64, copy=True)
    for row in out:
        if row[int(np.argmax(np.abs(row)))] < 0:
            row *= -1.0
    return out


def colours_from_projection(Y):
    """step 6 in the dtype of Y"""
    Y = np.asarray(Y)
    mn = Y.min(axis=0)
    r = Y.max(axis=0) - mn
    r[r == 0] = 1
    P = np.clip((Y - mn) / r, 0, 1)
    k = Y.shape[1]
    if k == 1:
        return np.repeat(P, 3, axis=1)
    if k == 2:
        return np.column_stack([P, np.full(len(P), 0.5, dtype=P.dtype)])
    return P


def restated(X, k):
    """steps 1-6 in fp64 -> dict(colors, pca_features, components, mean, explained_variance, explained_variance_ratio, eigenvalues).
    The covariance is formed from the centred rows: algebraically (X^T X - n m m^T) / (n - 1), without its cancellation."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    m = X.mean(axis=0)
    Xc = X - m
    C = Xc.T @ Xc / (n - 1)
    w, v = np.linalg.eigh(C)
    order = np.argsort(-w, kind="stable")
    components = sign_fixed(v[:, order[:k]].T)
    Y = Xc @ components.T
    return dict(colors=colours_from_projection(Y), pca_features=Y, components=components, mean=m, explained_variance=w[order[:k]],
                explained_variance_ratio=w[order[:k]] / np.trace(C), eigenvalues=w[order])


# ---- kernel-level inputs ----------------------------------------------------------------------------------------------------------
def integer_rows(n, d, seed):
    """integers in [-4, 4] (exact in fp32, fp16 and bf16) and an integer shift in [-2, 2]"""
    g = np.random.RandomState(seed)
    return g.randint(-4, 5, (n, d)).astype(np.int64), g.randint(-2, 3, d).astype(np.int64)


def uniform_rows(n, d, seed):
    return (np.random.RandomState(seed).rand(n, d) * 2.0 - 1.0).astype(np.float32)
