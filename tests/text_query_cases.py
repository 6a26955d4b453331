"""The numpy statement of DESIGN.md 8t (text queries on scene features) and seeded case builders for its tests.

Scores are stated in fp64 from the stored values; everything after step 1 (statistics, thresholds, selection, best) is stated on a
GIVEN fp32 score array, because the definition decides the selection on the device's own fp32 scores."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text_query.npz")
U = 2.0 ** -24


def score_tolerance(D):
    """|s - ref| of an fp32 dot product with a unit vector in any order, plus the norm and the division"""
    return (1.5 * D + 4) * U


def unit_rows(T):
    T = np.asarray(T, dtype=np.float64)
    n = np.sqrt((T * T).sum(axis=1, keepdims=True))
    return (T / np.maximum(n, 1e-12)).astype(np.float32)


def scores_fp64(X, T, valid=None):
    """step 1 in fp64: X (N, D) stored values, T (Q, D) -> (Q, N) fp64 with -inf in dead rows, and the live mask (N,)"""
    X = np.asarray(X, dtype=np.float64)
    t_hat = unit_rows(T).astype(np.float64)
    with np.errstate(all="ignore"):
        n = np.sqrt((X * X).sum(axis=1))
        s = (t_hat @ X.T) / np.maximum(n, 1e-12)
        live = (n != 0) & np.isfinite(s).all(axis=0)
    if valid is not None:
        live &= np.asarray(valid) != 0
    s = np.where(live[None], s, -np.inf)
    s[s == 0] = 0.0
    return s, live


def statistics(scores):
    """step 2: (Q, N) fp32 -> (Q, 3) fp64 {L, sum s, sum s^2} over the live rows"""
    scores = np.asarray(scores, dtype=np.float32)
    out = np.zeros((scores.shape[0], 3))
    for q, s in enumerate(scores):
        v = s[s > -np.inf].astype(np.float64)
        out[q] = (len(v), v.sum(), (v * v).sum())
    return out


def adaptive_threshold(stats, kappa=2.0, floor=0.0):
    """step 3 in fp64, rounded to fp32; +inf where there is no live row"""
    tau = np.full(len(stats), np.inf, dtype=np.float32)
    for q, (L, s1, s2) in enumerate(np.asarray(stats, dtype=np.float64)):
        if L > 0:
            mu = s1 / L
            tau[q] = np.float32(max(mu + kappa * np.sqrt(max(s2 / L - mu * mu, 0.0)), floor))
    return tau


def best_m(s, rows, m):
    """the m best of `rows` by the fp32 scores s: descending score, the lower row first, -0.0 as +0.0 -> ascending rows"""
    rows = np.asarray(rows, dtype=np.int64)
    v = s[rows].astype(np.float64) + 0.0                                # (-0.0 + 0.0 = +0.0)
    order = np.lexsort((rows, -v))[:max(int(m), 0)]
    return np.sort(rows[order])


def select(s, tau, m):
    """steps 4 and 5 for one query on its fp32 score row s: tau fp32 (-inf: no threshold), m (negative: no cap)
    -> (ascending rows int32, tau_out fp32): tau_out = tau, but the score of the last row kept when the cap binds (m < |S|) or when
    there is no threshold and m >= 0; +inf when nothing is kept then"""
    s = np.asarray(s, dtype=np.float32)
    tau = np.float32(tau)
    cand = np.nonzero((s > -np.inf) & (s >= tau))[0]
    if m < 0:
        return cand.astype(np.int32), tau
    kept = best_m(s, cand, m)
    if m < len(cand) or tau == -np.inf:
        tau = np.float32(s[kept].min() + np.float32(0.0)) if len(kept) else np.float32(np.inf)
    return kept.astype(np.int32), tau


def best_query(scores, selections):
    """step 5: per row the selecting query of highest score (the lowest q among equals), -1 when none"""
    Q, N = scores.shape
    best = np.full(N, -1, dtype=np.int32)
    top = np.full(N, -np.inf)
    for q in range(Q):
        rows = np.asarray(selections[q], dtype=np.int64)
        v = scores[q, rows].astype(np.float64)
        win = (best[rows] < 0) | (v > top[rows])
        best[rows[win]] = q
        top[rows[win]] = v[win]
    return best


def query(scores, method="threshold", threshold=0.15, k=None, kappa=2.0, floor=0.0, max_points=None):
    """query_scene after its score pass, on a given (Q, N) fp32 score array -> dict(indices, counts, thresholds, best, num_live)"""
    scores = np.asarray(scores, dtype=np.float32)
    Q = scores.shape[0]
    stats = statistics(scores)
    if method == "threshold":
        tau = np.full(Q, np.float32(threshold), dtype=np.float32)
    elif method == "adaptive":
        tau = adaptive_threshold(stats, kappa, floor)
    else:
        tau = np.full(Q, -np.inf, dtype=np.float32)
    cap = k if method == "topk" else (-1 if max_points is None else max_points)
    if method == "topk" and max_points is not None:
        cap = min(cap, max_points)
    picked = [select(scores[q], tau[q], cap) for q in range(Q)]
    indices = [p[0] for p in picked]
    return dict(indices=indices, counts=np.array([len(i) for i in indices], dtype=np.int64),
                thresholds=np.array([p[1] for p in picked], dtype=np.float32), best=best_query(scores, indices),
                num_live=int(stats[0, 0]))


# ---- seeded case builders -----------------------------------------------------------------------------------------------------------
def uniform_case(n, d, q, seed):
    """features and embeddings uniform in [-1, 1): X (n, d) fp32, T (q, d) fp32"""
    g = np.random.RandomState(seed)
    return (g.rand(n, d) * 2.0 - 1.0).astype(np.float32), (g.rand(q, d) * 2.0 - 1.0).astype(np.float32)


def dead_rows(n, block):
    """rows 0 and n - 1 and the two rows on either side of every `block` edge below n"""
    rows = {0, n - 1}
    for e in range(block, n, block):
        rows.update((e - 1, e))
    return sorted(r for r in rows if 0 <= r < n)


TIE_VALUES = np.array([-0.5, -0.0, 0.0, 0.25, 0.5], dtype=np.float32)


def tie_scores(q, n, seed, dead_fraction=0.1):
    """(q, n) fp32 drawn from TIE_VALUES (long runs of equal keys), some rows dead (-inf) in every query"""
    g = np.random.RandomState(seed)
    s = TIE_VALUES[g.randint(0, len(TIE_VALUES), (q, n))]
    dead = g.rand(n) < dead_fraction
    s[:, dead] = -np.inf
    return s


def exact_scores(q, n, seed):
    """(q, n) fp32 multiples of 2^-10 in [-1, 1]: every fp64 sum of them and of their squares is exact in any order"""
    g = np.random.RandomState(seed)
    return (g.randint(-1024, 1025, (q, n)) / 1024.0).astype(np.float32)


def fixture_features(embeddings, n=600, noise=0.6, seed=20):
    """n rows, each a (unit) class embedding plus Gaussian noise of length ~noise, stored fp16 -> (features fp16 (n, D), class id (n,))"""
    g = np.random.RandomState(seed)
    emb = unit_rows(embeddings).astype(np.float64)
    cls = g.randint(0, emb.shape[0], n)
    x = emb[cls] + (noise / np.sqrt(emb.shape[1])) * g.randn(n, emb.shape[1])
    return x.astype(np.float16), cls.astype(np.int32)
