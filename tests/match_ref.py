"""numpy restatement of sfmba_match_descriptors (include/sfmba.h), written for this project: the full distance matrix in
int64 for integer input and fp64 otherwise, the candidates of a query ordered by (d^2, train index), the ratio rule and
the statuses of the header.  Also the generators of the fixtures that the host and the GPU tests share."""
import os
import re

import numpy as np

from conftest import ROOT

OK, FEW = 0, 1


def match_constant(name):
    src = open(os.path.join(ROOT, "sfm-python_amd", "csrc", "match_kernels.hpp")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


def dist_sq_matrix(q, t):
    """(nq, nt) squared L2 distances: exact int64 for integer dtypes, else sum (a - b)^2 in fp64."""
    q, t = np.asarray(q), np.asarray(t)
    if np.issubdtype(q.dtype, np.integer) and np.issubdtype(t.dtype, np.integer):
        q, t = q.astype(np.int64), t.astype(np.int64)
        return (q * q).sum(1)[:, None] + (t * t).sum(1)[None, :] - 2 * (q @ t.T)
    q, t = q.astype(np.float64), t.astype(np.float64)
    out = np.empty((len(q), len(t)))
    with np.errstate(all="ignore"):
        for i in range(len(q)):
            out[i] = ((t - q[i]) ** 2).sum(1)
    return out


def match_edge(q, t, ratio=0.5, depth=2):
    """One edge -> dict(idx (nq, depth) int32, dist_sq (nq, depth) float64, good (nq) bool, status).  depth > 2 returns
    further neighbours (the contested-query test looks at the third)."""
    q, t = np.asarray(q), np.asarray(t)
    nq, nt = len(q), len(t)
    idx = np.full((nq, depth), -1, dtype=np.int32)
    dist = np.full((nq, depth), np.inf)
    good = np.zeros(nq, dtype=bool)
    if nq < 1 or nt < 2:
        return dict(idx=idx, dist_sq=dist, good=good, status=FEW)
    d = dist_sq_matrix(q, t).astype(np.float64)          # (integers below 2^53: exact)
    d[~np.isfinite(d)] = np.inf
    order = np.argsort(d, axis=1, kind="stable")[:, :depth]              # stable: the lower index first among equals
    for k in range(order.shape[1]):
        dk = d[np.arange(nq), order[:, k]]
        have = np.isfinite(dk)
        idx[have, k] = order[have, k]
        dist[have, k] = dk[have]
    r2 = np.float64(ratio) * np.float64(ratio)
    good = (idx[:, 0] >= 0) & (idx[:, 1] >= 0) & (dist[:, 0] < r2 * dist[:, 1])
    return dict(idx=idx, dist_sq=dist, good=good, status=OK)


def match_batch(descs, edges, ratio=0.5):
    """The whole call -> dict(query_ptr, idx, dist_sq, good, edge_good, edge_status, n_ok)."""
    res = [match_edge(descs[u], descs[v], ratio) for u, v in edges]
    ptr = np.concatenate([[0], np.cumsum([len(descs[u]) for u, _ in edges])]).astype(np.int64)
    cat = lambda key, shape, dt: (np.concatenate([r[key] for r in res]) if res else np.empty(shape, dtype=dt))
    status = np.array([r["status"] for r in res], dtype=np.int32)
    return dict(query_ptr=ptr, idx=cat("idx", (0, 2), np.int32), dist_sq=cat("dist_sq", (0, 2), np.float64),
                good=cat("good", (0,), bool), edge_good=np.array([int(r["good"].sum()) for r in res], dtype=np.int32),
                edge_status=status, n_ok=int((status == OK).sum()))


def good_pairs(q, t, ratio=0.5):
    """The reference's good_pairs (sfm.py:96) of one edge."""
    r = match_edge(q, t, ratio)
    k = np.flatnonzero(r["good"])
    return np.stack([k, r["idx"][k, 0]], axis=1).astype(int)


# ---- fixtures of form B -------------------------------------------------------------------------------------------------
FORM_B_SHAPES = ((128, 300, 517), (40, 130, 257), (256, 67, 1030))      # (D, n_query, n_train)
FORM_B_SEED = 0
CONTESTED_CAP = 0.05


def rootsift_rows(rng, n, D):
    """Unit-norm RootSIFT-like rows: squares of Gaussians, L1-normalised, then the square root."""
    x = rng.standard_normal((n, D)) ** 2
    return np.sqrt(x / x.sum(1, keepdims=True))


def form_b_fixture(D, nq, nt, seed=FORM_B_SEED):
    """(query, train) float32: half the queries are a train row plus 0.02 x Gaussian noise."""
    rng = np.random.default_rng([seed, D, nq, nt])
    train = rootsift_rows(rng, nt, D)
    query = rootsift_rows(rng, nq, D)
    near = np.arange(nq) % 2 == 0
    query[near] = train[rng.integers(0, nt, size=int(near.sum()))] + 0.02 * rng.standard_normal((int(near.sum()), D))
    return query.astype(np.float32), train.astype(np.float32)


def contested(q, t, ratio=0.5):
    """Queries whose result the fp32 dot product may decide differently: in the fp64 reference d2 - d1, d3 - d2 or
    |d1 - ratio^2 d2| is below tau = 4 D 2^-24 |q| max|t|, twice the bound 2 D u |a| |b| on the error of
    |a|^2 + |b|^2 - 2 fl32(a.b) with a dot product of length D summed in fp32 in any order."""
    q, t = np.asarray(q, dtype=np.float64), np.asarray(t, dtype=np.float64)
    D = q.shape[1]
    r = match_edge(q, t, ratio, depth=3)
    d = r["dist_sq"]
    tn = np.linalg.norm(t, axis=1)
    tau = 4.0 * D * 2.0 ** -24 * np.linalg.norm(q, axis=1) * tn[np.isfinite(tn)].max()
    r2 = ratio * ratio
    with np.errstate(invalid="ignore"):
        return (d[:, 1] - d[:, 0] < tau) | (d[:, 2] - d[:, 1] < tau) | (np.abs(d[:, 0] - r2 * d[:, 1]) < tau)
