"""Float64 numpy restatement of seminmf.m (Ding, Li & Jordan's semi-NMF) and of the deterministic k-means that gives its default H_init.

Nothing in the package imports this file: it is the parity oracle of tests/golden/make_seminmf_golden.py and of the tests.  The W step solves
with a Cholesky factor of H*H', so that it refuses exactly what the device refuses (a pivot <= 0 or not finite).

k-means (the restatement libnmfx's nmfx_kmeans implements; MATLAB's own random stream cannot be reproduced):
  seeding     k-means++ on the columns of X from k host uniforms u: the first centre is floor(u[0]*n); centre j is the first index at which the
              running sum of D^2 (64-point chunks summed in order, the chunk totals accumulated in order, then the points of the chunk in order)
              exceeds u[j]*sum(D^2).  D^2 is sum_i (x_i - c_i)^2 accumulated over i in order.
  assignment  squared Euclidean distance in the form |x|^2 + |c|^2 - 2 c'x; the first assignment takes the lowest index on ties, later ones move a
              point only if the new centre is strictly closer than its own.
  update      centroids = X*E' ./ counts (E the indicator matrix), batch Lloyd iterations only; the total distance is checked before every reassignment:
              if it did not decrease the previous assignment is restored and the loop ends (a rounding guard: in exact arithmetic the total
              strictly decreases after any move, so only floating-point error can make it fire).
  empty       every empty cluster, in index order, takes the point farthest from its own centroid (among clusters of two or more points; the
              lowest index on ties) as a singleton, then all centroids are recomputed.
"""
import numpy as np

CHUNK = 64


class SeminmfError(ValueError):
    pass


def _dist2_col(X, c):
    d = np.zeros(X.shape[1])
    for i in range(X.shape[0]):
        t = X[i] - c[i]
        d = d + t * t
    return d


def _chunk_pick(D2, u):
    n = D2.shape[0]
    nc = (n + CHUNK - 1) // CHUNK
    sums = np.zeros(nc)
    for b in range(nc):
        s = 0.0
        for x in D2[b * CHUNK:(b + 1) * CHUNK]:
            s = s + x
        sums[b] = s
    total = 0.0
    for s in sums:
        total = total + s
    if not total > 0.0:
        raise SeminmfError("kmeans: fewer distinct points than clusters (sum of D^2 is 0 during seeding)")
    t = u * total
    run = 0.0
    for b in range(nc):
        if run + sums[b] > t:
            for j in range(b * CHUNK, min((b + 1) * CHUNK, n)):
                run = run + D2[j]
                if run > t:
                    return j
            return min((b + 1) * CHUNK, n) - 1
        run = run + sums[b]
    return n - 1   # (u*total rounded up to total: the last point)


def _centroids(X, labels, k):
    E = np.zeros((k, X.shape[1]))
    E[labels, np.arange(X.shape[1])] = 1.0
    counts = E.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        C = (X @ E.T) / counts
    return C, counts.astype(np.int64)


def kmeans(X, k, u, maxiter=100, trace=None):
    """labels (0-based), centroids (m x k), Lloyd iterations of the deterministic k-means above on the columns of X.  trace (a dict, optional)
    counts the events of the rarer branches: 'empty' (clusters refilled by the singleton rule), 'moves' (points moved), 'revert' (restores)"""
    trace = {} if trace is None else trace
    for key in ("empty", "moves", "revert"):
        trace.setdefault(key, 0)
    X = np.asarray(X, dtype=np.float64)
    m, n = X.shape
    if n < k:
        raise SeminmfError("kmeans: %d points for %d clusters" % (n, k))
    centres = [min(int(np.floor(u[0] * n)), n - 1)]
    D2 = _dist2_col(X, X[:, centres[0]])
    for j in range(1, k):
        c = _chunk_pick(D2, u[j])
        centres.append(c)
        D2 = np.minimum(D2, _dist2_col(X, X[:, c]))
    xx = np.sum(X * X, axis=0)
    C = X[:, centres]
    d = xx + np.sum(C * C, axis=0)[:, None] - 2.0 * (C.T @ X)
    labels = np.argmin(d, axis=0)
    prev, prev_total, it = None, np.inf, 0
    while True:
        it += 1
        C, counts = _centroids(X, labels, k)
        if np.any(counts == 0):
            own = xx + np.sum(C * C, axis=0)[labels] - 2.0 * np.sum(C[:, labels] * X, axis=0)
            for c in np.nonzero(counts == 0)[0]:
                trace["empty"] += 1
                cand = np.where(counts[labels] >= 2, own, -np.inf)
                j = int(np.argmax(cand))
                counts[labels[j]] -= 1
                labels[j] = c
                counts[c] = 1
                own[j] = 0.0
            C, counts = _centroids(X, labels, k)
        d = xx + np.sum(C * C, axis=0)[:, None] - 2.0 * (C.T @ X)
        total = float(np.sum(d[labels, np.arange(n)]))
        if prev_total <= total:
            trace["revert"] += 1
            labels, it = prev, it - 1
            C, _ = _centroids(X, labels, k)
            break
        if it >= maxiter:
            break
        best = np.argmin(d, axis=0)
        move = d[best, np.arange(n)] < d[labels, np.arange(n)]
        if not np.any(move):
            break
        trace["moves"] += int(np.sum(move))
        prev, prev_total = labels.copy(), total
        labels = np.where(move, best, labels)
    return labels, C, it


def default_H(labels, k):
    """seminmf.m:109-117: the indicator matrix of the clusters plus 0.2"""
    H = np.zeros((k, labels.shape[0]))
    H[labels, np.arange(labels.shape[0])] = 1.0
    return H + 0.2


def _solve_right(N, A, it):
    """N * inv(A) through the Cholesky factor of A (seminmf.m:68, W = V*H'/(H*H')); a pivot <= 0 or not finite is the error the device raises"""
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        raise SeminmfError("seminmf: H*H' is not positive definite at iteration %d" % it)
    if not np.all(np.isfinite(L)) or not np.all(np.diag(L) > 0):
        raise SeminmfError("seminmf: H*H' is not positive definite at iteration %d" % it)
    Y = np.linalg.solve(L, N.T)
    return np.linalg.solve(L.T, Y).T


def seminmf(V, K, config):
    """W, H, cost of seminmf.m:65-89 with config holding W_init, H_init (required here), W_fixed, H_fixed, maxiter, tolerance (< 0: no stop rule)"""
    V = np.asarray(V, dtype=np.float64)
    W = np.array(config["W_init"], dtype=np.float64)
    H = np.array(config["H_init"], dtype=np.float64)
    maxiter = int(config.get("maxiter", 100))
    tol = float(config.get("tolerance", 1e-3))
    wf, hf = bool(config.get("W_fixed", False)), bool(config.get("H_fixed", False))
    cost = np.zeros(maxiter)
    for it in range(maxiter):
        if not wf:
            W = _solve_right(V @ H.T, H @ H.T, it + 1)
        if not hf:
            B = W.T @ V
            Cg = W.T @ W
            Bp, Bn = np.maximum(B, 0.0), np.maximum(-B, 0.0)
            Cp, Cn = np.maximum(Cg, 0.0), np.maximum(-Cg, 0.0)
            with np.errstate(invalid="ignore", divide="ignore"):
                H = H * np.sqrt((Bp + Cn @ H) / (Bn + Cp @ H))
        R = V - W @ H
        cost[it] = 0.5 * np.sum(R * R)
        if tol >= 0 and it > 0 and cost[it] < cost[it - 1] and cost[it - 1] - cost[it] < tol:
            return W, H, cost[: it + 1]
    return W, H, cost
