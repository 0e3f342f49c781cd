"""numpy fp64 restatement of Spark's NNLS solver and of the nonnegative ALS fit built on it
(K13) — test infrastructure only.

nnls_solve restates org.apache.spark.mllib.optimization.NNLS.solve statement by statement
(projected gradient with conjugate-gradient directions, the sequential wall clamp, the
stopping tests and iterMax = max(400, 20 k)); the normal equations, the lambda * n
regularisation, the implicit YtY merge and the sweep order are oracle.als_oracle's, because
Spark's `nonnegative` only swaps the per-row solver.
"""
import numpy as np

from oracle import als_oracle as O


def nnls_solve(A, b, info=None):
    """Spark's NNLS.solve(ata, atb) in fp64: the x >= 0 minimising x^T A x / 2 - b^T x.
    info: an optional dict that receives "iters" (iterno at return) and "first_step" (the
    step length of iteration 0 before any test)."""
    A = np.asarray(A, np.float64)
    b = np.asarray(b, np.float64)
    n = len(b)
    x = np.zeros(n)
    last_dir = np.zeros(n)
    last_norm = 0.0
    last_wall = 0
    iterno = 0
    iter_max = max(400, 20 * n)
    first_step = None

    def steplen(d, res):
        return float(d @ res) / (float((A @ d) @ d) + 1e-20)

    def stop(step, ndir, nx):
        return (step != step or step < 1e-7 or step > 1e40 or ndir < 1e-12 * nx
                or ndir < 1e-32)

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        while iterno < iter_max:
            res = A @ x - b
            grad = res.copy()
            grad[(grad > 0) & (x == 0)] = 0.0
            ngrad = float(grad @ grad)
            d = grad.copy()
            step = steplen(grad, res)
            if first_step is None:
                first_step = step
            nx = float(x @ x)
            if iterno > last_wall + 1:
                d = grad + (ngrad / last_norm) * last_dir
                dstep = steplen(d, res)
                ndir = float(d @ d)
                if stop(dstep, ndir, nx):  # reject the CG step
                    d = grad.copy()
                    ndir = float(d @ d)
                else:
                    step = dstep
            else:
                ndir = float(d @ d)
            if stop(step, ndir, nx):
                break
            # Spark's two loops over i.  The first is sequential in i (each clamp lowers the
            # step the later tests see); only d[i] > 0 can pass its test, because step > 0
            # and x >= 0 here.  The second loop's tests do not depend on one another.
            for i in np.nonzero(d > 0)[0]:
                if step * d[i] > x[i]:
                    step = x[i] / d[i]
            hit = step * d > x * (1 - 1e-14)
            x = np.where(hit, 0.0, x - step * d)
            if hit.any():
                last_wall = iterno
            iterno += 1
            last_dir = d
            last_norm = ngrad
    if info is not None:
        info["iters"] = iterno
        info["first_step"] = first_step
    return x


def kkt(A, b, x):
    """|| min(x, A x - b) ||_2 / || b ||_2: zero exactly at the constrained minimiser (every
    coordinate either sits on the wall with a gradient >= 0 or has a zero gradient)."""
    A, b, x = (np.asarray(v, np.float64) for v in (A, b, x))
    nb = float(np.linalg.norm(b))
    return float(np.linalg.norm(np.minimum(x, A @ x - b))) / (nb if nb > 0 else 1.0)


def systems(indptr, indices, vals, Y, reg, implicit=False, alpha=1.0, n_src=None):
    """(A [n, k, k], b [n, k], n_used [n]) of every ragged row, with the regulariser (and YtY
    when implicit) already on A: als_fold_in's documented system.  Entries with a column
    outside [0, n_src) are skipped and not counted."""
    Y = np.asarray(Y, np.float32)
    n_src = Y.shape[0] if n_src is None else n_src
    k = Y.shape[1]
    n = len(indptr) - 1
    G = O.yty(Y[:n_src]) if implicit else None
    A = np.zeros((n, k, k))
    b = np.zeros((n, k))
    used = np.zeros(n, np.int64)
    for r in range(n):
        c = np.asarray(indices[indptr[r]:indptr[r + 1]], np.int64)
        v = np.asarray(vals[indptr[r]:indptr[r + 1]], np.float32)
        ok = (c >= 0) & (c < n_src)
        c, v = c[ok], v[ok]
        a1, b1, ne = O.normal_equations(np.array([0, len(c)]), c, v, Y, implicit, alpha)
        A[r] = a1[0] + (G if implicit else 0.0) + reg * float(ne[0]) * np.eye(k)
        b[r] = b1[0]
        used[r] = len(c)
    return A, b, used


def solve_rows(indptr, indices, vals, Y, reg, implicit=False, alpha=1.0, n_src=None,
               iters=None):
    """The fp32 nonnegative factor row of every ragged row (x.toFloat)."""
    A, b, _ = systems(indptr, indices, vals, Y, reg, implicit, alpha, n_src)
    X = np.zeros(b.shape, np.float32)
    for r in range(len(b)):
        info = {}
        X[r] = nnls_solve(A[r], b[r], info).astype(np.float32)
        if iters is not None:
            iters.append(info["iters"])
    return X


def half_sweep(indptr, indices, vals, Y, reg, implicit=False, alpha=1.0):
    """computeFactors with NNLSSolver for every dst row of one CSR side."""
    return solve_rows(indptr, indices, vals, Y, reg, implicit, alpha)


def fit(users, items, ratings, rank, iterations, reg, implicit=False, alpha=1.0, U0=None,
        seed=0, history=None):
    """oracle.als_oracle.train with the nonnegative solver: items from users, then users from
    items.  history: an optional list that receives (U, V) copies after every iteration.
    Returns (U, V, umap, imap, uids, iids)."""
    users = np.asarray(users, np.int64)
    items = np.asarray(items, np.int64)
    ratings = np.asarray(ratings, np.float32)
    umap, uids = O.index_build(users, int(users.max()) + 1)
    imap, iids = O.index_build(items, int(items.max()) + 1)
    ur, ic = umap[users], imap[items]
    u_ptr, u_idx, u_val = O.csr_build(ur, ic, ratings, len(uids))
    i_ptr, i_idx, i_val = O.csr_build(ic, ur, ratings, len(iids))
    U = O.initialize(len(uids), rank, seed) if U0 is None else np.asarray(U0, np.float32)
    V = np.zeros((len(iids), rank), np.float32)
    for _ in range(iterations):
        V = half_sweep(i_ptr, i_idx, i_val, U, reg, implicit, alpha)
        U = half_sweep(u_ptr, u_idx, u_val, V, reg, implicit, alpha)
        if history is not None:
            history.append((U.copy(), V.copy()))
    return U, V, umap, imap, uids, iids
