"""numpy fp64 reference of the ALS training objective (K10), test infrastructure only.

The objective is the function whose row-wise minimiser a half-sweep computes (Spark's
NormalEquation / CholeskySolver as restated in oracle/als_oracle.py normal_equations + solve,
lambda = regParam scaled by numExplicits), with s = x_u . y_i in fp64 over the fp32 factors:

  explicit  L = sum_obs (r - s)^2 + reg (sum_u n_u |x_u|^2 + sum_i n_i |y_i|^2)
  implicit  L = sum_all c (p - s)^2 + reg (sum_u n+_u |x_u|^2 + sum_i n+_i |y_i|^2)
            c = 1 + alpha |r|, p = [r > 0] per rating; an unobserved pair has c = 1, p = 0

n = ratings of the row, n+ = those with r > 0.  Duplicates of a pair are separate ratings
(each adds its own c (p - s)^2 - s^2 on top of the pair's single s^2), as in Spark.

users / items are DENSE rows of U / V here.  alpha is rounded to fp32 first: that is the
value the solver's C ABI carries (`float alpha`), so it is the alpha of the function being
minimised.

objective(...)        the sparse form: the Frobenius product of the two fp64 Grams plus a
                      correction over the ratings
objective_dense(...)  implicit only: a loop over every (u, i) pair with its c and p
Both return {"objective", "data", "reg", "scale", "n", "n_positive"}; scale = the sum of the
absolute values of everything added (|rating terms|, the all-pairs sum of s^2, the
regulariser), the size rounding errors are relative to.
"""
import numpy as np


def _prep(users, items, ratings, U, V, alpha):
    u = np.asarray(users, np.int64)
    i = np.asarray(items, np.int64)
    r = np.asarray(ratings, np.float32).astype(np.float64)
    U = np.asarray(U, np.float32).astype(np.float64)
    V = np.asarray(V, np.float32).astype(np.float64)
    return u, i, r, U, V, float(np.float32(alpha))


def _regulariser(u, i, r, U, V, implicit):
    w = (r > 0).astype(np.float64) if implicit else np.ones_like(r)
    n_u = np.bincount(u, weights=w, minlength=U.shape[0])
    n_i = np.bincount(i, weights=w, minlength=V.shape[0])
    return float((n_u * (U * U).sum(1)).sum()), float((n_i * (V * V).sum(1)).sum())


def _pack(data, scale_data, reg, reg_u, reg_i, r):
    regv = float(reg) * (reg_u + reg_i)
    return {"objective": data + regv, "data": data, "reg": regv, "scale": scale_data + regv,
            "n": int(len(r)), "n_positive": int((r > 0).sum())}


def objective(users, items, ratings, U, V, reg, implicit=False, alpha=1.0):
    u, i, r, U, V, alpha = _prep(users, items, ratings, U, V, alpha)
    s = (U[u] * V[i]).sum(1)
    if implicit:
        c = 1.0 + alpha * np.abs(r)
        p = (r > 0).astype(np.float64)
        terms = c * (p - s) ** 2 - s * s
        frob = float(((U.T @ U) * (V.T @ V)).sum())
    else:
        terms = (r - s) ** 2
        frob = 0.0
    reg_u, reg_i = _regulariser(u, i, r, U, V, implicit)
    return _pack(float(terms.sum()) + frob, float(np.abs(terms).sum()) + abs(frob), reg, reg_u,
                 reg_i, r)


def objective_dense(users, items, ratings, U, V, reg, alpha=1.0):
    """The implicit objective with the all-pairs sum formed pair by pair (small problems)."""
    u, i, r, U, V, alpha = _prep(users, items, ratings, U, V, alpha)
    by_pair = {}
    for a, b, x in zip(u.tolist(), i.tolist(), r.tolist()):
        by_pair.setdefault((a, b), []).append(x)
    data = 0.0
    for a in range(U.shape[0]):
        for b in range(V.shape[0]):
            s = float(U[a] @ V[b])
            rs = by_pair.get((a, b))
            if not rs:
                data += s * s                       # c = 1, p = 0
                continue
            # the pair's own s^2 is replaced by its first rating's term; further copies of
            # the pair are extra ratings, each with the confidence ABOVE the baseline 1
            for t, x in enumerate(rs):
                c = 1.0 + alpha * abs(x)
                p = 1.0 if x > 0 else 0.0
                data += c * (p - s) ** 2 - (s * s if t > 0 else 0.0)
    reg_u, reg_i = _regulariser(u, i, r, U, V, True)
    return _pack(data, abs(data), reg, reg_u, reg_i, r)


def side(rows, cols, vals, X, Y, implicit=False, alpha=1.0, n_cols=None):
    """What one rating pass over one CSR side returns (als_objective_side's five numbers):
    [sum of the rating terms, sum of their absolute values, sum_row n_row |x_row|^2, ratings,
    ratings with r > 0]; X = the side's own factors, Y = the other side's (None: no terms).
    n_cols given: a rating whose col is outside [0, n_cols) adds no term to the first two, and
    still counts in the other three (the contract of include/als_hip.h)."""
    a, b, r, X, _, alpha = _prep(rows, cols, vals, X, X, alpha)
    w = (r > 0).astype(np.float64) if implicit else np.ones_like(r)
    reg = float((np.bincount(a, weights=w, minlength=X.shape[0]) * (X * X).sum(1)).sum())
    if Y is None:
        return [0.0, 0.0, reg, float(len(r)), float((r > 0).sum())]
    n, n_pos = float(len(r)), float((r > 0).sum())
    if n_cols is not None:
        keep = (b >= 0) & (b < n_cols)
        a, b, r = a[keep], b[keep], r[keep]
    s = (X[a] * np.asarray(Y, np.float32).astype(np.float64)[b]).sum(1)
    if implicit:
        terms = (1.0 + alpha * np.abs(r)) * ((r > 0) - s) ** 2 - s * s
    else:
        terms = (r - s) ** 2
    return [float(terms.sum()), float(np.abs(terms).sum()), reg, n, n_pos]


GROUPS = 5


def grouped_problem(n_u=200, n_i=150, nnz=4000, seed=11):
    """The monotonicity protocol's data: users and items in GROUPS taste groups (id modulo
    GROUPS), every user and item with at least 5 in-group ratings, the rest 90 % in-group;
    ratings uniform on the half stars 0.5 .. 5.  Returns (users, items, ratings)."""
    rng = np.random.default_rng(seed)
    gu, gi = np.arange(n_u) % GROUPS, np.arange(n_i) % GROUPS
    us, it = [], []
    for u in range(n_u):
        for i in rng.choice(np.flatnonzero(gi == gu[u]), 5, replace=False):
            us.append(u), it.append(int(i))
    for i in range(n_i):
        for u in rng.choice(np.flatnonzero(gu == gi[i]), 5, replace=False):
            us.append(int(u)), it.append(i)
    while len(us) < nnz:
        u = int(rng.integers(0, n_u))
        i = int(rng.choice(np.flatnonzero(gi == gu[u]))) if rng.random() < 0.9 else \
            int(rng.integers(0, n_i))
        us.append(u), it.append(i)
    r = (rng.integers(1, 11, nnz) / 2).astype(np.float32)
    return np.array(us, np.int32), np.array(it, np.int32), r


def grouped_start(n_u, k, seed=5):
    """The protocol's fixed U0: each user's group indicator (dimension group mod k) plus 0.1
    |gaussian| noise, rows normalised.  It carries the block structure of grouped_problem, so
    the very first item half-sweep can fit it: with the CPU oracle's half-sweeps the first
    one takes L to 0.16 - 0.30 of its start in every protocol configuration (ranks 8, 48,
    128, explicit and implicit alpha = 1), where a gaussian start reaches only 0.5 - 0.87."""
    rng = np.random.default_rng(seed)
    x = 0.1 * np.abs(rng.standard_normal((n_u, k)))
    x[np.arange(n_u), (np.arange(n_u) % GROUPS) % k] += 1.0
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def csr(rows, cols, vals, n_rows):
    """(row_ptr int64, col int32, val f32) of a COO list, input order kept within a row."""
    rows = np.asarray(rows, np.int64)
    order = np.argsort(rows, kind="stable")
    ptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n_rows), out=ptr[1:])
    return ptr, np.asarray(cols, np.int32)[order], np.asarray(vals, np.float32)[order]
