"""numpy fp64 reference of K11 (als_explain): per-rating contributions of a score.

For one row with entries (col_j, r_j) against the factor table Y (n_src rows), with K7's
rules (include/als_hip.h, als_fold_in): entries with col < 0 or col >= n_src are skipped,
duplicates are kept, n = used entries, n+ = used entries with r > 0,
  explicit:  A = sum y y^T + reg*n*I,            wb_j = r_j
  implicit:  A = YtY + sum c1 y y^T + reg*n+*I,  wb_j = 1 + c1 if r_j > 0 else 0, c1 = alpha*|r|
and for a target t:  z = A^-1 y_t,  contribution_j = wb_j * (z . y_j),  score = sum_j.
The list is every used entry ordered by contribution descending, ties by ascending entry
position (the offset inside the row, skipped entries counted).
"""
import numpy as np


def row_system(cols, vals, Y, reg, implicit, alpha, yty=None):
    """(A [k, k], wb [m], pos [m], Yu [m, k]) over the used entries of one row, or None when
    the row has none.  yty: Y^T Y in fp64 (computed when None and implicit)."""
    cols = np.asarray(cols, np.int64)
    vals = np.asarray(vals, np.float32).astype(np.float64)
    Y = np.asarray(Y, np.float32).astype(np.float64)
    used = (cols >= 0) & (cols < len(Y))
    pos = np.nonzero(used)[0]
    if len(pos) == 0:
        return None
    Yu, r = Y[cols[pos]], vals[pos]
    k = Y.shape[1]
    if implicit:
        c1 = alpha * np.abs(r)
        A = (Y.T @ Y if yty is None else yty) + (Yu * c1[:, None]).T @ Yu
        A = A + reg * float((r > 0).sum()) * np.eye(k)
        wb = np.where(r > 0, 1.0 + c1, 0.0)
    else:
        A = Yu.T @ Yu + reg * float(len(pos)) * np.eye(k)
        wb = r
    return A, wb, pos, Yu


def explain_row(cols, vals, Y, targets, reg, implicit, alpha, yty=None):
    """Per target of one row: (score, pos [m], contrib [m]) with the full ordered list, or
    (0.0, empty, empty) for an unknown target or a row without a used entry."""
    Yd = np.asarray(Y, np.float32).astype(np.float64)
    sysm = row_system(cols, vals, Y, reg, implicit, alpha, yty)
    empty = (0.0, np.zeros(0, np.int64), np.zeros(0))
    out = []
    for t in targets:
        if sysm is None or t < 0 or t >= len(Yd):
            out.append(empty)
            continue
        A, wb, pos, _ = sysm
        z = np.linalg.solve(A, Yd[t])
        # one dot per item, looked up per entry: entries of one item get the same bits
        # whatever a BLAS does with row position, so equal ratings tie exactly
        c = wb * (Yd @ z)[np.asarray(cols, np.int64)[pos]]
        order = np.lexsort((pos, -c))       # contribution descending, then position ascending
        out.append((float(c.sum()), pos[order], c[order]))
    return out


def solve_row(cols, vals, Y, reg, implicit, alpha, yty=None):
    """x = A^-1 b of the row (zeros when it has no used entry): what K7 returns."""
    sysm = row_system(cols, vals, Y, reg, implicit, alpha, yty)
    if sysm is None:
        return np.zeros(np.asarray(Y).shape[1])
    A, wb, _, Yu = sysm
    return np.linalg.solve(A, Yu.T @ wb)


def well_separated(c, pos, tol=1e-9):
    """True when no two consecutive contributions of the ordered list are closer than
    tol * max|c| unless they are exactly equal: the order is then decided by the values
    (and the tie rule), not by rounding."""
    c = np.asarray(c, np.float64)
    if len(c) < 2:
        return True
    gap = np.abs(np.diff(c))
    return bool(((gap == 0) | (gap >= tol * np.abs(c).max())).all())
