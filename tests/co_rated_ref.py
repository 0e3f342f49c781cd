"""numpy restatement of K19's contract (include/als_hip.h, als_co_rated), for small shapes.

B is the dense int64 multiplicity matrix [rows of the other side, rows of the queried side]:
B[u, a] = stored entries (u, a), duplicates counted.  Query a's common counts are row a of
C = B^T B, its length n_a the column sum.  Everything below applies the contract literally:
the fp64 expression rounded once to fp32, the filters, the order (-score, row), open slots
(-1, -inf, 0).  No scipy."""
import numpy as np

MEASURES = ("count", "jaccard", "cosine")


def multiplicity(rows_other, rows_q, n_other, n):
    """B [n_other, n] from parallel entry arrays (dense rows of both sides)."""
    B = np.zeros((int(n_other), int(n)), np.int64)
    np.add.at(B, (np.asarray(rows_other, np.int64), np.asarray(rows_q, np.int64)), 1)
    return B


def csr(rows, cols, n_rows):
    """(row_ptr int64 [n_rows + 1], col int32) of entries sorted stably by row: the layout
    als_csr_build gives (rows ascending, a row's entries in input order)."""
    rows = np.asarray(rows, np.int64)
    order = np.argsort(rows, kind="stable")
    row_ptr = np.zeros(int(n_rows) + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=int(n_rows)), out=row_ptr[1:])
    return row_ptr, np.asarray(cols, np.int32)[order]


def scores(measure, c, n_a, n_b):
    """fp32 scores of counts c (int64 array) against lengths n_a (int) and n_b (array)."""
    c = c.astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if measure == "count":
            s = c.astype(np.float64)
        elif measure == "jaccard":
            s = c.astype(np.float64) / (np.int64(n_a) + n_b.astype(np.int64) - c).astype(np.float64)
        elif measure == "cosine":
            s = c.astype(np.float64) / np.sqrt(np.float64(n_a) * n_b.astype(np.float64))
        else:
            raise ValueError(measure)
    return s.astype(np.float32)


def co_rated(B, q_rows, top, measure, min_common=1, allow=None):
    """(idx int32 [m, top], score f32 [m, top], common int32 [m, top]) for the dense query
    rows q_rows of the side B's columns index.  allow: bool [n] or None."""
    n = B.shape[1]
    lens = B.sum(0)
    m = len(q_rows)
    idx = np.full((m, top), -1, np.int32)
    score = np.full((m, top), -np.inf, np.float32)
    common = np.zeros((m, top), np.int32)
    for qi, a in enumerate(q_rows):
        a = int(a)
        if a < 0 or a >= n or lens[a] == 0:
            continue
        c = B[:, a] @ B                      # row a of B^T B
        ok = (c >= min_common) & (np.arange(n) != a)
        if allow is not None:
            ok &= np.asarray(allow, bool)
        b = np.nonzero(ok)[0]
        s = scores(measure, c[b], lens[a], lens[b])
        order = np.lexsort((b, -s.astype(np.float64)))[:top]   # score descending, then row
        k = len(order)
        idx[qi, :k], score[qi, :k], common[qi, :k] = b[order], s[order], c[b][order]
    return idx, score, common


def ulp_apart(x, y):
    """|x - y| in fp32 units in the last place, for finite positive x, y (int64 array)."""
    return np.abs(np.asarray(x, np.float32).view(np.int32).astype(np.int64)
                  - np.asarray(y, np.float32).view(np.int32).astype(np.int64))


def near_tie_positions(score_ext):
    """bool [m, top + 1]: positions of a reference list (computed with one slot more than
    the test compares) whose score is within 1 ulp of a neighbouring position's without
    being equal to it.  Only such positions may legitimately hold another row when the
    device's fp64 square root or quotient rounds differently from numpy's."""
    s = np.asarray(score_ext, np.float32)
    fin = np.isfinite(s)
    pair = fin[:, :-1] & fin[:, 1:] & (s[:, :-1] != s[:, 1:])
    d = np.where(pair, ulp_apart(np.where(fin, s, 1)[:, :-1], np.where(fin, s, 1)[:, 1:]), 99)
    close = d <= 1
    near = np.zeros(s.shape, bool)
    near[:, :-1] |= close
    near[:, 1:] |= close
    return near
