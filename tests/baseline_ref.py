"""numpy fp64 reference of K16 (rating statistics and bias baselines), written from the
definitions in include/als_hip.h; it calls nothing of the code under test.

A CSR side is (row_ptr int64 [n + 1], col int32 [nnz], val fp32 [nnz]).  The terms of a row are
e_j = float64(val_j) - offset - (other[col_j] if other is given and 0 <= col_j < n_cols else 0).
"""
import numpy as np

U53 = 2.0 ** -53


def csr_from_lengths(lengths, n_cols, rng, values="half"):
    """A CSR side with the given row lengths: columns uniform in [0, n_cols), values
    "half" (multiples of 0.5 in [0.5, 5]), "wide" (normal(3, 1e3)) or "shifted" (1e4 +
    normal(0, 1)), as fp32."""
    lengths = np.asarray(lengths, np.int64)
    row_ptr = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=row_ptr[1:])
    nnz = int(row_ptr[-1])
    col = rng.integers(0, max(n_cols, 1), nnz).astype(np.int32)
    if values == "half":
        val = (rng.integers(1, 11, nnz) * 0.5).astype(np.float32)
    elif values == "wide":
        val = rng.normal(3.0, 1e3, nnz).astype(np.float32)
    elif values == "shifted":
        val = (1e4 + rng.normal(0.0, 1.0, nnz)).astype(np.float32)
    else:
        raise ValueError(values)
    return row_ptr, col, val


def csr_from_triples(rows, cols, vals, n_rows):
    """Dense (row, col, val) triples -> CSR, input order kept inside a row."""
    rows = np.asarray(rows, np.int64)
    order = np.argsort(rows, kind="stable")
    row_ptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n_rows), out=row_ptr[1:])
    return row_ptr, np.asarray(cols, np.int32)[order], np.asarray(vals, np.float32)[order]


def terms(col, val, n_cols, other=None, offset=0.0):
    e = val.astype(np.float64) - np.float64(offset)
    if other is not None:
        ok = (col >= 0) & (col < n_cols)
        g = np.zeros(len(col), np.float64)
        g[ok] = np.asarray(other, np.float64)[col[ok]]
        e = e - g
    return e


def _five(e):
    if len(e) == 0:
        return [0.0, 0.0, 0.0, np.nan, np.nan]
    s = float(np.sum(e))                      # numpy's pairwise fp64 sum
    m = s / len(e)
    return [float(len(e)), s, float(np.sum((e - m) ** 2)), float(e.min()), float(e.max())]


def row_moments(row_ptr, col, val, n_cols, other=None, offset=0.0):
    """(moments [n_rows, 5], total [5], abs_sum [n_rows + 1], sq_sum [n_rows + 1]): n, sum,
    two-pass M2, min, max per row and over everything; abs_sum / sq_sum = sum |e| and
    sum e^2 per row, the last entry over everything (what the error bounds scale with)."""
    e = terms(col, val, n_cols, other, offset)
    n_rows = len(row_ptr) - 1
    mom = np.empty((n_rows, 5), np.float64)
    a, q = np.empty(n_rows + 1), np.empty(n_rows + 1)
    for r in range(n_rows):
        er = e[row_ptr[r]:row_ptr[r + 1]]
        mom[r] = _five(er)
        a[r], q[r] = np.abs(er).sum(), (er * er).sum()
    a[-1], q[-1] = np.abs(e).sum(), (e * e).sum()
    return mom, np.asarray(_five(e)), a, q


def bias_update(mom, damping):
    n, s = mom[:, 0], mom[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(n > 0, s / (np.float64(damping) + n), 0.0)


def objective(user_side, mu, bu, bi, reg_user, reg_item):
    """SSE + reg_user sum bu^2 + reg_item sum bi^2 over the ratings of the user-side CSR."""
    row_ptr, col, val = user_side
    rows = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    res = val.astype(np.float64) - mu - bu[rows] - bi[col]
    return float((res * res).sum() + reg_user * (bu * bu).sum() + reg_item * (bi * bi).sum())


def fit(user_side, item_side, method="bias", reg_user=10.0, reg_item=25.0, sweeps=10):
    """(mu, bu, bi, history) of the alternating fit from zero biases: item update given bu,
    then user update given bi; history = objective() after every sweep (one entry for the
    one-step methods)."""
    n_u, n_i = len(user_side[0]) - 1, len(item_side[0]) - 1
    val = item_side[2].astype(np.float64)
    mu = float(val.sum() / len(val))
    bu, bi = np.zeros(n_u), np.zeros(n_i)
    if method == "item":
        bi = bias_update(row_moments(*item_side, n_u, None, mu)[0], reg_item)
    elif method == "user":
        bu = bias_update(row_moments(*user_side, n_i, None, mu)[0], reg_user)
    elif method == "bias":
        hist = []
        for _ in range(sweeps):
            bi = bias_update(row_moments(*item_side, n_u, bu, mu)[0], reg_item)
            bu = bias_update(row_moments(*user_side, n_i, bi, mu)[0], reg_user)
            hist.append(objective(user_side, mu, bu, bi, reg_user, reg_item))
        return mu, bu, bi, hist
    elif method != "global":
        raise ValueError(method)
    return mu, bu, bi, [objective(user_side, mu, bu, bi, reg_user, reg_item)]


def predict(urow, irow, mu, bu, bi):
    """(pred fp32, known uint8): mu + bu[urow] + bi[irow] in fp64, rounded once; a row outside
    its table (-1 included) is unknown and adds 0."""
    urow, irow = np.asarray(urow, np.int64), np.asarray(irow, np.int64)
    n_u = 0 if bu is None else len(bu)
    n_i = 0 if bi is None else len(bi)
    return predict_sized(urow, irow, mu, bu, n_u, bi, n_i)


def predict_sized(urow, irow, mu, bu, n_u, bi, n_i):
    urow, irow = np.asarray(urow, np.int64), np.asarray(irow, np.int64)
    ku, ki = (urow >= 0) & (urow < n_u), (irow >= 0) & (irow < n_i)
    p = np.full(len(urow), np.float64(mu))
    if bu is not None:
        p[ku] += np.asarray(bu, np.float64)[urow[ku]]
    if bi is not None:
        p[ki] += np.asarray(bi, np.float64)[irow[ki]]
    return p.astype(np.float32), (ku.astype(np.uint8) | (ki.astype(np.uint8) << 1))


def top_rated(ids, count, total, num, min_count=0, damping=0.0):
    """[(id, sum / (damping + count), count)] of the rows with count > min_count, by
    descending score, ties by ascending id; at most num."""
    rows = [(int(a), float(s) / (float(damping) + int(c)), int(c))
            for a, c, s in zip(ids, count, total) if int(c) > min_count and int(c) > 0]
    rows.sort(key=lambda t: (-t[1], t[0]))
    return rows[:int(num)]


def textbook_m2(e):
    """sum e^2 - (sum e)^2 / n in fp64: the formula K16 must not use."""
    e = np.asarray(e, np.float64)
    return float((e * e).sum() - e.sum() ** 2 / len(e))
