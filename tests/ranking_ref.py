"""numpy fp64 restatement of Spark 3.x RankingMetrics (binary relevance), for the
ranking-metric tests, plus the seeded problems those tests share.

Per row, with `pred` the list in rank order (a negative entry is an empty slot), `lab`
the distinct relevant ids, m = len(lab), hit(p) = pred[p] in lab, c(p) = hits at 0..p:
  precisionAt(k)              = c(k-1) / k            (k, not the list length)
  recallAt(k)                 = c(k-1) / m
  meanAveragePrecisionAt(k)   = (sum_{p<k, hit} c(p) / (p+1)) / min(m, k)
  ndcgAt(k)                   = (sum_{p<k, hit} d(p)) / (sum_{p<min(m,k)} d(p)),
                                d(p) = 1 / log2(p + 2)
  meanAveragePrecision        = (sum_{p, hit} c(p) / (p+1)) / m   over the whole list
A row with m = 0 scores 0 everywhere.  Sums run in position order.
"""
import numpy as np


def row_metrics(pred, lab, k):
    """(precision, recall, AP, NDCG) at k of one row; zeros when lab is empty."""
    lab = np.unique(np.asarray(lab, np.int64).reshape(-1))
    m = len(lab)
    if m == 0:
        return (0.0, 0.0, 0.0, 0.0)
    pred = np.asarray(pred, np.int64).reshape(-1)[:k]
    hit = (pred >= 0) & np.isin(pred, lab)
    pos = np.arange(len(pred), dtype=np.float64)
    c = np.cumsum(hit).astype(np.float64)
    # np.cumsum adds left to right (np.sum pairs its terms up); a 0.0 term changes nothing
    ap = np.cumsum(np.where(hit, c / (pos + 1.0), 0.0))[-1] if len(pred) else 0.0
    dcg = np.cumsum(np.where(hit, 1.0 / np.log2(pos + 2.0), 0.0))[-1] if len(pred) else 0.0
    n = min(m, k)
    ideal = np.cumsum(1.0 / np.log2(np.arange(n, dtype=np.float64) + 2.0))[-1]
    h = c[-1] if len(pred) else 0.0
    return (float(h / np.float64(k)), float(h / np.float64(m)),
            float(ap / np.float64(n)), float(dcg / ideal))


def per_row(rows, k):
    """[len(rows), 4] fp64 of row_metrics over (pred, lab) rows."""
    return np.array([row_metrics(p, l, k) for p, l in rows], np.float64).reshape(-1, 4)


def sums(rows, k):
    """The six sums als_rank_metrics reports: the four metric sums, rows with labels,
    rows with at least one hit."""
    v = per_row(rows, k)
    has = np.array([len(set(int(x) for x in l)) > 0 for _, l in rows], bool)
    return np.array([v[:, 0].sum(), v[:, 1].sum(), v[:, 2].sum(), v[:, 3].sum(),
                     float(has.sum()), float((v[:, 0] > 0).sum())])


def means(rows, k):
    """Spark's RankingMetrics means: over every row given (label-less rows count as 0)."""
    v = per_row(rows, k)
    return dict(zip(("precision", "recall", "map", "ndcg"), v.mean(axis=0).tolist()))


def mean_average_precision(rows):
    out = []
    for pred, lab in rows:
        lab = set(int(x) for x in lab)
        c, s = 0, 0.0
        for p, j in enumerate(pred):
            if int(j) in lab:
                c += 1
                s += c / (p + 1)
        out.append(s / len(lab) if lab else 0.0)
    return float(np.mean(out))


# the three rows of upstream Spark's RankingMetricsSuite
SPARK_ROWS = [([1, 6, 2, 7, 8, 3, 9, 10, 4, 5], [1, 2, 3, 4, 5]),
              ([4, 1, 5, 6, 2, 7, 3, 8, 9, 10], [1, 2, 3]),
              ([1, 2, 3, 4, 5], [])]
SPARK_MAP = 0.355026
SPARK_PRECISION = {1: 1 / 3, 2: 1 / 3, 3: 1 / 3, 4: 0.75 / 3, 5: 0.8 / 3, 10: 0.8 / 3, 15: 8 / 45}
SPARK_RECALL = {1: 1 / 15, 2: 8 / 45, 3: 11 / 45, 5: 16 / 45, 10: 2 / 3, 15: 2 / 3}
SPARK_MAP_AT = {1: 1 / 3, 2: 0.25, 3: 0.2407407}
SPARK_NDCG = {3: 1 / 3, 5: 0.328788, 10: 0.487913, 15: 0.487913}


# ---- the end-to-end problem: the smoke-sized fit with a seeded 20% held out ----
E2E_USERS, E2E_ITEMS, E2E_RANK, E2E_ITERS, E2E_REG, E2E_FIT_SEED = 300, 200, 8, 5, 0.1, 5
E2E_SPLIT_SEED = 1
E2E_THRESHOLD = 3.0


def e2e_problem():
    """((train u, i, r), (test u, i, r)): the smoke()-shaped 300 x 200 rating set, with a
    seeded 20% of the ratings held out."""
    rng = np.random.default_rng(0)
    n_u, n_i = E2E_USERS, E2E_ITEMS
    mask = rng.random((n_u, n_i)) < 0.08
    mask[np.arange(n_u), rng.integers(0, n_i, n_u)] = True
    mask[rng.integers(0, n_u, n_i), np.arange(n_i)] = True
    u, i = np.nonzero(mask)
    r = np.clip(np.round(3.5 + rng.normal(0, 1, len(u))), 1, 5).astype(np.float32)
    u, i = u.astype(np.int32), i.astype(np.int32)
    held = np.random.default_rng(E2E_SPLIT_SEED).random(len(u)) < 0.2
    return (u[~held], i[~held], r[~held]), (u[held], i[held], r[held])


def held_out_rows(lists, test, known_items, threshold=None):
    """(pred, lab) rows for the users of `lists` ({user: ranked item ids}): lab = the
    user's held-out items that the model knows (rating >= threshold when given); users
    without any are left out, as the engine's query rows are."""
    tu, ti, tr = test
    ok = np.isin(ti, known_items)
    if threshold is not None:
        ok &= tr >= threshold
    rows = []
    for user in sorted(set(tu[ok].tolist())):
        if user in lists:
            rows.append((lists[user], np.unique(ti[ok & (tu == user)]).tolist()))
    return rows
