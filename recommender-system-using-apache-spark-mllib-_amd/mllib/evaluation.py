"""pyspark.mllib.evaluation-compatible RankingMetrics and RegressionMetrics on the MI355X.

``RankingMetrics(predictionAndLabels)`` takes an iterable of (predicted ids in rank
order, relevant ids) pairs, as Spark's takes an RDD of them, and offers
``precisionAt(k)``, ``recallAt(k)``, ``ndcgAt(k)``, ``meanAveragePrecisionAt(k)`` and
``meanAveragePrecision`` with upstream's definitions (mllib/evaluation/
RankingMetrics.scala, Spark 3.x, binary relevance): precision divides by k even when a
list is shorter, the ideal DCG has min(labels, k) terms, and a row without labels
scores 0 and still counts in the mean.

The at-k metrics run on the device (kernel K6, als_rank_metrics): the lists are padded
with -1 into one [rows, width] matrix once, the label sets become sorted ranges
(filters.relevance_lists), and each call is one pass over the matrix.  k <= 256.
``meanAveragePrecision`` scores whole lists of any length and divides by the number of
labels; it is computed on the host from the same padded matrix.

To score a fitted model against held-out ratings without moving its lists to the host
at all, use ``MatrixFactorizationModel.rankingMetrics`` / ``ALSModel.evaluateRanking``.

``RegressionMetrics(predictionAndObservations)`` takes an iterable of (prediction,
observation) pairs — prediction first, as Spark's does — and offers ``explainedVariance``,
``meanAbsoluteError``, ``meanSquaredError``, ``rootMeanSquaredError`` and ``r2`` with
upstream's definitions (mllib/evaluation/RegressionMetrics.scala): one pass of kernel K8
(als_regression_moments_cols) over the two fp64 columns.  For a fitted model use
``MatrixFactorizationModel.regressionMetrics`` / ``ALSModel.evaluateRegression``, which
form the predictions inside the same pass.

``ListMetrics(lists)`` has no Spark counterpart: the beyond-accuracy measures of a set of
recommendation lists taken together (catalogue coverage, Gini index and entropy of item
exposure, personalisation, novelty, average popularity, long-tail share), for lists from
anywhere; kernels K15.  For a fitted model use ``MatrixFactorizationModel.listMetrics`` /
``ALSModel.evaluateListQuality``.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from .. import engine as _engine
from .. import filters as _filters
from .._data import check_integers

__all__ = ["RankingMetrics", "RegressionMetrics", "ListMetrics"]


def _id_array(x, what: str) -> np.ndarray:
    a = np.asarray(x if isinstance(x, np.ndarray) else list(x))
    return check_integers(a.reshape(-1), what) if a.size else np.zeros(0, np.int32)


class RankingMetrics:
    """Evaluator for ranking algorithms (pyspark.mllib.evaluation.RankingMetrics)."""

    def __init__(self, predictionAndLabels):
        _lib.require_gpu()
        self.device = torch.device("cuda", torch.cuda.current_device())
        preds, labs = [], []
        for p, l in predictionAndLabels:
            preds.append(_id_array(p, "prediction"))
            labs.append(_id_array(l, "label"))
        self.rows = n = len(preds)
        p_len = np.array([len(p) for p in preds], np.int64)
        l_len = np.array([len(l) for l in labs], np.int64)
        # any int32 id -> dense non-negative value (-1 is the matrix's empty slot)
        flat = np.concatenate(preds + labs) if n else np.zeros(0, np.int32)
        uniq, dense = np.unique(flat, return_inverse=True)
        dense = dense.reshape(-1).astype(np.int32)
        n_pred = int(p_len.sum())
        self._n_ids = max(len(uniq), 1)
        self._width = max(int(p_len.max()) if n else 0, 1)
        idx = np.full((n, self._width), -1, np.int32)
        row = np.repeat(np.arange(n), p_len)
        pos = np.arange(n_pred) - np.repeat(np.cumsum(p_len) - p_len, p_len)
        idx[row, pos] = dense[:n_pred]
        self._idx_host = idx
        self._idx = torch.as_tensor(idx, device=self.device)
        self._lab_row = np.repeat(np.arange(n), l_len)
        self._lab_col = dense[n_pred:].astype(np.int64)
        self._rel = _filters.relevance_lists(
            torch.as_tensor(self._lab_row, device=self.device),
            torch.as_tensor(self._lab_col, device=self.device), n)
        self._ws = _engine.Workspace(self.device)
        self._sums = {}

    def _lists(self, k: int) -> torch.Tensor:
        """The list matrix at width max(k, longest list), padded with -1."""
        if self._idx.shape[1] < k:
            wide = torch.full((self.rows, k), -1, dtype=torch.int32, device=self.device)
            wide[:, :self._idx.shape[1]] = self._idx
            self._idx = wide
        return self._idx

    def _mean(self, k, which: int) -> float:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError(f"ranking position k should be positive, got {k!r}")
        if k > _engine.MAX_RANK_AT:
            raise ValueError(f"k = {k} > {_engine.MAX_RANK_AT} is not supported by the "
                             "ranking-metrics kernel")
        k = int(k)
        if k not in self._sums:
            sums, _ = _engine.rank_metrics_rows(self._lists(k), k, *self._rel, self._ws)
            self._sums[k] = sums.tolist()
        # rows without labels score 0 and count: the divisor is every row given
        return self._sums[k][which] / self.rows if self.rows else float("nan")

    def precisionAt(self, k: int) -> float:
        return self._mean(k, 0)

    def recallAt(self, k: int) -> float:
        return self._mean(k, 1)

    def meanAveragePrecisionAt(self, k: int) -> float:
        return self._mean(k, 2)

    def ndcgAt(self, k: int) -> float:
        return self._mean(k, 3)

    @property
    def meanAveragePrecision(self) -> float:
        """Mean over rows of (sum over hit positions p of hits(0..p) / (p + 1)) / labels,
        over each whole list (Spark's meanAveragePrecision); host fp64."""
        if not self.rows:
            return float("nan")
        idx = self._idx_host.astype(np.int64)
        base = np.arange(self.rows, dtype=np.int64)[:, None] * self._n_ids
        rel = np.unique(self._lab_row * self._n_ids + self._lab_col)
        hit = (idx >= 0) & np.isin(base + idx, rel)
        m = np.bincount((rel // self._n_ids), minlength=self.rows).astype(np.float64)
        terms = np.where(hit, np.cumsum(hit, axis=1) / np.arange(1, idx.shape[1] + 1), 0.0)
        ap = np.divide(terms.sum(axis=1), m, out=np.zeros(self.rows), where=m > 0)
        return float(ap.sum() / self.rows)


def moments_of_columns(label, pred) -> list:
    """K8's 8 moments (engine.MOMENT_NAMES) of two host columns, uploaded as fp64."""
    _lib.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    lab = torch.as_tensor(np.ascontiguousarray(label, dtype=np.float64)).to(dev)
    prd = torch.as_tensor(np.ascontiguousarray(pred, dtype=np.float64)).to(dev)
    return _engine.regression_moments_cols(lab, prd, _engine.Workspace(dev)).tolist()


class RegressionMetrics:
    """Evaluator for regression (pyspark.mllib.evaluation.RegressionMetrics)."""

    def __init__(self, predictionAndObservations, throughOrigin: bool = False):
        _lib.require_gpu()
        rows = predictionAndObservations
        a = np.asarray(rows if isinstance(rows, np.ndarray) else list(rows), dtype=np.float64)
        if a.size == 0:
            a = a.reshape(0, 2)
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError("expected rows of 2 values (prediction, observation)")
        self._m = _engine.regression_dict(moments_of_columns(a[:, 1], a[:, 0]),
                                          bool(throughOrigin))

    @property
    def explainedVariance(self) -> float:
        return self._m["var"]

    @property
    def meanAbsoluteError(self) -> float:
        return self._m["mae"]

    @property
    def meanSquaredError(self) -> float:
        return self._m["mse"]

    @property
    def rootMeanSquaredError(self) -> float:
        return self._m["rmse"]

    @property
    def r2(self) -> float:
        return self._m["r2"]


class ListMetrics:
    """What a set of recommendation lists looks like as a whole (K15).

    lists: an iterable of id sequences, one per user, at most 256 ids each (shorter lists are
    padded with open slots).  popularity: {id: count} or (ids, counts), how often each item
    was rated; without it novelty, averagePopularity and longTailShare are NaN.  numUsers: the
    number of raters the counts come from (None: the number of lists).  catalog: the ids
    exposure is measured over (None: every id named by popularity or by a list, taken together;
    with a catalog, a listed id outside it is skipped).  The long tail is what lies outside the
    most-rated fifth of the catalogue.  The ids are mapped to dense rows on the host, the three
    measures run on the device (als_list_exposure, als_list_concentration,
    als_list_novelty).  Each field of engine.LIST_METRIC_FIELDS is an attribute; toDict()
    returns them all."""

    def __init__(self, lists, popularity=None, numUsers=None, catalog=None):
        lists = [_id_array(x, "list") for x in lists]
        width = max([len(x) for x in lists] + [1])
        if width > _engine.LIST_MAX_AT:
            raise ValueError(f"lists of {width} entries > {_engine.LIST_MAX_AT} are not "
                             "supported by the list-metrics kernels")
        if numUsers is not None and int(numUsers) < 1:
            raise ValueError(f"numUsers must be >= 1, got {numUsers}")
        pop_ids = pop_cnt = None
        if popularity is not None:
            if isinstance(popularity, dict):
                pop_ids, pop_cnt = list(popularity.keys()), list(popularity.values())
            else:
                pop_ids, pop_cnt = popularity
            pop_ids = _id_array(pop_ids, "popularity id")
            pop_cnt = _id_array(pop_cnt, "popularity count")
            if len(pop_ids) != len(pop_cnt):
                raise ValueError("popularity: ids and counts must have the same length")
        flat = np.concatenate(lists) if lists else np.zeros(0, np.int32)
        if catalog is not None:
            cat = np.unique(_id_array(catalog, "catalog"))
        elif pop_ids is not None:
            cat = np.unique(np.concatenate([pop_ids, flat]))
        else:
            cat = np.unique(flat)
        n_v = len(cat)

        def dense(ids):
            if n_v == 0:
                return np.full(len(ids), -1, np.int64)
            pos = np.minimum(np.searchsorted(cat, ids), n_v - 1)
            return np.where(cat[pos] == ids, pos, -1)

        idx = np.full((len(lists), width), -1, np.int32)
        for r, x in enumerate(lists):
            idx[r, :len(x)] = dense(x)
        _lib.require_gpu()
        dev = torch.device("cuda", torch.cuda.current_device())
        pop = None
        if pop_ids is not None:
            host = np.zeros(n_v, np.int32)
            d = dense(pop_ids)
            host[d[d >= 0]] = pop_cnt[d >= 0]
            pop = torch.as_tensor(host, device=dev)
        n_pop = int(numUsers) if numUsers is not None else max(len(lists), 1)
        self._m, _ = _engine.list_metrics_rows(
            torch.as_tensor(idx, device=dev), width, n_v, _engine.Workspace(dev), pop=pop,
            n_pop=n_pop)

    def toDict(self) -> dict:
        return dict(self._m)

    def __getattr__(self, name):
        if name in _engine.LIST_METRIC_FIELDS:
            return self._m[name]
        raise AttributeError(name)
