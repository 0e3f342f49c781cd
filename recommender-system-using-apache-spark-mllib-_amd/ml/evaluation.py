"""pyspark.ml.evaluation-compatible RankingEvaluator and RegressionEvaluator on the MI355X.

``RankingEvaluator(metricName=, k=, predictionCol=, labelCol=).evaluate(dataset)``
scores two array-valued columns (predicted ids in rank order, relevant ids) of a pandas
DataFrame or dict of columns, with Spark's metric names and defaults
(ml/evaluation/RankingEvaluator.scala).  The arithmetic is
als_mi355x.mllib.evaluation.RankingMetrics (kernel K6).

``RegressionEvaluator(metricName=, labelCol=, predictionCol=, throughOrigin=)
.evaluate(dataset)`` scores two numeric columns with Spark's metric names and defaults
(ml/evaluation/RegressionEvaluator.scala): the columns go to the device as fp64 and one
pass of kernel K8 (als_regression_moments_cols) gives every metric.  ``evaluateFused(model,
dataset)`` is this project's extension for an ALSModel: the predictions are formed inside
the same pass (als_regression_moments) and never materialised.  ``weightCol`` is not
offered.

``FullRankingEvaluator(metricName=, labelCol=, weighted=, exclude=).evaluateFused(model,
dataset)`` is this project's evaluator for implicit-feedback fits: the expected percentile
rank, AUC and reciprocal rank of the held-out items in each user's ordering of all items
(kernel K9, als_rank_positions).
"""
from __future__ import annotations

import numpy as np

from .. import _lib
from .. import engine as _engine
from ..mllib.evaluation import RankingMetrics, moments_of_columns

__all__ = ["RankingEvaluator", "RegressionEvaluator", "FullRankingEvaluator"]

_METRICS = ("meanAveragePrecision", "meanAveragePrecisionAtK", "precisionAtK", "ndcgAtK",
            "recallAtK")


def _check_metric(name):
    if name not in _METRICS:
        raise ValueError(f"RankingEvaluator parameter metricName given invalid value {name!r} "
                         f"(supported: {', '.join(_METRICS)})")
    return name


def _check_k(k):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError(f"RankingEvaluator parameter k given invalid value {k!r} (must be > 0)")
    return int(k)


def _array_column(dataset, col: str):
    try:
        values = dataset[col]
    except (KeyError, IndexError, TypeError):
        raise ValueError(f"dataset has no column {col!r}") from None
    return list(values)


class RankingEvaluator:
    """Evaluator for ranking (pyspark.ml.evaluation.RankingEvaluator)."""

    def __init__(self, metricName: str = "meanAveragePrecision", k: int = 10,
                 predictionCol: str = "prediction", labelCol: str = "label"):
        self._p = dict(metricName=_check_metric(metricName), k=_check_k(k),
                       predictionCol=predictionCol, labelCol=labelCol)

    def setMetricName(self, value):
        self._p["metricName"] = _check_metric(value)
        return self

    def getMetricName(self) -> str:
        return self._p["metricName"]

    def setK(self, value):
        self._p["k"] = _check_k(value)
        return self

    def getK(self) -> int:
        return self._p["k"]

    def setPredictionCol(self, value):
        self._p["predictionCol"] = value
        return self

    def getPredictionCol(self) -> str:
        return self._p["predictionCol"]

    def setLabelCol(self, value):
        self._p["labelCol"] = value
        return self

    def getLabelCol(self) -> str:
        return self._p["labelCol"]

    def setParams(self, **kw):
        for name, value in kw.items():
            if name not in self._p:
                raise TypeError(f"unknown parameter {name}")
            getattr(self, "set" + name[0].upper() + name[1:])(value)
        return self

    def isLargerBetter(self) -> bool:
        return True

    def evaluate(self, dataset) -> float:
        p = self._p
        pred = _array_column(dataset, p["predictionCol"])
        lab = _array_column(dataset, p["labelCol"])
        if len(pred) != len(lab):
            raise ValueError("prediction and label columns must have the same length")
        m = RankingMetrics(zip(pred, lab))
        name, k = p["metricName"], p["k"]
        if name == "meanAveragePrecision":
            return m.meanAveragePrecision
        return {"meanAveragePrecisionAtK": m.meanAveragePrecisionAt, "precisionAtK": m.precisionAt,
                "ndcgAtK": m.ndcgAt, "recallAtK": m.recallAt}[name](k)


_REG_METRICS = ("rmse", "mse", "r2", "mae", "var")


def _check_reg_metric(name):
    if name not in _REG_METRICS:
        raise ValueError(f"RegressionEvaluator parameter metricName given invalid value {name!r} "
                         f"(supported: {', '.join(_REG_METRICS)})")
    return name


def _numeric_column(dataset, col: str) -> np.ndarray:
    try:
        values = dataset[col]
    except (KeyError, IndexError, TypeError):
        raise ValueError(f"dataset has no column {col!r}") from None
    return np.asarray(values, dtype=np.float64).reshape(-1)


class RegressionEvaluator:
    """Evaluator for regression (pyspark.ml.evaluation.RegressionEvaluator): rmse (the
    default), mse, r2, mae, var (explained variance), with upstream's RegressionMetrics
    definitions (engine.regression_dict).  weightCol is out of scope."""

    def __init__(self, metricName: str = "rmse", labelCol: str = "label",
                 predictionCol: str = "prediction", throughOrigin: bool = False):
        self._p = dict(metricName=_check_reg_metric(metricName), labelCol=labelCol,
                       predictionCol=predictionCol, throughOrigin=bool(throughOrigin))

    def setMetricName(self, value):
        self._p["metricName"] = _check_reg_metric(value)
        return self

    def getMetricName(self) -> str:
        return self._p["metricName"]

    def setLabelCol(self, value):
        self._p["labelCol"] = value
        return self

    def getLabelCol(self) -> str:
        return self._p["labelCol"]

    def setPredictionCol(self, value):
        self._p["predictionCol"] = value
        return self

    def getPredictionCol(self) -> str:
        return self._p["predictionCol"]

    def setThroughOrigin(self, value):
        self._p["throughOrigin"] = bool(value)
        return self

    def getThroughOrigin(self) -> bool:
        return self._p["throughOrigin"]

    def setParams(self, **kw):
        for name, value in kw.items():
            if name not in self._p:
                raise TypeError(f"unknown parameter {name}")
            getattr(self, "set" + name[0].upper() + name[1:])(value)
        return self

    def isLargerBetter(self) -> bool:
        return self._p["metricName"] in ("r2", "var")

    def evaluate(self, dataset) -> float:
        """The metric over the labelCol and predictionCol columns of a pandas DataFrame or a
        dict of columns (K8, column form).  A NaN prediction gives NaN, as in Spark."""
        p = self._p
        _lib.require_gpu()
        lab = _numeric_column(dataset, p["labelCol"])
        pred = _numeric_column(dataset, p["predictionCol"])
        if len(lab) != len(pred):
            raise ValueError("prediction and label columns must have the same length")
        m = moments_of_columns(lab, pred)
        return _engine.regression_dict(m, p["throughOrigin"])[p["metricName"]]

    def evaluateFused(self, model, dataset) -> float:
        """evaluate(model.transform(dataset)) without the prediction column: the model's
        user and item columns and this evaluator's labelCol of `dataset` go through the
        fused pass (K8 over K4's fp64 gather-dot; transform rounds its predictions to
        fp32, so the two agree to that rounding).  The model's coldStartStrategy decides
        what a pair with an unknown id does: "drop" leaves it out, "nan" makes the result
        NaN — the number Spark gives for a NaN prediction."""
        from .._data import check_integers, columns_of, to_float32
        p, mp = self._p, model._p
        _lib.require_gpu()
        u, i, r = columns_of(dataset, (mp["userCol"], mp["itemCol"], p["labelCol"]))
        d = model.engine.regression_metrics(check_integers(u, mp["userCol"]),
                                            check_integers(i, mp["itemCol"]), to_float32(r),
                                            through_origin=p["throughOrigin"])
        if d["dropped"] > 0 and str(mp["coldStartStrategy"]).lower() != "drop":
            return float("nan")
        return d[p["metricName"]]


_FULL_METRICS = ("expectedPercentileRank", "meanPercentileRank", "auc", "mrr")


def _check_full_metric(name):
    if name not in _FULL_METRICS:
        raise ValueError(f"FullRankingEvaluator parameter metricName given invalid value "
                         f"{name!r} (supported: {', '.join(_FULL_METRICS)})")
    return name


class FullRankingEvaluator:
    """Evaluator over each user's ordering of ALL items (this project's extension; Spark has
    no counterpart): expectedPercentileRank (the default; Hu, Koren & Volinsky's measure
    for implicit feedback, 0.5 = random, lower is better), meanPercentileRank, auc, mrr —
    ALSModel.evaluateFullRanking's keys (kernel K9).  The metric needs the model's factors,
    not a prediction column, so evaluateFused(model, dataset) is the only way to score and
    evaluate(dataset) raises; TrainValidationSplit / CrossValidator go through
    evaluateFused.  labelCol is read for weighted=True only (the pairs' weights).
    exclude: None, "train" (rank among the items the scored model was not fitted on) or a
    dataset of (user, item) pairs."""

    def __init__(self, metricName: str = "expectedPercentileRank", labelCol: str = "rating",
                 weighted: bool = False, exclude="train"):
        self._p = dict(metricName=_check_full_metric(metricName), labelCol=labelCol,
                       weighted=bool(weighted), exclude=exclude)

    def setMetricName(self, value):
        self._p["metricName"] = _check_full_metric(value)
        return self

    def getMetricName(self) -> str:
        return self._p["metricName"]

    def setLabelCol(self, value):
        self._p["labelCol"] = value
        return self

    def getLabelCol(self) -> str:
        return self._p["labelCol"]

    def setWeighted(self, value):
        self._p["weighted"] = bool(value)
        return self

    def getWeighted(self) -> bool:
        return self._p["weighted"]

    def setExclude(self, value):
        self._p["exclude"] = value
        return self

    def getExclude(self):
        return self._p["exclude"]

    def setParams(self, **kw):
        for name, value in kw.items():
            if name not in self._p:
                raise TypeError(f"unknown parameter {name}")
            getattr(self, "set" + name[0].upper() + name[1:])(value)
        return self

    def isLargerBetter(self) -> bool:
        return self._p["metricName"] in ("auc", "mrr")

    def evaluate(self, dataset) -> float:
        raise TypeError("FullRankingEvaluator scores a model, not a prediction column: the "
                        "position of an item among ALL items needs the factors; call "
                        "evaluateFused(model, dataset)")

    def evaluateFused(self, model, dataset) -> float:
        """The metric of `model` (an ALSModel) over the held-out rows of `dataset`: the
        model's user and item columns, and this evaluator's labelCol when weighted."""
        from .._data import check_integers, columns_of, to_float32
        p, mp = self._p, model._p
        _lib.require_gpu()
        cols = (mp["userCol"], mp["itemCol"]) + ((p["labelCol"],) if p["weighted"] else ())
        got = columns_of(dataset, cols)
        d = model.engine.full_rank_metrics(
            check_integers(got[0], mp["userCol"]), check_integers(got[1], mp["itemCol"]),
            ratings=to_float32(got[2]) if p["weighted"] else None, weighted=p["weighted"],
            **model._filters(p["exclude"], None, True))
        return d[p["metricName"]]
