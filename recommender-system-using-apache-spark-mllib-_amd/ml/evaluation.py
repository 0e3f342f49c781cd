"""pyspark.ml.evaluation-compatible RankingEvaluator on the MI355X.

``RankingEvaluator(metricName=, k=, predictionCol=, labelCol=).evaluate(dataset)``
scores two array-valued columns (predicted ids in rank order, relevant ids) of a pandas
DataFrame or dict of columns, with Spark's metric names and defaults
(ml/evaluation/RankingEvaluator.scala).  The arithmetic is
als_mi355x.mllib.evaluation.RankingMetrics (kernel K6).
"""
from __future__ import annotations

import numpy as np

from ..mllib.evaluation import RankingMetrics

__all__ = ["RankingEvaluator"]

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
