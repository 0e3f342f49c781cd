"""pyspark.ml.tuning-compatible model selection: ParamGridBuilder, TrainValidationSplit,
CrossValidator (and Param, the key of a param map).

The reference script is a model-selection script: it fits ALS at ranks 4, 8 and 12, scores
each fit by validation RMSE and keeps the best (RecommenderSystem.py:136-159).  In Spark's
ml API that is ``TrainValidationSplit(estimator=als, estimatorParamMaps=grid,
evaluator=RegressionEvaluator(...)).fit(ratings)``; this module offers the same classes
over pandas DataFrames (or dicts of columns).

What differs from Spark, on purpose:
  * The splits are made on the host from a seeded numpy generator: the train/validation
    split is ``datasets.random_split``, and the folds draw one uniform number per row,
    fold f taking [f / k, (f + 1) / k).  Neither reproduces Spark's samplers bit for bit.
  * One engine per training split.  For an ``ALS`` estimator the rating blocks (K1: id
    maps, both CSR sides, schedules) are built once per training split and every param map
    is fitted on that engine, one after the other, each fit re-initialising the factors
    and being scored before the next starts; the engine is rebuilt only when a map
    changes userCol, itemCol or ratingCol.  A fit on the shared engine gives the same
    bits as a stand-alone fit (tests/test_gpu_tuning.py).  Tuning fits write no
    checkpoints; the final refit of the best map on the whole dataset is an ordinary
    ``estimator.fit`` on a fresh engine.
  * A ``RegressionEvaluator`` scoring an ``ALSModel`` goes through ``evaluateFused`` (K8
    over K4: no prediction column); every other estimator / evaluator pair goes through
    ``evaluator.evaluate(model.transform(validation))``.
  * A NaN metric never wins, and when every metric is NaN ``fit`` raises ValueError
    instead of returning an arbitrary model (Spark's argmax / argmin over NaN picks one
    silently).  With ALS the usual cause is coldStartStrategy="nan" and a validation row
    whose user or item is not in the training split: use coldStartStrategy="drop".
  * ``parallelism`` is accepted and ignored: the fits share one GPU and run in sequence.
  * ``stratify="user"`` (not in Spark) splits per user on the GPU instead of per row on the
    host (K20, ``ALSCore.split``): every user's validation share is 1 - trainRatio of their
    ratings (or ``holdOut`` ratings: ``holdOut=1`` is leave-one-out), and a CrossValidator's
    folds cut every user's ratings into numFolds parts whose sizes differ by at most one.
    No item leaves a training part, so no validation pair is cold.  The full rating set is
    built once; each training split is compacted from it on the device and is, bit for bit,
    the engine a stand-alone fit on the kept rows would build.  ``stratify=None`` is the
    host split described above, unchanged.
"""
from __future__ import annotations

import itertools
import zlib

import numpy as np

from .. import datasets as _datasets
from .param import Param

__all__ = ["Param", "ParamGridBuilder", "TrainValidationSplit", "TrainValidationSplitModel",
           "CrossValidator", "CrossValidatorModel", "fold_assignment", "best_index"]


class ParamGridBuilder:
    """Builder of a param grid (pyspark.ml.tuning.ParamGridBuilder): ``build()`` returns the
    cartesian product of the grids as a list of maps, keys in insertion order, the last key
    varying fastest."""

    def __init__(self):
        self._grid = {}

    def addGrid(self, param, values):
        if not isinstance(param, (Param, str)):
            raise TypeError(f"param must be a Param or a parameter name, got {param!r}")
        self._grid[param] = list(values)
        return self

    def baseOn(self, *args):
        """Fix params to single values: a dict, or (param, value) pairs."""
        if len(args) == 1 and isinstance(args[0], dict):
            args = tuple(args[0].items())
        for param, value in args:
            self.addGrid(param, [value])
        return self

    def build(self):
        keys = list(self._grid)
        return [dict(zip(keys, combo)) for combo in itertools.product(*self._grid.values())]


# ---------------------------------------------------------------- datasets on the host
def _n_rows(dataset) -> int:
    if isinstance(dataset, dict):
        return len(next(iter(dataset.values()))) if dataset else 0
    return len(dataset)


def _take(dataset, idx):
    """The rows `idx` (ascending positions) of a DataFrame, dict of columns, array or list."""
    if hasattr(dataset, "iloc"):
        return dataset.iloc[idx].reset_index(drop=True)
    if isinstance(dataset, dict):
        return {k: np.asarray(v)[idx] for k, v in dataset.items()}
    if isinstance(dataset, np.ndarray):
        return dataset[idx]
    return [dataset[int(j)] for j in idx]


def fold_assignment(n: int, numFolds: int, seed: int) -> np.ndarray:
    """Fold of each of n rows: one seeded uniform x per row, fold f = [f / k, (f + 1) / k)."""
    x = np.random.default_rng(seed).random(n)
    return np.minimum((x * numFolds).astype(np.int64), numFolds - 1)


def best_index(metrics, larger_is_better: bool) -> int:
    """Index of the best metric, the first among equals.  NaN never wins; all NaN raises."""
    m = np.asarray(metrics, np.float64)
    if m.size == 0 or np.isnan(m).all():
        raise ValueError(
            "every param map's metric is NaN, so no model can be chosen.  With ALS this "
            "means a validation row's user or item is missing from the training split "
            "while coldStartStrategy is \"nan\": use coldStartStrategy=\"drop\"")
    return int(np.nanargmax(m) if larger_is_better else np.nanargmin(m))


def _default_seed(obj) -> int:
    return zlib.crc32(type(obj).__name__.encode())


# ---------------------------------------------------------------- fitting and scoring
def _score(evaluator, model, validation) -> float:
    from .evaluation import FullRankingEvaluator, RegressionEvaluator
    from .recommendation import ALSModel
    if isinstance(evaluator, FullRankingEvaluator):   # needs the model: no column form
        return float(evaluator.evaluateFused(model, validation))
    if isinstance(evaluator, RegressionEvaluator) and isinstance(model, ALSModel):
        return float(evaluator.evaluateFused(model, validation))
    return float(evaluator.evaluate(model.transform(validation)))


def _fit_and_score(estimator, maps, evaluator, train, validation, collect: bool, core=None):
    """(metric per map, sub-model per map or None) of one training split.  core: the
    training engine of an ALS estimator when the caller has made it (stratified splits)."""
    from .recommendation import ALS, ALSModel
    metrics, subs = [], ([] if collect else None)
    if not isinstance(estimator, ALS):
        for m in maps:
            model = estimator.fit(train, m)
            metrics.append(_score(evaluator, model, validation))
            if collect:
                subs.append(model)
        return metrics, subs
    from .. import engine as _engine
    built_for = None
    for m in maps:
        est = estimator.copy(m)
        cols = tuple(est.getOrDefault(c) for c in ("userCol", "itemCol", "ratingCol"))
        if core is None or (built_for is not None and cols != built_for):
            core = _engine.make_engine(*est._columns(train))
        built_for = cols
        est._fit_core(core, checkpoints=False)
        model = ALSModel(core, dict(est._p), solver=est.getSolver())
        metrics.append(_score(evaluator, model, validation))   # before the next fit
        if collect:  # the shared engine's factors are overwritten by the next fit
            uids, U = core.user_factors()
            iids, V = core.item_factors()
            subs.append(ALSModel(_engine.ALSCore.from_factors(uids, U, iids, V), dict(est._p),
                                 solver=est.getSolver()))
    return metrics, subs


def _check_stratify(stratify):
    if stratify not in (None, "user"):
        raise ValueError(f"stratify must be None or \"user\", got {stratify!r}")
    return stratify


def _stratified_splits(estimator, maps, dataset, split_args, seed):
    """For each kwargs of `split_args` (count / fraction / fold for ALSCore.split) one
    (train, validation, core): the full engine is built once from the estimator's columns and
    split on the device.  With an ALS estimator `core` is the training engine and `train` is
    not materialised; any other estimator gets host dicts of columns for both parts."""
    from .. import engine as _engine
    from .recommendation import ALS
    if isinstance(estimator, ALS):
        ests = [estimator.copy(m) for m in maps]
        names = {tuple(e.getOrDefault(c) for c in ("userCol", "itemCol", "ratingCol"))
                 for e in ests}
        if len(names) != 1:
            raise ValueError("stratify=\"user\" needs one userCol / itemCol / ratingCol for "
                             "every param map")
        names, = names
        trip = ests[0]._columns(dataset)
    else:   # the estimator's own column params, else the names every estimator here defaults to
        get = getattr(estimator, "getOrDefault", None)
        names = tuple(get(c) if get is not None else d for c, d in
                      (("userCol", "user"), ("itemCol", "item"), ("ratingCol", "rating")))
        from .._data import check_integers, columns_of, to_float32
        u, i, r = columns_of(dataset, names)
        trip = check_integers(u, names[0]), check_integers(i, names[1]), to_float32(r)
    full = _engine.ALSCore(*trip)
    for kw in split_args:
        core, held = full.split(seed=seed, **kw)
        if held[0].numel() == 0:
            raise ValueError("the stratified split left the validation side empty")
        validation = {n: x.cpu().numpy() for n, x in zip(names, held)}
        if isinstance(estimator, ALS):
            yield None, validation, core
        else:
            kept = _datasets.core_triples(core)
            yield {n: x.cpu().numpy() for n, x in zip(names, kept)}, validation, None


class _Tuner:
    def _init_common(self, estimator, estimatorParamMaps, evaluator, seed, parallelism,
                     collectSubModels):
        maps = list(estimatorParamMaps) if estimatorParamMaps is not None else []
        if not maps:
            raise ValueError("estimatorParamMaps must hold at least one param map")
        if any(not isinstance(m, dict) for m in maps):
            raise TypeError("estimatorParamMaps must be a list of param maps (dicts)")
        if isinstance(parallelism, bool) or not isinstance(parallelism, (int, np.integer)) \
                or parallelism < 1:
            raise ValueError(f"parallelism must be >= 1, got {parallelism!r}")
        self.estimator, self.estimatorParamMaps, self.evaluator = estimator, maps, evaluator
        self.seed = _default_seed(self) if seed is None else int(seed)
        self.parallelism = int(parallelism)
        self.collectSubModels = bool(collectSubModels)

    def getEstimator(self):
        return self.estimator

    def getEstimatorParamMaps(self):
        return self.estimatorParamMaps

    def getEvaluator(self):
        return self.evaluator

    def getSeed(self) -> int:
        return self.seed

    def getStratify(self):
        return self.stratify


class _TunedModel:
    def transform(self, dataset):
        return self.bestModel.transform(dataset)


class TrainValidationSplitModel(_TunedModel):
    """bestModel (the best map refitted on the whole dataset), validationMetrics (one per
    map), subModels (one per map with collectSubModels, else None)."""

    def __init__(self, bestModel, validationMetrics, subModels=None):
        self.bestModel = bestModel
        self.validationMetrics = list(validationMetrics)
        self.subModels = subModels


class TrainValidationSplit(_Tuner):
    """pyspark.ml.tuning.TrainValidationSplit: one seeded split into trainRatio /
    (1 - trainRatio), every map fitted on the training part and scored on the rest."""

    def __init__(self, estimator, estimatorParamMaps, evaluator, trainRatio: float = 0.75,
                 seed=None, parallelism: int = 1, collectSubModels: bool = False,
                 stratify=None, holdOut=None):
        """stratify="user": the split is made per user on the GPU (module docstring), every
        user giving 1 - trainRatio of their ratings to the validation part, or `holdOut`
        ratings when that is given (holdOut=1 is leave-one-out, the protocol HR@k, NDCG@k and
        MRR are usually reported under)."""
        if not 0.0 < float(trainRatio) < 1.0:
            raise ValueError(f"trainRatio must be in (0, 1), got {trainRatio!r}")
        self.trainRatio = float(trainRatio)
        self.stratify = _check_stratify(stratify)
        if holdOut is not None:
            if stratify is None:
                raise ValueError("holdOut needs stratify=\"user\"")
            if isinstance(holdOut, bool) or int(holdOut) != holdOut or int(holdOut) < 1:
                raise ValueError(f"holdOut must be an integer >= 1, got {holdOut!r}")
            holdOut = int(holdOut)
        self.holdOut = holdOut
        self._init_common(estimator, estimatorParamMaps, evaluator, seed, parallelism,
                          collectSubModels)

    def getTrainRatio(self) -> float:
        return self.trainRatio

    def getHoldOut(self):
        return self.holdOut

    def split(self, n: int):
        """(training rows, validation rows) of an n-row dataset: datasets.random_split."""
        return _datasets.random_split(n, (self.trainRatio, 1.0 - self.trainRatio), self.seed)

    def fit(self, dataset) -> TrainValidationSplitModel:
        if self.stratify:
            kw = (dict(count=self.holdOut) if self.holdOut is not None
                  else dict(fraction=1.0 - self.trainRatio))
            (train, va, core), = _stratified_splits(self.estimator, self.estimatorParamMaps,
                                                    dataset, [kw], self.seed)
            metrics, subs = _fit_and_score(self.estimator, self.estimatorParamMaps,
                                           self.evaluator, train, va, self.collectSubModels,
                                           core)
            best = best_index(metrics, self.evaluator.isLargerBetter())
            return TrainValidationSplitModel(
                self.estimator.fit(dataset, self.estimatorParamMaps[best]), metrics, subs)
        tr, va = self.split(_n_rows(dataset))
        if len(tr) == 0 or len(va) == 0:
            raise ValueError("the train/validation split left one side empty")
        metrics, subs = _fit_and_score(self.estimator, self.estimatorParamMaps, self.evaluator,
                                       _take(dataset, tr), _take(dataset, va),
                                       self.collectSubModels)
        best = best_index(metrics, self.evaluator.isLargerBetter())
        return TrainValidationSplitModel(
            self.estimator.fit(dataset, self.estimatorParamMaps[best]), metrics, subs)


class CrossValidatorModel(_TunedModel):
    """bestModel (the best map refitted on the whole dataset), avgMetrics / stdMetrics (mean
    and population standard deviation over the folds, one per map), subModels
    ([fold][map] with collectSubModels, else None)."""

    def __init__(self, bestModel, avgMetrics, stdMetrics, subModels=None):
        self.bestModel = bestModel
        self.avgMetrics = list(avgMetrics)
        self.stdMetrics = list(stdMetrics)
        self.subModels = subModels


class CrossValidator(_Tuner):
    """pyspark.ml.tuning.CrossValidator: numFolds folds (seeded, or read from the integer
    column foldCol with values in [0, numFolds)); every map is fitted on the other folds
    and scored on each fold in turn."""

    def __init__(self, estimator, estimatorParamMaps, evaluator, numFolds: int = 3,
                 foldCol: str = "", seed=None, parallelism: int = 1,
                 collectSubModels: bool = False, stratify=None):
        """stratify="user": fold f holds, of every user, part f of numFolds parts of their
        ratings (sizes within one of each other), made on the GPU (module docstring); it
        cannot be combined with foldCol."""
        if isinstance(numFolds, bool) or not isinstance(numFolds, (int, np.integer)) \
                or numFolds < 2:
            raise ValueError(f"numFolds must be >= 2, got {numFolds!r}")
        self.numFolds = int(numFolds)
        self.foldCol = str(foldCol or "")
        self.stratify = _check_stratify(stratify)
        if self.stratify and self.foldCol:
            raise ValueError("foldCol and stratify cannot be combined: the folds come from one "
                             "or the other")
        self._init_common(estimator, estimatorParamMaps, evaluator, seed, parallelism,
                          collectSubModels)

    def getNumFolds(self) -> int:
        return self.numFolds

    def getFoldCol(self) -> str:
        return self.foldCol

    def folds(self, dataset) -> np.ndarray:
        """Fold of every row of `dataset`."""
        if not self.foldCol:
            return fold_assignment(_n_rows(dataset), self.numFolds, self.seed)
        try:
            col = np.asarray(dataset[self.foldCol])
        except (KeyError, IndexError, TypeError):
            raise ValueError(f"dataset has no column {self.foldCol!r}") from None
        if col.dtype.kind not in "iu":
            if col.dtype.kind != "f" or not np.all(col == np.round(col)):
                raise ValueError(f"foldCol {self.foldCol!r} must hold integers")
        f = col.astype(np.int64)
        if f.size and (f.min() < 0 or f.max() >= self.numFolds):
            raise ValueError(f"foldCol {self.foldCol!r} must hold values in [0, {self.numFolds}), "
                             f"got {int(f.min())} .. {int(f.max())}")
        return f

    def _splits(self, dataset):
        """(train, validation, training engine or None) of every fold."""
        if self.stratify:
            kws = [dict(fold=(f, self.numFolds)) for f in range(self.numFolds)]
            yield from _stratified_splits(self.estimator, self.estimatorParamMaps, dataset, kws,
                                          self.seed)
            return
        fold = self.folds(dataset)
        for f in range(self.numFolds):
            va, tr = np.nonzero(fold == f)[0], np.nonzero(fold != f)[0]
            if len(tr) == 0 or len(va) == 0:
                raise ValueError(f"fold {f} left the training or the validation side empty")
            yield _take(dataset, tr), _take(dataset, va), None

    def fit(self, dataset) -> CrossValidatorModel:
        all_metrics, subs = [], ([] if self.collectSubModels else None)
        for train, va, core in self._splits(dataset):
            m, s = _fit_and_score(self.estimator, self.estimatorParamMaps, self.evaluator,
                                  train, va, self.collectSubModels, core)
            all_metrics.append(m)
            if subs is not None:
                subs.append(s)
        all_metrics = np.asarray(all_metrics, np.float64)
        avg, std = all_metrics.mean(axis=0), all_metrics.std(axis=0)
        best = best_index(avg, self.evaluator.isLargerBetter())
        return CrossValidatorModel(self.estimator.fit(dataset, self.estimatorParamMaps[best]),
                                   avg.tolist(), std.tolist(), subs)
