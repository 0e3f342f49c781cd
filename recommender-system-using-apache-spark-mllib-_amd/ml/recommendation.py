"""pyspark.ml.recommendation-compatible surface: ALS (estimator) and ALSModel.

Drop-in for the north-star API of the reference's ALS path
(``pyspark.ml.recommendation.ALS(rank, maxIter, regParam, implicitPrefs,
alpha, coldStartStrategy, ...)`` with ``fit()`` / ``transform()`` /
``recommendForAllUsers()``), backed by the MI355X engine (als_mi355x.engine).
Datasets are pandas DataFrames (or dicts of arrays) instead of Spark
DataFrames; column names, parameter names, defaults and error conditions
follow Spark's ``ALSParams`` (ml/recommendation/ALS.scala, upstream).
"""
from __future__ import annotations

import zlib
from typing import Optional

import numpy as np
import torch

from .. import engine as _engine
from .._data import check_integers, columns_of, to_float32
from .param import Param

__all__ = ["ALS", "ALSModel", "BaselinePredictor", "BaselineModel"]

_DEFAULT_SEED = zlib.crc32(b"org.apache.spark.ml.recommendation.ALS")
_COLD = ("nan", "drop")
_SOLVERS = ("cholesky", "nnls")


def _validate(p: dict) -> None:
    """ALSParams validators (ParamValidators.gtEq / inArray), IllegalArgumentException -> ValueError."""
    if not isinstance(p["rank"], (int, np.integer)) or p["rank"] < 1:
        raise ValueError(f"ALS_rank parameter rank given invalid value {p['rank']} (must be >= 1)")
    if not isinstance(p["maxIter"], (int, np.integer)) or p["maxIter"] < 0:
        raise ValueError(f"ALS_maxIter parameter maxIter given invalid value {p['maxIter']}")
    if p["regParam"] < 0:
        raise ValueError(f"ALS_regParam parameter regParam given invalid value {p['regParam']}")
    if p["alpha"] < 0:
        raise ValueError(f"ALS_alpha parameter alpha given invalid value {p['alpha']}")
    if p["numUserBlocks"] < 1 or p["numItemBlocks"] < 1:
        raise ValueError("numUserBlocks/numItemBlocks must be >= 1")
    if p["checkpointInterval"] < 1 and p["checkpointInterval"] != -1:
        raise ValueError("checkpointInterval must be -1 or >= 1")
    if str(p["coldStartStrategy"]).lower() not in _COLD:
        raise ValueError(f"ALS_coldStartStrategy parameter coldStartStrategy given invalid value "
                         f"{p['coldStartStrategy']} (supported: {', '.join(_COLD)})")
    if p["rank"] > 128:
        raise NotImplementedError("rank > 128 is not supported by this build of the HIP kernels")
    if p["nonnegative"]:
        raise NotImplementedError(
            "the Spark parameter nonnegative=True is not wired to the NNLS solver yet: use "
            "ALS.setSolver(\"nnls\") (K13), which fits the same nonnegative model")


class _Params:
    _defaults = dict(rank=10, maxIter=10, regParam=0.1, numUserBlocks=10, numItemBlocks=10,
                     implicitPrefs=False, alpha=1.0, userCol="user", itemCol="item", seed=None,
                     ratingCol="rating", nonnegative=False, checkpointInterval=10,
                     intermediateStorageLevel="MEMORY_AND_DISK",
                     finalStorageLevel="MEMORY_AND_DISK", coldStartStrategy="nan",
                     blockSize=4096, predictionCol="prediction")

    def _init_params(self, kw):
        unknown = set(kw) - set(self._defaults)
        if unknown:
            raise TypeError(f"unexpected keyword argument(s): {sorted(unknown)}")
        self._p = dict(self._defaults)
        self._p.update(kw)

    def getOrDefault(self, name):
        return self._p[name.name if isinstance(name, Param) else name]


def _make_accessors(cls, names):
    for n in names:
        cap = n[0].upper() + n[1:]

        def setter(self, value, _n=n):
            self._p[_n] = value
            return self

        def getter(self, _n=n):
            return self._p[_n]

        setattr(cls, "set" + cap, setter)
        setattr(cls, "get" + cap, getter)


class ALS(_Params):
    """Alternating Least Squares (explicit or implicit feedback) on one MI355X.

    ``numUserBlocks`` / ``numItemBlocks`` / storage levels are accepted for signature
    compatibility and have no effect (the ratings are a single device-resident CSR
    per side).  ``checkpointInterval`` acts as in Spark once a checkpoint directory
    is set (``setCheckpointDir``, the role of ``SparkContext.setCheckpointDir``):
    the factors are written every ``checkpointInterval`` iterations, and a fit of
    the same ratings and params in that directory resumes from the checkpoint
    (checkpoint.py) instead of starting over.
    """

    def __init__(self, **kw):
        self._init_params(kw)
        self._checkpoint_dir = None
        self._objective_every = 0
        self._objective_tol = None
        self._solver = "cholesky"

    def setSolver(self, value):
        """The per-row solver of every half-sweep: "cholesky" (the default, Spark's
        CholeskySolver) or "nnls" — Spark's NNLSSolver, what `nonnegative=True` selects in
        Spark: every factor of the fitted model is >= 0 (K13).  Not a Spark Param: it is not
        saved with the model nor enumerated by the tuners, and copy() carries it over.  The
        fitted model's `solver` records it, and the model's fold-in methods follow it.  Not
        together with a checkpoint directory (a checkpoint does not record the solver)."""
        if value not in _SOLVERS:
            raise ValueError(f"solver must be one of {_SOLVERS}, got {value!r}")
        self._solver = value
        return self

    def getSolver(self) -> str:
        return self._solver

    def setCheckpointDir(self, path):
        """Directory for factor checkpoints (None disables)."""
        self._checkpoint_dir = None if path is None else str(path)
        return self

    def setObjectiveHistory(self, every=1, tol=None):
        """Record the training objective (K10: the loss ALS itself minimises, on the training
        data the engine holds) after every `every`-th iteration and after the last one, and
        with `tol` stop the fit once an evaluated iteration lowers it by no more than
        tol * its previous value.  every=0 and tol=None switch both off (the default: fit
        evaluates nothing).  Not a Spark Param: it is not saved with the model nor
        enumerated by the tuners, and copy() carries it over.  The fitted model's
        objectiveHistory / objectiveIterations hold the values."""
        every = int(every)
        if every < 0:
            raise ValueError(f"every must be >= 0, got {every}")
        if tol is not None and not float(tol) >= 0:
            raise ValueError(f"tol must be >= 0, got {tol}")
        self._objective_every = every
        self._objective_tol = None if tol is None else float(tol)
        return self

    def setParams(self, **kw):
        for k, v in kw.items():
            if k not in self._defaults:
                raise TypeError(f"unknown parameter {k}")
            self._p[k] = v
        return self

    def setNumBlocks(self, value):
        self._p["numUserBlocks"] = value
        self._p["numItemBlocks"] = value
        return self

    def copy(self, extra=None) -> "ALS":
        """A new estimator with the same params, checkpoint directory, solver and
        objective-history setting; `extra` (a param map: Param objects or names -> values) is applied to the
        copy."""
        other = ALS(**self._p)
        other._checkpoint_dir = self._checkpoint_dir
        other._objective_every = self._objective_every
        other._objective_tol = self._objective_tol
        other._solver = self._solver
        for key, value in self._param_map(extra).items():
            other._p[key] = value
        return other

    @classmethod
    def _param_map(cls, params) -> dict:
        """A param map with its keys resolved to names; anything else is refused."""
        if params is None:
            return {}
        if not isinstance(params, dict):
            raise TypeError("params must be a param map (dict of Param or name -> value), a "
                            f"list/tuple of them, or None; got {type(params).__name__}")
        out = {}
        for key, value in params.items():
            if isinstance(key, Param):
                if key.parent != cls.__name__ or key.name not in cls._defaults:
                    raise ValueError(f"{key!r} is not a parameter of {cls.__name__}")
                name = key.name
            elif isinstance(key, str):
                if key not in cls._defaults:
                    raise ValueError(f"{key!r} is not a parameter of {cls.__name__}")
                name = key
            else:
                raise TypeError(f"param map keys must be Param objects or names, got {key!r}")
            out[name] = value
        return out

    def _columns(self, dataset):
        """(users int32, items int32, ratings f32) of `dataset` by this estimator's columns."""
        p = self._p
        u, i, r = columns_of(dataset, (p["userCol"], p["itemCol"], p["ratingCol"]))
        return check_integers(u, p["userCol"]), check_integers(i, p["itemCol"]), to_float32(r)

    def _fit_core(self, core, checkpoints: bool = True):
        """One fit of `core` (re-initialising its factors) with this estimator's params."""
        p = self._p
        _validate(p)
        seed = _DEFAULT_SEED if p["seed"] is None else int(p["seed"])
        observe = {}
        if self._objective_every or self._objective_tol is not None:
            observe = dict(objective_every=self._objective_every, tol=self._objective_tol)
        if self._solver == "nnls":
            observe["nonnegative"] = True
        core.fit(int(p["rank"]), int(p["maxIter"]), float(p["regParam"]),
                 bool(p["implicitPrefs"]), float(p["alpha"]), seed=seed,
                 checkpoint_dir=self._checkpoint_dir if checkpoints else None,
                 checkpoint_interval=int(p["checkpointInterval"]), resume="auto", **observe)
        return core

    def fit(self, dataset, params=None):
        """Fit on `dataset`.  params: a param map (Param objects or names -> values) applied
        to a copy of this estimator, or a list / tuple of maps, which returns the list of
        their models (pyspark's Estimator.fit)."""
        if isinstance(params, (list, tuple)):
            return [self.fit(dataset, m) for m in params]
        if params is not None:
            return self.copy(params).fit(dataset)
        _validate(self._p)
        core = _engine.make_engine(*self._columns(dataset))
        model = ALSModel(self._fit_core(core), dict(self._p), solver=self._solver)
        # ALSModel.update's refit records the objective as this fit did
        model._objective_every = self._objective_every or int(self._objective_tol is not None)
        return model

    def fitHoldout(self, dataset, *, count: int = 1, k: int = 10, seed=None, exclude="train"):
        """The usual leave-one-out report in one call: hold `count` ratings of every user out
        (ALSCore.split on the GPU, K20: chosen from (seed, user id, item id), no item leaves
        the training part), fit on the rest and score the held-out rows.  Returns (model,
        metrics): the model fitted on the training part and evaluateRanking at k merged with
        evaluateFullRanking (whose "rows" is kept as "fullRows"), both with `exclude`.  seed
        None = this estimator's seed."""
        _validate(self._p)
        p = self._p
        full = _engine.make_engine(*self._columns(dataset))
        if not isinstance(full, _engine.ALSCore):
            raise NotImplementedError("fitHoldout needs the single-GPU engine")
        seed = (_DEFAULT_SEED if p["seed"] is None else int(p["seed"])) if seed is None else seed
        core, held = full.split(count=int(count), seed=int(seed))
        del full
        model = ALSModel(self._fit_core(core), dict(p), solver=self._solver)
        test = {c: x.cpu().numpy() for c, x in zip((p["userCol"], p["itemCol"], p["ratingCol"]),
                                                   held)}
        metrics = dict(model.evaluateRanking(test, int(k), exclude=exclude))
        full_rank = model.evaluateFullRanking(test, exclude=exclude)
        metrics.update({("fullRows" if key == "rows" else key): v
                        for key, v in full_rank.items()})
        return model, metrics


_make_accessors(ALS, list(_Params._defaults))
for _name in _Params._defaults:  # ALS.rank, als.regParam, ...: the keys of a param map
    setattr(ALS, _name, Param("ALS", _name))
del _name


class ALSModel:
    """Fitted factors resident in HBM; mirrors pyspark.ml.recommendation.ALSModel."""

    def __init__(self, core: "_engine.ALSCore", params: dict, solver: str = "cholesky"):
        self._core = core
        self._p = params
        self._solver = solver
        # the fit's (iteration, objective) pairs, copied: a tuner refits the same core
        self._objective_history = list(getattr(core, "objective_history", ()))
        self._objective_every = 0   # ALS.fit sets it from setObjectiveHistory

    # -- params used at transform time --
    def setUserCol(self, v):
        self._p["userCol"] = v
        return self

    def setItemCol(self, v):
        self._p["itemCol"] = v
        return self

    def setPredictionCol(self, v):
        self._p["predictionCol"] = v
        return self

    def setColdStartStrategy(self, v):
        if str(v).lower() not in _COLD:
            raise ValueError(f"ALS_coldStartStrategy parameter coldStartStrategy given invalid "
                             f"value {v} (supported: {', '.join(_COLD)})")
        self._p["coldStartStrategy"] = v
        return self

    def setBlockSize(self, v):
        self._p["blockSize"] = v
        return self

    @property
    def rank(self) -> int:
        return self._core.rank

    @property
    def engine(self) -> "_engine.ALSCore":
        return self._core

    @property
    def solver(self) -> str:
        """The per-row solver the model was fitted with (ALS.setSolver): "cholesky" or
        "nnls".  It is not saved: a loaded model says "cholesky"."""
        return self._solver

    def _nonnegative(self, nonnegative) -> bool:
        return self._solver == "nnls" if nonnegative is None else bool(nonnegative)

    @property
    def objectiveHistory(self):
        """The training objective after each evaluated iteration of the fit (named after
        Spark's training summaries; ALS.setObjectiveHistory switches it on).  Empty when
        the fit recorded none and for a loaded model."""
        return [v for _, v in self._objective_history]

    @property
    def objectiveIterations(self):
        """The iteration number (1-based) of each entry of objectiveHistory."""
        return [it for it, _ in self._objective_history]

    def trainingObjective(self) -> dict:
        """The objective of the model's factors on its training data, for the regParam /
        implicitPrefs / alpha it was fitted with (K10, ALSCore.objective): {"objective",
        "data", "reg", "scale", "n", "n_positive"}.  Raises ValueError on a loaded model,
        which holds no training data."""
        p = self._p
        return self._core.objective(float(p["regParam"]), bool(p["implicitPrefs"]),
                                    float(p["alpha"]))

    def update(self, dataset, maxIter: int = 2, mode: str = "refit", replace: bool = False
               ) -> "ALSModel":
        """Add the ratings of `dataset` (this model's userCol / itemCol / ratingCol) to the
        model's training data and bring the factors up to date, without building the model
        again (K17, ALSCore.add_ratings).  THIS MODEL IS CHANGED IN PLACE and returned; new
        users and items become rows of userFactors / itemFactors.
        mode: "refit"   maxIter warm iterations over all rows from the current user factors,
                        with the regParam / implicitPrefs / alpha / solver of the fit;
                        objectiveHistory then holds the refit's values when the estimator
                        had setObjectiveHistory on
              "refresh" only the users and items of `dataset` are solved again, everyone
                        else keeps their factors (ALSCore.refresh)
              "none"    the ratings are merged and new rows get fold-in factors; nothing
                        else moves.
        replace=True: a rating of a (user, item) pair the model already holds takes the
        place of every stored one instead of standing beside it, and of a pair that is
        several times in `dataset` the last counts (K18, ALSCore.set_ratings).
        Not on a loaded model (no training data) nor on the sharded engine."""
        if mode not in ("refit", "refresh", "none"):
            raise ValueError(f"mode must be 'refit', 'refresh' or 'none', got {mode!r}")
        p = self._p
        u, i, r = columns_of(dataset, (p["userCol"], p["itemCol"], p["ratingCol"]))
        seed = _DEFAULT_SEED if p["seed"] is None else int(p["seed"])
        change = self._core.set_ratings if replace else self._core.add_ratings
        change(check_integers(u, p["userCol"]), check_integers(i, p["itemCol"]), to_float32(r),
               seed=seed)
        return self._bring_up_to_date(maxIter, mode)

    def _bring_up_to_date(self, maxIter, mode) -> "ALSModel":
        if mode == "refit":
            observe = {"objective_every": self._objective_every} if self._objective_every else {}
            self._core.refit(int(maxIter), **observe)
            self._objective_history = list(self._core.objective_history)
        elif mode == "refresh":
            self._core.refresh()
        return self

    def remove(self, dataset, maxIter: int = 2, mode: str = "refit") -> "ALSModel":
        """Take the ratings of the (userCol, itemCol) pairs of `dataset` out of the model's
        training data — every stored rating of each pair — and bring the factors up to date
        without building the model again (K18, ALSCore.remove_ratings).  THIS MODEL IS
        CHANGED IN PLACE and returned.  A user or item left without a rating leaves
        userFactors / itemFactors; a pair the model does not hold is ignored.  mode as in
        update(): "refit", "refresh" (only the users and items that lost a rating are solved
        again) or "none".  Not on a loaded model nor on the sharded engine."""
        if mode not in ("refit", "refresh", "none"):
            raise ValueError(f"mode must be 'refit', 'refresh' or 'none', got {mode!r}")
        p = self._p
        u, i = columns_of(dataset, (p["userCol"], p["itemCol"]))
        self._core.remove_ratings(check_integers(u, p["userCol"]),
                                  check_integers(i, p["itemCol"]))
        return self._bring_up_to_date(maxIter, mode)

    def removeUsers(self, ids, maxIter: int = 2, mode: str = "refit") -> "ALSModel":
        """remove() of every rating of the listed user ids: they leave the model, and so
        does an item only they had rated."""
        if mode not in ("refit", "refresh", "none"):
            raise ValueError(f"mode must be 'refit', 'refresh' or 'none', got {mode!r}")
        self._core.remove_users(check_integers(np.asarray(list(ids)), self._p["userCol"]))
        return self._bring_up_to_date(maxIter, mode)

    def removeItems(self, ids, maxIter: int = 2, mode: str = "refit") -> "ALSModel":
        """remove() of every rating of the listed item ids."""
        if mode not in ("refit", "refresh", "none"):
            raise ValueError(f"mode must be 'refit', 'refresh' or 'none', got {mode!r}")
        self._core.remove_items(check_integers(np.asarray(list(ids)), self._p["itemCol"]))
        return self._bring_up_to_date(maxIter, mode)

    def _factors_df(self, ids, F):
        import pandas as pd
        ids = ids.cpu().numpy()
        F = F.float().cpu().numpy()
        return pd.DataFrame({"id": ids, "features": list(F)})

    def save(self, path: str, overwrite: bool = False) -> None:
        """ALSModel.save(path) / write().save(path) in Spark's layout."""
        from .. import persistence
        uids, U = self._core.user_factors()
        iids, V = self._core.item_factors()
        params = {k: v for k, v in self._p.items() if isinstance(v, (int, float, str, bool))}
        persistence.save_ml(path, "ALSModel_mi355x", params, self.rank, uids.cpu().numpy(),
                            U.cpu().numpy(), iids.cpu().numpy(), V.cpu().numpy(),
                            overwrite=overwrite)

    @classmethod
    def load(cls, path: str) -> "ALSModel":
        """ALSModel.load(path): factors back into HBM (serving only), params restored."""
        from .. import persistence
        _, params, _, uids, U, iids, V = persistence.load_ml(path)
        p = dict(_Params._defaults)
        p.update({k: v for k, v in params.items() if k in p})
        return cls(_engine.ALSCore.from_factors(uids, U, iids, V), p)

    @property
    def userFactors(self):
        return self._factors_df(*self._core.user_factors())

    @property
    def itemFactors(self):
        return self._factors_df(*self._core.item_factors())

    def transform(self, dataset):
        """Append the prediction column (fp32 <u, v>; NaN for unknown ids, or those rows
        dropped when coldStartStrategy == "drop")."""
        import pandas as pd
        p = self._p
        u, i = columns_of(dataset, (p["userCol"], p["itemCol"]))
        u = check_integers(u, p["userCol"])
        i = check_integers(i, p["itemCol"])
        pred = self._core.predict(u, i).float().cpu().numpy()
        if isinstance(dataset, pd.DataFrame):
            out = dataset.copy()
        else:
            out = pd.DataFrame({p["userCol"]: u, p["itemCol"]: i})
        out[p["predictionCol"]] = pred
        if str(p["coldStartStrategy"]).lower() == "drop":
            out = out[~np.isnan(pred)]
        return out

    def rmse(self, dataset, ratingCol: Optional[str] = None) -> float:
        """RMSE over rows whose user and item are known (fused gather-dot-reduce, K4) —
        the device form of RecommenderSystem.py:103-129's computeError."""
        p = self._p
        u, i, r = columns_of(dataset, (p["userCol"], p["itemCol"], ratingCol or p["ratingCol"]))
        rm, _ = self._core.rmse(check_integers(u, p["userCol"]), check_integers(i, p["itemCol"]),
                                to_float32(r))
        return rm

    def evaluateRegression(self, dataset, ratingCol: Optional[str] = None) -> dict:
        """Spark's RegressionMetrics of the model against the held-out rows of `dataset`
        (userCol, itemCol, ratingCol), fused on the device (K8, no prediction column):
        {"mse", "rmse", "mae", "r2", "var", "n", "dropped", "meanLabel", "varLabel"}.  Rows
        whose user or item is unknown are left out and counted in "dropped" (the inner join
        of rmse(), whatever coldStartStrategy says)."""
        p = self._p
        u, i, r = columns_of(dataset, (p["userCol"], p["itemCol"], ratingCol or p["ratingCol"]))
        return self._core.regression_metrics(check_integers(u, p["userCol"]),
                                             check_integers(i, p["itemCol"]), to_float32(r))

    # -- K16: what the training ratings themselves say --
    def _statistics_df(self, user_side: bool):
        import pandas as pd
        st = self._core.rating_stats(user_side=user_side)
        col = {k: st[k].cpu().numpy() for k in ("ids", "count", "mean", "std_sample", "min", "max")}
        return pd.DataFrame({"id": col["ids"], "count": col["count"], "mean": col["mean"],
                             "stddev": col["std_sample"], "min": col["min"], "max": col["max"]})

    def itemStatistics(self):
        """A DataFrame [id, count, mean, stddev, min, max] of the training ratings of every
        item, ascending id (K16, one sweep on the device; stddev is the sample standard
        deviation of Spark's describe(), NaN for a single rating).  Raises ValueError on a
        loaded model, which holds no training data."""
        return self._statistics_df(False)

    def userStatistics(self):
        """itemStatistics for the users."""
        return self._statistics_df(True)

    def topRatedItems(self, numItems: int, minCount: int = 0, damping: float = 0.0):
        """The reference's "movies with highest average rating and more than 500 reviews"
        (RecommenderSystem.py:75-86): a DataFrame [id, mean, count] of the numItems items with
        more than minCount training ratings, by descending sum / (damping + count), ties to
        the smaller id."""
        import pandas as pd
        ids, means, counts = self._core.top_rated(int(numItems), int(minCount), False,
                                                  float(damping))
        return pd.DataFrame({"id": ids.cpu().numpy(), "mean": means.cpu().numpy(),
                             "count": counts.cpu().numpy()})

    def compareToBaseline(self, dataset, method: str = "bias", regUser: float = 10.0,
                          regItem: float = 25.0, maxIter: int = 10,
                          ratingCol: Optional[str] = None) -> dict:
        """The model beside a trivial predictor fitted on the same training ratings
        (RecommenderSystem.py:167-177 in one call): {"model": evaluateRegression(dataset),
        "baseline": the same dict for ALSCore.fit_baseline(method, ...), every row used,
        "rmseRatio": model rmse / baseline rmse}."""
        p = self._p
        u, i, r = columns_of(dataset, (p["userCol"], p["itemCol"], ratingCol or p["ratingCol"]))
        u, i, r = check_integers(u, p["userCol"]), check_integers(i, p["itemCol"]), to_float32(r)
        base = self._core.fit_baseline(method, float(regUser), float(regItem), int(maxIter))
        mine = self._core.regression_metrics(u, i, r)
        theirs = base.regression_metrics(u, i, r)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = float(np.float64(mine["rmse"]) / np.float64(theirs["rmse"]))
        return {"model": mine, "baseline": theirs, "rmseRatio": ratio}

    def evaluateRanking(self, dataset, k: int, *, ratingThreshold: Optional[float] = None,
                        exclude=None, candidates=None) -> dict:
        """Ranking quality of each user's top-k list against the held-out rows of
        `dataset` (userCol, itemCol; ratingCol too when ratingThreshold is given: only
        rows with rating >= ratingThreshold are relevant): {"precision", "recall", "map",
        "ndcg", "hitRate", "rows"} with Spark's RankingMetrics definitions at k, means
        over the users with at least one relevant row.  exclude / candidates as
        recommendForAllUsers (exclude="train" ranks unseen items only).  Lists and
        metrics stay on the device (K5, K6)."""
        p = self._p
        cols = (p["userCol"], p["itemCol"]) + ((p["ratingCol"],) if ratingThreshold is not None
                                               else ())
        got = columns_of(dataset, cols)
        return self._core.rank_metrics(
            check_integers(got[0], p["userCol"]), check_integers(got[1], p["itemCol"]), int(k),
            ratings=to_float32(got[2]) if ratingThreshold is not None else None,
            threshold=ratingThreshold, **self._filters(exclude, candidates, True))

    def evaluateFullRanking(self, dataset, *, ratingThreshold: Optional[float] = None,
                            weighted: bool = False, exclude=None, candidates=None) -> dict:
        """Where the held-out rows of `dataset` (userCol, itemCol; ratingCol too for
        ratingThreshold / weighted) sit in each user's ordering of ALL admissible items:
        {"expectedPercentileRank" (0.5 = random, lower is better; with weighted=True the
        rating-weighted measure of the implicit-ALS paper), "meanPercentileRank", "auc",
        "mrr", "rows", "pairs", "inadmissible", "dropped"} — the way to judge an
        implicitPrefs fit, whose RMSE says nothing about ranking.  exclude / candidates as
        recommendForAllUsers (exclude="train" ranks among unseen items only).  One sweep of
        the whole score matrix on the device (K9)."""
        p = self._p
        need_r = ratingThreshold is not None or weighted
        cols = (p["userCol"], p["itemCol"]) + ((p["ratingCol"],) if need_r else ())
        got = columns_of(dataset, cols)
        return self._core.full_rank_metrics(
            check_integers(got[0], p["userCol"]), check_integers(got[1], p["itemCol"]),
            ratings=to_float32(got[2]) if need_r else None, threshold=ratingThreshold,
            weighted=bool(weighted), **self._filters(exclude, candidates, True))

    # -- recommendForAll (K5) --
    def _exclude_arg(self, exclude):
        """exclude= of the recommend* methods -> the engine's form: None, "train" (the
        pairs the model was fitted on) or a dataset of (userCol, itemCol) pairs, of any
        kind transform() takes."""
        if exclude is None or isinstance(exclude, str):
            return exclude
        p = self._p
        u, i = columns_of(exclude, (p["userCol"], p["itemCol"]))
        return check_integers(u, p["userCol"]), check_integers(i, p["itemCol"])

    def _filters(self, exclude, candidates, user_side: bool):
        ex = self._exclude_arg(exclude)
        if isinstance(ex, tuple) and not user_side:
            ex = (ex[1], ex[0])  # the engine takes (query ids, other ids)
        if candidates is not None:
            col = self._p["itemCol" if user_side else "userCol"]
            candidates = check_integers(np.asarray(candidates).reshape(-1), col)
        return dict(exclude=ex, candidates=candidates)

    def recommendForAllUsersArrays(self, numItems: int, *, exclude=None, candidates=None):
        """Device tensors (user ids [n_u], item ids [n_u, t], scores [n_u, t]),
        t = min(numItems, n_items).  Multi-GPU: this rank's users (its partition).
        exclude: (user, item) pairs never to list — "train" or a dataset with the
        model's user and item columns; candidates: item ids the lists are restricted
        to.  Slots past a user's admissible items have score -inf."""
        return self._core.recommend_all(int(numItems), True,
                                        **self._filters(exclude, candidates, True))

    def recommendForAllItemsArrays(self, numUsers: int, *, exclude=None, candidates=None):
        return self._core.recommend_all(int(numUsers), False,
                                        **self._filters(exclude, candidates, False))

    @staticmethod
    def _recs_df(key_col, keys, ids, sc):
        import pandas as pd
        keys = keys.cpu().numpy()
        ids = ids.cpu().numpy()
        sc = sc.cpu().numpy()
        # empty slots (score -inf: a query row whose every score is NaN) are dropped
        recs = [[(int(a), float(b)) for a, b in zip(ri, rs) if np.isfinite(b)]
                for ri, rs in zip(ids, sc)]
        return pd.DataFrame({key_col: keys, "recommendations": recs})

    def recommendForAllUsers(self, numItems: int, *, exclude=None, candidates=None):
        """DataFrame[userCol, recommendations: list of (item, rating)], rating desc
        (ties: lower item id first).  exclude="train" leaves out what each user has
        already rated (the reference's R:229); candidates= restricts the items (its
        R:245 "more than 75 ratings"); see recommendForAllUsersArrays."""
        return self._recs_df(self._p["userCol"], *self.recommendForAllUsersArrays(
            numItems, exclude=exclude, candidates=candidates))

    def recommendForAllItems(self, numUsers: int, *, exclude=None, candidates=None):
        return self._recs_df(self._p["itemCol"], *self.recommendForAllItemsArrays(
            numUsers, exclude=exclude, candidates=candidates))

    def recommendForUserSubset(self, dataset, numItems: int, *, exclude=None, candidates=None):
        """Top items for the distinct known users of `dataset[userCol]`."""
        col = self._p["userCol"]
        ids = check_integers(columns_of(dataset, (col,))[0], col)
        return self._recs_df(col, *self._core.recommend_subset(
            ids, int(numItems), True, **self._filters(exclude, candidates, True)))

    # -- fold-in (K7): users / items the model was not fitted on --
    def _fold_args(self, dataset, user_side: bool):
        """(grouping ids, other-side ids, ratings) of `dataset` (userCol, itemCol,
        ratingCol) and the model's own regParam / implicitPrefs / alpha."""
        p = self._p
        u, i, r = columns_of(dataset, (p["userCol"], p["itemCol"], p["ratingCol"]))
        u = check_integers(u, p["userCol"])
        i = check_integers(i, p["itemCol"])
        a, b = (u, i) if user_side else (i, u)
        return (a, b, to_float32(r)), dict(reg=float(p["regParam"]),
                                           implicit=bool(p["implicitPrefs"]),
                                           alpha=float(p["alpha"]), user_side=user_side)

    def _fold_in_df(self, dataset, user_side: bool, nonnegative=None):
        args, kw = self._fold_args(dataset, user_side)
        if self._nonnegative(nonnegative):
            kw["nonnegative"] = True
        keys, X, _ = self._core.fold_in(*args, **kw)
        return self._factors_df(keys, X)

    def foldInUsers(self, dataset, nonnegative=None):
        """Factors for users that are not in the model, from their ratings alone and
        without a refit: DataFrame[id, features], one row per distinct user of `dataset`
        (userCol, itemCol, ratingCol), each solved against the fixed item factors with
        the model's regParam / implicitPrefs / alpha — one row of one ALS half-sweep.
        Items the model does not know are skipped; the model itself is not changed.
        nonnegative: solve each row under x >= 0 (K13); None = as the model was fitted
        (`solver`), False for a loaded model."""
        return self._fold_in_df(dataset, True, nonnegative)

    def foldInItems(self, dataset, nonnegative=None):
        """foldInUsers for new items against the fixed user factors."""
        return self._fold_in_df(dataset, False, nonnegative)

    def recommendForNewUsers(self, dataset, numItems: int, *, excludeRated: bool = True,
                             candidates=None, nonnegative=None):
        """Top items for users that are not in the model (foldInUsers, then K5 over the
        folded rows), in recommendForUserSubset's form.  excludeRated: a user's own rated
        items are left out of their list; candidates: item ids the lists are restricted
        to.  Users without a single rating of a known item are absent.  nonnegative: as
        foldInUsers."""
        args, kw = self._fold_args(dataset, True)
        if self._nonnegative(nonnegative):
            kw["nonnegative"] = True
        if candidates is not None:
            candidates = check_integers(np.asarray(candidates).reshape(-1), self._p["itemCol"])
        return self._recs_df(self._p["userCol"], *self._core.recommend_new(
            *args, int(numItems), exclude_rated=bool(excludeRated), candidates=candidates, **kw))

    # -- explain (K11): why was this item recommended to this user? --
    def explainRecommendations(self, dataset, numContributions: int = 10, *, ratings=None):
        """Each (userCol, itemCol) pair of `dataset` explained by the user's own ratings:
        DataFrame[userCol, itemCol, predictionCol, contributions], contributions a list of
        (item, rating, contribution) — "because you rated item 4.0" — largest contribution
        first, at most numContributions (<= 32) of them.  A prediction is the sum of one
        term per rating of the user (over ALL of them, listed or not), exact for ALS: the
        user's factor solves normal equations that are linear in those ratings (K11), with
        the model's regParam / implicitPrefs / alpha.
        ratings=None explains from the ratings the model was fitted on; a loaded model holds
        none and needs ratings= — a dataset (userCol, itemCol, ratingCol) with the ratings
        of the users to explain, who need not be in the model.  Pairs of users without
        ratings are absent; an item the model does not know gives NaN and no contributions."""
        import pandas as pd
        p = self._p
        u, i = columns_of(dataset, (p["userCol"], p["itemCol"]))
        kw = dict(reg=float(p["regParam"]), implicit=bool(p["implicitPrefs"]),
                  alpha=float(p["alpha"]))
        if ratings is not None:
            ratings, _ = self._fold_args(ratings, True)  # the same three conventions
        uu, ii, sc, ids, rat, con, n = (x.cpu().numpy() for x in self._core.explain(
            check_integers(u, p["userCol"]), check_integers(i, p["itemCol"]),
            int(numContributions), ratings=ratings, **kw))
        lists = [[(int(a), float(b), float(c)) for a, b, c in zip(ids[r, :n[r]], rat[r, :n[r]],
                                                                  con[r, :n[r]])]
                 for r in range(len(uu))]
        return pd.DataFrame({p["userCol"]: uu, p["itemCol"]: ii, p["predictionCol"]: sc,
                             "contributions": lists})

    # -- similar items / users (K12): cosine nearest neighbours inside one side's factors --
    def _similar_ids(self, dataset_or_ids, col: str):
        """A dataset holding `col` (read with columns_of, as recommendForItemSubset reads
        it), or plain ids: a scalar or a one-dimensional sequence / array / tensor."""
        x = dataset_or_ids
        if isinstance(x, torch.Tensor) and x.dim() <= 1:
            x = x.detach().cpu().numpy()
        if np.isscalar(x) or (isinstance(x, np.ndarray) and x.ndim <= 1 and not x.dtype.names) \
                or (isinstance(x, (list, tuple)) and all(np.isscalar(v) for v in x)):
            return check_integers(np.asarray(x).reshape(-1), col)
        return check_integers(columns_of(x, (col,))[0], col)

    def _similar_df(self, key_col, keys, ids, sc):
        df = self._recs_df(key_col, keys, ids, sc)
        return df.rename(columns={"recommendations": "similar"})

    def _similar(self, dataset_or_ids, num, user_side: bool, candidates):
        col = self._p["userCol" if user_side else "itemCol"]
        if candidates is not None:
            candidates = check_integers(np.asarray(candidates).reshape(-1), col)
        return self._similar_df(col, *self._core.similar(
            self._similar_ids(dataset_or_ids, col), int(num), user_side, candidates=candidates))

    def similarItems(self, dataset_or_ids, numItems: int, *, candidates=None):
        """Which items are like these?  DataFrame[itemCol, similar: list of (item,
        similarity)] for the distinct known items of `dataset_or_ids` (a dataset with the
        item column, or item ids): the numItems nearest other items by the cosine of their
        factors, most similar first (ties: lower dense row first).  candidates= restricts
        the neighbours (not the queries) to those item ids.  An item is never its own
        neighbour; items whose factors are all zero or not finite are nobody's, and get an
        empty list.  Works on a loaded model: the factors alone suffice."""
        return self._similar(dataset_or_ids, numItems, False, candidates)

    def similarUsers(self, dataset_or_ids, numUsers: int, *, candidates=None):
        """similarItems among the user factors: DataFrame[userCol, similar]."""
        return self._similar(dataset_or_ids, numUsers, True, candidates)

    def similarItemsForAllItems(self, numItems: int, *, candidates=None):
        """similarItems for every item of the model, one device sweep for all of them."""
        col = self._p["itemCol"]
        if candidates is not None:
            candidates = check_integers(np.asarray(candidates).reshape(-1), col)
        return self._similar_df(col, *self._core.similar_all(int(numItems), False,
                                                             candidates=candidates))

    # -- co-rated neighbours (K19): "who rated X also rated Y", from the ratings themselves --
    @staticmethod
    def _co_rated_df(key_col, keys, ids, sc, common):
        import pandas as pd
        keys, ids = keys.cpu().numpy(), ids.cpu().numpy()
        sc, common = sc.cpu().numpy(), common.cpu().numpy()
        rows = [[(int(a), float(b)) for a, b, c in zip(ri, rs, rc) if c > 0]
                for ri, rs, rc in zip(ids, sc, common)]
        counts = [[int(c) for c in rc if c > 0] for rc in common]
        return pd.DataFrame({key_col: keys, "similar": rows, "common": counts})

    def _co_rated(self, dataset_or_ids, num, user_side: bool, measure, minCommon, candidates):
        col = self._p["userCol" if user_side else "itemCol"]
        if candidates is not None:
            candidates = check_integers(np.asarray(candidates).reshape(-1), col)
        return self._co_rated_df(col, *self._core.co_rated(
            self._similar_ids(dataset_or_ids, col), int(num), user_side, measure=measure,
            min_common=int(minCommon), candidates=candidates))

    def coRatedItems(self, dataset_or_ids, numItems: int, measure: str = "jaccard",
                     minCommon: int = 1, candidates=None):
        """"Who rated this item also rated": DataFrame[itemCol, similar: list of (item, score),
        common: list of shared-rater counts] for the distinct known items of
        `dataset_or_ids` (as similarItems reads them): the numItems items that share the most
        raters with each in the training ratings, strongest first (ties: lower dense row
        first).  measure: "count" (c), "jaccard" (c / (n_a + n_b - c)) or "cosine"
        (c / sqrt(n_a n_b)) of the two rater sets; an item is listed from minCommon shared
        raters and, with candidates=, only when it is among those ids.  Counted from the
        ratings, exactly (K19); the factors are not used, so this is the yardstick the
        factor neighbours of similarItems can be held against (neighbourAgreement).  Raises
        ValueError on a loaded model, which holds no ratings."""
        return self._co_rated(dataset_or_ids, numItems, False, measure, minCommon, candidates)

    def coRatedUsers(self, dataset_or_ids, numUsers: int, measure: str = "jaccard",
                     minCommon: int = 1, candidates=None):
        """coRatedItems among the users: DataFrame[userCol, similar, common], common = the
        items both rated."""
        return self._co_rated(dataset_or_ids, numUsers, True, measure, minCommon, candidates)

    def coRatedItemsForAllItems(self, numItems: int, measure: str = "jaccard", minCommon: int = 1,
                                candidates=None):
        """coRatedItems for every item of the model (ALSCore.co_rated_all, which states the
        cost: quadratic in the catalogue)."""
        col = self._p["itemCol"]
        if candidates is not None:
            candidates = check_integers(np.asarray(candidates).reshape(-1), col)
        return self._co_rated_df(col, *self._core.co_rated_all(
            int(numItems), False, measure=measure, min_common=int(minCommon),
            candidates=candidates))

    def neighbourAgreement(self, dataset_or_ids, numItems: int) -> float:
        """How far the factors learnt what the ratings say: the mean over the distinct known
        items of `dataset_or_ids` of |similarItems ∩ coRatedItems| / numItems (both lists of
        numItems, coRatedItems at its defaults), in [0, 1]; NaN when no item is known."""
        col = self._p["itemCol"]
        ids = self._similar_ids(dataset_or_ids, col)
        num = int(numItems)
        _, a, sa = self._core.similar(ids, num, False)
        _, b, _, cb = self._core.co_rated(ids, num, False)
        return self._list_agreement(a, torch.isfinite(sa), b, cb > 0, num)

    @staticmethod
    def _list_agreement(a, a_ok, b, b_ok, num: int) -> float:
        """Mean over rows of |{a[r, i]: a_ok} ∩ {b[r, j]: b_ok}| / num for two id tables with
        one row per query (ids distinct within a row)."""
        if a.shape[0] == 0:
            return float("nan")
        hit = (a.unsqueeze(2) == b.unsqueeze(1)) & a_ok.unsqueeze(2) & b_ok.unsqueeze(1)
        return float(hit.any(2).sum(1).double().mean() / num)

    def recommendForItemSubset(self, dataset, numUsers: int, *, exclude=None, candidates=None):
        col = self._p["itemCol"]
        ids = check_integers(columns_of(dataset, (col,))[0], col)
        return self._recs_df(col, *self._core.recommend_subset(
            ids, int(numUsers), False, **self._filters(exclude, candidates, False)))

    # -- diversified lists (K14): maximal marginal relevance over a K5 candidate pool --
    def _diverse_df(self, key_col, keys, ids, sc, ils):
        df = self._recs_df(key_col, keys, ids, sc)
        df["intraListSimilarity"] = ils.cpu().numpy()
        return df

    def _diverse(self, num, tradeOff, user_side: bool, ids, pool, exclude, candidates):
        return self._core.recommend_diverse(
            int(num), user_side, ids=ids, trade_off=float(tradeOff), pool=pool,
            **self._filters(exclude, candidates, user_side))

    def recommendForAllUsersDiverseArrays(self, numItems: int, tradeOff: float = 0.7, *,
                                          pool=None, exclude=None, candidates=None):
        """Device tensors (user ids [n_u], item ids [n_u, t], scores [n_u, t], intra-list
        similarity f64 [n_u]); see recommendForAllUsersDiverse."""
        return self._diverse(numItems, tradeOff, True, None, pool, exclude, candidates)

    def recommendForAllUsersDiverse(self, numItems: int, tradeOff: float = 0.7, *, pool=None,
                                    exclude=None, candidates=None):
        """recommendForAllUsers re-ranked so that a list covers more than one taste:
        DataFrame[userCol, recommendations: list of (item, rating), intraListSimilarity].
        The `pool` best items of each user (None: min(256, max(4 numItems, 50))) are the
        candidates; numItems of them are picked one by one, each the candidate with the
        largest tradeOff * relevance - (1 - tradeOff) * (largest cosine to the items already
        picked) — maximal marginal relevance, relevance = the rating rescaled to [0, 1] over
        the pool.  tradeOff = 1 is recommendForAllUsers; lower values trade rating for
        variety.  The list is in pick order with the plain ratings, so it is not descending.
        intraListSimilarity: the mean cosine between the factors of the listed items (NaN
        under two items) — compare with intraListSimilarity(recommendForAllUsers(...)).
        exclude / candidates as recommendForAllUsers.  Works on a loaded model; only
        exclude="train" needs the ratings."""
        return self._diverse_df(self._p["userCol"], *self.recommendForAllUsersDiverseArrays(
            numItems, tradeOff, pool=pool, exclude=exclude, candidates=candidates))

    def recommendForAllItemsDiverse(self, numUsers: int, tradeOff: float = 0.7, *, pool=None,
                                    exclude=None, candidates=None):
        """recommendForAllUsersDiverse from the item side: DataFrame[itemCol,
        recommendations: list of (user, rating), intraListSimilarity]."""
        return self._diverse_df(self._p["itemCol"], *self._diverse(
            numUsers, tradeOff, False, None, pool, exclude, candidates))

    def recommendForUserSubsetDiverse(self, dataset, numItems: int, tradeOff: float = 0.7, *,
                                      pool=None, exclude=None, candidates=None):
        """recommendForAllUsersDiverse for the distinct known users of `dataset[userCol]`."""
        col = self._p["userCol"]
        ids = check_integers(columns_of(dataset, (col,))[0], col)
        return self._diverse_df(col, *self._diverse(numItems, tradeOff, True, ids, pool, exclude,
                                                    candidates))

    def recommendForItemSubsetDiverse(self, dataset, numUsers: int, tradeOff: float = 0.7, *,
                                      pool=None, exclude=None, candidates=None):
        col = self._p["itemCol"]
        ids = check_integers(columns_of(dataset, (col,))[0], col)
        return self._diverse_df(col, *self._diverse(numUsers, tradeOff, False, ids, pool, exclude,
                                                    candidates))

    def intraListSimilarity(self, recommendations):
        """Intra-list similarity of lists in the shape recommendForAllUsers /
        recommendForAllItems return (a key column and `recommendations`: lists of (id,
        rating) of at most 256 entries): DataFrame[key column, intraListSimilarity], the mean
        cosine between the factors of each list's ids (ids the model does not know are
        skipped; NaN under two known ids).  The key column says which side the lists hold:
        userCol = lists of items, itemCol = lists of users."""
        import pandas as pd
        p = self._p
        user_side = p["userCol"] in recommendations
        key_col = p["userCol"] if user_side else p["itemCol"]
        if key_col not in recommendations:
            raise ValueError(f"recommendations must have a {p['userCol']!r} or {p['itemCol']!r} "
                             "column")
        lists = [[int(a) for a, _ in recs] for recs in recommendations["recommendations"]]
        m = max([len(x) for x in lists] + [1])
        _, _, oi, Vo = self._core._sides(user_side)
        ids = np.zeros((len(lists), m), np.int64)
        known = np.zeros((len(lists), m), bool)
        for r, x in enumerate(lists):
            ids[r, :len(x)] = x
            known[r, :len(x)] = True
        dev = self._core.device
        rows = oi.rows_of(torch.as_tensor(ids, device=dev))
        rows = torch.where(torch.as_tensor(known, device=dev), rows, -1).to(torch.int32)
        ils = _engine.list_similarity_rows(rows, Vo, oi.n, self._core.rank)
        return pd.DataFrame({key_col: np.asarray(recommendations[key_col]),
                             "intraListSimilarity": ils.cpu().numpy()})

    # -- the lists of all users together (K15): coverage, concentration, popularity --
    def _padded_rows(self, recommendations):
        """(user_side, key column, dense rows int32 [n, m] on the device, -1 = open slot) of
        lists in the shape recommendForAllUsers / recommendForAllItems return."""
        p = self._p
        user_side = p["userCol"] in recommendations
        key_col = p["userCol"] if user_side else p["itemCol"]
        if key_col not in recommendations:
            raise ValueError(f"recommendations must have a {p['userCol']!r} or {p['itemCol']!r} "
                             "column")
        lists = [[int(a) for a, _ in recs] for recs in recommendations["recommendations"]]
        m = max([len(x) for x in lists] + [1])
        _, _, oi, _ = self._core._sides(user_side)
        ids = np.zeros((len(lists), m), np.int64)
        known = np.zeros((len(lists), m), bool)
        for r, x in enumerate(lists):
            ids[r, :len(x)] = x
            known[r, :len(x)] = True
        dev = self._core.device
        rows = oi.rows_of(torch.as_tensor(ids, device=dev))
        rows = torch.where(torch.as_tensor(known, device=dev), rows, -1).to(torch.int32)
        return user_side, key_col, rows

    def _list_quality(self, recommendations, numItems, exclude, candidates, headFraction,
                      popularity, per_row):
        if (recommendations is None) == (numItems is None):
            raise ValueError("pass either recommendations or numItems=, not both and not neither")
        if popularity is not None:
            ids, cnt = popularity
            popularity = (check_integers(np.asarray(ids).reshape(-1), "popularity ids"),
                          check_integers(np.asarray(cnt).reshape(-1), "popularity counts"))
        kw = dict(popularity=popularity, head_fraction=float(headFraction), per_row=per_row)
        if numItems is not None:
            out = self._core.list_metrics(top=int(numItems), user_side=True,
                                          **self._filters(exclude, candidates, True), **kw)
            return out, self._p["userCol"], out.get("keys")
        if exclude is not None:
            raise ValueError("exclude= shapes the lists made with numItems=; given "
                             "recommendations are taken as they are")
        user_side, key_col, rows = self._padded_rows(recommendations)
        out = self._core._list_metrics_of_rows(
            rows, user_side, candidates=self._filters(None, candidates, user_side)["candidates"],
            **kw)
        return out, key_col, np.asarray(recommendations[key_col])

    def evaluateListQuality(self, recommendations=None, *, numItems=None, exclude=None,
                            candidates=None, headFraction: float = 0.2, popularity=None) -> dict:
        """Do all users get the same few blockbusters?  The lists of everybody looked at
        together (K15): {"coverage" (share of the catalogue listed at least once), "gini" and
        "entropy" of item exposure, "effectiveItems" (2 ** entropy), "personalization" (1 - the
        mean overlap of two users' lists), "topItemShare", "novelty" (mean self-information,
        bits), "averagePopularity", "longTailShare", "lists", "entries", "skipped"}.
        recommendations: a DataFrame as recommendForAllUsers / recommendForAllUsersDiverse
        return (lists of at most 256 entries; the key column decides the side, as in
        intraListSimilarity); or numItems=: the lists are made here, with exclude / candidates
        as recommendForAllUsers.  candidates also defines the catalogue.  headFraction: the
        most-rated share of the catalogue that is NOT the long tail.  Popularity is how often
        each item was rated in the data the model was fitted on; a loaded model has none and
        takes popularity=(item ids, counts) — without it the three popularity fields are NaN."""
        return self._list_quality(recommendations, numItems, exclude, candidates, headFraction,
                                  popularity, False)[0]

    def listQualityPerRow(self, recommendations=None, *, numItems=None, exclude=None,
                          candidates=None, headFraction: float = 0.2, popularity=None):
        """evaluateListQuality's popularity measures list by list: DataFrame[key column,
        novelty, averagePopularity, longTailShare], NaN where a list has nothing to measure."""
        import pandas as pd
        out, key_col, keys = self._list_quality(recommendations, numItems, exclude, candidates,
                                                headFraction, popularity, True)
        pr = out["per_row"].cpu().numpy()
        keys = keys.cpu().numpy() if isinstance(keys, torch.Tensor) else keys
        return pd.DataFrame({key_col: keys, "novelty": pr[:, 0], "averagePopularity": pr[:, 1],
                             "longTailShare": pr[:, 2]})


# ---------------------------------------------------------------------------
# K16: the baseline a recommender is judged against
# ---------------------------------------------------------------------------
_BASE_COLD = ("fallback", "nan", "drop")


class BaselinePredictor:
    """mu + b_u + b_i with damped biases (Koren's baseline predictor), fitted on the device
    (ALSCore.fit_baseline).  method: "global" (the training mean, RecommenderSystem.py:172-177),
    "item", "user" or "bias" (maxIter alternating sweeps).  regUser / regItem are the damping
    terms.  An estimator like ALS: fit(dataset, params), copy(extra), get/set accessors, and
    BaselinePredictor.regItem etc. as the keys of a param map, so TrainValidationSplit and
    CrossValidator take it as they take any estimator."""

    _defaults = dict(method="bias", regUser=10.0, regItem=25.0, maxIter=10, userCol="user",
                     itemCol="item", ratingCol="rating", predictionCol="prediction",
                     coldStartStrategy="fallback")

    def __init__(self, **kw):
        unknown = set(kw) - set(self._defaults)
        if unknown:
            raise TypeError(f"unexpected keyword argument(s): {sorted(unknown)}")
        self._p = dict(self._defaults)
        self._p.update(kw)

    def getOrDefault(self, name):
        return self._p[name.name if isinstance(name, Param) else name]

    _param_map = classmethod(ALS._param_map.__func__)

    def copy(self, extra=None) -> "BaselinePredictor":
        other = BaselinePredictor(**self._p)
        other._p.update(self._param_map(extra))
        return other

    @staticmethod
    def _validate(p: dict) -> None:
        if p["method"] not in _engine.BASELINE_METHODS:
            raise ValueError(f"method must be one of {_engine.BASELINE_METHODS}, got "
                             f"{p['method']!r}")
        if not float(p["regUser"]) >= 0 or not float(p["regItem"]) >= 0:
            raise ValueError("regUser and regItem must be >= 0")
        if not isinstance(p["maxIter"], (int, np.integer)) or p["maxIter"] < 1:
            raise ValueError(f"maxIter must be an integer >= 1, got {p['maxIter']!r}")
        if str(p["coldStartStrategy"]).lower() not in _BASE_COLD:
            raise ValueError(f"coldStartStrategy given invalid value {p['coldStartStrategy']} "
                             f"(supported: {', '.join(_BASE_COLD)})")

    def fit(self, dataset, params=None):
        """Fit on `dataset`; params as ALS.fit takes them (a map, or a list of maps)."""
        if isinstance(params, (list, tuple)):
            return [self.fit(dataset, m) for m in params]
        if params is not None:
            return self.copy(params).fit(dataset)
        p = self._p
        self._validate(p)
        u, i, r = columns_of(dataset, (p["userCol"], p["itemCol"], p["ratingCol"]))
        core = _engine.make_engine(check_integers(u, p["userCol"]),
                                   check_integers(i, p["itemCol"]), to_float32(r))
        base = core.fit_baseline(p["method"], float(p["regUser"]), float(p["regItem"]),
                                 int(p["maxIter"]))
        return BaselineModel(base, dict(p))


_make_accessors(BaselinePredictor, list(BaselinePredictor._defaults))
for _name in BaselinePredictor._defaults:
    setattr(BaselinePredictor, _name, Param("BaselinePredictor", _name))
del _name


class BaselineModel:
    """A fitted BaselinePredictor: globalMean, userBias / itemBias, transform and
    evaluateRegression.  Save / load are not offered."""

    def __init__(self, baseline: "_engine.Baseline", params: dict):
        self._base = baseline
        self._p = params

    @property
    def baseline(self) -> "_engine.Baseline":
        return self._base

    @property
    def globalMean(self) -> float:
        return self._base.mu

    @property
    def objectiveHistory(self):
        """SSE + regUser sum b_u^2 + regItem sum b_i^2 on the training data after every
        sweep."""
        return list(self._base.history)

    def _bias_df(self, idx, b):
        import pandas as pd
        return pd.DataFrame({"id": idx.ids().cpu().numpy(), "bias": b.cpu().numpy()})

    @property
    def userBias(self):
        return self._bias_df(self._base.uidx, self._base.bu)

    @property
    def itemBias(self):
        return self._bias_df(self._base.iidx, self._base.bi)

    def setColdStartStrategy(self, v):
        if str(v).lower() not in _BASE_COLD:
            raise ValueError(f"coldStartStrategy given invalid value {v} (supported: "
                             f"{', '.join(_BASE_COLD)})")
        self._p["coldStartStrategy"] = v
        return self

    def setPredictionCol(self, v):
        self._p["predictionCol"] = v
        return self

    def transform(self, dataset):
        """Append the prediction column (fp32).  coldStartStrategy "fallback": an unknown user
        or item adds a zero bias, so no row is NaN and a pair unknown on both sides gets
        globalMean; "nan": NaN where either id is unknown, as ALSModel; "drop": those rows
        dropped."""
        import pandas as pd
        p = self._p
        u, i = columns_of(dataset, (p["userCol"], p["itemCol"]))
        u, i = check_integers(u, p["userCol"]), check_integers(i, p["itemCol"])
        pred, known = self._base.predict(u, i, return_known=True)
        pred, known = pred.cpu().numpy(), known.cpu().numpy()
        cold = str(p["coldStartStrategy"]).lower()
        if cold != "fallback":
            pred = np.where(known == 3, pred, np.float32("nan"))
        if isinstance(dataset, pd.DataFrame):
            out = dataset.copy()
        else:
            out = pd.DataFrame({p["userCol"]: u, p["itemCol"]: i})
        out[p["predictionCol"]] = pred
        if cold == "drop":
            out = out[known == 3]
        return out

    def evaluateRegression(self, dataset, ratingCol: Optional[str] = None) -> dict:
        """ALSModel.evaluateRegression's dict for the baseline's predictions; every row is
        used (the fallback prediction), so "dropped" is 0."""
        p = self._p
        u, i, r = columns_of(dataset, (p["userCol"], p["itemCol"], ratingCol or p["ratingCol"]))
        return self._base.regression_metrics(check_integers(u, p["userCol"]),
                                             check_integers(i, p["itemCol"]), to_float32(r))
