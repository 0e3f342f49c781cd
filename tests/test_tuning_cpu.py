"""CPU tests of ml.tuning (no GPU): the grid builder, Param and ALS.copy / fit(dataset,
params), the folds, the choice of the winner and the two tuners' bookkeeping, with stub
estimator / model / evaluator classes (any pair that is not ALS + RegressionEvaluator goes
through evaluator.evaluate(model.transform(validation)))."""
import math

import numpy as np
import pandas as pd
import pytest

from als_mi355x.ml import tuning as T
from als_mi355x.ml.param import Param
from als_mi355x.ml.recommendation import ALS, ALSModel


# ------------------------------------------------------------------ stubs
class StubModel:
    def __init__(self, params, n_train, train_sum):
        self.params, self.n_train, self.train_sum = dict(params), n_train, train_sum

    def transform(self, dataset):
        out = dataset.copy()
        out["prediction"] = self.params.get("a", 0.0)
        out["model"] = [self] * len(out)
        return out


class StubEstimator:
    """fit(dataset, params) records its calls; the model remembers what it was fitted on."""

    def __init__(self):
        self.calls = []

    def fit(self, dataset, params=None):
        self.calls.append((len(dataset), dict(params or {})))
        return StubModel(params or {}, len(dataset), float(np.sum(dataset["y"])))


class StubEvaluator:
    """metric = table[a] (+ the validation fold's mean of y when by_fold) — or NaN."""

    def __init__(self, table, larger=False, by_fold=False):
        self.table, self.larger, self.by_fold = table, larger, by_fold
        self.seen = []

    def isLargerBetter(self):
        return self.larger

    def evaluate(self, dataset):
        a = float(dataset["prediction"].iloc[0])
        self.seen.append((a, len(dataset)))
        return self.table[a] + (float(dataset["y"].mean()) if self.by_fold else 0.0)


DATA = pd.DataFrame({"y": np.arange(200, dtype=np.float64), "fold": np.arange(200) % 4})
MAPS = [{"a": 1.0}, {"a": 2.0}, {"a": 3.0}]


# ------------------------------------------------------------------ Param, ALS
def test_param_is_a_dict_key_equal_by_parent_and_name():
    assert ALS.rank == Param("ALS", "rank") and hash(ALS.rank) == hash(Param("ALS", "rank"))
    assert ALS.rank != ALS.regParam and ALS.rank != Param("Other", "rank") and ALS.rank != "rank"
    als = ALS()
    assert als.rank is ALS.rank
    assert {als.rank: 1}[Param("ALS", "rank")] == 1
    for name in ALS._defaults:
        p = getattr(ALS, name)
        assert isinstance(p, Param) and (p.parent, p.name) == ("ALS", name)
    assert isinstance(ALSModel.rank, property)     # the fitted model's rank stays an int


def test_als_copy():
    als = ALS(rank=7, regParam=0.3).setCheckpointDir("/tmp/ckpt")
    c = als.copy()
    assert c is not als and c._p == als._p and c._p is not als._p
    assert c._checkpoint_dir == "/tmp/ckpt"
    d = als.copy({ALS.rank: 9, "maxIter": 2})
    assert (d.getRank(), d.getMaxIter(), d.getRegParam()) == (9, 2, 0.3)
    assert als.getRank() == 7 and als.getMaxIter() == 10      # the original is untouched
    assert d._checkpoint_dir == "/tmp/ckpt"


def test_fit_param_map_validation():
    df = pd.DataFrame({"user": [0, 1], "item": [0, 1], "rating": [1.0, 2.0]})
    als = ALS()
    with pytest.raises(ValueError, match="not a parameter of ALS"):
        als.fit(df, {"rnak": 3})
    with pytest.raises(ValueError, match="not a parameter of ALS"):
        als.fit(df, {Param("Other", "rank"): 3})
    with pytest.raises(ValueError, match="not a parameter of ALS"):
        als.fit(df, {Param("ALS", "bogus"): 3})
    with pytest.raises(TypeError, match="Param objects or names"):
        als.fit(df, {3: 4})
    with pytest.raises(TypeError, match="param map"):
        als.fit(df, 5)
    with pytest.raises(ValueError, match="rank given invalid value"):
        als.fit(df, {ALS.rank: 0})            # the map is applied, then validated as usual
    with pytest.raises(NotImplementedError):
        als.fit(df, [{ALS.rank: 4}, {ALS.rank: 129}][1])
    with pytest.raises(ValueError, match="rank given invalid value"):
        als.fit(df, [{ALS.rank: 0}])          # a list of maps fits each
    assert als.fit(df, []) == [] and als.fit(df, ()) == []
    assert als.getRank() == 10


# ------------------------------------------------------------------ grid
def test_param_grid_order_and_base_on():
    grid = T.ParamGridBuilder().addGrid(ALS.rank, [4, 8]).addGrid(ALS.regParam, [0.1, 0.2, 0.3]) \
        .build()
    assert grid == [{ALS.rank: r, ALS.regParam: l} for r in (4, 8) for l in (0.1, 0.2, 0.3)]
    assert [list(m) for m in grid] == [[ALS.rank, ALS.regParam]] * 6   # insertion order
    base = T.ParamGridBuilder().baseOn({ALS.maxIter: 5}).addGrid("rank", [1, 2]) \
        .baseOn((ALS.seed, 3), (ALS.alpha, 2.0)).build()
    assert base == [{ALS.maxIter: 5, "rank": r, ALS.seed: 3, ALS.alpha: 2.0} for r in (1, 2)]
    assert T.ParamGridBuilder().build() == [{}]
    assert T.ParamGridBuilder().addGrid(ALS.rank, [4]).addGrid(ALS.rank, [5, 6]).build() == \
        [{ALS.rank: 5}, {ALS.rank: 6}]        # a repeated param replaces its grid
    with pytest.raises(TypeError):
        T.ParamGridBuilder().addGrid(3, [1])


# ------------------------------------------------------------------ folds
def test_folds_are_disjoint_cover_every_row_and_repeat():
    n, k = 1000, 3
    a, b = T.fold_assignment(n, k, 7), T.fold_assignment(n, k, 7)
    np.testing.assert_array_equal(a, b)
    assert not np.array_equal(a, T.fold_assignment(n, k, 8))
    assert a.shape == (n,) and set(a.tolist()) == {0, 1, 2}
    x = np.random.default_rng(7).random(n)               # fold f = [f / k, (f + 1) / k)
    for f in range(k):
        np.testing.assert_array_equal(a == f, (x >= f / k) & (x < (f + 1) / k))
    counts = np.bincount(a, minlength=k)
    assert counts.sum() == n and (np.abs(counts / n - 1 / k) < 0.05).all()
    cv = T.CrossValidator(StubEstimator(), MAPS, StubEvaluator({}), numFolds=k, seed=7)
    np.testing.assert_array_equal(cv.folds(DATA), T.fold_assignment(len(DATA), k, 7))


def test_fold_col_is_honoured_and_checked():
    est, ev = StubEstimator(), StubEvaluator({1.0: 0.0, 2.0: 0.0, 3.0: 0.0})
    cv = T.CrossValidator(est, MAPS, ev, numFolds=4, foldCol="fold")
    np.testing.assert_array_equal(cv.folds(DATA), DATA["fold"].to_numpy())
    cv.fit(DATA)
    assert [n for n, _ in est.calls[:-1]] == [150] * 12 and est.calls[-1][0] == 200
    assert [n for _, n in ev.seen] == [50] * 12
    with pytest.raises(ValueError, match=r"values in \[0, 3\)"):
        T.CrossValidator(est, MAPS, ev, numFolds=3, foldCol="fold").fit(DATA)
    with pytest.raises(ValueError, match=r"values in \[0, 4\)"):
        T.CrossValidator(est, MAPS, ev, numFolds=4, foldCol="fold").fit(
            DATA.assign(fold=DATA["fold"] - 1))
    with pytest.raises(ValueError, match="no column"):
        T.CrossValidator(est, MAPS, ev, numFolds=4, foldCol="nope").fit(DATA)
    with pytest.raises(ValueError, match="integers"):
        T.CrossValidator(est, MAPS, ev, numFolds=4, foldCol="fold").fit(
            DATA.assign(fold=DATA["fold"] + 0.5))
    with pytest.raises(ValueError, match="empty"):   # fold 3 never occurs
        T.CrossValidator(est, MAPS, ev, numFolds=4, foldCol="fold").fit(
            DATA.assign(fold=DATA["fold"] % 3))


# ------------------------------------------------------------------ the winner
def test_best_index_both_directions_and_nan():
    nan = float("nan")
    assert T.best_index([0.9, 0.7, 0.8], False) == 1
    assert T.best_index([0.9, 0.7, 0.8], True) == 0
    assert T.best_index([0.7, 0.7], False) == 0 and T.best_index([0.7, 0.7], True) == 0
    assert T.best_index([nan, 0.9, 0.8], False) == 2
    assert T.best_index([nan, 0.9, 0.8], True) == 1
    assert T.best_index([0.5, nan], True) == 0 and T.best_index([0.5, nan], False) == 0
    for larger in (False, True):
        with pytest.raises(ValueError, match='coldStartStrategy="drop"'):
            T.best_index([nan, nan], larger)


@pytest.mark.parametrize("larger,best", [(False, 2.0), (True, 3.0)])
def test_train_validation_split(larger, best):
    est = StubEstimator()
    ev = StubEvaluator({1.0: 0.9, 2.0: 0.7, 3.0: 1.1}, larger)
    tvs = T.TrainValidationSplit(est, MAPS, ev, trainRatio=0.8, seed=3, parallelism=4)
    out = tvs.fit(DATA)
    tr, va = tvs.split(len(DATA))
    assert len(tr) + len(va) == 200 and len(np.intersect1d(tr, va)) == 0
    assert abs(len(tr) / 200 - 0.8) < 0.08
    assert out.validationMetrics == [0.9, 0.7, 1.1] and out.subModels is None
    # three fits on the training part, scored on the rest, then the best map on everything
    assert est.calls == [(len(tr), m) for m in MAPS] + [(200, {"a": best})]
    assert ev.seen == [(m["a"], len(va)) for m in MAPS]
    assert out.bestModel.params == {"a": best} and out.bestModel.n_train == 200
    assert out.bestModel.train_sum == float(DATA["y"].sum())
    assert out.transform(DATA)["model"].iloc[0] is out.bestModel
    again = T.TrainValidationSplit(StubEstimator(), MAPS, ev, trainRatio=0.8, seed=3)
    assert all(np.array_equal(a, b) for a, b in zip(again.split(200), (tr, va)))


def test_nan_never_wins_and_all_nan_raises():
    nan = float("nan")
    for larger in (False, True):
        out = T.TrainValidationSplit(StubEstimator(), MAPS,
                                     StubEvaluator({1.0: nan, 2.0: 0.7, 3.0: nan}, larger),
                                     seed=1).fit(DATA)
        assert out.bestModel.params == {"a": 2.0}
        assert math.isnan(out.validationMetrics[0]) and out.validationMetrics[1] == 0.7
        est = StubEstimator()
        with pytest.raises(ValueError, match='coldStartStrategy="drop"'):
            T.TrainValidationSplit(est, MAPS, StubEvaluator({1.0: nan, 2.0: nan, 3.0: nan},
                                                            larger), seed=1).fit(DATA)
        assert len(est.calls) == 3                      # no refit of an arbitrary map
        with pytest.raises(ValueError, match='coldStartStrategy="drop"'):
            T.CrossValidator(StubEstimator(), MAPS,
                             StubEvaluator({1.0: nan, 2.0: nan, 3.0: nan}, larger)).fit(DATA)


def test_cross_validator_mean_std_and_best():
    est = StubEstimator()
    ev = StubEvaluator({1.0: 0.0, 2.0: -5.0, 3.0: 5.0}, larger=False, by_fold=True)
    cv = T.CrossValidator(est, MAPS, ev, numFolds=4, foldCol="fold", collectSubModels=True)
    out = cv.fit(DATA)
    fold_means = np.array([DATA["y"][DATA["fold"] == f].mean() for f in range(4)])
    per_map = np.stack([fold_means + off for off in (0.0, -5.0, 5.0)], 1)     # [fold, map]
    np.testing.assert_allclose(out.avgMetrics, per_map.mean(axis=0), rtol=1e-15)
    np.testing.assert_allclose(out.stdMetrics, per_map.std(axis=0), rtol=1e-12)
    assert out.stdMetrics[0] > 0
    assert out.bestModel.params == {"a": 2.0} and out.bestModel.n_train == 200
    assert est.calls[-1] == (200, {"a": 2.0}) and len(est.calls) == 13
    assert len(out.subModels) == 4 and all(len(row) == 3 for row in out.subModels)
    for f, row in enumerate(out.subModels):
        assert [m.params for m in row] == MAPS and all(m.n_train == 150 for m in row)
        assert row[0].train_sum == float(DATA["y"][DATA["fold"] != f].sum())
    # a NaN in one fold makes that map's mean NaN: it cannot win
    nan_ev = StubEvaluator({1.0: 0.0, 2.0: float("nan"), 3.0: 5.0}, by_fold=True)
    out = T.CrossValidator(StubEstimator(), MAPS, nan_ev, numFolds=4, foldCol="fold").fit(DATA)
    assert math.isnan(out.avgMetrics[1]) and out.bestModel.params == {"a": 1.0}
    assert out.subModels is None


def test_collect_sub_models_shapes_for_the_split():
    out = T.TrainValidationSplit(StubEstimator(), MAPS, StubEvaluator({1.0: 1, 2.0: 2, 3.0: 3}),
                                 seed=0, collectSubModels=True).fit(DATA)
    assert [m.params for m in out.subModels] == MAPS
    assert all(m.n_train < 200 for m in out.subModels) and out.bestModel.n_train == 200


def test_constructor_validation():
    est, ev = StubEstimator(), StubEvaluator({})
    with pytest.raises(ValueError, match="at least one param map"):
        T.TrainValidationSplit(est, [], ev)
    with pytest.raises(TypeError):
        T.TrainValidationSplit(est, [3], ev)
    for bad in (0.0, 1.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="trainRatio"):
            T.TrainValidationSplit(est, MAPS, ev, trainRatio=bad)
    for bad in (1, 0, 2.5, True):
        with pytest.raises(ValueError, match="numFolds"):
            T.CrossValidator(est, MAPS, ev, numFolds=bad)
    with pytest.raises(ValueError, match="parallelism"):
        T.CrossValidator(est, MAPS, ev, parallelism=0)
    tvs = T.TrainValidationSplit(est, MAPS, ev)
    assert tvs.getTrainRatio() == 0.75 and tvs.getEstimator() is est and tvs.getEvaluator() is ev
    assert tvs.getEstimatorParamMaps() == MAPS and isinstance(tvs.getSeed(), int)
    cv = T.CrossValidator(est, MAPS, ev)
    assert cv.getNumFolds() == 3 and cv.getFoldCol() == ""


def test_dict_datasets_are_split_by_row():
    d = {"y": np.arange(10.0), "z": list(range(10))}
    got = T._take(d, np.array([1, 3]))
    assert got["y"].tolist() == [1.0, 3.0] and got["z"].tolist() == [1, 3]
    assert T._n_rows(d) == 10 and T._n_rows(DATA) == 200
    assert T._take([(0, 1), (2, 3), (4, 5)], np.array([0, 2])) == [(0, 1), (4, 5)]
