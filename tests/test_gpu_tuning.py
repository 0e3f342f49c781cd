"""ml.tuning on the GPU: TrainValidationSplit and CrossValidator over ALS against the hand
loop they replace (a fresh ALS(...).fit(train) followed by .rmse(valid) per map), on planted
600 x 400 data, density 0.08.

Finding recorded here and in DESIGN.md (K8): a fit on the engine the tuner shares between
param maps gives the same bits as a stand-alone fit — the arithmetic, the seeded start and
the chunk_for(rank) schedule are the same, and nothing a fit leaves behind (the workspace's
rating-scale word is re-measured after every scoring pass) reaches the next one.
"""
import math

import numpy as np
import pandas as pd
import pytest
import torch

from als_mi355x.ml.evaluation import RegressionEvaluator
from als_mi355x.ml.recommendation import ALS
from als_mi355x.ml.tuning import CrossValidator, ParamGridBuilder, TrainValidationSplit
from helpers import planted

pytestmark = pytest.mark.gpu
RANKS = (4, 8, 12)
BASE = dict(maxIter=5, regParam=0.1, seed=5, coldStartStrategy="drop")


@pytest.fixture(scope="module")
def data():
    u, i, r = planted(600, 400, density=0.08, seed=4, half_stars=False)
    return pd.DataFrame({"user": u, "item": i, "rating": r})


def _factors(model):
    (_, U), (_, V) = model.engine.user_factors(), model.engine.item_factors()
    return U, V


def _same_model(a, b):
    assert a.rank == b.rank
    for x, y in zip(_factors(a), _factors(b)):
        assert torch.equal(x, y)
    assert torch.equal(a.engine.user_factor_ids(), b.engine.user_factor_ids())


@pytest.fixture(scope="module")
def sweep(data):
    """(tuner, its model): the reference's sweep — ranks 4 / 8 / 12, 5 iterations, lambda 0.1."""
    grid = ParamGridBuilder().addGrid(ALS.rank, RANKS).build()
    tvs = TrainValidationSplit(ALS(**BASE), grid, RegressionEvaluator(labelCol="rating"),
                               trainRatio=0.75, seed=11, collectSubModels=True)
    return tvs, tvs.fit(data)


def test_train_validation_split_equals_the_hand_loop(data, sweep):
    tvs, out = sweep
    tr, va = tvs.split(len(data))
    train, valid = data.iloc[tr], data.iloc[va]
    assert len(out.validationMetrics) == len(out.subModels) == 3
    hand = []
    for j, rank in enumerate(RANKS):
        alone = ALS(rank=rank, **BASE).fit(train)
        hand.append(alone.rmse(valid))
        # the shared-engine fit is the stand-alone fit, bit for bit
        _same_model(out.subModels[j], alone)
        assert abs(out.validationMetrics[j] - hand[j]) <= 1e-12 * hand[j], (rank, hand)
    print(f"validation rmse by rank {dict(zip(RANKS, out.validationMetrics))}")
    assert all(0.5 < m < 1.5 for m in hand)
    best = RANKS[int(np.argmin(hand))]
    assert out.bestModel.rank == best
    _same_model(out.bestModel, ALS(rank=best, **BASE).fit(data))     # refit on everything
    pd.testing.assert_frame_equal(out.transform(valid), out.bestModel.transform(valid))


def test_sub_models_are_snapshots(sweep):
    """collectSubModels: each fit is copied out of the shared engine before the next one
    overwrites it — three models of three ranks, each serving on its own."""
    _, out = sweep
    assert [m.rank for m in out.subModels] == list(RANKS)
    engines = {id(m.engine) for m in out.subModels}
    assert len(engines) == 3 and id(out.bestModel.engine) not in engines
    assert all(m.engine.user_block is None for m in out.subModels)   # serving only


def test_cross_validator_equals_three_hand_fits(data):
    regs = (0.05, 0.5)
    grid = ParamGridBuilder().addGrid(ALS.regParam, regs).build()
    est = ALS(rank=8, maxIter=5, seed=5, coldStartStrategy="drop")
    cv = CrossValidator(est, grid, RegressionEvaluator(labelCol="rating"), numFolds=3, seed=2)
    out = cv.fit(data)
    fold = cv.folds(data)
    assert set(fold.tolist()) == {0, 1, 2}
    hand = np.array([[ALS(rank=8, maxIter=5, seed=5, regParam=reg).fit(data[fold != f])
                      .rmse(data[fold == f]) for reg in regs] for f in range(3)])
    assert np.isfinite(out.avgMetrics).all()
    np.testing.assert_allclose(out.avgMetrics, hand.mean(axis=0), rtol=1e-12)
    np.testing.assert_allclose(out.stdMetrics, hand.std(axis=0), rtol=1e-6, atol=1e-12)
    best = regs[int(np.argmin(hand.mean(axis=0)))]
    assert out.bestModel._p["regParam"] == best and out.subModels is None
    _same_model(out.bestModel, est.copy({ALS.regParam: best}).fit(data))


def test_cross_validator_nan_map_does_not_win(data):
    """coldStartStrategy="nan" with a user who has a single rating: in the fold that holds
    it the user has no training row, so that map's metric is NaN (what Spark reports) and
    the "drop" map wins; when every map is "nan" there is nothing to choose and fit raises."""
    lone = pd.DataFrame({"user": [10 ** 5], "item": [int(data["item"].iloc[0])], "rating": [3.0]})
    df = pd.concat([data, lone], ignore_index=True)
    grid = ParamGridBuilder().addGrid(ALS.coldStartStrategy, ["nan", "drop"]).build()
    est = ALS(rank=4, maxIter=2, regParam=0.1, seed=5)
    ev = RegressionEvaluator(labelCol="rating")
    out = CrossValidator(est, grid, ev, numFolds=3, seed=2).fit(df)
    assert math.isnan(out.avgMetrics[0]) and math.isfinite(out.avgMetrics[1])
    assert out.bestModel._p["coldStartStrategy"] == "drop"
    with pytest.raises(ValueError, match='coldStartStrategy="drop"'):
        CrossValidator(est, grid[:1], ev, numFolds=3, seed=2).fit(df)
