"""Regression moments (K8, als_regression_moments / _cols) on the GPU: both forms against the
two-pass fp64 reference (tests/regression_ref.py), edge sizes, ranks, id maps, unknown ids,
padding, cancellation, NaN, determinism, and the public surfaces.

Fused form: the reference is computed from the same device factors, predictions from
core.predict (K4's fp64 gather-dot, the same pair_dot), labels the fp32 ratings widened.
Bar: every moment and metric within rtol 1e-9 / atol 1e-12 (r2: atol 1e-9, it is one minus
a ratio near one) — the bar test_predict_and_rmse_inner_join holds K4 to; fp64 sums over at
most 65,537 terms (262,145 in one column case) leave about 100x margin.
"""
import functools
import math

import numpy as np
import pytest
import torch

import regression_ref as R
from als_mi355x import engine as E
from helpers import planted

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_USERS, N_ITEMS = 200, 150
SIZES = (0, 1, 15, 16, 17, 255, 256, 257, 65537)   # 65,537: 257 blocks, thread 0 merges two
RANKS = (1, 4, 63, 64, 65, 128)


# ------------------------------------------------------------------ helpers
@functools.lru_cache(maxsize=None)
def _core(rank, id_gap=1, shift=0):
    """A core fitted (2 iterations) on 200 x 150 planted data; ids = id_gap * dense + shift.
    Never modified by a test (the padding test restores what it writes)."""
    u, i, r = planted(N_USERS, N_ITEMS, density=0.08, seed=3, id_gap=id_gap)
    core = E.ALSCore(u + shift, i + shift, r, device=DEV)
    core.fit(rank, 2, 0.1, seed=1)
    return core


def _pairs(n, seed, id_gap=1, shift=0):
    rng = np.random.default_rng(seed)
    u = (rng.integers(0, N_USERS, n) * id_gap + shift).astype(np.int32)
    i = (rng.integers(0, N_ITEMS, n) * id_gap + shift).astype(np.int32)
    r = (rng.integers(1, 11, n) / 2).astype(np.float32)
    return u, i, r


def _fused(core, u, i, r):
    t = lambda a, d: torch.as_tensor(a).to(DEV, d).contiguous()
    m = E.regression_moments_pairs(t(u, torch.int32), t(i, torch.int32), t(r, torch.float32),
                                   core.uidx, core.iidx, core.U, core.V, core.rank,
                                   E.Workspace(torch.device(DEV)))
    return m.cpu().numpy()


def _reference(core, u, i, r):
    """(two-pass moments, labels, predictions of the known pairs)."""
    p = core.predict(u, i).cpu().numpy()
    known = ~np.isnan(p)
    lab = np.asarray(r, np.float32).astype(np.float64)[known]
    return R.moments(lab, p[known], dropped=int((~known).sum())), lab, p[known]


def _assert_moments(got, ref, what=""):
    print(f"K8 {what}: got {got.tolist()} ref {ref.tolist()}")
    assert got[0] == ref[0] and got[7] == ref[7], (what, got, ref)
    np.testing.assert_allclose(got[1:7], ref[1:7], rtol=1e-9, atol=1e-12, err_msg=what)


def _check_fused(core, u, i, r, what):
    got = _fused(core, u, i, r)
    ref, lab, p = _reference(core, u, i, r)
    _assert_moments(got, ref, what)
    for origin in (False, True):
        R.assert_metrics_close(E.regression_dict(got, origin),
                               R.metrics(lab, p, origin, dropped=int(ref[7])))
    return got


def _cols(lab, pred):
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64)).to(DEV)
    return E.regression_moments_cols(t(lab), t(pred), E.Workspace(torch.device(DEV)))


# ------------------------------------------------------------------ fused form
@pytest.mark.parametrize("n", SIZES)
def test_fused_sizes(n):
    core = _core(8)
    u, i, r = _pairs(n, seed=n)
    got = _check_fused(core, u, i, r, f"fused n={n}")
    assert got[0] == n and got[7] == 0
    if n:
        rm, cnt = core.rmse(u, i, r)
        assert cnt == n
        assert abs(E.regression_dict(got)["rmse"] - rm) <= 1e-12 * rm
    else:
        assert (got == 0).all()
        assert all(math.isnan(E.regression_dict(got)[k]) for k in R.METRIC_KEYS)


@pytest.mark.parametrize("rank", RANKS)
def test_fused_ranks(rank):
    core = _core(rank)
    u, i, r = _pairs(1000, seed=rank)
    got = _check_fused(core, u, i, r, f"fused rank={rank}")
    rm, _ = core.rmse(u, i, r)
    assert abs(E.regression_dict(got)["rmse"] - rm) <= 1e-12 * rm


@pytest.mark.parametrize("id_gap,shift", [(3, 0), (3, -50), (1, 1 << 27)],
                         ids=["gap", "gap-negative-offset", "high-offset"])
def test_fused_id_maps_and_unknown_ids(id_gap, shift):
    """Ids with a gap and an offset; unknown ids of each kind — negative (or below the
    offset), past the map, inside the map but mapped to -1 — are dropped and counted."""
    core = _core(8, id_gap, shift)
    assert core.uidx.offset == (shift if shift else 0)
    u, i, r = _pairs(600, seed=7, id_gap=id_gap, shift=shift)
    _check_fused(core, u, i, r, "all known")
    lo, hi = shift - 7, shift + id_gap * 1000      # below every id / past the map
    bad_u = [lo, hi] + ([shift + 1] if id_gap > 1 else [])     # + a gap id (map == -1)
    u2, i2 = u.copy(), i.copy()
    for j, b in enumerate(bad_u):
        u2[10 * j] = b
        i2[10 * j + 5] = b
    got = _check_fused(core, u2, i2, r, "with unknown ids")
    assert got[7] == 2 * len(bad_u) and got[0] == 600 - got[7]
    # every pair unknown: n = 0, NaN metrics, dropped = all
    got = _fused(core, np.full(40, lo, np.int32), i[:40], r[:40])
    assert got.tolist() == [0, 0, 0, 0, 0, 0, 0, 40]
    d = E.regression_dict(got)
    assert d["n"] == 0 and d["dropped"] == 40
    assert all(math.isnan(d[k]) for k in R.METRIC_KEYS)


@pytest.mark.parametrize("rank", (1, 63, 65))
def test_padding_columns_never_reach_a_result(rank):
    core = _core(rank)
    u, i, r = _pairs(700, seed=2)
    clean = _fused(core, u, i, r)
    assert core.U.shape[1] > rank
    try:
        core.U[:, rank:] = float("nan")
        core.V[:, rank:] = 1e30
        dirty = _fused(core, u, i, r)
    finally:
        core.U[:, rank:] = 0
        core.V[:, rank:] = 0
    assert np.array_equal(clean, dirty) and not np.isnan(dirty).any()


def test_fused_is_bitwise_reproducible():
    core = _core(64)
    u, i, r = _pairs(65537, seed=1)
    u[::97] = -3
    a, b = _fused(core, u, i, r), _fused(core, u, i, r)
    assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ column form
@pytest.mark.parametrize("n", SIZES + (262145,))   # 262,145: 257 column blocks of 1,024
def test_cols_sizes(n):
    rng = np.random.default_rng(n + 1)
    lab = rng.normal(3.5, 1.1, n)
    pred = lab + rng.normal(0.05, 0.6, n)
    got = _cols(lab, pred).cpu().numpy()
    _assert_moments(got, R.moments(lab, pred), f"cols n={n}")
    for origin in (False, True):
        R.assert_metrics_close(E.regression_dict(got, origin), R.metrics(lab, pred, origin))


def test_cols_cancellation():
    """Labels 1e9 + N(0, 1): sum x^2 - (sum x)^2 / n has no correct digit left (x^2 is 1e18,
    an ulp of it 128, the variance 1), so only the merge of centred partials passes."""
    rng = np.random.default_rng(0)
    n = 100_000
    lab = 1e9 + rng.standard_normal(n)
    pred = lab + 0.25 * rng.standard_normal(n)
    got = E.regression_dict(_cols(lab, pred).tolist())
    ref = R.metrics(lab, pred)
    print(f"cancellation: varLabel {got['varLabel']!r} ref {ref['varLabel']!r}; "
          f"r2 {got['r2']!r} ref {ref['r2']!r}")
    assert 0.98 < ref["varLabel"] < 1.02
    assert abs(got["varLabel"] - ref["varLabel"]) <= 1e-9 * ref["varLabel"]
    assert abs(got["r2"] - ref["r2"]) <= 1e-9 * abs(ref["r2"])
    assert abs(got["meanLabel"] - ref["meanLabel"]) <= 1e-9 * ref["meanLabel"]
    np.testing.assert_allclose(got["rmse"], ref["rmse"], rtol=1e-9)


@pytest.mark.parametrize("where", [0, 1234, 4999])
def test_cols_one_nan_prediction(where):
    rng = np.random.default_rng(4)
    lab = rng.normal(3.5, 1.0, 5000)
    pred = lab + rng.normal(0, 0.5, 5000)
    pred[where] = np.nan
    m = _cols(lab, pred).tolist()
    d = E.regression_dict(m)
    assert d["n"] == 5000 and d["dropped"] == 0           # n still counts every row
    assert all(math.isnan(d[k]) for k in ("mse", "rmse", "mae", "r2", "var"))
    np.testing.assert_allclose(d["varLabel"], lab.var(), rtol=1e-9)   # the labels are clean
    lab[where] = np.nan                                       # ... and a NaN label
    d = E.regression_dict(_cols(lab, np.nan_to_num(pred)).tolist())
    assert d["n"] == 5000
    assert all(math.isnan(d[k]) for k in ("mse", "rmse", "mae", "r2", "var"))


def test_cols_two_runs_are_bitwise_equal():
    rng = np.random.default_rng(8)
    lab = rng.normal(0, 1, 262145)
    pred = rng.normal(0, 1, 262145)
    a, b = _cols(lab, pred).cpu().numpy(), _cols(lab, pred).cpu().numpy()
    assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ surfaces
@pytest.fixture(scope="module")
def fitted():
    """(ml ALSModel with coldStartStrategy "drop", train frame, held-out frame): planted
    200 x 150, rank 8, a seeded 20 % held out (rows of users / items the training part
    does not know removed).  Never modified by a test."""
    import pandas as pd

    from als_mi355x.ml.recommendation import ALS
    u, i, r = planted(N_USERS, N_ITEMS, density=0.08, seed=9, half_stars=False)
    held = np.random.default_rng(1).random(len(u)) < 0.2
    ok = held & np.isin(u, u[~held]) & np.isin(i, i[~held])
    frame = lambda s: pd.DataFrame({"user": u[s], "item": i[s], "rating": r[s]})
    model = ALS(rank=8, maxIter=5, regParam=0.1, seed=5, coldStartStrategy="drop").fit(
        frame(~held))
    return model, frame(~held), frame(ok)


def _ref_of(model, df):
    p = model.engine.predict(df["user"].to_numpy(), df["item"].to_numpy()).cpu().numpy()
    assert not np.isnan(p).any()
    return R.metrics(df["rating"].to_numpy(np.float64), p), p


def test_evaluate_against_evaluate_fused(fitted):
    """evaluate(transform(df)) sees fp32 predictions, evaluateFused fp64 ones: |p32 - p| <=
    |p| 2^-24 per row, and rmse is a norm over sqrt(n), so by the triangle inequality the
    two differ by at most max|p| 2^-24 (+ 1e-12 for the fp64 arithmetic of both)."""
    from als_mi355x.ml.evaluation import RegressionEvaluator
    model, _, test = fitted
    ref, p = _ref_of(model, test)
    ev = RegressionEvaluator(labelCol="rating")
    fused = ev.evaluateFused(model, test)
    cols = ev.evaluate(model.transform(test))
    bound = np.abs(p).max() * 2.0 ** -24 + 1e-12
    print(f"rmse fused {fused!r} cols {cols!r} diff {abs(fused - cols):.3e} bound {bound:.3e}")
    assert abs(fused - cols) <= bound
    np.testing.assert_allclose(fused, ref["rmse"], rtol=1e-9)
    for name in ("mse", "mae", "r2", "var"):
        ev.setMetricName(name)
        np.testing.assert_allclose(ev.evaluateFused(model, test), ref[name], rtol=1e-9,
                                   atol=1e-9 if name == "r2" else 1e-12)
        np.testing.assert_allclose(ev.evaluate(model.transform(test)), ref[name], rtol=1e-5)
    ev.setMetricName("r2").setThroughOrigin(True)
    np.testing.assert_allclose(
        ev.evaluateFused(model, test),
        R.metrics(test["rating"].to_numpy(np.float64), p, True)["r2"], rtol=1e-9, atol=1e-9)


def test_cold_start_nan_against_drop(fitted):
    import pandas as pd

    from als_mi355x.ml.evaluation import RegressionEvaluator
    from als_mi355x.ml.recommendation import ALSModel
    model, _, test = fitted
    cold = pd.concat([test, pd.DataFrame({"user": [10 ** 6], "item": [3], "rating": [4.0]})],
                     ignore_index=True)
    ev = RegressionEvaluator(labelCol="rating")
    clean = ev.evaluateFused(model, test)
    assert ev.evaluateFused(model, cold) == clean                  # "drop": left out
    np.testing.assert_allclose(ev.evaluate(model.transform(cold)), clean, rtol=1e-6)
    nan_model = ALSModel(model.engine, dict(model._p, coldStartStrategy="nan"))
    assert math.isnan(ev.evaluateFused(nan_model, cold))           # what Spark would report
    assert math.isnan(ev.evaluate(nan_model.transform(cold)))
    assert ev.evaluateFused(nan_model, test) == clean              # nothing dropped: a number
    d = nan_model.evaluateRegression(cold)                         # the dict is the inner join
    assert d["dropped"] == 1 and d["n"] == len(test) and d["rmse"] == clean


def test_model_surfaces_fitted_and_loaded(fitted, tmp_path):
    from als_mi355x.ml.recommendation import ALSModel
    from als_mi355x.mllib.evaluation import RegressionMetrics
    from als_mi355x.mllib.recommendation import MatrixFactorizationModel
    model, _, test = fitted
    ref, p = _ref_of(model, test)
    rm = RegressionMetrics(zip(p.tolist(), test["rating"].tolist()))       # prediction first
    for prop, key in (("explainedVariance", "var"), ("meanAbsoluteError", "mae"),
                      ("meanSquaredError", "mse"), ("rootMeanSquaredError", "rmse"),
                      ("r2", "r2")):
        np.testing.assert_allclose(getattr(rm, prop), ref[key], rtol=1e-9,
                                   atol=1e-9 if key == "r2" else 1e-12, err_msg=prop)
    origin = RegressionMetrics(np.stack([p, test["rating"].to_numpy(np.float64)], 1), True)
    np.testing.assert_allclose(
        origin.r2, R.metrics(test["rating"].to_numpy(np.float64), p, True)["r2"], rtol=1e-9)
    model.save(str(tmp_path / "ml"))
    mf = MatrixFactorizationModel(model.engine)
    mf.save(None, str(tmp_path / "mllib"))
    trip = test[["user", "item", "rating"]].to_numpy()
    first = model.evaluateRegression(test)
    R.assert_metrics_close(first, ref)
    assert abs(first["rmse"] - model.rmse(test)) <= 1e-12 * first["rmse"]
    for got in (ALSModel.load(str(tmp_path / "ml")).evaluateRegression(test),
                mf.regressionMetrics(trip),
                MatrixFactorizationModel.load(None, str(tmp_path / "mllib"))
                .regressionMetrics(trip),
                model.evaluateRegression(test.rename(columns={"rating": "stars"}), "stars")):
        assert got == first          # the same factors and pairs: the same bits


def test_mean_rating_baseline_identity(fitted):
    """The reference's baseline (RecommenderSystem.py:172-177): the training mean as every
    test prediction has RMSE sqrt(varLabel + (meanLabel - c)^2) of the test moments."""
    model, train, test = fitted
    c = float(train["rating"].mean())
    lab = test["rating"].to_numpy(np.float64)
    direct = math.sqrt(np.mean((lab - c) ** 2))
    d = model.evaluateRegression(test)
    assert abs(math.sqrt(d["varLabel"] + (d["meanLabel"] - c) ** 2) - direct) <= 1e-12 * direct
    from als_mi355x.ml.evaluation import RegressionEvaluator
    base = RegressionEvaluator(labelCol="rating").evaluate(
        {"rating": lab, "prediction": np.full(len(lab), c)})
    assert abs(base - direct) <= 1e-12 * direct
