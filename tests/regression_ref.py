"""numpy fp64 two-pass restatement of Spark's RegressionMetrics, for the regression-metric
tests (test code only).

With l the labels, p the predictions, n rows (mllib/evaluation/RegressionMetrics.scala,
upstream, not vendored: the formulas are stated here as the project states them):
  SSerr = sum (l - p)^2            SStot = sum (l - mean l)^2
  SSy   = sum l^2                  SSreg = sum (p - mean l)^2
  mse = SSerr / n, rmse = sqrt(mse), mae = sum |l - p| / n, var = SSreg / n,
  r2 = 1 - SSerr / SStot, or 1 - SSerr / SSy through the origin.
Every sum of deviations is taken in a second pass around the mean of the first
(math.fsum: exactly rounded), so the reference itself carries no cancellation.
"""
import math

import numpy as np

MOMENT_NAMES = ("n", "mean_label", "M2_label", "mean_pred", "M2_pred", "sse", "sae", "n_dropped")


def _fsum(x) -> float:
    return math.fsum(np.asarray(x, np.float64).tolist())


def moments(label, pred, dropped: int = 0) -> np.ndarray:
    """The 8 numbers als_regression_moments writes, two-pass."""
    l = np.asarray(label, np.float64).reshape(-1)
    p = np.asarray(pred, np.float64).reshape(-1)
    n = len(l)
    if n == 0:
        return np.array([0, 0, 0, 0, 0, 0, 0, dropped], np.float64)
    ml, mp = _fsum(l) / n, _fsum(p) / n
    return np.array([n, ml, _fsum((l - ml) ** 2), mp, _fsum((p - mp) ** 2), _fsum((l - p) ** 2),
                     _fsum(np.abs(l - p)), dropped], np.float64)


def metrics(label, pred, through_origin: bool = False, dropped: int = 0) -> dict:
    """Spark's five metrics (and n, dropped, meanLabel, varLabel) directly from the columns;
    IEEE division (constant labels: -inf or nan; n = 0: nan)."""
    l = np.asarray(label, np.float64).reshape(-1)
    p = np.asarray(pred, np.float64).reshape(-1)
    n = np.float64(len(l))
    with np.errstate(divide="ignore", invalid="ignore"):
        ml = np.float64(_fsum(l)) / n
        ss_err = np.float64(_fsum((l - p) ** 2))
        ss_tot = np.float64(_fsum((l - ml) ** 2))
        ss_y = np.float64(_fsum(l ** 2))
        ss_reg = np.float64(_fsum((p - ml) ** 2))
        out = {"mse": ss_err / n, "rmse": np.sqrt(ss_err / n),
               "mae": np.float64(_fsum(np.abs(l - p))) / n,
               "r2": 1.0 - ss_err / (ss_y if through_origin else ss_tot), "var": ss_reg / n,
               "meanLabel": ml, "varLabel": ss_tot / n}
    out = {k: float(v) for k, v in out.items()}
    out["n"] = int(n)
    out["dropped"] = int(dropped)
    return out


METRIC_KEYS = ("mse", "rmse", "mae", "r2", "var", "meanLabel", "varLabel")


def assert_metrics_close(got: dict, ref: dict, rtol=1e-9, atol=1e-12, r2_atol=1e-9):
    """The bar of the GPU tests: every metric within rtol / atol, r2 with atol 1e-9 (it is
    one minus a ratio near one); n and dropped exact."""
    assert got["n"] == ref["n"] and got["dropped"] == ref["dropped"], (got, ref)
    for k in METRIC_KEYS:
        np.testing.assert_allclose(got[k], ref[k], rtol=rtol, atol=r2_atol if k == "r2" else atol,
                                   equal_nan=True, err_msg=k)
