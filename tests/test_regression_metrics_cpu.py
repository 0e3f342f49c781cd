"""CPU tests of the regression-metrics boundary (K8, als_regression_moments; no GPU, no
compute launched).

* The header, the library and the ctypes table agree on the three entry points (ABI 9).
* Argument checks run host-side and return the documented codes (small integers stand in
  for pointers; nothing is dereferenced before the checks).
* engine.regression_dict, pure host arithmetic, against the two-pass reference.
* Parameter handling of both evaluators, and their refusal to run without a GPU.
* The sharded engine carries regression_metrics and refuses it.
"""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import regression_ref as R
from als_mi355x import _lib, filters
from als_mi355x import engine as E
from als_mi355x.ml.evaluation import RegressionEvaluator
from als_mi355x.mllib.evaluation import RegressionMetrics
from test_abi import _header_signatures, declared_functions

NAMES = ("als_regression_moments", "als_regression_moments_cols",
         "als_regression_moments_workspace_bytes")


def _fused(**over):
    a = dict(u=16, i=16, r=16, n=5, umap=16, umap_size=4, imap=16, imap_size=4, U=16, V=16, ld=8,
             k=8, out=16, ws=16, ws_bytes=1 << 20, stream=0)
    a.update(over)
    return _lib.lib().als_regression_moments(*a.values())


def _cols(**over):
    a = dict(label=16, pred=16, n=5, out=16, ws=16, ws_bytes=1 << 20, stream=0)
    a.update(over)
    return _lib.lib().als_regression_moments_cols(*a.values())


def test_header_library_and_binding_agree():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    hdr = _header_signatures()
    for name in NAMES:
        assert name in declared_functions()
        assert hasattr(raw, name)
        assert hdr[name] == _lib.SIGNATURES[name][1]
    assert _lib.SIGNATURES["als_regression_moments"][0] is ctypes.c_int
    assert _lib.SIGNATURES["als_regression_moments_cols"][0] is ctypes.c_int
    assert _lib.SIGNATURES["als_regression_moments_workspace_bytes"][0] is _lib.SZ
    # same arguments as als_rmse_partial, as the header says
    assert _lib.SIGNATURES["als_regression_moments"][1] == _lib.SIGNATURES["als_rmse_partial"][1]
    assert _lib.ABI_VERSION == 9 == _lib.lib().als_abi_version()  # a compatible addition
    assert E.MOMENT_NAMES == R.MOMENT_NAMES and len(E.MOMENT_NAMES) == 8


@pytest.mark.parametrize("over,code", [
    (dict(k=0), -1), (dict(ld=6), -1), (dict(ld=4), -1), (dict(n=-1), -1),
    (dict(u=0), -1), (dict(i=0), -1), (dict(r=0), -1), (dict(umap=0), -1), (dict(imap=0), -1),
    (dict(U=0), -1), (dict(V=0), -1), (dict(out=0), -1), (dict(umap_size=-1), -1),
    (dict(ws_bytes=8), -2), (dict(ws=0), -2), (dict(n=10 ** 9, ws_bytes=1 << 20), -2)])
def test_fused_argument_errors_before_any_device_call(over, code):
    L = _lib.lib()
    assert _fused(**over) == code
    assert L.als_last_error().startswith(b"als_regression_moments:")


@pytest.mark.parametrize("over,code", [
    (dict(n=-1), -1), (dict(label=0), -1), (dict(pred=0), -1), (dict(out=0), -1),
    (dict(ws_bytes=8), -2), (dict(ws=0), -2), (dict(n=10 ** 10, ws_bytes=1 << 20), -2)])
def test_cols_argument_errors_before_any_device_call(over, code):
    L = _lib.lib()
    assert _cols(**over) == code
    assert L.als_last_error().startswith(b"als_regression_moments_cols:")


def test_zero_rows_is_a_noop():
    assert _fused(u=0, i=0, r=0, n=0, umap=0, imap=0, U=0, V=0, out=0, ws=0, ws_bytes=0) == 0
    assert _fused(n=0, out=0, k=0) == -1          # k / ld are checked even then
    assert _cols(label=0, pred=0, n=0, out=0, ws=0, ws_bytes=0) == 0


def test_workspace_size_is_monotone():
    ws = _lib.lib().als_regression_moments_workspace_bytes
    sizes = [ws(n) for n in (0, 1, 256, 257, 65537, 10 ** 6, 10 ** 9)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    assert ws(256) < ws(65537) < ws(10 ** 6)   # sizes are rounded up to 256 bytes
    assert ws(10 ** 9) >= 8 * 8 * ((10 ** 9 + 255) // 256)   # one 8-double partial per block


# ------------------------------------------------------------------ regression_dict
def _close(got, ref):
    R.assert_metrics_close(got, ref, rtol=1e-12, atol=1e-14, r2_atol=1e-12)


@pytest.mark.parametrize("through_origin", [False, True])
@pytest.mark.parametrize("seed", range(4))
def test_regression_dict_matches_the_reference(seed, through_origin):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 400))
    lab = rng.normal(3.5, 1.0, n)
    pred = lab + rng.normal(0.1, 0.5, n)
    got = E.regression_dict(R.moments(lab, pred, dropped=seed), through_origin)
    _close(got, R.metrics(lab, pred, through_origin, dropped=seed))
    assert set(got) == {"mse", "rmse", "mae", "r2", "var", "n", "dropped", "meanLabel",
                        "varLabel"}
    assert isinstance(got["n"], int) and isinstance(got["dropped"], int)
    assert got["rmse"] == math.sqrt(got["mse"])


def test_regression_dict_zero_rows_and_constant_labels():
    z = E.regression_dict([0, 0, 0, 0, 0, 0, 0, 7])
    assert z["n"] == 0 and z["dropped"] == 7
    assert all(math.isnan(z[k]) for k in R.METRIC_KEYS)
    lab = np.full(10, 4.0)
    bad = E.regression_dict(R.moments(lab, lab + 0.5))        # sse > 0 over SStot = 0
    assert bad["r2"] == -math.inf and bad["varLabel"] == 0.0 and bad["mse"] == 0.25
    exact = E.regression_dict(R.moments(lab, lab))            # 0 / 0
    assert math.isnan(exact["r2"]) and exact["mse"] == 0.0
    # through the origin the denominator is sum l^2 > 0
    assert E.regression_dict(R.moments(lab, lab), True)["r2"] == 1.0
    _close(E.regression_dict(R.moments(lab, lab + 0.5), True), R.metrics(lab, lab + 0.5, True))


def test_baseline_identity_of_a_constant_prediction():
    """mse of the constant prediction c = varLabel + (meanLabel - c)^2 (engine.regression_dict's
    note on the reference's mean-rating baseline)."""
    rng = np.random.default_rng(5)
    lab = np.clip(np.round(rng.normal(3.5, 1.0, 500)), 1, 5)
    d = E.regression_dict(R.moments(lab, lab))
    for c in (3.2, float(lab.mean())):
        direct = math.sqrt(np.mean((lab - c) ** 2))
        assert abs(math.sqrt(d["varLabel"] + (d["meanLabel"] - c) ** 2) - direct) < 1e-12


# ------------------------------------------------------------------ evaluators
def test_regression_evaluator_params():
    ev = RegressionEvaluator()
    assert (ev.getMetricName(), ev.getLabelCol(), ev.getPredictionCol(), ev.getThroughOrigin()) \
        == ("rmse", "label", "prediction", False)
    ev = RegressionEvaluator(metricName="r2", labelCol="rating", predictionCol="p",
                             throughOrigin=True)
    assert (ev.getMetricName(), ev.getLabelCol(), ev.getPredictionCol(), ev.getThroughOrigin()) \
        == ("r2", "rating", "p", True)
    assert ev.setMetricName("mae").setLabelCol("y").setPredictionCol("yhat") \
        .setThroughOrigin(False) is ev
    assert (ev.getMetricName(), ev.getLabelCol(), ev.getPredictionCol(), ev.getThroughOrigin()) \
        == ("mae", "y", "yhat", False)
    assert ev.setParams(metricName="var", labelCol="l") is ev
    assert ev.getMetricName() == "var" and ev.getLabelCol() == "l"
    with pytest.raises(ValueError, match="metricName given invalid value"):
        RegressionEvaluator(metricName="rmsle")
    with pytest.raises(ValueError, match="supported: rmse, mse, r2, mae, var"):
        ev.setMetricName("RMSE")
    with pytest.raises(ValueError, match="metricName"):
        ev.setParams(metricName="nope")
    with pytest.raises(TypeError):
        ev.setParams(weightCol="w")
    with pytest.raises(TypeError):
        RegressionEvaluator(weightCol="w")      # out of scope: no such keyword
    assert "weightCol" not in inspect.signature(RegressionEvaluator.__init__).parameters


@pytest.mark.parametrize("name,larger", [("rmse", False), ("mse", False), ("mae", False),
                                         ("r2", True), ("var", True)])
def test_is_larger_better(name, larger):
    assert RegressionEvaluator(metricName=name).isLargerBetter() is larger


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_evaluators_refuse_to_run_without_gpu():
    data = {"label": [1.0, 2.0], "prediction": [1.5, 2.5]}
    with pytest.raises(_lib.ALSNativeError, match="no CPU fallback"):
        RegressionEvaluator().evaluate(data)
    with pytest.raises(_lib.ALSNativeError, match="no CPU fallback"):
        RegressionMetrics([(1.5, 1.0), (2.5, 2.0)])


def test_evaluator_input_errors_need_no_device_result():
    with pytest.raises(ValueError, match="float64"):
        E.regression_moments_cols(torch.zeros(2), torch.zeros(2), None)
    with pytest.raises(ValueError, match="one length"):
        E.regression_moments_cols(torch.zeros(2, dtype=torch.float64),
                                  torch.zeros(3, dtype=torch.float64), None)


def test_sharded_engine_rejects_regression_metrics():
    from als_mi355x import distributed as D
    from als_mi355x.engine import ALSCore
    assert D.reject_sharded_regression is filters.reject_sharded_regression
    eng = D.ShardedALS.__new__(D.ShardedALS)  # no process group needed: it refuses at once
    with pytest.raises(NotImplementedError, match="sharded"):
        eng.regression_metrics([1], [2], [3.0])
    with pytest.raises(NotImplementedError, match="sharded"):
        eng.regression_metrics([1], [2], [3.0], through_origin=True)
    sharded = inspect.signature(D.ShardedALS.regression_metrics)
    single = inspect.signature(ALSCore.regression_metrics)
    assert list(sharded.parameters) == list(single.parameters)
    assert sharded.parameters["through_origin"].default is False
