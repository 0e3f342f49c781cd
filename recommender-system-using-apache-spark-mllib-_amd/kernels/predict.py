"""K4, K8: predictions and regression moments of (user, item) pairs (csrc/predict.hip:
als_predict, als_rmse_partial; csrc/regression_metrics.hip: als_regression_moments,
als_regression_moments_cols)."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from .._lib import check, ptr, stream_ptr
from .workspace import Workspace
from .csr import IdIndex


def predict_pairs(u: torch.Tensor, i: torch.Tensor, uidx: IdIndex, iidx: IdIndex,
                  U: torch.Tensor, V: torch.Tensor, rank: int) -> torch.Tensor:
    L = _lib.lib()
    u, i = uidx.keys(u), iidx.keys(i)
    out = torch.empty(u.numel(), dtype=torch.float64, device=U.device)
    check(L.als_predict(ptr(u), ptr(i), u.numel(), ptr(uidx.map), uidx.id_space, ptr(iidx.map),
                        iidx.id_space, ptr(U), ptr(V), U.shape[1], rank, ptr(out),
                        stream_ptr(U.device)), "als_predict")
    return out


def rmse_pairs(u, i, r, uidx: IdIndex, iidx: IdIndex, U, V, rank: int, ws: Workspace):
    """(sse, count) over pairs with both ids known (computeError's join)."""
    L = _lib.lib()
    u, i = uidx.keys(u), iidx.keys(i)
    out = torch.empty(2, dtype=torch.float64, device=U.device)
    w = ws.get(L.als_rmse_workspace_bytes(u.numel()))
    check(L.als_rmse_partial(ptr(u), ptr(i), ptr(r), u.numel(), ptr(uidx.map), uidx.id_space,
                             ptr(iidx.map), iidx.id_space, ptr(U), ptr(V), U.shape[1], rank,
                             ptr(out), ptr(w), w.numel(), stream_ptr(U.device)),
          "als_rmse_partial")
    return out


# K8 (als_regression_moments): the 8 doubles both forms write, in order
MOMENT_NAMES = ("n", "mean_label", "M2_label", "mean_pred", "M2_pred", "sse", "sae", "n_dropped")


def regression_moments_pairs(u, i, r, uidx: IdIndex, iidx: IdIndex, U, V, rank: int,
                             ws: Workspace) -> torch.Tensor:
    """K8, fused form: f64 [8] (MOMENT_NAMES) of label = r against the fp64 gather-dot of
    K4 over the pairs with both ids known; the others are counted in n_dropped
    (computeError's join, as rmse_pairs)."""
    L = _lib.lib()
    u, i = uidx.keys(u), iidx.keys(i)
    out = torch.empty(8, dtype=torch.float64, device=U.device)
    w = ws.get(L.als_regression_moments_workspace_bytes(u.numel()))
    check(L.als_regression_moments(ptr(u), ptr(i), ptr(r), u.numel(), ptr(uidx.map),
                                   uidx.id_space, ptr(iidx.map), iidx.id_space, ptr(U), ptr(V),
                                   U.shape[1], rank, ptr(out), ptr(w), w.numel(),
                                   stream_ptr(U.device)), "als_regression_moments")
    return out


def regression_moments_cols(label: torch.Tensor, pred: torch.Tensor, ws: Workspace
                            ) -> torch.Tensor:
    """K8, column form: f64 [8] (MOMENT_NAMES) of two contiguous fp64 device vectors of one
    length; every row is used and a NaN in either makes the error-derived values NaN."""
    L = _lib.lib()
    if label.dtype != torch.float64 or pred.dtype != torch.float64:
        raise ValueError("regression_moments_cols: label and pred must be float64 tensors")
    if label.dim() != 1 or label.shape != pred.shape:
        raise ValueError("regression_moments_cols: label and pred must be vectors of one length")
    label, pred = label.contiguous(), pred.contiguous()
    out = torch.empty(8, dtype=torch.float64, device=label.device)
    w = ws.get(L.als_regression_moments_workspace_bytes(label.numel()))
    check(L.als_regression_moments_cols(ptr(label), ptr(pred), label.numel(), ptr(out), ptr(w),
                                        w.numel(), stream_ptr(label.device)),
          "als_regression_moments_cols")
    return out


def regression_dict(moments, through_origin: bool = False) -> dict:
    """Spark's RegressionMetrics (mllib/evaluation/RegressionMetrics.scala, upstream, not
    vendored) from K8's 8 numbers (a host sequence in MOMENT_NAMES order); pure host fp64:
      SSerr = sse, SStot = M2_label, SSy = M2_label + n mean_label^2,
      SSreg = M2_pred + n (mean_pred - mean_label)^2
      mse = SSerr / n, rmse = sqrt(mse), mae = sae / n, var = SSreg / n (explainedVariance),
      r2 = 1 - SSerr / SStot, or 1 - SSerr / SSy with through_origin.
    Also n, dropped (pairs the fused form left out), meanLabel and varLabel = M2_label / n
    (population variance).  Divisions are IEEE: constant labels give r2 = -inf (sse > 0) or
    NaN (sse = 0), and n = 0 gives NaN metrics, never an exception.
    A constant prediction c has mse = varLabel + (meanLabel - c)^2, so the reference's
    mean-rating baseline (RecommenderSystem.py:172-177: the training mean as every test
    prediction) is sqrt(varLabel + (meanLabel - c)^2) of the test moments, with no second
    pass over the data."""
    n, ml, m2l, mp, m2p, sse, sae, drop = (np.float64(x) for x in moments)
    with np.errstate(divide="ignore", invalid="ignore"):
        ss_tot = m2l + n * ml * ml if through_origin else m2l
        ss_reg = m2p + n * (mp - ml) * (mp - ml)
        mse = sse / n
        out = {"mse": mse, "rmse": np.sqrt(mse), "mae": sae / n, "r2": 1.0 - sse / ss_tot,
               "var": ss_reg / n, "meanLabel": ml if n > 0 else np.float64("nan"),
               "varLabel": m2l / n}
    out = {k: float(v) for k, v in out.items()}
    out["n"] = int(n)
    out["dropped"] = int(drop)
    return out
