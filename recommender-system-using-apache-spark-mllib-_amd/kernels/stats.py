"""K16: rating statistics and bias baselines (csrc/rating_stats.hip: als_row_moments,
als_bias_update, als_baseline_predict)."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from .. import _lib
from .._lib import check, ptr, stream_ptr
from .workspace import Workspace, _host_f64, _to_device
from .csr import IdIndex
from .schedule import RatingBlock
from .predict import regression_dict, regression_moments_cols

RATING_MOMENTS = ("n", "sum", "M2", "min", "max")   # als_row_moments' columns, and its total
BASELINE_METHODS = ("global", "item", "user", "bias")


def rating_stats_task() -> int:
    """Ratings per task of a long row in K16's sweep (als_rating_stats_task)."""
    return int(_lib.lib().als_rating_stats_task())


def rating_stats_group_rows() -> int:
    """Rows one workgroup of K16's sweep owns (als_rating_stats_group_rows)."""
    return int(_lib.lib().als_rating_stats_group_rows())


def row_moments(block_or_csr, n_cols: int, ws: Workspace, other: Optional[torch.Tensor] = None,
                offset: float = 0.0, moments: Optional[torch.Tensor] = None,
                total: Optional[torch.Tensor] = None):
    """K16's sweep over one CSR side (als_row_moments): a RatingBlock, or (row_ptr int64
    [n + 1], col int32, val fp32) device tensors.  Terms e = val - offset - other[col] (other:
    f64 [n_cols] on the device, or None).  Returns (moments f64 [n_rows, 5], total f64 [5]),
    columns in RATING_MOMENTS order; a row without ratings has n = sum = M2 = 0 and NaN min /
    max.  moments / total: device tensors to write into."""
    L = _lib.lib()
    if isinstance(block_or_csr, RatingBlock):
        row_ptr, col, val = block_or_csr.row_ptr, block_or_csr.col, block_or_csr.val
    else:
        row_ptr, col, val = block_or_csr
    dev = row_ptr.device
    n_rows, nnz = int(row_ptr.numel()) - 1, int(val.numel())
    if n_rows < 0 or int(col.numel()) != nnz:
        raise ValueError("row_moments: row_ptr needs n_rows + 1 entries and col / val one length")
    if other is not None:
        if other.dtype != torch.float64 or other.numel() != int(n_cols):
            raise ValueError("row_moments: other must be a float64 table of n_cols entries")
        other = other.contiguous()
    if moments is None:
        moments = torch.empty((n_rows, len(RATING_MOMENTS)), dtype=torch.float64, device=dev)
    if total is None:
        total = torch.empty(len(RATING_MOMENTS), dtype=torch.float64, device=dev)
    off = _host_f64(offset)
    w = ws.get(L.als_rating_stats_scratch_bytes(nnz, n_rows))
    check(L.als_row_moments(ptr(row_ptr), ptr(col), ptr(val), nnz, n_rows, int(n_cols),
                            ptr(other), ctypes.addressof(off), ptr(moments), ptr(total), ptr(w),
                            w.numel(), stream_ptr(dev)), "als_row_moments")
    return moments, total


def bias_update(moments: torch.Tensor, damping: float, out: Optional[torch.Tensor] = None
                ) -> torch.Tensor:
    """sum_row / (damping + n_row) of a moments table (als_bias_update): f64 [n_rows], 0 for a
    row without ratings."""
    L = _lib.lib()
    n_rows = int(moments.shape[0])
    if out is None:
        out = torch.empty(n_rows, dtype=torch.float64, device=moments.device)
    d = _host_f64(damping)
    check(L.als_bias_update(ptr(moments), n_rows, ctypes.addressof(d), ptr(out),
                            stream_ptr(moments.device)), "als_bias_update")
    return out


def baseline_predict_rows(urow: torch.Tensor, irow: torch.Tensor, mu: float,
                          bu: Optional[torch.Tensor], bi: Optional[torch.Tensor], n_users: int,
                          n_items: int):
    """mu + bu[urow] + bi[irow] for pairs of dense rows (int32; a row outside its table, -1
    included, is an unknown id and adds nothing): (pred f32 [n], known uint8 [n], bit 0 = user
    known, bit 1 = item known).  bu / bi: f64 device tables or None (all zero)."""
    L = _lib.lib()
    dev = urow.device
    urow, irow = urow.to(torch.int32).contiguous(), irow.to(torch.int32).contiguous()
    if urow.shape != irow.shape or urow.dim() != 1:
        raise ValueError("baseline_predict_rows: urow and irow must be vectors of one length")
    n = int(urow.numel())
    pred = torch.empty(n, dtype=torch.float32, device=dev)
    known = torch.empty(n, dtype=torch.uint8, device=dev)
    m = _host_f64(mu)
    check(L.als_baseline_predict(ptr(urow), ptr(irow), n, ctypes.addressof(m), ptr(bu),
                                 int(n_users), ptr(bi), int(n_items), ptr(pred), ptr(known),
                                 stream_ptr(dev)), "als_baseline_predict")
    return pred, known


def rating_stats_dict(moments: torch.Tensor) -> dict:
    """count (int64), mean, std (population), std_sample (n - 1 in the denominator, NaN where
    n <= 1), min and max of each row of a moments table; mean and the rest are NaN for a row
    without ratings.  Device tensors."""
    n, s, m2 = moments[:, 0], moments[:, 1], moments[:, 2]
    nan = torch.full_like(n, float("nan"))
    has = n > 0
    return {"count": n.to(torch.int64), "mean": torch.where(has, s / n, nan),
            "std": torch.where(has, torch.sqrt(m2 / n), nan),
            "std_sample": torch.where(n > 1, torch.sqrt(m2 / (n - 1)), nan),
            "min": moments[:, 3].clone(), "max": moments[:, 4].clone()}


class Baseline:
    """A fitted mean / bias predictor mu + b_u + b_i (ALSCore.fit_baseline): mu a float, bu /
    bi f64 device tables in dense order (zeros where the method fits none), uidx / iidx the
    id maps, history the training objective after every sweep."""

    def __init__(self, method, mu, bu, bi, uidx: IdIndex, iidx: IdIndex, history, ws: Workspace,
                 reg_user: float = 0.0, reg_item: float = 0.0):
        self.method, self.mu, self.bu, self.bi = method, float(mu), bu, bi
        self.uidx, self.iidx, self.history, self.ws = uidx, iidx, list(history), ws
        self.reg_user, self.reg_item = float(reg_user), float(reg_item)
        self.device = bu.device

    def predict(self, users, items, return_known: bool = False):
        """f32 prediction per pair; an id the fit did not see adds a zero bias, so a pair
        unknown on both sides gets mu.  return_known: also the uint8 flags (bit 0 = user
        known, bit 1 = item known)."""
        u = _to_device(users, torch.int32, self.device)
        i = _to_device(items, torch.int32, self.device)
        pred, known = baseline_predict_rows(self.uidx.rows_of(u).to(torch.int32),
                                            self.iidx.rows_of(i).to(torch.int32), self.mu,
                                            self.bu, self.bi, self.uidx.n, self.iidx.n)
        return (pred, known) if return_known else pred

    def regression_metrics(self, users, items, ratings, through_origin: bool = False) -> dict:
        """regression_dict's keys for the predictions against held-out ratings, every pair
        used (dropped = 0): the moments are K8's column form over (ratings, predict())."""
        r = _to_device(ratings, torch.float32, self.device)
        pred = self.predict(users, items)
        if r.numel() != pred.numel():
            raise ValueError("users, items and ratings must have the same length")
        m = regression_moments_cols(r.double(), pred.double(), self.ws)
        return regression_dict(m.tolist(), through_origin)
