"""K10: the training objective (csrc/objective.hip: als_objective_side,
als_gram_dot_f64)."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from .._lib import check, ptr, stream_ptr
from .workspace import Workspace
from .schedule import RatingBlock

OBJECTIVE_SIDE = ("data", "scale", "reg", "n", "n_positive")   # als_objective_side's out


def objective_span() -> int:
    """Ratings one workgroup of K10's rating pass owns (als_objective_span)."""
    return int(_lib.lib().als_objective_span())


def objective_side(block: RatingBlock, X: torch.Tensor, Y: Optional[torch.Tensor], n_cols: int,
                   rank: int, implicit: bool, alpha: float, ws: Workspace,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K10's rating pass over one CSR side (als_objective_side): f64 [5] in OBJECTIVE_SIDE
    order — the data terms of the side's ratings against X (its rows) and Y (its columns),
    their absolute sum, sum_row n_row |x_row|^2 (not yet times regParam) and the two counts.
    Y None: the regulariser and the counts only.  out: a device f64 [5] to write into."""
    L = _lib.lib()
    if out is None:
        out = torch.empty(len(OBJECTIVE_SIDE), dtype=torch.float64, device=X.device)
    w = ws.get(L.als_objective_workspace_bytes(block.nnz, block.n_rows, rank))
    check(L.als_objective_side(ptr(block.row_ptr), ptr(block.col), ptr(block.val), block.nnz,
                               block.n_rows, int(n_cols), ptr(X), ptr(Y), X.shape[1], rank,
                               int(bool(implicit)), float(alpha), ptr(out), ptr(w), w.numel(),
                               stream_ptr(X.device)), "als_objective_side")
    return out


def gram_dot(A: torch.Tensor, n_a: int, B: torch.Tensor, n_b: int, rank: int, ws: Workspace,
             grams: bool = False, out: Optional[torch.Tensor] = None):
    """K10's <A^T A, B^T B>_F over the first n_a / n_b rows of two fp32 tables of one leading
    dimension, the Grams formed in fp64 (als_gram_dot_f64): a device f64 [1]; with grams=True
    (dot, A^T A, B^T B), the Grams f64 [rank, rank]."""
    L = _lib.lib()
    if A.shape[1] != B.shape[1]:
        raise ValueError("gram_dot: the two tables must share a leading dimension")
    dev = A.device
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=dev)
    ga = torch.empty((rank, rank), dtype=torch.float64, device=dev) if grams else None
    gb = torch.empty((rank, rank), dtype=torch.float64, device=dev) if grams else None
    w = ws.get(L.als_objective_workspace_bytes(0, max(int(n_a), int(n_b)), rank))
    check(L.als_gram_dot_f64(ptr(A), int(n_a), ptr(B), int(n_b), A.shape[1], rank, ptr(out),
                             ptr(ga), ptr(gb), ptr(w), w.numel(), stream_ptr(dev)),
          "als_gram_dot_f64")
    return (out, ga, gb) if grams else out
