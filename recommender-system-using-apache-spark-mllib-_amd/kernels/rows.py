"""K7, K11, K13: the row-system kernels over ragged rows (csrc/fold_in.hip: als_fold_in;
csrc/explain.hip: als_explain; csrc/nnls.hip: als_nnls_rows; all three on
csrc/row_system.h)."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from .._lib import check, ptr, stream_ptr
from .workspace import Workspace, ld_for
from .schedule import DEFAULT_CHUNK


def fold_in_rows(row_ptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, Y: torch.Tensor,
                 n_src: int, rank: int, reg: float, implicit: bool, alpha: float,
                 yty: Optional[torch.Tensor], status: torch.Tensor, ws: Workspace):
    """K7 (als_fold_in): the factor row of every ragged row (row_ptr int64 [n + 1], col int32
    = dense rows of Y or -1, val f32: filters.ragged_rows) against the first n_src rows of
    the fixed factors Y, in one launch.  Returns (X f32 [n, ld_for(rank)], n_used int32
    [n]); a row without a used entry is zero.  status: device int32, row + 1 of a row whose
    normal equations were not positive definite (raise_status)."""
    L = _lib.lib()
    n = int(row_ptr.numel()) - 1
    dev = Y.device
    X = torch.empty((n, ld_for(rank)), dtype=torch.float32, device=dev)
    n_used = torch.empty(n, dtype=torch.int32, device=dev)
    need = int(L.als_fold_in_workspace_bytes(n, rank))
    w = ws.get(need) if need else None
    check(L.als_fold_in(ptr(row_ptr), ptr(col), ptr(val), n, ptr(Y), int(n_src), Y.shape[1],
                        rank, float(reg), int(bool(implicit)), float(alpha), ptr(yty), ptr(X),
                        X.shape[1], ptr(n_used), ptr(status), ptr(w), w.numel() if need else 0,
                        stream_ptr(dev)), "als_fold_in")
    return X, n_used


def nnls_rows(row_ptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, Y: torch.Tensor,
              n_src: int, rank: int, reg: float, implicit: bool, alpha: float,
              yty: Optional[torch.Tensor], ws: Workspace, chunk: int = DEFAULT_CHUNK,
              X: Optional[torch.Tensor] = None, iters: bool = False):
    """K13 (als_nnls_rows): fold_in_rows' rows solved under x >= 0 by Spark's NNLS solver —
    the same ragged input (a RatingBlock's row_ptr / col / val included) and the same
    normal equations, in three launches plus a device sort of the rows by degree.  chunk:
    ratings per task of a longer row.  X: the f32 [n, ld] table to write (a half-sweep's
    destination factors); None allocates [n, ld_for(rank)].  Returns (X, n_used int32 [n],
    iterations int32 [n] or None).  No row fails and there is no status word."""
    L = _lib.lib()
    n = int(row_ptr.numel()) - 1
    dev = Y.device
    if X is None:
        X = torch.empty((n, ld_for(rank)), dtype=torch.float32, device=dev)
    n_used = torch.empty(n, dtype=torch.int32, device=dev)
    it = torch.empty(n, dtype=torch.int32, device=dev) if iters else None
    if n == 0:
        return X, n_used, it
    if col.numel() == 0:  # rows without a single entry: never read, but not null
        col = torch.zeros(1, dtype=torch.int32, device=dev)
        val = torch.zeros(1, dtype=torch.float32, device=dev)
        nnz = 0
    else:
        nnz = int(col.numel())
    need = int(L.als_nnls_workspace_bytes(n, nnz, rank, int(chunk)))
    w = ws.get(need)
    check(L.als_nnls_rows(ptr(row_ptr), ptr(col), ptr(val), n, ptr(Y), int(n_src), Y.shape[1],
                          rank, float(reg), int(bool(implicit)), float(alpha), ptr(yty),
                          int(chunk), ptr(X), X.shape[1], ptr(n_used), ptr(it), ptr(w),
                          max(need, 256), stream_ptr(dev)), "als_nnls_rows")
    return X, n_used, it


EXPLAIN_MAX_TOP = 32


def explain_rows(row_ptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, Y: torch.Tensor,
                 n_src: int, rank: int, reg: float, implicit: bool, alpha: float,
                 yty: Optional[torch.Tensor], tgt_ptr: torch.Tensor, tgt: torch.Tensor,
                 top_n: int, status: torch.Tensor, ws: Workspace):
    """K11 (als_explain): every score of the ragged rows (fold_in_rows' inputs) against their
    ragged targets (tgt_ptr int64 [n + 1], tgt int32 = dense rows of Y or -1, tgt_ptr[n] ==
    tgt.numel() == T) split into one contribution per rating, in one launch.  Returns
    (score f32 [T], contrib_pos int32 [T, top_n] = entry offset inside the row or -1,
    contrib f32 [T, top_n] descending, n_used int32 [n]).  status as fold_in_rows."""
    L = _lib.lib()
    n = int(row_ptr.numel()) - 1
    T = int(tgt.numel())
    dev = Y.device
    if T == 0:  # the entry point wants addresses even when no slot is written
        tgt = torch.full((1,), -1, dtype=torch.int32, device=dev)
    score = torch.empty(max(T, 1), dtype=torch.float32, device=dev)
    pos = torch.empty((max(T, 1), int(top_n)), dtype=torch.int32, device=dev)
    contrib = torch.empty((max(T, 1), int(top_n)), dtype=torch.float32, device=dev)
    n_used = torch.empty(n, dtype=torch.int32, device=dev)
    if col.numel() == 0:  # rows without a single entry: never read, but not null
        col = torch.zeros(1, dtype=torch.int32, device=dev)
        val = torch.zeros(1, dtype=torch.float32, device=dev)
    need = int(L.als_explain_workspace_bytes(n, rank))
    w = ws.get(need) if need else None
    check(L.als_explain(ptr(row_ptr), ptr(col), ptr(val), n, ptr(Y), int(n_src), Y.shape[1],
                        rank, float(reg), int(bool(implicit)), float(alpha), ptr(yty),
                        ptr(tgt_ptr), ptr(tgt), int(top_n), ptr(score), ptr(pos), ptr(contrib),
                        ptr(n_used), ptr(status), ptr(w), w.numel() if need else 0,
                        stream_ptr(dev)), "als_explain")
    return score[:T], pos[:T], contrib[:T], n_used
