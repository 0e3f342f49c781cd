"""K19: co-rated neighbours, "who rated X also rated Y" (csrc/co_rated.hip: als_co_rated)."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from .._lib import check, ptr, stream_ptr
from .workspace import Workspace
from .schedule import RatingBlock

CO_RATED_MEASURES = ("count", "jaccard", "cosine")   # als_co_rated's measure codes 0, 1, 2
CO_RATED_MAX_TOP = 256
CO_RATED_PASS = 32        # queries in flight per pass when pass_queries is None
CO_RATED_MAX_PASS = 64


def co_rated_task() -> int:
    """Entries of a query row per task of K19's count pass (als_co_rated_task)."""
    return int(_lib.lib().als_co_rated_task())


def co_rated_window() -> int:
    """Slots of the LDS cache in front of a query's counters (als_co_rated_window)."""
    return int(_lib.lib().als_co_rated_window())


def _side(block):
    """(row_ptr, col, n_rows) of a RatingBlock or of a (row_ptr int64 [n + 1], col int32) pair."""
    if isinstance(block, RatingBlock):
        return block.row_ptr, block.col, int(block.n_rows)
    row_ptr, col = block[0], block[1]
    return row_ptr, col, int(row_ptr.numel()) - 1


def co_rated_rows(block_q, block_o, q_rows: torch.Tensor, top: int,
                  measure: str, min_common: int, allow_bits, ws: Workspace,
                  pass_queries: Optional[int] = None, task_entries: Optional[int] = None):
    """K19 (als_co_rated): for each dense row of q_rows (int32; rows of block_q's side) the
    `top` other rows of that side with the most raters in common.  block_q / block_o: the
    queried side's RatingBlock and the other side's, or (row_ptr int64 [n + 1], col int32)
    device tensors for each (the values are never read).
    measure: one of CO_RATED_MEASURES; min_common >= 1; allow_bits: the
    filters.pack_allow_bits mask or None.  pass_queries / task_entries: None = the library's
    defaults (tests force many passes and many tasks at small shapes).  Returns (idx int32
    [n_q, top], score f32 [n_q, top], common int32 [n_q, top]): score descending, ties by
    ascending row; open slots idx -1, score -inf, common 0.  Integer adds only: exact, and
    the same bits for every pass_queries / task_entries."""
    top, min_common = int(top), int(min_common)
    if measure not in CO_RATED_MEASURES:
        raise ValueError(f"measure must be one of {CO_RATED_MEASURES}, got {measure!r}")
    if not 1 <= top <= CO_RATED_MAX_TOP:
        raise ValueError(f"top must be in [1, {CO_RATED_MAX_TOP}], got {top}")
    if min_common < 1:
        raise ValueError(f"min_common must be >= 1, got {min_common}")
    p = 0 if pass_queries is None else int(pass_queries)
    t = 0 if task_entries is None else int(task_entries)
    if not 0 <= p <= CO_RATED_MAX_PASS or (pass_queries is not None and p < 1):
        raise ValueError(f"pass_queries must be in [1, {CO_RATED_MAX_PASS}], got {pass_queries}")
    if task_entries is not None and t < 1:
        raise ValueError(f"task_entries must be >= 1, got {task_entries}")
    L = _lib.lib()
    rp_q, col_q, n = _side(block_q)
    rp_o, col_o, n_o = _side(block_o)
    dev = rp_q.device
    q_rows = q_rows.to(device=dev, dtype=torch.int32).contiguous()
    n_q = int(q_rows.numel())
    idx = torch.empty((n_q, top), dtype=torch.int32, device=dev)
    score = torch.empty((n_q, top), dtype=torch.float32, device=dev)
    common = torch.empty((n_q, top), dtype=torch.int32, device=dev)
    w = ws.get(L.als_co_rated_scratch_bytes(n, n_q, top, p))
    check(L.als_co_rated(ptr(rp_q), ptr(col_q), n, ptr(rp_o), ptr(col_o), n_o, ptr(q_rows), n_q,
                         CO_RATED_MEASURES.index(measure), min_common, ptr(allow_bits), top, p, t,
                         ptr(idx), ptr(score), ptr(common), ptr(w), w.numel(), stream_ptr(dev)),
          "als_co_rated")
    return idx, score, common
