"""K1's schedule half (csrc/csr_build.hip: als_schedule_count, als_schedule_build): one
side's CSR plus the work schedule of its half-sweep (RatingBlock), the heavy-row task
length and the dual-path row limit the schedule is cut by."""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .. import _lib
from .._lib import check, ptr, stream_ptr
from .workspace import Workspace
from .csr import IdIndex, build_csr

DEFAULT_CHUNK = 4096  # ratings per heavy-row task (round 5: profiles/r05/ab_chunk*.jsonl)


def chunk_for(rank: int, implicit: bool) -> int:
    """Heavy-row task length of a half-sweep (ALSCore's default): a task's fp32 partial
    slot grows as k^2, so explicit fits at rank > 64 take four times the ratings per slot.
    Measured round 5 (profiles/r05/ab_chunk2.jsonl, ab_chunk3.jsonl): configs[3] (k = 128,
    explicit) 4096 / 8192 / 16384 ratings 275.1 / 270.6 / 266.3 ms/iter; at configs[1]
    (k = 64) 8192 took the longest rows' error to 1.2e-6 and at configs[2] (implicit) the
    >2048-rating rows sit at 8e-7 with 4096 already, so those keep 4096."""
    return 4 * DEFAULT_CHUNK if (rank > 64 and not implicit) else DEFAULT_CHUNK


DUAL_MAX_RATINGS = 96  # explicit, 64 < k <= 128: rows this short go through the n x n dual
# (round 5, configs[3]: limit 64 / 80 / 96 -> 288.9 / 275.8 / 267.2 ms/iter, profiles/r05/ab_dual_limit.jsonl)
DUAL_MAX_RATINGS_64 = 32  # explicit, 32 < k <= 64: the same for rows this short


def dual_limit(rank: int) -> int:
    """Longest row (ratings) solved through the n x n dual system at this rank; 0 = none.
    The dual system Y_S Y_S^T + lambda n I is full rank only while n <= rank: a longer
    row would trade the full-rank k x k primal for a rank-deficient n x n system whose
    smallest eigenvalues are lambda n (fp32 error growing as lambda shrinks), so the
    limit is min(96, rank) above rank 64 and 32 (< rank) at ranks 33-64."""
    if rank > 64:
        return min(DUAL_MAX_RATINGS, rank)
    return DUAL_MAX_RATINGS_64 if rank > 32 else 0


@dataclass
class RatingBlock:
    """One side's ratings in HBM as CSR plus its half-sweep work schedule."""
    n_rows: int
    nnz: int
    row_ptr: torch.Tensor
    col: torch.Tensor
    val: torch.Tensor
    chunk: int
    n_light: int
    n_heavy: int
    n_chunks: int
    light_rows: torch.Tensor
    heavy_rows: torch.Tensor
    heavy_slot_begin: torch.Tensor
    chunk_row: torch.Tensor
    chunk_begin: torch.Tensor
    chunk_end: torch.Tensor
    # short_counts[d] = light rows with <= d ratings, d = 0..DUAL_MAX_RATINGS (host ints)
    short_counts: tuple = ()
    short_nnz: tuple = ()   # ratings of those rows

    @property
    def n_short(self) -> int:
        return self.short_counts[-1] if self.short_counts else 0

    def n_dual(self, rank: int) -> int:
        """Light rows solved through the n x n dual system at this rank (explicit, reg > 0):
        the tail of the longest-first light list with <= dual_limit(rank) ratings."""
        d = dual_limit(rank)
        return self.short_counts[d] if (d and self.short_counts) else 0

    def dual_nnz(self, rank: int) -> int:
        """Ratings of the dual-path rows at this rank."""
        d = dual_limit(rank)
        return self.short_nnz[d] if (d and self.short_nnz) else 0


def build_block(row_ids: torch.Tensor, row_index: IdIndex, col_ids: torch.Tensor,
                col_index: IdIndex, vals: torch.Tensor, ws: Workspace,
                chunk: int = DEFAULT_CHUNK) -> RatingBlock:
    row_ptr, col, val = build_csr(row_ids, row_index, col_ids, col_index, vals, ws)
    return schedule_block(row_index.n, int(row_ids.numel()), row_ptr, col, val, ws, chunk)


def schedule_block(n_rows, nnz, row_ptr, col, val, ws: Workspace, chunk: int = DEFAULT_CHUNK
                   ) -> RatingBlock:
    L = _lib.lib()
    dev = row_ptr.device
    counts = torch.zeros(3, dtype=torch.int32, device=dev)
    check(L.als_schedule_count(ptr(row_ptr), n_rows, chunk, ptr(counts), stream_ptr(dev)),
          "als_schedule_count")
    n_light, n_heavy, n_chunks = (int(x) for x in counts.tolist())
    i32 = dict(dtype=torch.int32, device=dev)
    light = torch.empty(max(n_light, 1), **i32)
    heavy = torch.empty(max(n_heavy, 1), **i32)
    slot_begin = torch.empty(n_heavy + 1, **i32)
    crow = torch.empty(max(n_chunks, 1), **i32)
    cbeg = torch.empty(max(n_chunks, 1), dtype=torch.int64, device=dev)
    cend = torch.empty(max(n_chunks, 1), dtype=torch.int64, device=dev)
    w = ws.get(L.als_schedule_workspace_bytes(n_rows))
    check(L.als_schedule_build(ptr(row_ptr), n_rows, chunk, n_light, n_heavy, n_chunks,
                               ptr(light), ptr(heavy), ptr(slot_begin), ptr(crow), ptr(cbeg),
                               ptr(cend), ptr(w), w.numel(), stream_ptr(dev)),
          "als_schedule_build")
    counts, nzs = (0,) * (DUAL_MAX_RATINGS + 1), (0,) * (DUAL_MAX_RATINGS + 1)
    if n_light > 0:  # light rows are ordered by decreasing degree: the short ones are last
        lr = light[:n_light].long()
        deg = row_ptr[lr + 1] - row_ptr[lr]
        short = deg[deg <= DUAL_MAX_RATINGS]
        h = torch.bincount(short, minlength=DUAL_MAX_RATINGS + 1).to(torch.int64)
        w = h * torch.arange(DUAL_MAX_RATINGS + 1, device=h.device)
        counts = tuple(int(x) for x in torch.cumsum(h, 0).tolist())
        nzs = tuple(int(x) for x in torch.cumsum(w, 0).tolist())
    return RatingBlock(n_rows, nnz, row_ptr, col, val, chunk, n_light, n_heavy, n_chunks, light,
                       heavy, slot_begin, crow, cbeg, cend, counts, nzs)
