"""Device-resident ALS engine (one process per GPU).

This is the host side of the hot path that replaces Spark's
``ml.recommendation.ALS.train`` (upstream) as reached from
RecommenderSystem.py:148-149 / :163 / :218, and ``predictAll`` +
``computeError`` (RecommenderSystem.py:103-129, :150, :165, :222, :232).
Every arithmetic step runs in libals_hip.so (HIP, gfx950); torch supplies
device memory, streams and the RNG for the initial factors only.

Data layout in HBM (DESIGN.md "Data layout"):
  users/items id maps  int32[id_space]   (id -> dense row or -1)
  user side  CSR       row_ptr int64[n_u+1], col int32[nnz] (dense item), val f32[nnz]
  item side  CSR       row_ptr int64[n_i+1], col int32[nnz] (dense user), val f32[nnz]
  factors              U f32[n_u, ld], V f32[n_i, ld], ld = roundup(rank, 4), pad cols 0
  schedule per side    light rows (LPT order), heavy rows, chunk tasks
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from . import filters as _filters
from ._lib import check, ptr, stream_ptr

DEFAULT_CHUNK = 4096  # ratings per heavy-row task (round 5: profiles/r05/ab_chunk*.jsonl)


def chunk_for(rank: int, implicit: bool) -> int:
    """Heavy-row task length of a half-sweep (ALSCore's default): a task's fp32 partial
    slot grows as k^2, so explicit fits at rank > 64 take four times the ratings per slot.
    Measured round 5 (profiles/r05/ab_chunk2.jsonl, ab_chunk3.jsonl): configs[3] (k = 128,
    explicit) 4096 / 8192 / 16384 ratings 275.1 / 270.6 / 266.3 ms/iter; at configs[1]
    (k = 64) 8192 took the longest rows' error to 1.2e-6 and at configs[2] (implicit) the
    >2048-rating rows sit at 8e-7 with 4096 already, so those keep 4096."""
    return 4 * DEFAULT_CHUNK if (rank > 64 and not implicit) else DEFAULT_CHUNK
MAX_RANK = 128       # k <= 64: gram_solve_kernel; 64 < k <= 128: W1 (one wavefront per system)
DUAL_MAX_RATINGS = 96  # explicit, 64 < k <= 128: rows this short go through the n x n dual
# (round 5, configs[3]: limit 64 / 80 / 96 -> 288.9 / 275.8 / 267.2 ms/iter, profiles/r05/ab_dual_limit.jsonl)
DUAL_MAX_RATINGS_64 = 32  # explicit, 32 < k <= 64: the same for rows this short

# als_solve_half phase bits (include/als_hip.h ALS_PHASE_*)
PHASE_LAUNCH1, PHASE_LAUNCH2, PHASE_PREP, PHASE_RSCALE, PHASE_DUAL, PHASE_RESCUE = 1, 2, 4, 8, 16, 32
PHASE_ALL = 63


def dual_limit(rank: int) -> int:
    """Longest row (ratings) solved through the n x n dual system at this rank; 0 = none.
    The dual system Y_S Y_S^T + lambda n I is full rank only while n <= rank: a longer
    row would trade the full-rank k x k primal for a rank-deficient n x n system whose
    smallest eigenvalues are lambda n (fp32 error growing as lambda shrinks), so the
    limit is min(96, rank) above rank 64 and 32 (< rank) at ranks 33-64."""
    if rank > 64:
        return min(DUAL_MAX_RATINGS, rank)
    return DUAL_MAX_RATINGS_64 if rank > 32 else 0


def ld_for(rank: int) -> int:
    return (rank + 3) // 4 * 4


class Workspace:
    """One growable device scratch buffer; the library never allocates on a compute call.

    shared_rating_scale: every block solved with this workspace has the same ratings
    (ALSCore's user- and item-major CSR of one rating set), so the rating scale word
    that als_solve_half's phase 8 leaves at the start of the buffer stays valid until
    another call uses the buffer or it is reallocated; solve_half then skips phase 8."""

    def __init__(self, device, shared_rating_scale: bool = False):
        self.device = device
        self.buf: Optional[torch.Tensor] = None
        self.shared_rating_scale = shared_rating_scale
        self.rating_scale_key = None

    def get(self, nbytes: int, keep_scale: bool = False) -> torch.Tensor:
        nbytes = max(int(nbytes), 256)
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            # the scale / rescue-count words: a call without PREP on a fresh buffer
            # must not start from garbage
            self.buf[:256].zero_()
            self.rating_scale_key = None
        if not keep_scale:
            self.rating_scale_key = None
        return self.buf


def _to_device(x, dtype, device) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=dtype).contiguous()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x)), device=device).to(dtype).contiguous()


# ---------------------------------------------------------------------------
# K1: id maps, CSR, schedule
# ---------------------------------------------------------------------------
@dataclass
class IdIndex:
    """Dense id map of one side (the device form of Spark's sorted InBlock.srcIds).

    Spark accepts any Int id (negative ones included).  The map is indexed by
    `id - offset`; `offset` is the smallest id when ids are negative or the id
    range starts far above 0, else 0 (ids used directly)."""
    map: torch.Tensor       # int32 [id_space], (id - offset) -> dense row or -1
    uniq: torch.Tensor      # int32 [n]   ascending ids - offset
    n: int
    offset: int = 0

    @property
    def id_space(self) -> int:
        return int(self.map.numel())

    def ids(self) -> torch.Tensor:
        """The original ids of the dense rows (ascending), int32."""
        return self.uniq if self.offset == 0 else (self.uniq.long() + self.offset).to(torch.int32)

    def rows_of(self, ids: torch.Tensor) -> torch.Tensor:
        """Dense row (int64) of each id, -1 when unknown."""
        k = ids.long() - self.offset
        ok = (k >= 0) & (k < self.id_space)
        out = torch.full_like(k, -1)
        out[ok] = self.map[k[ok]].long()
        return out

    def keys(self, ids: torch.Tensor) -> torch.Tensor:
        """Query ids -> map keys; ids outside the mapped range -> -1 (unknown)."""
        if self.offset == 0:
            return ids.to(torch.int32).contiguous()
        s = ids.long() - self.offset
        return torch.where((s >= 0) & (s < self.id_space), s, -1).to(torch.int32).contiguous()


MAX_ID_SPACE = 2 ** 31 - 1   # the map is indexed by int32


def id_offset(lo: int, hi: int) -> int:
    """Map offset for ids in [lo, hi]: 0 for the usual non-negative, compact ids."""
    off = 0 if (lo >= 0 and hi < (1 << 26)) else lo
    if hi - off + 1 > MAX_ID_SPACE:
        raise ValueError(f"id range [{lo}, {hi}] spans more than 2^31-1 values; this build "
                         "indexes ids through a dense int32 map")
    return off


def build_index(ids: torch.Tensor, id_space: int, ws: Workspace) -> IdIndex:
    L = _lib.lib()
    dev = ids.device
    mp = torch.empty(id_space, dtype=torch.int32, device=dev)
    uniq = torch.empty(id_space, dtype=torch.int32, device=dev)
    nu = torch.zeros(1, dtype=torch.int32, device=dev)
    need = L.als_index_workspace_bytes(ids.numel(), id_space)
    w = ws.get(need)
    check(L.als_index_build(ptr(ids), ids.numel(), id_space, ptr(mp), ptr(uniq), ptr(nu), ptr(w),
                            w.numel(), stream_ptr(dev)), "als_index_build")
    n = int(nu.item())
    return IdIndex(mp, uniq[:n].clone(), n)


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


def build_csr(row_ids: torch.Tensor, row_index: IdIndex, col_ids: torch.Tensor,
              col_index: IdIndex, vals: torch.Tensor, ws: Workspace):
    """K1 (als_csr_build) alone: (row_ptr int64 [n + 1], col int32, val f32) of one side,
    without a schedule."""
    L = _lib.lib()
    dev = row_ids.device
    nnz = int(row_ids.numel())
    n_rows = row_index.n
    row_ptr = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
    col = torch.empty(nnz, dtype=torch.int32, device=dev)
    val = torch.empty(nnz, dtype=torch.float32, device=dev)
    w = ws.get(L.als_csr_workspace_bytes(nnz, n_rows))
    check(L.als_csr_build(ptr(row_ids), ptr(row_index.map), ptr(col_ids), ptr(col_index.map),
                          ptr(vals), nnz, n_rows, ptr(row_ptr), ptr(col), ptr(val), ptr(w),
                          w.numel(), stream_ptr(dev)), "als_csr_build")
    return row_ptr, col, val


def build_block(row_ids: torch.Tensor, row_index: IdIndex, col_ids: torch.Tensor,
                col_index: IdIndex, vals: torch.Tensor, ws: Workspace,
                chunk: int = DEFAULT_CHUNK) -> RatingBlock:
    row_ptr, col, val = build_csr(row_ids, row_index, col_ids, col_index, vals, ws)
    return schedule_block(row_index.n, int(row_ids.numel()), row_ptr, col, val, ws, chunk)


def csr_merge_tile() -> int:
    """Output entries per workgroup of als_csr_merge (tests size their shapes from it)."""
    return int(_lib.lib().als_csr_merge_tile())


def merge_csr(row_ptr_old, col_old, val_old, n_cols_old: int, row_map, col_map, row_ptr_add,
              col_add, val_add):
    """K17 (als_csr_merge): the CSR K1 would build from concat(old ratings, batch), from the
    old side's CSR and the batch's CSR (built by K1 against the grown id maps), in one pass
    with no sort.  row_map / col_map: int32 [n_old] / [n_cols_old], the dense row each old
    row of this / the other side has after the growth, None where the side gained no id.
    Returns (row_ptr int64 [n_new + 1], col int32, val f32); the contract is in
    include/als_hip.h."""
    L = _lib.lib()
    dev = row_ptr_old.device
    n_old, n_new = int(row_ptr_old.numel()) - 1, int(row_ptr_add.numel()) - 1
    nnz_old, nnz_add = int(col_old.numel()), int(col_add.numel())
    row_ptr = torch.empty(n_new + 1, dtype=torch.int64, device=dev)
    col = torch.empty(nnz_old + nnz_add, dtype=torch.int32, device=dev)
    val = torch.empty(nnz_old + nnz_add, dtype=torch.float32, device=dev)
    check(L.als_csr_merge(ptr(row_ptr_old), ptr(col_old), ptr(val_old), nnz_old, n_old,
                          int(n_cols_old), ptr(row_map), ptr(col_map), ptr(row_ptr_add),
                          ptr(col_add), ptr(val_add), nnz_add, n_new, ptr(row_ptr), ptr(col),
                          ptr(val), stream_ptr(dev)), "als_csr_merge")
    return row_ptr, col, val


def grow_index(index: IdIndex, ids: torch.Tensor, ws: Workspace):
    """The id map of `index`'s ids plus `ids` (int32 original ids, device), as a fresh
    build_index over the union would make it: (grown IdIndex, new_of_old, new_rows).
    new_of_old: int32 [index.n], the dense row each old row has now (strictly increasing),
    None when no id is new; new_rows: int64, the dense rows of the new ids, ascending.  A new
    id below the old offset, or a negative one, re-bases the map (id_offset of the union)."""
    dev = ids.device
    old_lo, old_hi = int(index.uniq[0]) + index.offset, int(index.uniq[-1]) + index.offset
    lo, hi = min(old_lo, int(ids.min())), max(old_hi, int(ids.max()))
    off = id_offset(lo, hi)
    old_keys = (index.uniq.long() + (index.offset - off))
    keys = torch.cat([old_keys, ids.long() - off]).to(torch.int32).contiguous()
    grown = build_index(keys, hi - off + 1, ws)
    grown.offset = off
    if grown.n == index.n:
        return grown, None, torch.empty(0, dtype=torch.int64, device=dev)
    new_of_old = grown.map[old_keys].contiguous()
    is_new = torch.ones(grown.n, dtype=torch.bool, device=dev)
    is_new[new_of_old.long()] = False
    return grown, new_of_old, is_new.nonzero().flatten()


def csr_remove_tile() -> int:
    """Stored entries per workgroup of K18 (tests size their shapes from it)."""
    return int(_lib.lib().als_csr_remove_tile())


def remove_mark(row_ptr_old, col_old, row_ptr_del, col_del, ws: Workspace, count_hits=False):
    """K18, first call (als_csr_remove_mark): which stored entries of one side stay when the
    pairs of the delete CSR (row_ptr_del int64 [n + 1], col_del int32, every row's columns
    ascending; both None = delete nothing) leave.  Returns (keep_bits, tile_off, row_ptr_kept,
    del_hits): one bit per stored entry (int64 words holding the uint64 bits), the exclusive
    scan of the tiles' kept counts (tile_off[-1] = the entries that stay), the kept entries
    before every old row, and with count_hits the stored copies dropped per listed pair
    (else None).  The contract is in include/als_hip.h."""
    L = _lib.lib()
    dev = row_ptr_old.device
    n_old, nnz_old = int(row_ptr_old.numel()) - 1, int(col_old.numel())
    nnz_del = 0 if col_del is None else int(col_del.numel())
    tiles = -(-nnz_old // csr_remove_tile())
    keep_bits = torch.empty(-(-nnz_old // 64), dtype=torch.int64, device=dev)
    tile_off = torch.empty(tiles + 1, dtype=torch.int64, device=dev)
    row_ptr_kept = torch.empty(n_old + 1, dtype=torch.int64, device=dev)
    hits = torch.empty(nnz_del, dtype=torch.int32, device=dev) if count_hits else None
    w = ws.get(L.als_csr_remove_scratch_bytes(nnz_old, n_old))
    check(L.als_csr_remove_mark(ptr(row_ptr_old), ptr(col_old), nnz_old, n_old, ptr(row_ptr_del),
                                ptr(col_del), nnz_del, ptr(keep_bits), ptr(tile_off),
                                ptr(row_ptr_kept), ptr(hits), ptr(w), w.numel(), stream_ptr(dev)),
          "als_csr_remove_mark")
    return keep_bits, tile_off, row_ptr_kept, hits


def remove_compact(col_old, val_old, keep_bits, tile_off, col_map, n_cols_old: int,
                   nnz_out: int):
    """K18, second call (als_csr_remove_compact): (col int32 [nnz_out], val f32 [nnz_out]), the
    kept entries in their stored order, columns passed through col_map (int32 [n_cols_old], the
    dense row each old row of the other side has now, None = unchanged)."""
    L = _lib.lib()
    dev = col_old.device
    col = torch.empty(int(nnz_out), dtype=torch.int32, device=dev)
    val = torch.empty(int(nnz_out), dtype=torch.float32, device=dev)
    check(L.als_csr_remove_compact(ptr(col_old), ptr(val_old), int(col_old.numel()),
                                   ptr(keep_bits), ptr(tile_off), ptr(col_map), int(n_cols_old),
                                   ptr(col), ptr(val), int(nnz_out), stream_ptr(dev)),
          "als_csr_remove_compact")
    return col, val


def shrink_index(index: IdIndex, leaving_rows: torch.Tensor, ws: Workspace):
    """The mirror of grow_index: the id map of `index` without the dense rows `leaving_rows`
    (int64, device), as a fresh build_index over the remaining ids would make it — offset and
    id_space are derived again, so they move when the smallest or the largest id leaves.
    Returns (IdIndex, new_of_old): new_of_old int32 [index.n], the dense row each old row has
    now, -1 for a row that left; (index, None) when none leaves.  At least one row must stay."""
    if leaving_rows.numel() == 0:
        return index, None
    dev = index.uniq.device
    stay = torch.ones(index.n, dtype=torch.bool, device=dev)
    stay[leaving_rows] = False
    ids = index.uniq[stay].long() + index.offset
    if ids.numel() == 0:
        raise ValueError("shrink_index: every row leaves")
    lo, hi = int(ids[0]), int(ids[-1])
    off = id_offset(lo, hi)
    shrunk = build_index((ids - off).to(torch.int32).contiguous(), hi - off + 1, ws)
    shrunk.offset = off
    new_of_old = torch.full((index.n,), -1, dtype=torch.int32, device=dev)
    new_of_old[stay] = torch.arange(shrunk.n, dtype=torch.int32, device=dev)
    return shrunk, new_of_old


def _delete_csr(rows: torch.Tensor, cols: torch.Tensor, n_rows: int):
    """(row_ptr int64 [n_rows + 1], col int32) of distinct (row, col) pairs that are sorted by
    row, then column: every row's columns ascending, as als_csr_remove_mark wants them."""
    row_ptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=rows.device)
    row_ptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n_rows), 0)
    return row_ptr, cols.to(torch.int32).contiguous()


def gather_rows(row_ptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, rows: torch.Tensor):
    """The ragged rows `rows` (int64 dense rows) of a CSR as a CSR of their own, each row's
    entries in its stored order: (row_ptr int64 [m + 1], col int32, val f32), the input of
    fold_in_rows / nnls_rows."""
    beg = row_ptr[rows]
    ln = row_ptr[rows + 1] - beg
    out_ptr = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=row_ptr.device)
    out_ptr[1:] = torch.cumsum(ln, 0)
    src = torch.repeat_interleave(beg - out_ptr[:-1], ln) + torch.arange(
        int(out_ptr[-1]), device=row_ptr.device)
    return out_ptr, col[src].contiguous(), val[src].contiguous()


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


# ---------------------------------------------------------------------------
# K2/K3/K2b
# ---------------------------------------------------------------------------
def k_pad(rank: int) -> int:
    return int(_lib.lib().als_k_pad(rank))


def compute_yty(Y: torch.Tensor, n: int, rank: int, ws: Workspace) -> torch.Tensor:
    """fp64 YtY (lower-packed, k_pad) of the first n rows of Y."""
    L = _lib.lib()
    kp = k_pad(rank)
    out = torch.empty(kp * (kp + 1) // 2, dtype=torch.float64, device=Y.device)
    w = ws.get(L.als_yty_workspace_bytes(n, rank))
    check(L.als_yty(ptr(Y), n, Y.shape[1], rank, ptr(out), ptr(w), w.numel(),
                    stream_ptr(Y.device)), "als_yty")
    return out


def solve_half(block: RatingBlock, Y: torch.Tensor, X: torch.Tensor, rank: int, reg: float,
               implicit: bool, alpha: float, yty: Optional[torch.Tensor],
               status: torch.Tensor, ws: Workspace, phases: int = PHASE_ALL,
               ws_chunks: Optional[int] = None, dual: bool = True,
               ws_rows: Optional[int] = None) -> None:
    """One computeFactors pass: X[row] <- solve(A_row, b_row) for every row of `block`.
    phases (PHASE_* bits, als_hip.h ALS_PHASE_*): PREP (max |Y|, split table), RSCALE
    (rating scale), LAUNCH1 (chunk partials + primal light rows), DUAL (dual-path light
    rows), LAUNCH2 (heavy rows), RESCUE (rows outside the split window); PHASE_ALL = all
    in order.  ws_chunks / ws_rows: size the workspace for this many heavy-row chunks /
    rows (blocks sharing one Y prep).
    dual: explicit, reg > 0 — rows with <= dual_limit(rank) ratings are solved through
    the equivalent n x n dual system (als_hip.h n_light_primal); False keeps every row
    on the k x k normal equations."""
    L = _lib.lib()
    use_dual = dual and not implicit and reg > 0
    n_primal = block.n_light - block.n_dual(rank) if use_dual else block.n_light
    n_rows = max(block.n_light + block.n_heavy, ws_rows or 0)
    w = ws.get(L.als_solve_workspace_bytes(rank, max(block.n_chunks, ws_chunks or 0), Y.shape[0],
                                           n_rows), keep_scale=True)
    key = (w.data_ptr(), w.numel())
    if (phases & PHASE_RSCALE) and ws.shared_rating_scale and ws.rating_scale_key == key:
        phases &= ~PHASE_RSCALE  # the rating scale word of this rating set is already in place
        if phases == 0:
            return
    check(L.als_solve_half(ptr(block.row_ptr), ptr(block.col), ptr(block.val),
                           ptr(block.light_rows), block.n_light, n_primal,
                           ptr(block.heavy_rows),
                           ptr(block.heavy_slot_begin), block.n_heavy, ptr(block.chunk_row),
                           ptr(block.chunk_begin), ptr(block.chunk_end), block.n_chunks, 0, 0,
                           ptr(Y), Y.shape[0], ptr(X), X.shape[1], rank, float(reg),
                           int(bool(implicit)),
                           float(alpha), ptr(yty), ptr(status), ptr(w), w.numel(), int(phases),
                           stream_ptr(X.device)), "als_solve_half")
    if (phases & PHASE_RSCALE) and ws.shared_rating_scale:
        ws.rating_scale_key = key


@dataclass
class SplitSchedule:
    """Two-segment schedule of one CSR block (ABI 6, the sharded engine's pipelined item
    half-sweep).  Row r's ratings are [row_ptr[r], seg[r]) — the early segment, whose
    source rows lie in the first n_src_early rows of Y (already gathered) — then
    [seg[r], row_ptr[r+1]) (the late segment: the source chunk still arriving).  Each
    segment is cut into <= chunk-rating tasks; every row goes through the heavy-row
    path (fp32 task partials summed per row in fp64, then solved), early slots first.
    Slots are numbered from slot_base (several blocks sharing one workspace and one Y
    prep keep disjoint slot ranges: ShardedALS's item chunks)."""
    n_src_early: int
    rows: torch.Tensor          # int32 [n]: every row of the block, ascending
    slot_begin: torch.Tensor    # int32 [n+1]: early slots of row r
    slot_begin2: torch.Tensor   # int32 [n+1]: late slots of row r (after all early ones)
    early: tuple                # (chunk_row, chunk_begin, chunk_end, n_tasks)
    late: tuple
    slot_base: int = 0          # first slot of this block's range in the workspace

    @property
    def n_slots(self) -> int:
        """Slots of the workspace up to this block's last (slot_base included)."""
        return self.slot_base + self.early[3] + self.late[3]


def _segment_tasks(row_ids, begin, end, chunk: int, dev):
    """<= chunk-rating tasks over the per-row ranges [begin[r], end[r])."""
    ln = (end - begin).clamp(min=0)
    cnt = (ln + chunk - 1) // chunk
    n = int(cnt.sum())
    slot_begin = torch.zeros(len(ln) + 1, dtype=torch.int64, device=dev)
    slot_begin[1:] = torch.cumsum(cnt, 0)
    if n == 0:
        z32, z64 = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64,
                                                                              device=dev)
        return slot_begin, (z32, z64, z64, 0)
    crow = torch.repeat_interleave(torch.arange(len(ln), device=dev), cnt)
    j = torch.arange(n, device=dev) - slot_begin[:-1][crow]
    cb = begin[crow] + j * chunk
    ce = torch.minimum(cb + chunk, end[crow])
    return slot_begin, (row_ids[crow].to(torch.int32).contiguous(), cb.contiguous(),
                        ce.contiguous(), n)


def split_schedule(block: RatingBlock, seg: torch.Tensor, n_src_early: int,
                   chunk: int = DEFAULT_CHUNK, slot_base: int = 0) -> SplitSchedule:
    """The two-segment schedule of `block` (its rows' ratings ordered early-first, seg[r]
    = end of row r's early segment), its slots numbered from slot_base."""
    dev = block.row_ptr.device
    n = block.n_rows
    rp = block.row_ptr
    seg = seg.to(dev, torch.int64)
    rows = torch.arange(max(n, 1), dtype=torch.int32, device=dev)
    sb1, early = _segment_tasks(rows[:n], rp[:-1], seg, chunk, dev)
    sb2, late = _segment_tasks(rows[:n], seg, rp[1:], chunk, dev)
    sb1 = sb1 + slot_base
    sb2 = sb2 + early[3] + slot_base
    return SplitSchedule(int(n_src_early), rows, sb1.to(torch.int32).contiguous(),
                         sb2.to(torch.int32).contiguous(), early, late, int(slot_base))


def solve_half_split(block: RatingBlock, sched: SplitSchedule, part: str, Y: torch.Tensor,
                     X: torch.Tensor, rank: int, reg: float, implicit: bool, alpha: float,
                     yty: Optional[torch.Tensor], status: torch.Tensor, ws: Workspace,
                     prep: bool = True, ws_slots: Optional[int] = None,
                     ws_rows: Optional[int] = None) -> None:
    """One half of a two-segment half-sweep (ABI 6).  part "early": the early segments'
    task partials from the first sched.n_src_early rows of Y (PREP over that prefix,
    RSCALE, LAUNCH1), while the rest of Y may still be arriving; "late": the late
    segments' partials from all of Y, then every row's slots summed and solved
    (LAUNCH2) and the rescue (RESCUE, over the row's full ratings).  Both calls on
    the same workspace, early first, in stream order.  Both pass slot_begin2 (it marks
    the schedule two-segment: no heavy row is solved before its late partials).
    prep=False: Y's prep for this part was done by an earlier call on this workspace
    (blocks sharing one workspace with disjoint slot ranges, sized by ws_slots /
    ws_rows for the largest: all early calls first, then all late ones)."""
    L = _lib.lib()
    n = block.n_rows
    w = ws.get(L.als_solve_workspace_bytes(rank, max(sched.n_slots, ws_slots or 0), Y.shape[0],
                                           max(n, ws_rows or 0)))
    if part == "early":
        crow, cb, ce, nt = sched.early
        ph, slot0, n_src = PHASE_PREP | PHASE_RSCALE | PHASE_LAUNCH1, sched.slot_base, sched.n_src_early
    elif part == "late":
        crow, cb, ce, nt = sched.late
        ph = PHASE_PREP | PHASE_RSCALE | PHASE_LAUNCH1 | PHASE_LAUNCH2 | PHASE_RESCUE
        slot0, n_src = sched.slot_base + sched.early[3], Y.shape[0]
    else:
        raise ValueError(f"part must be 'early' or 'late', got {part!r}")
    if not prep:
        ph &= ~PHASE_PREP
    sb2 = sched.slot_begin2
    check(L.als_solve_half(ptr(block.row_ptr), ptr(block.col), ptr(block.val),
                           ptr(block.light_rows), 0, 0, ptr(sched.rows), ptr(sched.slot_begin), n,
                           ptr(crow), ptr(cb), ptr(ce), nt, ptr(sb2), slot0,
                           ptr(Y), n_src, ptr(X), X.shape[1], rank, float(reg),
                           int(bool(implicit)), float(alpha), ptr(yty), ptr(status), ptr(w),
                           w.numel(), int(ph), stream_ptr(X.device)), "als_solve_half (split)")


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


def group_pairs(rows: torch.Tensor, n_rows: int):
    """Pairs' row index (int64, in [0, n_rows)) -> (order, tgt_ptr int64 [n_rows + 1]):
    `order` lists the pairs grouped by row (stable: input order within a row), so pair
    order[s] fills target slot s of als_explain and each row is factored once."""
    rows = rows.reshape(-1).long()
    order = torch.sort(rows, stable=True).indices
    tgt_ptr = torch.zeros(int(n_rows) + 1, dtype=torch.int64, device=rows.device)
    if rows.numel():
        tgt_ptr[1:] = torch.cumsum(torch.bincount(rows, minlength=int(n_rows)), 0)
    return order, tgt_ptr


def raise_status(s: int, where: str = "") -> None:
    """Raise for a non-zero solve status word: row + 1 of a failed Cholesky (Spark's
    dppsv info > 0), or -1 when the fp64 rescue list overflowed (als_solve_half's
    LAUNCH phases ran twice without the RESCUE phase between them)."""
    if s < 0:
        raise RuntimeError(f"als_solve_half rescue list overflow{where}: the LAUNCH phases ran "
                           "again before the RESCUE phase consumed the list (unsolved rows)")
    if s > 0:
        raise RuntimeError(
            f"Cholesky failed (non-positive pivot) for dense row {s - 1}{where}: the normal "
            "equations are not positive definite (Spark raises from LAPACK dppsv here)")


# ---------------------------------------------------------------------------
# K4/K5
# ---------------------------------------------------------------------------
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


def ids_of(ids: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """Ids of top-k dense rows.  A slot the kernel left empty (idx -1, score -inf: every
    score of that query row NaN, from non-finite factors) keeps a placeholder id; the
    callers drop slots whose score is not finite (valid_slots)."""
    return ids[idx.long().clamp(min=0)]


def topk_rows(Q: torch.Tensor, n_q: int, V: torch.Tensor, n_v: int, rank: int, top: int):
    """(idx int32 [n_q, top], score f32 [n_q, top]); idx = dense V row, -1 past n_v."""
    L = _lib.lib()
    idx = torch.empty((n_q, top), dtype=torch.int32, device=Q.device)
    sc = torch.empty((n_q, top), dtype=torch.float32, device=Q.device)
    w = torch.empty(int(L.als_topk_workspace_bytes(n_q, n_v, rank, top)), dtype=torch.uint8,
                    device=Q.device)
    check(L.als_topk(ptr(Q), n_q, ptr(V), n_v, Q.shape[1], rank, top, ptr(idx), ptr(sc), ptr(w),
                     w.numel(), stream_ptr(Q.device)), "als_topk")
    return idx, sc


def topk_rows_filtered(Q: torch.Tensor, n_q: int, V: torch.Tensor, n_v: int, rank: int, top: int,
                       ex_begin, ex_end, ex_col, allow_bits):
    """topk_rows over the admissible rows of V only (als_topk_filtered): query row r may
    not list the V rows ex_col[ex_begin[r]:ex_end[r]] (int64 / int64 / int32 device
    tensors, ascending within a row; all three None = no exclusions) nor a row whose bit
    in allow_bits (int32 words of the uint32 mask; None = every row) is clear.  Slots
    past a row's admissible rows hold idx -1, score -inf.  All four None: topk_rows."""
    L = _lib.lib()
    idx = torch.empty((n_q, top), dtype=torch.int32, device=Q.device)
    sc = torch.empty((n_q, top), dtype=torch.float32, device=Q.device)
    w = torch.empty(int(L.als_topk_workspace_bytes(n_q, n_v, rank, top)), dtype=torch.uint8,
                    device=Q.device)
    check(L.als_topk_filtered(ptr(Q), n_q, ptr(V), n_v, Q.shape[1], rank, top, ptr(ex_begin),
                              ptr(ex_end), ptr(ex_col), ptr(allow_bits), ptr(idx), ptr(sc),
                              ptr(w), w.numel(), stream_ptr(Q.device)), "als_topk_filtered")
    return idx, sc


SIMILAR_MAX_TOP = 256     # als_similar: neighbours per query
SIMILAR_MAX_SLICES = 4096
# Distinct query rows from which ALSCore.similar leaves the table sweep (K12, one pass over
# the table per 16 queries) for the unit copy + K5 route (one set-up, then every query in
# one sweep).  Set from the measured crossover: DESIGN.md section K12,
# profiles/k12_similar_cost.json.
SIMILAR_SWEEP_MIN_ROWS = 256


def similar_rows(Q: torch.Tensor, n_q: int, T: torch.Tensor, n: int, rank: int, top: int,
                 self_rows, allow_bits, slices: int = 0):
    """K12 (als_similar): the `top` rows of the table T [n, ld] nearest in cosine to each of
    the n_q query vectors Q [n_q, ldq], from the raw fp32 rows.  self_rows (int32 [n_q] or
    None): the table row a query must never list, -1 for none; allow_bits: the
    filters.pack_allow_bits mask or None; slices: 0 = auto (tests pin it).  Returns (idx
    int32 [n_q, top], score f32 [n_q, top]), score descending, ties by ascending row;
    empty slots idx -1, score -inf."""
    n_q, n, rank, top, slices = int(n_q), int(n), int(rank), int(top), int(slices)
    if not 1 <= top <= SIMILAR_MAX_TOP:
        raise ValueError(f"top must be in [1, {SIMILAR_MAX_TOP}], got {top}")
    if not 1 <= rank <= MAX_RANK:
        raise ValueError(f"rank must be in [1, {MAX_RANK}], got {rank}")
    if not 0 <= slices <= SIMILAR_MAX_SLICES:
        raise ValueError(f"slices must be in [0, {SIMILAR_MAX_SLICES}] (0 = auto), got {slices}")
    if n_q < 0 or n < 0:
        raise ValueError("n_q and n must be >= 0")
    L = _lib.lib()
    dev = Q.device
    idx = torch.empty((n_q, top), dtype=torch.int32, device=dev)
    sc = torch.empty((n_q, top), dtype=torch.float32, device=dev)
    w = torch.empty(max(int(L.als_similar_workspace_bytes(n, min(n_q, 16), top, slices)), 256),
                    dtype=torch.uint8, device=dev)
    check(L.als_similar(ptr(T), n, T.shape[1], rank, ptr(Q), n_q, Q.shape[1], ptr(self_rows),
                        ptr(allow_bits), top, slices, ptr(idx), ptr(sc), ptr(w), w.numel(),
                        stream_ptr(dev)), "als_similar")
    return idx, sc


def unit_rows(T: torch.Tensor, n: int, rank: int, allow_bits=None):
    """als_similar_unit_rows: (unit-norm fp32 copy of T's first n rows, allow mask, valid
    int32 [n]).  The mask is a copy of allow_bits (or all ones) with the bit of every row
    that can be nobody's neighbour (zero norm, NaN, Inf) cleared, in the same launch; such
    rows are zeros in the copy and 0 in valid."""
    L = _lib.lib()
    n = int(n)
    dev = T.device
    out = torch.empty((n, T.shape[1]), dtype=torch.float32, device=dev)
    valid = torch.empty(n, dtype=torch.int32, device=dev)
    if allow_bits is None:
        bits = torch.full((max((n + 31) // 32, 1),), -1, dtype=torch.int32, device=dev)
    else:
        bits = allow_bits.clone()
    check(L.als_similar_unit_rows(ptr(T), n, T.shape[1], int(rank), ptr(out), ptr(bits),
                                  ptr(valid), stream_ptr(dev)), "als_similar_unit_rows")
    return out, bits, valid


def similar_rows_unit(rows: Optional[torch.Tensor], T: torch.Tensor, n: int, rank: int, top: int,
                      allow_bits=None):
    """The many-query route to similar_rows' contract, built from K5: a unit-norm copy of
    the table (unit_rows) is both Q and V of topk_rows_filtered, each query excludes its own
    row through the exclusion arrays (begin = r, end = r + 1 into col = arange(n)), and the
    lists of query rows without a direction (zero norm, NaN, Inf) are blanked afterwards —
    K5 would list the first rows by index at score 0.  rows: dense table rows (int64) that
    are the queries, None = every row.  Scores agree with similar_rows within 1e-5; pairs
    closer than that may be ordered differently by the two routes."""
    if not 1 <= int(top) <= SIMILAR_MAX_TOP:
        raise ValueError(f"top must be in [1, {SIMILAR_MAX_TOP}], got {top}")
    n = int(n)
    dev = T.device
    Tn, bits, valid = unit_rows(T, n, rank, allow_bits)
    col = torch.arange(max(n, 1), dtype=torch.int32, device=dev)
    if rows is None:
        Qn, beg, ok = Tn, torch.arange(n, dtype=torch.int64, device=dev), valid
    else:
        rows = rows.long()
        Qn, beg, ok = Tn.index_select(0, rows).contiguous(), rows.contiguous(), valid[rows]
    idx, sc = topk_rows_filtered(Qn, int(beg.numel()), Tn, n, rank, int(top), beg,
                                 (beg + 1).contiguous(), col, bits)
    dead = ok == 0
    idx[dead] = -1
    sc[dead] = float("-inf")
    return idx, sc


DIVERSIFY_MAX_POOL = 256  # als_diversify / als_list_similarity: slots per row
# Pool arrays (idx int32 + score f32 per slot) ALSCore.recommend_diverse keeps alive at once.
DIVERSIFY_POOL_BYTES = 1 << 30


def _check_lists(idx: torch.Tensor, n_v: int, rank: int) -> None:
    if idx.dim() != 2:
        raise ValueError(f"idx must be [n_q, m], got shape {tuple(idx.shape)}")
    if not 1 <= int(idx.shape[1]) <= DIVERSIFY_MAX_POOL:
        raise ValueError(f"lists must have 1 to {DIVERSIFY_MAX_POOL} slots, got {idx.shape[1]}")
    if not 1 <= int(rank) <= MAX_RANK:
        raise ValueError(f"rank must be in [1, {MAX_RANK}], got {rank}")
    if int(n_v) < 0:
        raise ValueError("n_v must be >= 0")


def diversify_rows(idx: torch.Tensor, sc: torch.Tensor, V: torch.Tensor, n_v: int, rank: int,
                   top: int, lam: float):
    """K14 (als_diversify): maximal-marginal-relevance re-ranking of each row's candidate
    pool.  idx int32 [n_q, m] / sc f32 [n_q, m]: the pool as topk_rows / topk_rows_filtered
    return it (dense rows of V [n_v, ld], open slots -1 / -inf), m <= DIVERSIFY_MAX_POOL;
    1 <= top <= m; lam in [0, 1] (1 = pure relevance, 0 = pure diversity after the first
    pick; rounded to fp32 on its way to the library).  Returns (idx int32 [n_q, top], score
    f32 [n_q, top], ils f64 [n_q]): the picks in pick order with their original scores, open
    slots -1 / -inf, and each list's mean pairwise cosine (NaN under two picks).  The
    contract is in include/als_hip.h."""
    _check_lists(idx, n_v, rank)
    if tuple(sc.shape) != tuple(idx.shape):
        raise ValueError(f"idx {tuple(idx.shape)} and sc {tuple(sc.shape)} must have one shape")
    n_q, m = int(idx.shape[0]), int(idx.shape[1])
    top, lam = int(top), float(lam)
    if not 1 <= top <= m:
        raise ValueError(f"top must be in [1, pool = {m}], got {top}")
    if not 0.0 <= lam <= 1.0:   # (a NaN fails both comparisons)
        raise ValueError(f"lam must be in [0, 1], got {lam}")
    L = _lib.lib()
    dev = V.device
    idx = idx.to(torch.int32).contiguous()
    sc = sc.to(torch.float32).contiguous()
    out_i = torch.empty((n_q, top), dtype=torch.int32, device=dev)
    out_s = torch.empty((n_q, top), dtype=torch.float32, device=dev)
    ils = torch.empty(n_q, dtype=torch.float64, device=dev)
    check(L.als_diversify(ptr(V), int(n_v), V.shape[1], int(rank), ptr(idx), ptr(sc), n_q, m, top,
                          lam, ptr(out_i), ptr(out_s), ptr(ils), stream_ptr(dev)),
          "als_diversify")
    return out_i, out_s, ils


def list_similarity_rows(idx: torch.Tensor, V: torch.Tensor, n_v: int, rank: int):
    """K14 (als_list_similarity): ils f64 [n_q], the mean cosine over the unordered pairs of
    the slots of idx int32 [n_q, m] (m <= DIVERSIFY_MAX_POOL) that name a row of V [n_v, ld]
    (0 <= idx < n_v; anything else, such as the -1 of an open slot, is skipped); NaN with
    fewer than two.  A row of V without a direction (zero norm, NaN, Inf) counts with
    cosine 0."""
    _check_lists(idx, n_v, rank)
    L = _lib.lib()
    dev = V.device
    idx = idx.to(torch.int32).contiguous()
    n_q, m = int(idx.shape[0]), int(idx.shape[1])
    out = torch.empty(n_q, dtype=torch.float64, device=dev)
    check(L.als_list_similarity(ptr(V), int(n_v), V.shape[1], int(rank), ptr(idx), n_q, m,
                                ptr(out), stream_ptr(dev)), "als_list_similarity")
    return out


# ---------------------------------------------------------------------------
# K15: the lists of all rows together (exposure, concentration, popularity)
# ---------------------------------------------------------------------------
LIST_MAX_AT = 256  # als_list_exposure / als_list_novelty: list positions read per row
LIST_METRIC_FIELDS = ("coverage", "gini", "entropy", "effectiveItems", "personalization",
                      "topItemShare", "novelty", "averagePopularity", "longTailShare", "lists",
                      "entries", "skipped")


def _list_rows_args(idx, at, who: str):
    """(n_q, idx_ld, at) of a list matrix for the K15 calls; raises before the library is
    touched."""
    if (not isinstance(idx, torch.Tensor) or idx.dtype != torch.int32 or idx.dim() != 2
            or (idx.shape[1] > 1 and idx.stride(1) != 1)):
        raise ValueError(f"{who}: idx must be an int32 [n_q, width] tensor with unit stride "
                         "along a row")
    at = int(at)
    if not 1 <= at <= LIST_MAX_AT:
        raise ValueError(f"{who}: at must be in [1, {LIST_MAX_AT}], got {at}")
    if idx.shape[1] < at:
        raise ValueError(f"{who}: lists of width {idx.shape[1]} < at = {at}")
    n_q = int(idx.shape[0])
    ld = int(idx.stride(0)) if n_q > 1 else int(idx.shape[1])  # one row: any stride
    return n_q, ld, at


def list_exposure_window() -> int:
    """Rows per LDS counter window of als_list_exposure (0: the kernel keeps none)."""
    return int(_lib.lib().als_list_exposure_window())


def list_exposure_rows(idx: torch.Tensor, at: int, n_v: int, allow_bits=None, *, counts=None,
                       skipped=None):
    """K15 (als_list_exposure) over the lists idx (int32 [n_q, >= at], dense rows): how often
    each of the n_v rows is named in the first `at` positions.  An entry outside [0, n_v) —
    the -1 of an open slot — or with its bit clear in allow_bits (filters.pack_allow_bits;
    None: every row) is skipped.  Returns (counts int32 [n_v], skipped int64 [1]), both on
    the device; given `counts` (and `skipped`) from an earlier call, the new lists are added
    to them, so lists can be fed in chunks.  Integer adds: exact, and the same bits every
    run."""
    n_q, ld, at = _list_rows_args(idx, at, "list_exposure_rows")
    n_v = int(n_v)
    if n_v < 0:
        raise ValueError("list_exposure_rows: n_v must be >= 0")
    accumulate = counts is not None
    if accumulate and (counts.dtype != torch.int32 or counts.numel() != n_v
                       or not counts.is_contiguous()):
        raise ValueError(f"list_exposure_rows: counts must be a contiguous int32 [{n_v}] tensor")
    if skipped is not None and not accumulate:
        raise ValueError("list_exposure_rows: skipped= continues an earlier call: pass its "
                         "counts too")
    L = _lib.lib()
    dev = idx.device
    if counts is None:
        counts = torch.empty(n_v, dtype=torch.int32, device=dev)
    if skipped is None:
        skipped = torch.zeros(1, dtype=torch.int64, device=dev)
    check(L.als_list_exposure(ptr(idx), n_q, ld, at, n_v, ptr(allow_bits), int(accumulate),
                              ptr(counts), ptr(skipped), stream_ptr(dev)), "als_list_exposure")
    return counts, skipped


def list_concentration(counts: torch.Tensor, n_v: int, allow_bits, n_lists: int, at: int,
                       ws: Workspace) -> torch.Tensor:
    """K15 (als_list_concentration): f64 [7] on the device = catalogue rows, rows listed, total,
    Gini index, Shannon entropy (bits), pair overlap sum c (c - 1) / 2, largest count, over the
    counts of the catalogue rows (every row, or those set in allow_bits).  Gini and entropy are
    NaN when nothing is listed."""
    n_v = int(n_v)
    if counts.dtype != torch.int32 or counts.numel() != n_v or not counts.is_contiguous():
        raise ValueError(f"list_concentration: counts must be a contiguous int32 [{n_v}] tensor")
    if not 1 <= int(at) <= LIST_MAX_AT:
        raise ValueError(f"list_concentration: at must be in [1, {LIST_MAX_AT}], got {at}")
    L = _lib.lib()
    dev = counts.device
    out = torch.empty(7, dtype=torch.float64, device=dev)
    w = ws.get(L.als_list_concentration_scratch_bytes(n_v))
    check(L.als_list_concentration(ptr(counts), n_v, ptr(allow_bits), int(n_lists), int(at),
                                   ptr(out), ptr(w), w.numel(), stream_ptr(dev)),
          "als_list_concentration")
    return out


def list_novelty_rows(idx: torch.Tensor, at: int, n_v: int, pop: torch.Tensor, n_pop: int,
                      ws: Workspace, allow_bits=None, tail_bits=None, per_row: bool = False):
    """K15 (als_list_novelty) over the lists idx (as list_exposure_rows): pop int32 [n_v] = how
    often each row was rated, n_pop = rows of the listing side, tail_bits = the long-tail rows
    (the form of allow_bits; None: no long-tail share).  Returns (sums f64 [7] = sum of row
    novelty (mean log2(n_pop / pop) over the entries with pop > 0), rows with one, sum of row
    mean popularity, rows with a valid entry, sum of row long-tail share, valid entries, skipped
    entries; per-row f64 [n_q, 3] = novelty, mean popularity, long-tail share with NaN where
    undefined, or None)."""
    n_q, ld, at = _list_rows_args(idx, at, "list_novelty_rows")
    n_v = int(n_v)
    if pop.dtype != torch.int32 or pop.numel() != n_v or not pop.is_contiguous():
        raise ValueError(f"list_novelty_rows: pop must be a contiguous int32 [{n_v}] tensor")
    if int(n_pop) < 1:
        raise ValueError(f"list_novelty_rows: n_pop must be >= 1, got {n_pop}")
    L = _lib.lib()
    dev = idx.device
    out = torch.empty(7, dtype=torch.float64, device=dev)
    rows = torch.empty((n_q, 3), dtype=torch.float64, device=dev) if per_row else None
    w = ws.get(L.als_list_novelty_scratch_bytes(n_q))
    check(L.als_list_novelty(ptr(idx), n_q, ld, at, n_v, ptr(allow_bits), ptr(pop), int(n_pop),
                             ptr(tail_bits), ptr(out), ptr(rows), ptr(w), w.numel(),
                             stream_ptr(dev)), "als_list_novelty")
    return out, rows


def long_tail_bits(pop: torch.Tensor, n_v: int, head_fraction: float, cat_rows=None):
    """The long tail as a bit mask (filters.pack_allow_bits): every catalogue row (cat_rows,
    ascending dense rows; None: all n_v) outside the floor(head_fraction * n) most-rated ones,
    n = the catalogue's size.  Rows rated equally often at the cut go to the head by ascending
    row (one stable torch.sort)."""
    head_fraction = float(head_fraction)
    if not 0.0 < head_fraction < 1.0:
        raise ValueError(f"head_fraction must be inside (0, 1), got {head_fraction}")
    n_v = int(n_v)
    if cat_rows is None:
        cat_rows = torch.arange(n_v, device=pop.device)
    cat_rows = cat_rows.long()
    n_head = int(math.floor(head_fraction * int(cat_rows.numel())))
    order = torch.sort(pop[cat_rows].long(), descending=True, stable=True).indices
    return _filters.pack_allow_bits(cat_rows[order[n_head:]], n_v)


def list_metrics_dict(conc, nov, n_lists: int, at: int, skipped: int = 0,
                      tail: bool = True) -> dict:
    """K15's raw sums (host lists: als_list_concentration's 7, als_list_novelty's 7 or None
    when no popularity is known) as the beyond-accuracy measures of n_lists lists of `at`
    slots:
      coverage          catalogue rows listed at least once / catalogue rows
      gini, entropy     of the exposure counts (entropy in bits); effectiveItems = 2 ** entropy
      personalization   1 - mean overlap of two lists = 1 - pairs / (C(n_lists, 2) at);
                        NaN under two lists
      topItemShare      the share of the lists that name the most listed row
      novelty           mean over the lists of the mean log2(n_pop / popularity)
      averagePopularity mean over the lists of the mean popularity of what they name
      longTailShare     mean over the lists of the share of long-tail rows
      lists, entries (valid ones), skipped (open slots, unknown ids, rows off the catalogue)
    The three popularity fields are NaN without `nov` (longTailShare also with tail=False)."""
    nan = float("nan")

    def ratio(a, b):
        return a / b if b > 0 else nan
    n_lists, at = int(n_lists), int(at)
    pairs = n_lists * (n_lists - 1) // 2
    entropy = conc[4]
    out = {"coverage": ratio(conc[1], conc[0]), "gini": conc[3], "entropy": entropy,
           "effectiveItems": 2.0 ** entropy if entropy == entropy else nan,
           "personalization": 1.0 - conc[5] / (pairs * at) if pairs > 0 else nan,
           "topItemShare": ratio(conc[6], n_lists),
           "novelty": nan, "averagePopularity": nan, "longTailShare": nan,
           "lists": n_lists, "entries": int(conc[2]), "skipped": int(skipped)}
    if nov is not None:
        out["novelty"] = ratio(nov[0], nov[1])
        out["averagePopularity"] = ratio(nov[2], nov[3])
        if tail:
            out["longTailShare"] = ratio(nov[4], nov[3])
        out["skipped"] = int(nov[6])
    return out


def list_metrics_rows(rows: torch.Tensor, at: int, n_v: int, ws: Workspace, *, allow_bits=None,
                      cat_rows=None, pop=None, n_pop=None, head_fraction: float = 0.2,
                      per_row: bool = False):
    """The three K15 calls over one list matrix (int32 [n, >= at] dense rows) and
    list_metrics_dict of their sums.  allow_bits / cat_rows: the catalogue as a mask and as
    ascending rows (both None: all n_v rows).  pop / n_pop as list_novelty_rows; without pop
    the popularity fields are NaN.  Returns (dict, per-row f64 [n, 3] or None)."""
    n, _, at = _list_rows_args(rows, at, "list_metrics_rows")
    head_fraction = float(head_fraction)
    if not 0.0 < head_fraction < 1.0:
        raise ValueError(f"head_fraction must be inside (0, 1), got {head_fraction}")
    counts, skipped = list_exposure_rows(rows, at, n_v, allow_bits)
    conc = list_concentration(counts, n_v, allow_bits, n, at, ws)
    nov = pr = None
    if pop is not None:
        tail = long_tail_bits(pop, n_v, head_fraction, cat_rows)
        nov, pr = list_novelty_rows(rows, at, n_v, pop, n_pop, ws, allow_bits, tail, per_row)
        nov = nov.tolist()
    elif per_row:
        pr = torch.full((n, 3), float("nan"), dtype=torch.float64, device=rows.device)
    return list_metrics_dict(conc.tolist(), nov, n, at, int(skipped.item())), pr


MAX_RANK_AT = 256  # als_rank_metrics: list positions scored per row


def rank_metrics_rows(idx: torch.Tensor, at: int, begin, end, col, ws: Workspace,
                      per_row: bool = False):
    """K6 over the lists idx (int32 [n_q, >= at], dense rows, negative = empty slot)
    against the relevant sets col[begin[r]:end[r]] (strictly ascending: filters.
    relevance_lists).  Returns (sums f64 [6] = sum precision, sum recall, sum AP, sum
    NDCG, rows with a relevant set, rows with a hit; per-row f64 [n_q, 4] or None)."""
    L = _lib.lib()
    if idx.dtype != torch.int32 or idx.dim() != 2 or (idx.shape[1] > 1 and idx.stride(1) != 1):
        raise ValueError("rank_metrics_rows: idx must be an int32 [n_q, width] tensor with "
                         "unit stride along a row")
    if idx.shape[1] < int(at):
        raise ValueError(f"rank_metrics_rows: lists of width {idx.shape[1]} < at = {at}")
    n_q = int(idx.shape[0])
    out = torch.empty(6, dtype=torch.float64, device=idx.device)
    rows = torch.empty((n_q, 4), dtype=torch.float64, device=idx.device) if per_row else None
    w = ws.get(L.als_rank_metrics_workspace_bytes(n_q))
    ld = int(idx.stride(0)) if n_q > 1 else int(idx.shape[1])  # one row: any stride
    check(L.als_rank_metrics(ptr(idx), n_q, ld, int(at),
                             ptr(begin), ptr(end), ptr(col), ptr(out), ptr(rows), ptr(w),
                             w.numel(), stream_ptr(idx.device)), "als_rank_metrics")
    return out, rows


def rank_metrics_dict(sums, rows: int) -> dict:
    """The means over `rows` query rows of K6's sums (host list of 6); NaN when rows == 0."""
    def mean(x):
        return x / rows if rows > 0 else float("nan")
    return {"precision": mean(sums[0]), "recall": mean(sums[1]), "map": mean(sums[2]),
            "ndcg": mean(sums[3]), "hitRate": mean(sums[5]), "rows": int(rows)}


FULL_RANK_SUMS = ("sum_w_pr", "sum_w", "sum_row_pr", "sum_auc", "auc_rows", "sum_rr", "rr_rows",
                  "rows", "pairs", "inadmissible", "pr_rows")   # als_full_rank_metrics' sums_out


def rank_positions_table() -> int:
    """Relevant entries one workgroup of K9 ranks per sweep of V (its LDS threshold table)."""
    return int(_lib.lib().als_rank_positions_table())


def rank_positions_rows(Q: torch.Tensor, n_q: int, V: torch.Tensor, n_v: int, rank: int,
                        rel_begin, rel_end, rel_col, ex_begin=None, ex_end=None, ex_col=None,
                        allow_bits=None):
    """K9's sweep (als_rank_positions): for every relevant entry rel_col[e] of query row r
    (rel_begin / rel_end / rel_col as filters.relevance_lists gives them) the admissible rows
    of V that score strictly higher and equal, and per query row the admissible rows.  The
    ex_* / allow_bits filter is topk_rows_filtered's.  Returns (above int32 [len(rel_col)],
    tied int32, n_adm int32 [n_q]); above = tied = -1 for an entry that is itself
    inadmissible or scores NaN, and for entries of rel_col no row points at."""
    L = _lib.lib()
    dev = Q.device
    above = torch.full((max(int(rel_col.numel()), 1),), -1, dtype=torch.int32, device=dev)
    tied = torch.full_like(above, -1)
    n_adm = torch.zeros(max(int(n_q), 1), dtype=torch.int32, device=dev)
    check(L.als_rank_positions(ptr(Q), int(n_q), ptr(V), int(n_v), Q.shape[1], int(rank),
                               ptr(rel_begin), ptr(rel_end), ptr(rel_col), ptr(ex_begin),
                               ptr(ex_end), ptr(ex_col), ptr(allow_bits), ptr(above), ptr(tied),
                               ptr(n_adm), 0, 0, stream_ptr(dev)), "als_rank_positions")
    return above[:rel_col.numel()], tied[:rel_col.numel()], n_adm[:int(n_q)]


def full_rank_sums_rows(above, tied, n_adm, rel_begin, rel_end, ws: Workspace, weights=None,
                        per_row: bool = False):
    """K9's reduction (als_full_rank_metrics) of rank_positions_rows' counts: (sums f64 [11] in
    FULL_RANK_SUMS order; per-row f64 [n_q, 3] = mean percentile rank, AUC, RR, or None)."""
    L = _lib.lib()
    n_q = int(n_adm.numel())
    dev = n_adm.device
    out = torch.empty(len(FULL_RANK_SUMS), dtype=torch.float64, device=dev)
    rows = torch.empty((n_q, 3), dtype=torch.float64, device=dev) if per_row else None
    w = ws.get(L.als_full_rank_workspace_bytes(n_q))
    check(L.als_full_rank_metrics(ptr(above), ptr(tied), ptr(n_adm), n_q, ptr(rel_begin),
                                  ptr(rel_end), ptr(weights), ptr(out), ptr(rows), ptr(w),
                                  w.numel(), stream_ptr(dev)), "als_full_rank_metrics")
    return out, rows


def full_rank_dict(sums) -> dict:
    """The full-ranking metrics from K9's sums (host list of 11, FULL_RANK_SUMS order).
    expectedPercentileRank = sum w pr / sum w over the valid pairs (Hu, Koren & Volinsky's
    measure when w is the held-out rating; 0.5 = random, lower is better),
    meanPercentileRank = mean of the rows' mean percentile rank, auc / mrr = means of the
    row AUC / reciprocal rank over the rows where each is defined.  A mean with an empty
    denominator is NaN.  rows = query rows with a valid pair, pairs = valid pairs,
    inadmissible = pairs left out because the filter excludes the item itself or its score
    is NaN."""
    s = [float(x) for x in sums]
    if len(s) != len(FULL_RANK_SUMS):
        raise ValueError(f"full_rank_dict: {len(FULL_RANK_SUMS)} sums expected, got {len(s)}")

    def ratio(a, b):
        return a / b if b > 0 else float("nan")
    return {"expectedPercentileRank": ratio(s[0], s[1]), "meanPercentileRank": ratio(s[2], s[10]),
            "auc": ratio(s[3], s[4]), "mrr": ratio(s[5], s[6]), "rows": int(s[7]),
            "pairs": int(s[8]), "inadmissible": int(s[9])}


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


# ---------------------------------------------------------------------------
# K16: rating statistics and bias baselines
# ---------------------------------------------------------------------------
RATING_MOMENTS = ("n", "sum", "M2", "min", "max")   # als_row_moments' columns, and its total
BASELINE_METHODS = ("global", "item", "user", "bias")


def rating_stats_task() -> int:
    """Ratings per task of a long row in K16's sweep (als_rating_stats_task)."""
    return int(_lib.lib().als_rating_stats_task())


def rating_stats_group_rows() -> int:
    """Rows one workgroup of K16's sweep owns (als_rating_stats_group_rows)."""
    return int(_lib.lib().als_rating_stats_group_rows())


def _host_f64(x) -> ctypes.c_double:
    """A host double the library reads through its address before the call returns."""
    return ctypes.c_double(float(x))


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


# ---------------------------------------------------------------------------
# The engine
# ---------------------------------------------------------------------------
def make_engine(users, items, ratings, device=None):
    """The engine behind ALS.fit / ALS.train: one GPU (ALSCore), or — when this process
    is one rank of an initialised torch.distributed group of world size > 1 —
    the sharded engine (distributed.ShardedALS), fed with this rank's partition
    of the ratings (the role of a Spark DataFrame partition)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        from .distributed import ShardedALS
        return ShardedALS(users, items, ratings, device=device)
    return ALSCore(users, items, ratings, device=device)


class ALSCore:
    """Ratings, id maps, both CSR sides and both factor matrices resident on one GPU."""

    def __init__(self, users, items, ratings, device=None, chunk: Optional[int] = None):
        """chunk: ratings per heavy-row task; None = chunk_for(rank, implicit) of each
        half-sweep (the blocks are rescheduled when a fit asks for another length)."""
        _lib.require_gpu()
        self._auto_chunk = chunk is None
        chunk = DEFAULT_CHUNK if chunk is None else chunk
        self.device = torch.device(device) if device is not None else torch.device(
            "cuda", torch.cuda.current_device())
        # both CSR sides hold the same ratings: one rating scale for every half-sweep
        self.ws = Workspace(self.device, shared_rating_scale=True)
        # computeYtY's task slots in a buffer of their own: written over the solve
        # workspace they would clobber its rating scale word, re-measured every half-sweep
        self.ws_yty = Workspace(self.device)
        u = _to_device(users, torch.int32, self.device)
        i = _to_device(items, torch.int32, self.device)
        r = _to_device(ratings, torch.float32, self.device)
        if not (u.numel() == i.numel() == r.numel()):
            raise ValueError("users, items and ratings must have the same length")
        if u.numel() == 0:
            raise ValueError("ALS needs at least one rating")
        umin, umax = int(u.min()), int(u.max())
        imin, imax = int(i.min()), int(i.max())
        uoff, ioff = id_offset(umin, umax), id_offset(imin, imax)
        if uoff:
            u = (u.long() - uoff).to(torch.int32)
        if ioff:
            i = (i.long() - ioff).to(torch.int32)
        self.nnz = int(u.numel())
        self.uidx = build_index(u, umax - uoff + 1, self.ws)
        self.iidx = build_index(i, imax - ioff + 1, self.ws)
        self.uidx.offset, self.iidx.offset = uoff, ioff
        self.user_block = build_block(u, self.uidx, i, self.iidx, r, self.ws, chunk)
        self.item_block = build_block(i, self.iidx, u, self.uidx, r, self.ws, chunk)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._train_ex = {}  # user_side -> sorted training exclusion list (train_exclusion)
        self._fit_params = None  # reg / implicit / alpha / nonnegative of the last fit
        self._touched = None     # (user rows, item rows) that took ratings since the last fit
        self.objective_history = []   # (iteration, objective) pairs of the last fit (K10)
        self.iterations_run = 0       # where the last fit stopped
        self.U: Optional[torch.Tensor] = None
        self.V: Optional[torch.Tensor] = None
        self.rank = 0

    @classmethod
    def from_factors(cls, user_ids, U, item_ids, V, device=None) -> "ALSCore":
        """A serving-only core (no ratings, cannot fit) from saved factors: ids ascending,
        U/V host or device arrays [n, rank].  predict / rmse / top-k run as after fit()."""
        _lib.require_gpu()
        self = cls.__new__(cls)
        self.device = torch.device(device) if device is not None else torch.device(
            "cuda", torch.cuda.current_device())
        self.ws = Workspace(self.device)
        self.ws_yty = self.ws
        self.nnz = 0
        self._auto_chunk = False
        self.user_block = self.item_block = None
        self._train_ex = {}
        self._fit_params = None
        self._touched = None
        self.objective_history = []
        self.iterations_run = 0
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        U = _to_device(U, torch.float32, self.device)
        V = _to_device(V, torch.float32, self.device)
        rank = int(U.shape[1])
        if V.shape[1] != rank or not (1 <= rank <= MAX_RANK):
            raise ValueError(f"factor ranks {U.shape[1]}/{V.shape[1]} invalid (max {MAX_RANK})")
        idx = []
        for ids, F in ((user_ids, U), (item_ids, V)):
            ids = _to_device(ids, torch.int32, self.device)
            if ids.numel() != F.shape[0] or ids.numel() == 0:
                raise ValueError("factor ids must be non-empty and match the rows")
            if ids.numel() > 1 and not bool((ids[1:] > ids[:-1]).all()):
                raise ValueError("factor ids must be strictly ascending")
            off = id_offset(int(ids.min()), int(ids.max()))
            key = (ids.long() - off)
            mp = torch.full((int(key.max()) + 1,), -1, dtype=torch.int32, device=self.device)
            mp[key] = torch.arange(ids.numel(), dtype=torch.int32, device=self.device)
            idx.append(IdIndex(mp, key.to(torch.int32), int(ids.numel()), off))
        self.uidx, self.iidx = idx
        self.rank = rank
        ld = ld_for(rank)
        self.U = torch.zeros((U.shape[0], ld), dtype=torch.float32, device=self.device)
        self.V = torch.zeros((V.shape[0], ld), dtype=torch.float32, device=self.device)
        self.U[:, :rank] = U
        self.V[:, :rank] = V
        return self

    @property
    def n_users(self) -> int:
        return self.uidx.n

    @property
    def n_items(self) -> int:
        return self.iidx.n

    # Spark ALS.initialize: unit-norm Gaussian rows, fp32.
    def init_factors(self, rank: int, seed: int = 0, U0=None) -> None:
        if rank < 1 or rank > MAX_RANK:
            raise ValueError(f"rank must be in [1, {MAX_RANK}] on this build, got {rank}")
        self.rank = rank
        ld = ld_for(rank)
        self.U = torch.zeros((self.n_users, ld), dtype=torch.float32, device=self.device)
        self.V = torch.zeros((self.n_items, ld), dtype=torch.float32, device=self.device)
        if U0 is not None:
            U0 = _to_device(U0, torch.float32, self.device)
            if tuple(U0.shape) != (self.n_users, rank):
                raise ValueError(f"U0 must have shape {(self.n_users, rank)}")
            self.U[:, :rank] = U0
        else:
            g = torch.Generator(device=self.device)
            g.manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)
            x = torch.randn((self.n_users, rank), generator=g, device=self.device,
                            dtype=torch.float32)
            self.U[:, :rank] = x / torch.linalg.vector_norm(x, dim=1, keepdim=True)

    def schedule_for(self, implicit: bool) -> None:
        """The default heavy-row task length for this fit's rank and feedback type (no-op
        when the core was built with an explicit chunk)."""
        if self._auto_chunk:
            self.rechunk(chunk_for(self.rank, implicit))

    def rechunk(self, chunk: int) -> None:
        """Reschedule both sides for `chunk`-rating heavy-row tasks (same CSR)."""
        for name in ("user_block", "item_block"):
            b = getattr(self, name)
            if b.chunk != chunk:
                setattr(self, name, schedule_block(b.n_rows, b.nnz, b.row_ptr, b.col, b.val,
                                                   self.ws, chunk))

    def _half_sweep_nnls(self, block, Y, n_src, X, reg, implicit, alpha):
        """One computeFactors pass with Spark's NNLSSolver (K13); a buffer of its own, so the
        solve workspace keeps its rating scale."""
        if getattr(self, "ws_nnls", None) is None:
            self.ws_nnls = Workspace(self.device)
        yty = compute_yty(Y, n_src, self.rank, self.ws_yty) if implicit else None
        nnls_rows(block.row_ptr, block.col, block.val, Y, n_src, self.rank, reg, implicit, alpha,
                  yty, self.ws_nnls, DEFAULT_CHUNK, X=X)

    def half_sweep_items(self, reg, implicit=False, alpha=1.0, nonnegative=False):
        if nonnegative:
            return self._half_sweep_nnls(self.item_block, self.U, self.n_users, self.V, reg,
                                         implicit, alpha)
        self.schedule_for(implicit)
        yty = compute_yty(self.U, self.n_users, self.rank, self.ws_yty) if implicit else None
        solve_half(self.item_block, self.U, self.V, self.rank, reg, implicit, alpha, yty,
                   self.status, self.ws)

    def half_sweep_users(self, reg, implicit=False, alpha=1.0, nonnegative=False):
        if nonnegative:
            return self._half_sweep_nnls(self.user_block, self.V, self.n_items, self.U, reg,
                                         implicit, alpha)
        self.schedule_for(implicit)
        yty = compute_yty(self.V, self.n_items, self.rank, self.ws_yty) if implicit else None
        solve_half(self.user_block, self.V, self.U, self.rank, reg, implicit, alpha, yty,
                   self.status, self.ws)

    def iterate(self, reg, implicit=False, alpha=1.0, nonnegative=False):
        """One ALS iteration in Spark's order: items from users, then users from items.
        nonnegative: every row is solved under x >= 0 (K13, Spark's NNLSSolver)."""
        if nonnegative:
            self.half_sweep_items(reg, implicit, alpha, nonnegative=True)
            self.half_sweep_users(reg, implicit, alpha, nonnegative=True)
            return
        self.half_sweep_items(reg, implicit, alpha)
        self.half_sweep_users(reg, implicit, alpha)

    def check_status(self) -> None:
        raise_status(int(self.status.item()))

    def objective(self, reg, implicit=False, alpha=1.0) -> dict:
        """The training objective of the current factors: the function each half-sweep
        minimises row by row (K10; Spark's lambda * numExplicits weighting, als_hip.h):
          explicit  sum_obs (r - s)^2 + reg (sum_u n_u |x_u|^2 + sum_i n_i |y_i|^2)
          implicit  sum_all c (p - s)^2 + reg (sum_u n+_u |x_u|^2 + sum_i n+_i |y_i|^2)
        in fp64 over the stored fp32 factors.  Returns {"objective", "data" (implicit: the
        all-pairs term, <U^T U, V^T V>_F plus the correction over the ratings), "reg"
        (times reg already), "scale" (the sum of the absolute values of everything added:
        the size rounding errors are relative to), "n", "n_positive"}.  Deterministic: two
        calls on the same factors return the same bits.  One host sync."""
        if self.user_block is None:
            raise ValueError("objective needs the ratings the model was fitted on; this core "
                             "was built from saved factors (from_factors / load) and has none")
        if self.U is None or self.V is None:
            raise ValueError("objective needs factors: fit() the core or init_factors() first")
        if reg < 0 or alpha < 0:
            raise ValueError(f"reg and alpha must be >= 0, got {reg}, {alpha}")
        if getattr(self, "ws_obj", None) is None:
            # a buffer of its own: the solve workspace keeps the rating scale between
            # half-sweeps, and observing a fit must not make it re-measure anything
            self.ws_obj = Workspace(self.device)
        n = len(OBJECTIVE_SIDE)
        out = torch.zeros(2 * n + 1, dtype=torch.float64, device=self.device)
        objective_side(self.user_block, self.U, self.V, self.n_items, self.rank, implicit, alpha,
                       self.ws_obj, out[:n])
        objective_side(self.item_block, self.V, None, self.n_users, self.rank, implicit, alpha,
                       self.ws_obj, out[n:2 * n])
        if implicit:
            gram_dot(self.U, self.n_users, self.V, self.n_items, self.rank, self.ws_obj,
                     out=out[2 * n:])
        v = out.tolist()
        side_u, side_i, frob = dict(zip(OBJECTIVE_SIDE, v[:n])), dict(zip(OBJECTIVE_SIDE, v[n:])), v[2 * n]
        data = side_u["data"] + frob
        regv = float(reg) * (side_u["reg"] + side_i["reg"])
        return {"objective": data + regv, "data": data, "reg": regv,
                "scale": side_u["scale"] + abs(frob) + regv, "n": int(side_u["n"]),
                "n_positive": int(side_u["n_positive"])}

    def fit(self, rank, max_iter, reg, implicit=False, alpha=1.0, seed=0, U0=None,
            checkpoint_dir=None, checkpoint_interval=10, resume=False, objective_every=0,
            tol=None, nonnegative=False):
        """max_iter ALS iterations from the seeded (or given U0) start.  checkpoint_dir:
        write U, V every checkpoint_interval iterations (checkpoint.py); resume
        (True / "auto"): continue from the checkpoint there at its iteration.
        objective_every = m > 0: evaluate objective() after iterations m, 2m, ... and after
        the last one, into self.objective_history as (iteration, value) pairs (a resumed fit
        starts its list at the first evaluated iteration after the checkpoint).  tol: stop
        after an evaluated iteration whose decrease L_prev - L_cur <= tol * L_prev (tol
        alone evaluates every iteration); a checkpoint due at that iteration is still
        written.  self.iterations_run is where the fit stopped.  With both off (the default)
        nothing is evaluated and no host sync is added.
        nonnegative: Spark's `nonnegative=true` — the same seeded signed start, then every
        half-sweep solves its rows under x >= 0 (K13), so all factors are >= 0 from the first
        one on; objective_every / tol evaluate the same objective.  Not with checkpoint_dir:
        a checkpoint does not record the solver, and resuming a Cholesky fit as NNLS (or
        the reverse) must not happen silently."""
        from . import checkpoint as C
        nonnegative = bool(nonnegative)
        if nonnegative and checkpoint_dir:
            raise ValueError("nonnegative=True cannot be combined with checkpoint_dir: a "
                             "checkpoint does not record the solver")
        every = int(objective_every)
        if every < 0:
            raise ValueError(f"objective_every must be >= 0, got {objective_every}")
        if tol is not None:
            tol = float(tol)
            if not tol >= 0:
                raise ValueError(f"tol must be >= 0, got {tol}")
            every = every or 1
        init = C.init_key(seed, U0) if checkpoint_dir else None
        start, Uc, Vc = C.resume_point(checkpoint_dir, resume, self, rank, reg, implicit, alpha,
                                       max_iter, init)
        self.init_factors(rank, seed, Uc if Uc is not None else U0)
        if Vc is not None:
            self.V[:, :rank] = _to_device(Vc, torch.float32, self.device)
        self.status.zero_()
        self._fit_params = {"reg": float(reg), "implicit": bool(implicit), "alpha": float(alpha),
                            "nonnegative": nonnegative}
        self._touched = None   # a fit re-solves every row
        self.objective_history = []
        self.iterations_run = start
        prev = None
        for it in range(start, max_iter):
            if nonnegative:
                self.iterate(reg, implicit, alpha, nonnegative=True)
            else:
                self.iterate(reg, implicit, alpha)
            stop = False
            if every and ((it + 1) % every == 0 or it + 1 == max_iter):
                cur = self.objective(reg, implicit, alpha)["objective"]
                self.objective_history.append((it + 1, cur))
                stop = tol is not None and prev is not None and prev - cur <= tol * prev
                prev = cur
            C.maybe_save(checkpoint_dir, checkpoint_interval, it + 1, self, rank, reg, implicit,
                         alpha, init=init)
            self.iterations_run = it + 1
            if stop:
                break
        self.check_status()
        return self

    # ---- K17: ratings that arrive after the fit ----
    def _solve_rows(self, csr, rows, Y, n_src, p, yty_of=None):
        """(X f32 [m, ld], n_used int32 [m]) of the dense rows `rows` of the CSR (row_ptr,
        col, val), each from its full rating list in stored order against the fixed factors
        Y: K7, or K13 when the fit was nonnegative.  yty_of: (table, rows) the implicit YtY
        is taken of, None = Y.  Raises, before anything is stored, for a row that is not
        positive definite."""
        row_ptr, col, val = gather_rows(*csr, rows)
        yty = compute_yty(*(yty_of or (Y, n_src)), self.rank, self.ws_yty) if p["implicit"] else None
        if p["nonnegative"]:
            if getattr(self, "ws_nnls", None) is None:
                self.ws_nnls = Workspace(self.device)
            X, n_used, _ = nnls_rows(row_ptr, col, val, Y, n_src, self.rank, p["reg"],
                                     p["implicit"], p["alpha"], yty, self.ws_nnls)
            return X, n_used
        if getattr(self, "ws_rows", None) is None:
            # a buffer of its own: the solve workspace keeps its rating scale word
            self.ws_rows = Workspace(self.device)
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        X, n_used = fold_in_rows(row_ptr, col, val, Y, n_src, self.rank, p["reg"], p["implicit"],
                                 p["alpha"], yty, status, self.ws_rows)
        raise_status(int(status.item()), " of the rows being re-solved (ascending dense row)")
        return X, n_used

    def _update_params(self, reg=None, implicit=None, alpha=None, nonnegative=None) -> dict:
        p = dict(self._fit_params or {})
        for k, v in (("reg", reg), ("implicit", implicit), ("alpha", alpha),
                     ("nonnegative", nonnegative)):
            if v is not None:
                p[k] = v
        if "reg" not in p:
            raise ValueError("no fit to take reg / implicit / alpha / nonnegative from: fit() "
                             "the core first, or pass reg=")
        p = {"reg": float(p["reg"]), "implicit": bool(p.get("implicit", False)),
             "alpha": float(p.get("alpha", 1.0)), "nonnegative": bool(p.get("nonnegative", False))}
        if p["reg"] < 0 or p["alpha"] < 0:
            raise ValueError(f"reg and alpha must be >= 0, got {p['reg']}, {p['alpha']}")
        return p

    def add_ratings(self, users, items, ratings, *, seed=0) -> dict:
        """Add a batch of ratings to the core in place (the reference adds a new user's
        twelve ratings to the training set and fits again, RecommenderSystem.py:207-247).
        users / items / ratings: host or device arrays of one length; new ids on either side
        are welcome, and a pair that is already rated (or twice in the batch) is one more
        rating, as Spark keeps duplicates.  After the call every rating-derived thing — both
        id maps, both CSR sides and their schedules, nnz — is what ALSCore(concat(old,
        batch)) would hold, bit for bit:
          a. both id maps grow (als_index_build over the old ids plus the batch's; a new id
             below the offset, or a negative one, re-bases the map)
          b. K1 builds the batch's two small CSRs against the grown maps
          c. K17 (als_csr_merge) writes each side's merged CSR in one pass with no sort, and
             the side is scheduled again at its current chunk
          d. on a core with factors, the rows of U and V move to their new places bit for
             bit and every NEW row gets factors: new users from their ratings against the
             current V (K7, or K13 after a nonnegative fit; the parameters of the last fit;
             a rating of an item that is new as well is left out, as fold_in leaves out an
             unknown item), then new items against the grown U.  A new row without a used
             rating — a new user who rated only new items — gets a unit-norm Gaussian row
             from `seed`, as init_factors gives: a zero row would stay zero through every
             later sweep.  Rows that existed keep their factors until refresh() or refit()
          e. everything cached from the ratings (the train exclusion lists, the workspace's
             rating scale) is dropped.
        Needs one transient second copy of each side's col and val (8 B per rating and
        side, until the call returns).  An empty batch is a no-op; before any fit only the ratings are
        merged.  Nothing is changed when the call raises.
        Returns {"added", "new_users", "new_items" (ids, ascending), "touched_users",
        "touched_items" (int64 dense rows in the grown maps, ascending: the rows whose
        rating lists changed)}; the touched rows of every add since the last fit are kept
        for refresh()."""
        if self.user_block is None:
            raise ValueError("add_ratings needs the ratings the model was fitted on; this core "
                             "was built from saved factors (from_factors / load) and has none")
        u = _to_device(users, torch.int32, self.device)
        i = _to_device(items, torch.int32, self.device)
        r = _to_device(ratings, torch.float32, self.device)
        if not (u.numel() == i.numel() == r.numel()):
            raise ValueError("users, items and ratings must have the same length")
        empty = torch.empty(0, dtype=torch.int64, device=self.device)
        if u.numel() == 0:
            return {"added": 0, "new_users": empty.to(torch.int32), "new_items":
                    empty.to(torch.int32), "touched_users": empty, "touched_items": empty}
        return self._add_commit(self._add_compute(u, i, r, seed))

    def _add_compute(self, u, i, r, seed, user_csr=None, item_csr=None, nnz=None) -> dict:
        """add_ratings steps a-d on device arrays, storing nothing: the grown state of the
        core's id maps and of the two CSR sides (the core's own blocks, or the (row_ptr, col,
        val) triples given, which hold `nnz` ratings and may have empty rows: set_ratings
        passes the sides it has just compacted)."""
        ub, ib = self.user_block, self.item_block
        user_csr = user_csr or (ub.row_ptr, ub.col, ub.val)
        item_csr = item_csr or (ib.row_ptr, ib.col, ib.val)
        uidx, umap, new_u = grow_index(self.uidx, u, self.ws)
        iidx, imap, new_i = grow_index(self.iidx, i, self.ws)
        uk, ik = uidx.keys(u), iidx.keys(i)
        add_u = build_csr(uk, uidx, ik, iidx, r, self.ws)
        user_csr = merge_csr(*user_csr, ib.n_rows, umap, imap, *add_u)
        add_i = build_csr(ik, iidx, uk, uidx, r, self.ws)
        item_csr = merge_csr(*item_csr, ub.n_rows, imap, umap, *add_i)
        nnz = (self.nnz if nnz is None else int(nnz)) + int(u.numel())
        touched_u = (add_u[0][1:] > add_u[0][:-1]).nonzero().flatten()
        touched_i = (add_i[0][1:] > add_i[0][:-1]).nonzero().flatten()
        U = V = None
        if self.rank > 0 and self.U is not None:
            U, V = self._grown_factors(uidx.n, iidx.n, umap, imap, new_u, new_i, user_csr,
                                       item_csr, int(seed))
        return dict(added=int(u.numel()), uidx=uidx, iidx=iidx, umap=umap, imap=imap,
                    new_u=new_u, new_i=new_i, user_csr=user_csr, item_csr=item_csr, nnz=nnz,
                    touched_u=touched_u, touched_i=touched_i, U=U, V=V)

    def _add_commit(self, st: dict) -> dict:
        """Store what _add_compute made and return add_ratings' report: nothing before this
        touched the core, and from here on it cannot fail half-way."""
        uidx, iidx, umap, imap, nnz = st["uidx"], st["iidx"], st["umap"], st["imap"], st["nnz"]
        new_u, new_i, touched_u, touched_i = (st[k] for k in ("new_u", "new_i", "touched_u",
                                                              "touched_i"))
        U, V = st["U"], st["V"]
        ub, ib = self.user_block, self.item_block
        self.user_block = schedule_block(uidx.n, nnz, *st["user_csr"], self.ws, ub.chunk)
        self.item_block = schedule_block(iidx.n, nnz, *st["item_csr"], self.ws, ib.chunk)
        self.uidx, self.iidx, self.nnz = uidx, iidx, nnz
        if U is not None:
            self.U, self.V = U, V
        self._train_ex = {}
        self.ws.rating_scale_key = None   # the batch may hold the largest |rating|
        if self._touched is not None:    # rows touched earlier, in the grown numbering
            tu, ti = self._touched
            tu = tu if umap is None else umap[tu].long()
            ti = ti if imap is None else imap[ti].long()
            touched_all = (torch.unique(torch.cat([tu, touched_u])),
                           torch.unique(torch.cat([ti, touched_i])))
        else:
            touched_all = (touched_u, touched_i)
        self._touched = touched_all
        return {"added": st["added"], "new_users": uidx.ids()[new_u], "new_items":
                iidx.ids()[new_i], "touched_users": touched_u, "touched_items": touched_i}

    def _grown_factors(self, n_u, n_i, umap, imap, new_u, new_i, user_csr, item_csr, seed):
        """add_ratings step d: (U, V) for the grown id maps."""
        ld = ld_for(self.rank)

        def moved(F, n, mp):
            if mp is None:
                return F.clone()
            out = torch.zeros((n, ld), dtype=torch.float32, device=self.device)
            out[mp.long()] = F
            return out

        U, V = moved(self.U, n_u, umap), moved(self.V, n_i, imap)
        p = self._update_params() if self._fit_params else None
        g = torch.Generator(device=self.device)
        g.manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)

        def fill(F, rows, csr, Y, n_src, unknown_cols, yty_of=None):
            if rows.numel() == 0:
                return
            X = torch.zeros((rows.numel(), ld), dtype=torch.float32, device=self.device)
            n_used = torch.zeros(rows.numel(), dtype=torch.int32, device=self.device)
            if p is not None:
                row_ptr, col, val = csr
                if unknown_cols.numel():   # a column that has no factors yet is not used
                    hide = torch.zeros(n_src, dtype=torch.bool, device=self.device)
                    hide[unknown_cols] = True
                    col = torch.where(hide[col.long()], -1, col).to(torch.int32)
                X, n_used = self._solve_rows((row_ptr, col, val), rows, Y, n_src, p, yty_of)
            blank = (n_used == 0).nonzero().flatten()
            if blank.numel():
                x = torch.randn((blank.numel(), self.rank), generator=g, device=self.device,
                                dtype=torch.float32)
                X[blank] = 0
                X[blank, :self.rank] = x / torch.linalg.vector_norm(x, dim=1, keepdim=True)
            F[rows] = X

        # YtY of the V the model had: the rows just added are zero and add nothing, and the
        # sum keeps the bits fold_in would have used before the growth
        fill(U, new_u, user_csr, V, n_i, new_i, (self.V, self.n_items))
        fill(V, new_i, item_csr, U, n_u, new_u[:0])
        return U, V

    def refresh(self, *, reg=None, implicit=None, alpha=None, nonnegative=None, sweeps=1):
        """Re-solve only the rows add_ratings touched since the last fit — the "serve it
        now" path between add_ratings and the next refit: touched users against V, then
        touched items against the new U, `sweeps` times, each row from its full merged rating
        list in block order (K7 als_fold_in, or K13 als_nnls_rows when nonnegative; YtY of
        the fixed side when implicit).  Every other row keeps its bits.  reg / implicit /
        alpha / nonnegative default to those of the last fit.  One workgroup per row in
        fp64, so it pays for a handful of rows only: on the ML-25M shape at rank 64 one new
        user's 12 ratings (1 + 12 rows) take 1.0 ms, 0.6 of a full iteration, but a batch of
        10^4 ratings (19 thousand rows) 12.6 ms, 7.5 iterations — there refit(1) is the
        cheaper call.  Returns self."""
        if self.user_block is None:
            raise ValueError("refresh needs the ratings the model was fitted on; this core "
                             "was built from saved factors (from_factors / load) and has none")
        if self.U is None or self.V is None:
            raise ValueError("refresh needs factors: fit() the core first")
        p = self._update_params(reg, implicit, alpha, nonnegative)
        if int(sweeps) < 1:
            raise ValueError(f"sweeps must be >= 1, got {sweeps}")
        if self._touched is None:
            return self
        tu, ti = self._touched
        for _ in range(int(sweeps)):
            if tu.numel():
                b = self.user_block
                X, _ = self._solve_rows((b.row_ptr, b.col, b.val), tu, self.V, self.n_items, p)
                self.U[tu] = X
            if ti.numel():
                b = self.item_block
                X, _ = self._solve_rows((b.row_ptr, b.col, b.val), ti, self.U, self.n_users, p)
                self.V[ti] = X
        return self

    def refit(self, max_iter, **fit_kwargs):
        """The warm start: fit(rank, max_iter, ..., U0=the current U) with the parameters of
        the last fit (fit_kwargs override them and pass objective_every / tol through).
        Spark's order solves the items first from U alone and never reads V, so continuing
        from the current U is continuing the fit."""
        if self.user_block is None:
            raise ValueError("refit needs the ratings the model was fitted on; this core "
                             "was built from saved factors (from_factors / load) and has none")
        if self.U is None or self.rank < 1:
            raise ValueError("refit needs factors: fit() the core first")
        if "U0" in fit_kwargs or "rank" in fit_kwargs:
            raise ValueError("refit starts from the current U at the current rank")
        kw = self._update_params(*(fit_kwargs.pop(k, None) for k in
                                   ("reg", "implicit", "alpha", "nonnegative")))
        kw.update(fit_kwargs)
        return self.fit(self.rank, int(max_iter), U0=self.U[:, :self.rank].clone(), **kw)

    # ---- K18: ratings that are taken back after the fit ----
    def _listed_pairs(self, users, items, who: str):
        """The distinct (user, item) pairs of a batch: (u int32, i int32, ur, ir int64 dense
        rows, -1 = unknown)."""
        if self.user_block is None:
            raise ValueError(f"{who} needs the ratings the model was fitted on; this core "
                             "was built from saved factors (from_factors / load) and has none")
        u = _to_device(users, torch.int32, self.device)
        i = _to_device(items, torch.int32, self.device)
        if u.numel() != i.numel():
            raise ValueError("users and items must have the same length")
        if u.numel():
            key = torch.unique((u.long() << 32) | (i.long() & 0xFFFFFFFF))
            low = key & 0xFFFFFFFF
            u = (key >> 32).to(torch.int32)
            i = torch.where(low >= (1 << 31), low - (1 << 32), low).to(torch.int32)
        return u, i, self.uidx.rows_of(u), self.iidx.rows_of(i)

    def _mark_removed(self, ur, ir):
        """Both sides' K18 mark pass for the distinct stored-id pairs (ur, ir) (int64 dense
        rows).  Returns (user marks, item marks, stored copies dropped per pair in (ur, ir)
        order of the user side's sort)."""
        n_u, n_i = self.n_users, self.n_items
        ub, ib = self.user_block, self.item_block
        ku = torch.sort(ur * n_i + ir).values            # by user row, then item row
        ki = torch.sort(ir * n_u + ur).values            # by item row, then user row
        del_u = _delete_csr(ku // n_i, ku % n_i, n_u)
        del_i = _delete_csr(ki // n_u, ki % n_u, n_i)
        mu = remove_mark(ub.row_ptr, ub.col, *del_u, self.ws, count_hits=True)
        mi = remove_mark(ib.row_ptr, ib.col, *del_i, self.ws)
        return mu, mi, mu[3]

    def remove_ratings(self, users, items) -> dict:
        """Take ratings back from the core in place: every stored copy of every listed (user,
        item) pair goes (a pair listed twice is listed once).  After the call every
        rating-derived thing — both id maps, both CSR sides and their schedules, nnz — is what
        ALSCore(the training triples with those pairs filtered out, order kept) would hold,
        bit for bit:
          a. ids are mapped to dense rows; a pair with an unknown id is counted as missing
          b. K18's mark pass (als_csr_remove_mark) flags the stored entries of both sides
             that stay, against a small delete CSR per side with ascending columns, and
             gives the kept entries before every row; a listed pair that no stored entry
             matched is counted as missing as well
          c. a user or an item left without a rating leaves the model (an empty row would
             make Spark's lambda * n * I system singular): both id maps shrink
             (shrink_index: offset and id_space are derived again), the factor rows of the
             rows that stay move to their new places bit for bit
          d. K18's compact pass (als_csr_remove_compact) writes each side's kept entries in
             stored order, columns renumbered through the OTHER side's shrunk map; the row
             pointer is the kept count before every surviving row, and the side is scheduled
             again at its current chunk
          e. everything cached from the ratings (the train exclusion lists, the workspace's
             rating scale) is dropped.
        Rows that stay keep their factors until refresh() or refit(); the surviving rows whose
        rating lists changed join the rows refresh() re-solves, rows touched by earlier adds
        are renumbered, and those that left are dropped.  Needs one transient second copy of
        each side's col and val.  An empty batch is a no-op; a call that would remove every
        rating raises ValueError; nothing is changed when the call raises.
        Measured on the ML-25M shape (tools/remove_cost.py): 2.5 ms for
        12 pairs, 3.5 ms for 10^6, 2.9 ms for the busiest user and 3.7 ms for the most-rated
        item, against 7.9-8.4 ms for ALSCore(the filtered triples): 2.3 to 3.4 times cheaper.
        Returns {"removed" (stored ratings dropped), "missing" (distinct listed pairs that
        matched nothing), "left_users", "left_items" (ids, ascending), "touched_users",
        "touched_items" (int64 dense rows in the new numbering, ascending)}."""
        u, i, ur, ir = self._listed_pairs(users, items, "remove_ratings")
        empty = torch.empty(0, dtype=torch.int64, device=self.device)
        info = {"removed": 0, "missing": int(u.numel()), "left_users": empty.to(torch.int32),
                "left_items": empty.to(torch.int32), "touched_users": empty,
                "touched_items": empty}
        known = (ur >= 0) & (ir >= 0)
        if not bool(known.any()):
            return info
        mu, mi, hits = self._mark_removed(ur[known], ir[known])
        nnz = int(mu[1][-1])
        if nnz != int(mi[1][-1]):
            raise RuntimeError("remove_ratings: the two sides disagree on what stays")
        if nnz == self.nnz:
            return info
        if nnz == 0:
            raise ValueError("remove_ratings would remove every rating: a model needs one")
        ub, ib = self.user_block, self.item_block
        side = []
        for block, idx, marks in ((ub, self.uidx, mu), (ib, self.iidx, mi)):
            kept = marks[2][1:] - marks[2][:-1]
            had = block.row_ptr[1:] - block.row_ptr[:-1]
            left = (kept == 0).nonzero().flatten()
            shrunk, mp = shrink_index(idx, left, self.ws)
            changed = ((kept > 0) & (kept < had)).nonzero().flatten()
            side.append(dict(idx=shrunk, map=mp, left=idx.ids()[left], kept=kept,
                             touched=changed if mp is None else mp[changed].long()))
        su, si = side
        csr = []
        for block, marks, me, other, n_cols in ((ub, mu, su, si, ib.n_rows),
                                                (ib, mi, si, su, ub.n_rows)):
            col, val = remove_compact(block.col, block.val, marks[0], marks[1], other["map"],
                                      n_cols, nnz)
            stays = torch.ones(block.n_rows + 1, dtype=torch.bool, device=self.device)
            stays[:-1] = me["kept"] > 0               # the last word is nnz
            csr.append((marks[2][stays].contiguous(), col, val))
        U = V = None
        if self.rank > 0 and self.U is not None:
            U = self.U if su["map"] is None else self.U[su["kept"] > 0].contiguous()
            V = self.V if si["map"] is None else self.V[si["kept"] > 0].contiguous()
        # nothing above touched the core: from here on it cannot fail half-way
        self.user_block = schedule_block(su["idx"].n, nnz, *csr[0], self.ws, ub.chunk)
        self.item_block = schedule_block(si["idx"].n, nnz, *csr[1], self.ws, ib.chunk)
        removed, self.nnz = self.nnz - nnz, nnz
        self.uidx, self.iidx = su["idx"], si["idx"]
        if U is not None:
            self.U, self.V = U, V
        self._train_ex = {}
        self.ws.rating_scale_key = None   # the largest |rating| may have left
        touched = []
        for s, earlier in zip(side, self._touched or (empty, empty)):
            if s["map"] is not None:      # rows touched earlier, in the new numbering
                earlier = s["map"][earlier].long()
                earlier = earlier[earlier >= 0]
            touched.append(torch.unique(torch.cat([earlier, s["touched"]])))
        self._touched = tuple(touched)
        info.update(removed=removed,
                    missing=int(u.numel()) - int(known.sum()) + int((hits == 0).sum()),
                    left_users=su["left"], left_items=si["left"], touched_users=su["touched"],
                    touched_items=si["touched"])
        return info

    def _remove_rows(self, ids, user_side: bool, who: str) -> dict:
        if self.user_block is None:
            raise ValueError(f"{who} needs the ratings the model was fitted on; this core "
                             "was built from saved factors (from_factors / load) and has none")
        ids = torch.unique(_to_device(ids, torch.int32, self.device))
        idx, block, other = ((self.uidx, self.user_block, self.iidx) if user_side else
                             (self.iidx, self.item_block, self.uidx))
        rows = idx.rows_of(ids)
        unknown = int((rows < 0).sum())
        rows = rows[rows >= 0]
        row_ptr, col, _ = gather_rows(block.row_ptr, block.col, block.val, rows)
        mine = torch.repeat_interleave(idx.ids()[rows], row_ptr[1:] - row_ptr[:-1])
        theirs = other.ids()[col.long()]
        info = self.remove_ratings(*((mine, theirs) if user_side else (theirs, mine)))
        info["missing"] += unknown
        return info

    def remove_users(self, ids) -> dict:
        """Forget users: remove_ratings of every rating of the listed user ids (their rows
        expanded into pairs on the device).  An unknown id is counted in "missing"; the
        users, and every item only they had rated, are in "left_users" / "left_items"."""
        return self._remove_rows(ids, True, "remove_users")

    def remove_items(self, ids) -> dict:
        """Withdraw items: remove_users for the other side."""
        return self._remove_rows(ids, False, "remove_items")

    def set_ratings(self, users, items, ratings, *, seed=0) -> dict:
        """Replace ratings: every stored copy of each listed pair goes, then the batch is
        added as add_ratings adds it; of a pair that is several times in the batch the LAST
        rating wins (the earlier ones are dropped, the order of the rest is kept).  The result
        is what ALSCore(the old triples without the listed pairs, then the de-duplicated
        batch) would hold, bit for bit.  A pair that is not stored, or whose ids are new, is
        simply added.  No row leaves on the way: every row that loses a rating gets one
        back, so a user whose only rating is replaced keeps the factor row and its bits (K18
        leaves such a row empty between the two steps, K17 takes empty rows).  The removed
        state and the added state are computed first and stored at the end: nothing is
        changed when the call raises.  Returns add_ratings' report for the de-duplicated
        batch plus "replaced", the stored ratings that went."""
        if self.user_block is None:
            raise ValueError("set_ratings needs the ratings the model was fitted on; this core "
                             "was built from saved factors (from_factors / load) and has none")
        u = _to_device(users, torch.int32, self.device)
        i = _to_device(items, torch.int32, self.device)
        r = _to_device(ratings, torch.float32, self.device)
        if not (u.numel() == i.numel() == r.numel()):
            raise ValueError("users, items and ratings must have the same length")
        if u.numel() == 0:
            return dict(self.add_ratings(u, i, r), replaced=0)
        key = (u.long() << 32) | (i.long() & 0xFFFFFFFF)
        uniq, inv = torch.unique(key, return_inverse=True)
        last = torch.full((uniq.numel(),), -1, dtype=torch.int64, device=self.device)
        last.scatter_reduce_(0, inv, torch.arange(key.numel(), device=self.device), "amax")
        pick = torch.sort(last).values                   # last occurrences, in batch order
        u, i, r = u[pick].contiguous(), i[pick].contiguous(), r[pick].contiguous()
        ur, ir = self.uidx.rows_of(u), self.iidx.rows_of(i)
        known = (ur >= 0) & (ir >= 0)
        ucsr = icsr = None
        nnz = self.nnz
        if bool(known.any()):
            mu, mi, _ = self._mark_removed(ur[known], ir[known])
            nnz = int(mu[1][-1])
            if nnz != int(mi[1][-1]):
                raise RuntimeError("set_ratings: the two sides disagree on what stays")
            if nnz != self.nnz:   # rows stay where they are, empty or not: no map, no shrink
                ub, ib = self.user_block, self.item_block
                ucsr = (mu[2],) + remove_compact(ub.col, ub.val, mu[0], mu[1], None, ib.n_rows, nnz)
                icsr = (mi[2],) + remove_compact(ib.col, ib.val, mi[0], mi[1], None, ub.n_rows, nnz)
        replaced = self.nnz - nnz
        info = self._add_commit(self._add_compute(u, i, r, seed, ucsr, icsr, nnz))
        info["replaced"] = replaced
        return info

    def fingerprint(self) -> dict:
        """Order-independent identity of the training ratings (checkpoint matching)."""
        v = self.user_block.val
        return {"nnz": int(self.nnz), "n_users": int(self.n_users), "n_items": int(self.n_items),
                "rating_bits": int(v.view(torch.int32).long().sum()),
                "item_id_sum": int(self.iidx.ids().long().sum())}

    def user_factor_ids(self) -> torch.Tensor:
        return self.uidx.ids()

    # ---- K4 / K5 (the serving protocol shared with distributed.ShardedALS) ----
    def predict(self, users, items) -> torch.Tensor:
        """fp64 <u, v> per pair (MatrixFactorizationModel.predict's ddot); NaN where
        either id is unknown."""
        u = _to_device(users, torch.int32, self.device)
        i = _to_device(items, torch.int32, self.device)
        return predict_pairs(u, i, self.uidx, self.iidx, self.U, self.V, self.rank)

    def rmse(self, users, items, ratings):
        """(sqrt(sum (r - p)^2 / n), n) over the pairs whose ids are both known —
        computeError (RecommenderSystem.py:103-129) fused into one pass."""
        u = _to_device(users, torch.int32, self.device)
        i = _to_device(items, torch.int32, self.device)
        r = _to_device(ratings, torch.float32, self.device)
        sse, n = rmse_pairs(u, i, r, self.uidx, self.iidx, self.U, self.V, self.rank,
                            self.ws).tolist()
        return (math.sqrt(sse / n) if n > 0 else float("nan")), int(n)

    def _sides(self, user_side: bool):
        if user_side:
            return self.uidx, self.U, self.iidx, self.V
        return self.iidx, self.V, self.uidx, self.U

    def train_exclusion(self, user_side: bool = True):
        """The pairs this core was fitted on as an exclusion list for one side's queries:
        (row_ptr int64 [n + 1], col int32 [nnz]), row r's other-side dense rows ascending in
        col[row_ptr[r]:row_ptr[r + 1]] (duplicates kept).  Built once per side and cached.
        RatingBlock.col is in input order, so the list is made by K1 itself: the OPPOSITE
        block's CSR, expanded to COO, has the wanted index ascending already, and
        als_csr_build's sort by this side's row is stable (O(nnz) memory, no 64-bit
        sort of the ratings)."""
        got = self._train_ex.get(bool(user_side))
        if got is not None:
            return got
        if self.user_block is None:
            raise ValueError("exclude='train' needs the ratings the model was fitted on; this "
                             "core was built from saved factors (from_factors / load) and has "
                             "none: pass the pairs to exclude explicitly")
        L = _lib.lib()
        mine, opp = (self.user_block, self.item_block) if user_side else (self.item_block,
                                                                          self.user_block)
        dev = self.device
        i32 = dict(dtype=torch.int32, device=dev)
        deg = opp.row_ptr[1:] - opp.row_ptr[:-1]
        # COO of the opposite block: its row (= the other side's dense row) per entry,
        # ascending; its col = this side's dense row
        other = torch.repeat_interleave(torch.arange(opp.n_rows, **i32), deg)
        row_map = torch.arange(mine.n_rows, **i32)
        col_map = torch.arange(opp.n_rows, **i32)
        row_ptr = torch.empty(mine.n_rows + 1, dtype=torch.int64, device=dev)
        col = torch.empty(max(opp.nnz, 1), **i32)
        val = torch.empty(max(opp.nnz, 1), dtype=torch.float32, device=dev)  # (unused copy)
        w = self.ws.get(L.als_csr_workspace_bytes(opp.nnz, mine.n_rows))
        check(L.als_csr_build(ptr(opp.col), ptr(row_map), ptr(other), ptr(col_map), ptr(opp.val),
                              opp.nnz, mine.n_rows, ptr(row_ptr), ptr(col), ptr(val), ptr(w),
                              w.numel(), stream_ptr(dev)), "als_csr_build (exclusion list)")
        # K1 has no way to skip the values: the fp32 copy and the COO index go as soon as
        # the sort has run (peak: 3 x 4 B per rating beside the two rating blocks and
        # K1's workspace; kept: 4 B per rating per side)
        del val, other
        self._train_ex[bool(user_side)] = (row_ptr, col)
        return row_ptr, col

    def _filter_args(self, exclude, candidates, user_side: bool, rows=None):
        """(ex_begin, ex_end, ex_col, allow_bits) of a filtered top-k over the query rows
        `rows` (dense, int64; None = every row of the side).  exclude: None, "train", or
        (query ids, other ids) pairs (host or device; unknown ids dropped, as predict's
        inner join does); candidates: None or ids of the other side (unknown dropped)."""
        qi, _, oi, _ = self._sides(user_side)
        beg = end = col = bits = None
        if isinstance(exclude, str):
            if exclude != "train":
                raise ValueError(f"exclude must be None, 'train' or (ids, ids) pairs, got {exclude!r}")
            rp, col = self.train_exclusion(user_side)
            beg, end = rp[:-1], rp[1:]
        elif exclude is not None:
            a, b = exclude
            a = _to_device(a, torch.int32, self.device)
            b = _to_device(b, torch.int32, self.device)
            beg, end, col = _filters.exclusion_lists(qi.rows_of(a), oi.rows_of(b), qi.n)
        if beg is not None:
            if rows is not None:
                beg, end = beg[rows], end[rows]
            beg, end = beg.contiguous(), end.contiguous()
        if candidates is not None:
            c = _to_device(candidates, torch.int32, self.device)
            bits = _filters.pack_allow_bits(oi.rows_of(c), oi.n)
        return beg, end, col, bits

    def _topk(self, Q, n_q, user_side, top, exclude, candidates, rows=None):
        _, _, oi, Vo = self._sides(user_side)
        if exclude is None and candidates is None:
            return topk_rows(Q, n_q, Vo, oi.n, self.rank, top)
        return topk_rows_filtered(Q, n_q, Vo, oi.n, self.rank, top,
                                  *self._filter_args(exclude, candidates, user_side, rows))

    def recommend_all(self, top: int, user_side: bool = True, *, exclude=None, candidates=None):
        """recommendForAll: for every row of one side (dense order) its `top` best
        rows of the other side.  Returns (keys [n], ids [n, t], scores [n, t]) on the
        device, t = min(top, rows of the other side), scores descending.
        exclude: pairs a row must not list — "train" (the pairs the core was fitted on)
        or (query ids, other ids); candidates: ids of the other side the lists are
        restricted to.  Slots past a row's admissible rows have score -inf."""
        qi, Q, oi, Vo = self._sides(user_side)
        idx, sc = self._topk(Q, qi.n, user_side, top, exclude, candidates)
        t = min(int(top), oi.n)
        return qi.ids(), ids_of(oi.ids(), idx[:, :t]), sc[:, :t]

    def recommend_subset(self, ids, top: int, user_side: bool = True, *, exclude=None,
                         candidates=None):
        """recommendForUserSubset / ForItemSubset: distinct known ids of `ids`
        (ascending) -> (keys, ids [m, t], scores [m, t]).  exclude / candidates as
        recommend_all (the subset's rows point into the one exclusion list)."""
        qi, Q, oi, Vo = self._sides(user_side)
        q = _to_device(ids, torch.int32, self.device)
        keys = torch.unique(q)
        rows = qi.rows_of(keys)
        known = rows >= 0
        keys, rows = keys[known], rows[known]
        t = min(int(top), oi.n)
        if keys.numel() == 0:
            return keys, torch.empty((0, t), dtype=torch.int32, device=self.device), \
                torch.empty((0, t), dtype=torch.float32, device=self.device)
        Qs = Q.index_select(0, rows.long()).contiguous()
        idx, sc = self._topk(Qs, keys.numel(), user_side, top, exclude, candidates, rows.long())
        return keys, ids_of(oi.ids(), idx[:, :t]), sc[:, :t]

    # ---- K12: which rows are like this one? ----
    def _similar_args(self, top, user_side: bool, candidates):
        """(index, table, t, kernel top, allow mask) of a neighbour search on one side."""
        if self.U is None or self.V is None:
            raise ValueError("similar needs factors: fit() the core or build it from_factors")
        top = int(top)
        if not 1 <= top <= SIMILAR_MAX_TOP:
            raise ValueError(f"top must be in [1, {SIMILAR_MAX_TOP}], got {top}")
        qi, T, _, _ = self._sides(user_side)
        bits = None
        if candidates is not None:
            c = _to_device(candidates, torch.int32, self.device)
            bits = _filters.pack_allow_bits(qi.rows_of(c), qi.n)
        return qi, T, min(top, qi.n - 1), bits

    def similar(self, ids, top: int, user_side: bool = False, *, candidates=None):
        """Cosine nearest neighbours inside one side's factors: for the distinct known ids
        of `ids` (ascending; unknown ids dropped, as recommend_subset drops them) the `top`
        most similar OTHER rows of the same side — items by default, users with
        user_side=True.  Returns (keys [m], ids [m, t], scores [m, t]) on the device,
        t = min(top, n - 1), cosine descending, ties by ascending dense row.
        candidates: ids of the same side the neighbours (not the queries) are restricted
        to.  Never listed: the row itself (by index: a different row with the same factors
        is, at similarity 1), and a row whose factors are all zero or hold a NaN / Inf;
        such a row as a query gets an empty list.  Empty slots have score -inf.
        Fewer than SIMILAR_SWEEP_MIN_ROWS queries sweep the raw table (K12, als_similar);
        more take the unit copy + K5 route (similar_rows_unit).  Both keep this contract,
        scores within 1e-5 of each other; neighbours closer than that may swap places."""
        qi, T, t, bits = self._similar_args(top, user_side, candidates)
        q = _to_device(ids, torch.int32, self.device)
        keys = torch.unique(q)
        rows = qi.rows_of(keys)
        known = rows >= 0
        keys, rows = keys[known], rows[known]
        m = int(keys.numel())
        if m == 0 or t == 0:
            return keys, torch.empty((m, t), dtype=torch.int32, device=self.device), \
                torch.empty((m, t), dtype=torch.float32, device=self.device)
        if m >= SIMILAR_SWEEP_MIN_ROWS:
            idx, sc = similar_rows_unit(rows, T, qi.n, self.rank, t, bits)
        else:
            Q = T.index_select(0, rows).contiguous()
            idx, sc = similar_rows(Q, m, T, qi.n, self.rank, t, rows.to(torch.int32).contiguous(),
                                   bits)
        return keys, ids_of(qi.ids(), idx), sc

    def similar_all(self, top: int, user_side: bool = False, *, candidates=None):
        """similar for every row of the side, in dense order: (keys [n], ids [n, t], scores
        [n, t]).  One unit-norm copy of the table, then one K5 sweep with the copy on both
        sides (never n / 16 passes of K12)."""
        qi, T, t, bits = self._similar_args(top, user_side, candidates)
        if t == 0:
            return qi.ids(), torch.empty((qi.n, 0), dtype=torch.int32, device=self.device), \
                torch.empty((qi.n, 0), dtype=torch.float32, device=self.device)
        idx, sc = similar_rows_unit(None, T, qi.n, self.rank, t, bits)
        return qi.ids(), ids_of(qi.ids(), idx), sc

    # ---- K14: lists that cover more than one taste ----
    def recommend_diverse(self, top: int, user_side: bool = True, *, ids=None,
                          trade_off: float = 0.7, pool=None, exclude=None, candidates=None,
                          chunk_rows=None):
        """recommend_all / recommend_subset re-ranked for diversity: K5 (or filtered K5) lists
        `pool` candidates per row, then K14 (als_diversify) picks `top` of them greedily by
        maximal marginal relevance, trade_off * relevance - (1 - trade_off) * (largest cosine
        to what the list already holds); trade_off = 1 gives the plain lists.
        ids: None = every row of the side in dense order, else the distinct known ids
        ascending (as recommend_subset).  pool: None = min(256, max(4 top, 50)), at most
        DIVERSIFY_MAX_POOL, capped at the other side's row count.  exclude / candidates as
        recommend_all.  Returns (keys [n], ids [n, t], scores [n, t], ils f64 [n]) on the
        device, t = min(top, pool): the picks in pick order with their K5 scores (not
        descending), open slots score -inf, and each list's intra-list similarity (mean
        pairwise cosine, NaN under two picks).
        The query rows go through in chunks of chunk_rows (None: as many as keep the pool
        arrays within DIVERSIFY_POOL_BYTES); the result does not depend on the chunking."""
        if self.U is None or self.V is None:
            raise ValueError("recommend_diverse needs factors: fit() the core or build it "
                             "from_factors")
        top, lam = int(top), float(trade_off)
        if top < 1:
            raise ValueError(f"top must be >= 1, got {top}")
        if not 0.0 <= lam <= 1.0:
            raise ValueError(f"trade_off must be in [0, 1], got {trade_off}")
        if pool is None:
            pool = min(DIVERSIFY_MAX_POOL, max(4 * top, 50))
        pool = int(pool)
        if not 1 <= pool <= DIVERSIFY_MAX_POOL:
            raise ValueError(f"pool must be in [1, {DIVERSIFY_MAX_POOL}], got {pool}")
        if chunk_rows is not None and int(chunk_rows) < 1:
            raise ValueError(f"chunk_rows must be >= 1, got {chunk_rows}")
        qi, Q, oi, Vo = self._sides(user_side)
        pool = min(pool, oi.n)
        t = min(top, pool)
        dev = self.device
        if ids is None:
            keys, rows, n = qi.ids(), None, qi.n
        else:
            keys = torch.unique(_to_device(ids, torch.int32, dev))
            rows = qi.rows_of(keys)
            keys, rows = keys[rows >= 0], rows[rows >= 0]
            n = int(keys.numel())
        out_i = torch.empty((n, t), dtype=torch.int32, device=dev)
        out_s = torch.empty((n, t), dtype=torch.float32, device=dev)
        ils = torch.empty(n, dtype=torch.float64, device=dev)
        if n == 0 or t == 0:
            return keys, out_i, out_s, ils
        filtered = exclude is not None or candidates is not None
        beg, end, col, bits = self._filter_args(exclude, candidates, user_side, rows)
        step = int(chunk_rows) if chunk_rows is not None else max(1, DIVERSIFY_POOL_BYTES
                                                                 // (8 * pool))
        for r0 in range(0, n, step):
            r1 = min(n, r0 + step)
            Qc = Q[r0:r1] if rows is None else Q.index_select(0, rows[r0:r1]).contiguous()
            if filtered:
                pi, ps = topk_rows_filtered(
                    Qc, r1 - r0, Vo, oi.n, self.rank, pool,
                    None if beg is None else beg[r0:r1].contiguous(),
                    None if end is None else end[r0:r1].contiguous(), col, bits)
            else:
                pi, ps = topk_rows(Qc, r1 - r0, Vo, oi.n, self.rank, pool)
            out_i[r0:r1], out_s[r0:r1], ils[r0:r1] = diversify_rows(pi, ps, Vo, oi.n, self.rank,
                                                                    t, lam)
            del pi, ps
        return keys, ids_of(oi.ids(), out_i), out_s, ils

    def list_similarity(self, id_lists, user_side: bool = True):
        """Intra-list similarity of any lists: id_lists [n, m] (m <= DIVERSIFY_MAX_POOL) hold
        ids of the OTHER side — items for user_side=True, as recommend_all's ids — and the
        result is f64 [n] on the device, each list's mean pairwise cosine between the factor
        rows of its known ids (an unknown id is an open slot; NaN under two known ids)."""
        if self.U is None or self.V is None:
            raise ValueError("list_similarity needs factors: fit() the core or build it "
                             "from_factors")
        _, _, oi, Vo = self._sides(user_side)
        lists = _to_device(id_lists, torch.int32, self.device)
        if lists.dim() != 2:
            raise ValueError(f"id_lists must be [n, m], got shape {tuple(lists.shape)}")
        rows = oi.rows_of(lists).to(torch.int32)
        return list_similarity_rows(rows, Vo, oi.n, self.rank)

    # ---- K15: do all rows get the same few blockbusters? ----
    def popularity(self, user_side: bool = True):
        """How often each row of the OTHER side was rated (int32 [n], dense order): the
        row-pointer differences of its rating block, no pass over the ratings.  None on a
        core built from saved factors."""
        block = self.item_block if user_side else self.user_block
        if block is None:
            return None
        return (block.row_ptr[1:] - block.row_ptr[:-1]).to(torch.int32).contiguous()

    def list_metrics(self, id_lists=None, *, top=None, user_side: bool = True, exclude=None,
                     candidates=None, popularity=None, head_fraction: float = 0.2,
                     per_row: bool = False) -> dict:
        """The lists of ALL rows looked at together (K15): {"coverage", "gini", "entropy",
        "effectiveItems", "personalization", "topItemShare", "novelty", "averagePopularity",
        "longTailShare", "lists", "entries", "skipped"} as list_metrics_dict defines them.
        Exactly one of
          id_lists [n, m]  ids of the OTHER side (items for user_side=True), m <= 256, from
                           anywhere; an id the model does not know is an open slot, as in
                           list_similarity
          top              the lists are made here: recommend_all(top) with the same
                           exclude / candidates
        candidates also defines the catalogue the coverage group is measured over.
        Popularity is the other side's rating counts (popularity()), the listing side's row
        count standing for the number of raters; a core built from_factors has no ratings and
        takes popularity=(ids, counts) — without it the three popularity fields are NaN and
        the rest is returned all the same.  The long tail is every catalogue row outside the
        floor(head_fraction * catalogue rows) most-rated ones (ties by ascending dense row).
        per_row: also "per_row" (f64 [n, 3] on the device: novelty, mean popularity, long-tail
        share of each list, NaN where undefined) and, with top=, "keys" (the ids of the
        rows)."""
        if (id_lists is None) == (top is None):
            raise ValueError("list_metrics takes either id_lists or top=, not both and not "
                             "neither")
        head_fraction = float(head_fraction)
        if not 0.0 < head_fraction < 1.0:
            raise ValueError(f"head_fraction must be inside (0, 1), got {head_fraction}")
        if top is not None and not 1 <= int(top) <= LIST_MAX_AT:
            raise ValueError(f"top must be in [1, {LIST_MAX_AT}], got {top}")
        if id_lists is not None:
            shape = tuple(id_lists.shape) if hasattr(id_lists, "shape") else np.shape(id_lists)
            if len(shape) != 2 or not 1 <= int(shape[1]) <= LIST_MAX_AT:
                raise ValueError(f"id_lists must be [n, m] with 1 <= m <= {LIST_MAX_AT}, got "
                                 f"shape {shape}")
            if exclude is not None:
                raise ValueError("exclude= shapes the lists made with top=; lists given as "
                                 "id_lists are taken as they are")
        if self.U is None or self.V is None:
            raise ValueError("list_metrics needs factors: fit() the core or build it "
                             "from_factors")
        qi, Q, oi, _ = self._sides(user_side)
        keys = None
        if id_lists is not None:
            rows = oi.rows_of(_to_device(id_lists, torch.int32, self.device)).to(torch.int32)
        else:
            at = min(int(top), oi.n)
            idx, _ = self._topk(Q, qi.n, user_side, at, exclude, candidates)
            rows, keys = idx[:, :at], qi.ids()
        out = self._list_metrics_of_rows(rows, user_side, candidates=candidates,
                                        popularity=popularity, head_fraction=head_fraction,
                                        per_row=per_row)
        if per_row and keys is not None:
            out["keys"] = keys
        return out

    def _list_metrics_of_rows(self, rows: torch.Tensor, user_side: bool = True, *,
                             candidates=None, popularity=None, head_fraction: float = 0.2,
                             per_row: bool = False) -> dict:
        """list_metrics for lists that hold DENSE rows of the other side already (int32
        [n, m] on the device, -1 = open slot): the catalogue from `candidates`, popularity
        from the rating blocks or from popularity=(ids, counts), then the three K15 calls."""
        qi, _, oi, _ = self._sides(user_side)
        dev = self.device
        bits = cat_rows = None
        if candidates is not None:
            c = _to_device(candidates, torch.int32, dev)
            cat_rows = torch.unique(oi.rows_of(c))
            cat_rows = cat_rows[cat_rows >= 0]
            bits = _filters.pack_allow_bits(cat_rows, oi.n)
        pop = self.popularity(user_side)
        if popularity is not None:
            ids, cnt = popularity
            r = oi.rows_of(_to_device(ids, torch.int32, dev))
            cnt = _to_device(cnt, torch.int32, dev).reshape(-1)
            if r.numel() != cnt.numel():
                raise ValueError("popularity: ids and counts must have the same length")
            pop = torch.zeros(oi.n, dtype=torch.int32, device=dev)
            pop[r[r >= 0]] = cnt[r >= 0]
        out, pr = list_metrics_rows(rows, int(rows.shape[1]), oi.n, self.ws, allow_bits=bits,
                                    cat_rows=cat_rows, pop=pop, n_pop=qi.n,
                                    head_fraction=head_fraction, per_row=per_row)
        if per_row:
            out["per_row"] = pr
        return out

    # ---- K7: rows the model has never seen ----
    def _fold_in(self, ids, other_ids, ratings, reg, implicit, alpha, user_side,
                 nonnegative=False):
        """(keys, X [m, ld], n_used, row_ptr, col) of fold_in, X with its padding columns."""
        if self.U is None or self.V is None:
            raise ValueError("fold_in needs factors: fit() the core or build it from_factors")
        if reg < 0 or alpha < 0:
            raise ValueError(f"reg and alpha must be >= 0, got {reg}, {alpha}")
        _, _, oi, Y = self._sides(user_side)
        q = _to_device(ids, torch.int32, self.device)
        o = _to_device(other_ids, torch.int32, self.device)
        r = _to_device(ratings, torch.float32, self.device)
        keys, row_ptr, col, val = _filters.ragged_rows(q, oi.rows_of(o), r)
        if keys.numel() == 0:
            return (keys, torch.empty((0, ld_for(self.rank)), dtype=torch.float32,
                                      device=self.device),
                    torch.empty(0, dtype=torch.int32, device=self.device), row_ptr, col)
        yty = compute_yty(Y, oi.n, self.rank, self.ws_yty) if implicit else None
        if nonnegative:
            X, n_used, _ = nnls_rows(row_ptr, col, val, Y, oi.n, self.rank, reg, implicit, alpha,
                                     yty, self.ws)
            return keys, X, n_used, row_ptr, col
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        X, n_used = fold_in_rows(row_ptr, col, val, Y, oi.n, self.rank, reg, implicit, alpha, yty,
                                 status, self.ws)
        raise_status(int(status.item()), " of the rows folded in (distinct ids ascending)")
        return keys, X, n_used, row_ptr, col

    def fold_in(self, ids, other_ids, ratings, *, reg, implicit=False, alpha=1.0,
                user_side: bool = True, nonnegative: bool = False):
        """Factor rows for rows the model was not fitted on, without a refit: one row of one
        half-sweep each (K7, als_fold_in), x = (sum y y^T + reg n I)^-1 sum r y over the
        row's ratings against the fixed other side (the implicit form with YtY when
        `implicit`).  ids: the grouping key of each rating — new users (new items when
        user_side is False); they may or may not collide with ids the model knows, and the
        model's own U / V are never touched.  other_ids: the rated items (users); one the
        model does not know is skipped.  reg / implicit / alpha as in fit().
        Returns (keys [m] = the distinct ids ascending, X f32 [m, rank], n_used int32 [m] =
        ratings used per row) on the device; a row whose every rating was skipped is zero
        with n_used 0.  Works on a from_factors core.  Raises RuntimeError when a row's
        normal equations are not positive definite (reg = 0 with fewer ratings than rank).
        nonnegative: the row is the minimiser under x >= 0 instead (K13, Spark's NNLS solver:
        what a half-sweep of fit(nonnegative=True) computes for it); no row fails."""
        keys, X, n_used, _, _ = self._fold_in(ids, other_ids, ratings, float(reg), bool(implicit),
                                              float(alpha), bool(user_side), bool(nonnegative))
        return keys, X[:, :self.rank], n_used

    def recommend_new(self, ids, other_ids, ratings, top: int, *, reg, implicit=False, alpha=1.0,
                      user_side: bool = True, exclude_rated: bool = True, candidates=None,
                      nonnegative: bool = False):
        """fold_in, then the `top` best rows of the other side for each folded row (K5 with
        the folded rows as the query matrix): (keys [m], ids [m, t], scores [m, t]) as
        recommend_subset returns them, t = min(top, rows of the other side).
        exclude_rated: a new row never lists what it rated itself (the reference's R:229
        for a user who is not in the model); candidates: ids of the other side the lists
        are restricted to (R:245).  Rows without a single used rating are dropped.
        nonnegative: as fold_in."""
        keys, X, n_used, row_ptr, col = self._fold_in(ids, other_ids, ratings, float(reg),
                                                      bool(implicit), float(alpha),
                                                      bool(user_side), bool(nonnegative))
        _, _, oi, Vo = self._sides(user_side)
        t = min(int(top), oi.n)
        keep = n_used > 0
        keys, Q = keys[keep], X[keep].contiguous()
        m = int(keys.numel())
        if m == 0:
            return keys, torch.empty((0, t), dtype=torch.int32, device=self.device), \
                torch.empty((0, t), dtype=torch.float32, device=self.device)
        beg = end = ex = bits = None
        if exclude_rated:
            n_all = int(row_ptr.numel()) - 1
            new_row = torch.repeat_interleave(torch.arange(n_all, device=self.device),
                                              row_ptr[1:] - row_ptr[:-1])
            beg, end, ex = _filters.exclusion_lists(new_row, col, n_all)
            beg, end = beg[keep].contiguous(), end[keep].contiguous()
        if candidates is not None:
            c = _to_device(candidates, torch.int32, self.device)
            bits = _filters.pack_allow_bits(oi.rows_of(c), oi.n)
        if beg is None and bits is None:
            idx, sc = topk_rows(Q, m, Vo, oi.n, self.rank, top)
        else:
            idx, sc = topk_rows_filtered(Q, m, Vo, oi.n, self.rank, top, beg, end, ex, bits)
        return keys, ids_of(oi.ids(), idx[:, :t]), sc[:, :t]

    # ---- K11: why was this recommended? ----
    def _explain_rows_of(self, q, user_side: bool, ratings):
        """(pair row int64 or -1, row_ptr, col, val): the rating rows behind the query ids
        q — slices of the training block (ratings None) or the caller's ratings grouped by
        filters.ragged_rows."""
        qi, _, oi, _ = self._sides(user_side)
        if ratings is not None:
            ids, other, vals = ratings
            keys, row_ptr, col, val = _filters.ragged_rows(
                _to_device(ids, torch.int32, self.device),
                oi.rows_of(_to_device(other, torch.int32, self.device)),
                _to_device(vals, torch.float32, self.device))
            if keys.numel() == 0:
                return torch.full_like(q, -1, dtype=torch.int64), row_ptr, col, val
            at = torch.searchsorted(keys, q).clamp_(max=keys.numel() - 1)
            return torch.where(keys[at] == q, at, -1), row_ptr, col, val
        block = self.user_block if user_side else self.item_block
        if block is None:
            raise ValueError("explain needs each row's ratings; this core was built from saved "
                             "factors (from_factors / load) and holds none: pass ratings=(ids, "
                             "other ids, values)")
        dense = qi.rows_of(q)
        uniq, inv = torch.unique(dense[dense >= 0], return_inverse=True)
        pair_row = torch.full_like(dense, -1)
        pair_row[dense >= 0] = inv
        beg = block.row_ptr[uniq]
        lens = block.row_ptr[uniq + 1] - beg
        row_ptr = torch.zeros(uniq.numel() + 1, dtype=torch.int64, device=self.device)
        row_ptr[1:] = torch.cumsum(lens, 0)
        src = (torch.repeat_interleave(beg - row_ptr[:-1], lens)
               + torch.arange(int(row_ptr[-1]), device=self.device))
        return pair_row, row_ptr, block.col[src].contiguous(), block.val[src].contiguous()

    def explain(self, users, items, top_n: int = 10, *, reg, implicit=False, alpha=1.0,
                user_side: bool = True, ratings=None):
        """Why each (user, item) pair scores what it does: the score as a sum with one term
        per rating the user gave, score = sum_j wb_j y_i^T A_u^-1 y_j over the user's
        normal equations (K11, als_explain; reg / implicit / alpha as in fit(), and as in
        fold_in they decide A_u).  Pairs are grouped by user, so a user is factored once
        however many items are explained.
        ratings=None: each user's ratings are the ones the core was fitted on.
        ratings=(ids, other_ids, values): the rows to explain from, grouped by id as fold_in
        groups them — users the model has never seen, or a core restored from_factors.
        user_side=False explains item rows against the user factors: the row is the item,
        its ratings are users, and the contributions name users.
        Returns device tensors over the pairs kept, in input order (a pair whose user has no
        rating row — unknown to the model, or absent from `ratings` — is dropped):
        (users [m], items [m], score f32 [m], ids int32 [m, top_n], ratings f32 [m, top_n],
        contrib f32 [m, top_n], n_contrib int32 [m]).  Row p lists its n_contrib[p] largest
        contributions, descending (ties: earlier rating first): the id of the other side
        that was rated, the rating, and its share of the score; slots past n_contrib hold
        id -1, rating 0 and contribution 0.  score sums ALL the row's contributions, not
        only the listed ones; it is NaN for a target the model does not know.  After a
        fit, score equals predict() to rounding on the side solved last (users)."""
        top_n = int(top_n)
        if not 1 <= top_n <= EXPLAIN_MAX_TOP:
            raise ValueError(f"top_n must be in [1, {EXPLAIN_MAX_TOP}], got {top_n}")
        if self.U is None or self.V is None:
            raise ValueError("explain needs factors: fit() the core or build it from_factors")
        reg, alpha = float(reg), float(alpha)
        if reg < 0 or alpha < 0:
            raise ValueError(f"reg and alpha must be >= 0, got {reg}, {alpha}")
        _, _, oi, Y = self._sides(user_side)
        u = _to_device(users, torch.int32, self.device).reshape(-1)
        i = _to_device(items, torch.int32, self.device).reshape(-1)
        if u.numel() != i.numel():
            raise ValueError("users and items must have the same length")
        q, o = (u, i) if user_side else (i, u)
        pair_row, row_ptr, col, val = self._explain_rows_of(q, bool(user_side), ratings)
        keep = pair_row >= 0
        u, i, o, pair_row = u[keep], i[keep], o[keep], pair_row[keep]
        m = int(u.numel())
        f32 = dict(dtype=torch.float32, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        if m == 0:
            return (u, i, torch.empty(0, **f32), torch.empty((0, top_n), **i32),
                    torch.empty((0, top_n), **f32), torch.empty((0, top_n), **f32),
                    torch.empty(0, **i32))
        n_rows = int(row_ptr.numel()) - 1
        order, tgt_ptr = group_pairs(pair_row, n_rows)
        tgt = oi.rows_of(o)[order].to(torch.int32).contiguous()
        yty = compute_yty(Y, oi.n, self.rank, self.ws_yty) if implicit else None
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        score, pos, contrib, _ = explain_rows(row_ptr, col, val, Y, oi.n, self.rank, reg,
                                              bool(implicit), alpha, yty, tgt_ptr, tgt, top_n,
                                              status, self.ws)
        raise_status(int(status.item()), " of the rows explained (distinct ids ascending)")
        # entry offset inside the row -> the rated id and its rating
        filled = pos >= 0
        entry = (row_ptr[pair_row[order]].unsqueeze(1) + pos.clamp(min=0).long())
        entry = torch.where(filled, entry, 0)
        ids = torch.where(filled, ids_of(oi.ids(), col[entry].clamp(min=0)), -1).to(torch.int32)
        rat = torch.where(filled, val[entry], 0.0)
        score = torch.where(tgt >= 0, score, float("nan"))
        back = torch.empty_like(order)
        back[order] = torch.arange(m, device=self.device)  # slot of each input pair
        return (u, i, score[back], ids[back], rat[back], contrib[back],
                filled.sum(1).to(torch.int32)[back])

    def rank_metrics(self, users, items, at: int, *, ratings=None, threshold=None,
                     user_side: bool = True, exclude=None, candidates=None,
                     per_row: bool = False) -> dict:
        """Ranking quality of the top-`at` lists against held-out (user, item) pairs:
        Spark's RankingMetrics precisionAt / recallAt / meanAveragePrecisionAt / ndcgAt
        (binary relevance), lists and metrics both on the device (K5 then K6).
        Pairs with an unknown id are dropped (rmse's inner join); with `threshold` only
        pairs with rating >= threshold are relevant (`ratings` required).  The query
        rows are the users (items when user_side is False) with at least one relevant
        pair; their lists come from the recommend path with top = min(at, rows of the
        other side) and exclude / candidates passed through (exclude="train" scores
        unseen items only).  Returns {"precision", "recall", "map", "ndcg", "hitRate"
        (rows with at least one hit), "rows"}: means over `rows`, NaN when rows == 0.
        per_row: also "keys" (ids of the query rows, ascending) and "per_row"
        (f64 [rows, 4]: precision, recall, AP, NDCG), both on the device."""
        qi, Q, oi, _ = self._sides(user_side)
        at = int(at)
        if at < 1 or at > MAX_RANK_AT:
            raise ValueError(f"at must be in [1, {MAX_RANK_AT}], got {at}")
        u = _to_device(users, torch.int32, self.device)
        i = _to_device(items, torch.int32, self.device)
        if u.numel() != i.numel():
            raise ValueError("users and items must have the same length")
        q, o = (qi.rows_of(u), oi.rows_of(i)) if user_side else (qi.rows_of(i), oi.rows_of(u))
        keep = (q >= 0) & (o >= 0)
        if threshold is not None:
            if ratings is None:
                raise ValueError("threshold needs the held-out ratings")
            r = _to_device(ratings, torch.float32, self.device)
            if r.numel() != u.numel():
                raise ValueError("users, items and ratings must have the same length")
            keep &= r >= float(threshold)
        rows, inv = torch.unique(q[keep], return_inverse=True)  # ascending dense rows
        n = int(rows.numel())
        if n == 0:
            out = rank_metrics_dict([0.0] * 6, 0)
            if per_row:
                out["keys"] = qi.ids()[:0]
                out["per_row"] = torch.empty((0, 4), dtype=torch.float64, device=self.device)
            return out
        beg, end, col = _filters.relevance_lists(inv, o[keep], n)
        t = min(at, oi.n)
        Qs = Q.index_select(0, rows).contiguous()
        idx, _ = self._topk(Qs, n, user_side, t, exclude, candidates, rows)
        sums, pr = rank_metrics_rows(idx, t, beg, end, col, self.ws, per_row)
        sums = sums.tolist()
        out = rank_metrics_dict(sums, int(sums[4]))
        if per_row:
            out["keys"] = qi.ids()[rows]
            out["per_row"] = pr
        return out

    def full_rank_metrics(self, users, items, *, ratings=None, threshold=None,
                          weighted: bool = False, user_side: bool = True, exclude=None,
                          candidates=None, per_row: bool = False,
                          positions: bool = False) -> dict:
        """Where the held-out (user, item) pairs sit in each user's ordering of ALL
        admissible items (K9: one sweep of the whole score matrix, nothing cut at k): the
        measure an implicit-feedback fit is judged by.  Pairs with an unknown id are left
        out and counted in "dropped" (rmse's inner join); with `threshold` only pairs with
        rating >= threshold are relevant; duplicates count once.  exclude / candidates as
        rank_metrics: an item they rule out for a user is not part of that user's ordering
        (exclude="train" ranks each held-out item among the unseen items only), and a
        held-out pair they rule out itself is left out and counted in "inadmissible".
        weighted: each pair weighs its rating in expectedPercentileRank (Hu, Koren &
        Volinsky's sum r * rank / sum r; a duplicate pair keeps its first rating).
        Returns full_rank_dict's keys — expectedPercentileRank, meanPercentileRank, auc, mrr,
        rows, pairs, inadmissible — and "dropped".  Ties are counted at mid-rank.
        per_row: also "keys" (ids of the query rows, ascending) and "per_row" (f64 [rows, 3]:
        mean percentile rank, AUC, reciprocal rank; NaN where undefined), on the device.
        positions: also "row" / "col" (query-row index into "keys" order and dense row of
        the other side, per relevant pair), "above", "tied" (int32 per pair, -1 for an
        inadmissible one) and "n_adm" (int32 per query row), on the device."""
        if self.U is None or self.V is None:
            raise ValueError("full_rank_metrics needs factors: fit() the core or build it "
                             "from_factors")
        qi, Q, oi, Vo = self._sides(user_side)
        u = _to_device(users, torch.int32, self.device)
        i = _to_device(items, torch.int32, self.device)
        if u.numel() != i.numel():
            raise ValueError("users and items must have the same length")
        r = None
        if threshold is not None or weighted:
            if ratings is None:
                raise ValueError("threshold / weighted need the held-out ratings")
            r = _to_device(ratings, torch.float32, self.device)
            if r.numel() != u.numel():
                raise ValueError("users, items and ratings must have the same length")
        q, o = (qi.rows_of(u), oi.rows_of(i)) if user_side else (qi.rows_of(i), oi.rows_of(u))
        keep = (q >= 0) & (o >= 0)
        dropped = int(u.numel()) - int(keep.sum().item())
        if threshold is not None:
            keep &= r >= float(threshold)
        rows, inv = torch.unique(q[keep], return_inverse=True)  # ascending dense rows
        n = int(rows.numel())
        i32 = dict(dtype=torch.int32, device=self.device)
        if n == 0:
            out = full_rank_dict([0.0] * len(FULL_RANK_SUMS))
            out["dropped"] = dropped
            if per_row:
                out["keys"] = qi.ids()[:0]
                out["per_row"] = torch.empty((0, 3), dtype=torch.float64, device=self.device)
            if positions:
                out.update(row=torch.empty(0, **i32), col=torch.empty(0, **i32),
                           above=torch.empty(0, **i32), tied=torch.empty(0, **i32),
                           n_adm=torch.empty(0, **i32))
                out.setdefault("keys", qi.ids()[:0])
            return out
        wts = None
        if weighted:
            beg, end, col, wts = _filters.relevance_lists_weighted(inv, o[keep], r[keep], n)
        else:
            beg, end, col = _filters.relevance_lists(inv, o[keep], n)
        Qs = Q.index_select(0, rows).contiguous()
        above, tied, n_adm = rank_positions_rows(
            Qs, n, Vo, oi.n, self.rank, beg, end, col,
            *self._filter_args(exclude, candidates, user_side, rows))
        sums, pr = full_rank_sums_rows(above, tied, n_adm, beg, end, self.ws, wts, per_row)
        out = full_rank_dict(sums.tolist())
        out["dropped"] = dropped
        if per_row or positions:
            out["keys"] = qi.ids()[rows]
        if per_row:
            out["per_row"] = pr
        if positions:
            out["row"] = torch.repeat_interleave(torch.arange(n, **i32), end - beg)
            out["col"] = col[:above.numel()]
            out.update(above=above, tied=tied, n_adm=n_adm)
        return out

    def regression_metrics(self, users, items, ratings, through_origin: bool = False) -> dict:
        """Spark's RegressionMetrics of the model's predictions against held-out ratings, in
        one fused pass (K8, als_regression_moments): no prediction column is materialised.
        Pairs with an unknown id are left out and counted (rmse's inner join).  Returns
        regression_dict's keys: mse, rmse, mae, r2, var, n, dropped, meanLabel, varLabel."""
        if self.U is None or self.V is None:
            raise ValueError("regression_metrics needs factors: fit() the core or build it "
                             "from_factors")
        u = _to_device(users, torch.int32, self.device)
        i = _to_device(items, torch.int32, self.device)
        r = _to_device(ratings, torch.float32, self.device)
        if not (u.numel() == i.numel() == r.numel()):
            raise ValueError("users, items and ratings must have the same length")
        m = regression_moments_pairs(u, i, r, self.uidx, self.iidx, self.U, self.V, self.rank,
                                     self.ws)
        return regression_dict(m.tolist(), through_origin)

    # ---- K16: rating statistics and bias baselines ----
    def _stats_block(self, user_side: bool, what: str) -> RatingBlock:
        block = self.user_block if user_side else self.item_block
        if block is None:
            raise ValueError(f"{what} needs the training ratings: a core built from_factors "
                             "holds none")
        return block

    def rating_stats(self, user_side: bool = False) -> dict:
        """Per-row statistics of the training ratings (K16; getCountsAndAverages plus spread
        and range), items by default: {"ids", "count", "mean", "std", "std_sample", "min",
        "max"} as rating_stats_dict defines them, device tensors in dense (ascending id)
        order."""
        block = self._stats_block(user_side, "rating_stats")
        mom, _ = row_moments(block, self.n_items if user_side else self.n_users, self.ws)
        out = {"ids": (self.uidx if user_side else self.iidx).ids()}
        out.update(rating_stats_dict(mom))
        return out

    def global_stats(self) -> dict:
        """{count, mean, std, min, max} of all training ratings (std: population), host
        numbers."""
        block = self._stats_block(False, "global_stats")
        _, total = row_moments(block, self.n_users, self.ws)
        n, s, m2, lo, hi = total.tolist()
        return {"count": int(n), "mean": s / n if n else float("nan"),
                "std": math.sqrt(m2 / n) if n else float("nan"), "min": lo, "max": hi}

    def top_rated(self, num: int, min_count: int = 0, user_side: bool = False,
                  damping: float = 0.0):
        """The `num` rows with more than `min_count` ratings (strictly) and the highest
        sum / (damping + count) — the plain mean at damping 0 — highest first, ties to the
        smaller id: (ids, means, counts), device tensors."""
        if int(num) < 0 or float(damping) < 0:
            raise ValueError("top_rated: num and damping must be >= 0")
        block = self._stats_block(user_side, "top_rated")
        mom, _ = row_moments(block, self.n_items if user_side else self.n_users, self.ws)
        n, s = mom[:, 0], mom[:, 1]
        keep = ((n > float(min_count)) & (n > 0)).nonzero().flatten()   # dense = ascending id
        score = s[keep] / (float(damping) + n[keep])
        order = torch.sort(score, descending=True, stable=True).indices[:int(num)]
        rows = keep[order]
        return ((self.uidx if user_side else self.iidx).ids()[rows], score[order],
                n[rows].to(torch.int64))

    def fit_baseline(self, method: str = "bias", reg_user: float = 10.0, reg_item: float = 25.0,
                     sweeps: int = 10) -> Baseline:
        """The mean / damped-bias predictor of the training ratings (K16):
          "global"  mu, the training mean (RecommenderSystem.py:172-177)
          "item"    mu + b_i, b_i = sum_i (r - mu) / (reg_item + n_i)
          "user"    mu + b_u, b_u = sum_u (r - mu) / (reg_user + n_u)
          "bias"    mu + b_u + b_i: `sweeps` times (b_i given b_u, then b_u given b_i) from zero
        Each update minimises SSE + reg_user sum b_u^2 + reg_item sum b_i^2 over its table
        exactly, so Baseline.history (that objective after every sweep; one entry for the
        other methods) never rises.  It comes from the sweep's own moments — a row updated to b
        keeps M2_row + n_row (mean_row - b)^2 of squared error — with no further pass over
        the ratings."""
        if method not in BASELINE_METHODS:
            raise ValueError(f"method must be one of {BASELINE_METHODS}, got {method!r}")
        if float(reg_user) < 0 or float(reg_item) < 0 or int(sweeps) < 1:
            raise ValueError("fit_baseline: reg_user, reg_item must be >= 0 and sweeps >= 1")
        ib = self._stats_block(False, "fit_baseline")
        ub = self._stats_block(True, "fit_baseline")
        f64 = dict(dtype=torch.float64, device=self.device)
        bu, bi = torch.zeros(self.n_users, **f64), torch.zeros(self.n_items, **f64)
        _, total = row_moments(ib, self.n_users, self.ws)
        n, s, m2 = total.tolist()[:3]
        mu = s / n

        def update(block, n_cols, other, damping, out):
            mom, _ = row_moments(block, n_cols, self.ws, other=other, offset=mu)
            bias_update(mom, damping, out=out)
            cnt, mean = mom[:, 0], torch.where(mom[:, 0] > 0, mom[:, 1] / mom[:, 0], 0.0)
            return (mom[:, 2] + cnt * (mean - out) ** 2).sum()

        history = []
        if method == "global":
            history.append(m2)
        elif method == "item":
            sse = update(ib, self.n_users, None, reg_item, bi)
            history.append(float(sse + reg_item * (bi * bi).sum()))
        elif method == "user":
            sse = update(ub, self.n_items, None, reg_user, bu)
            history.append(float(sse + reg_user * (bu * bu).sum()))
        else:
            for _ in range(int(sweeps)):
                update(ib, self.n_users, bu, reg_item, bi)
                sse = update(ub, self.n_items, bi, reg_user, bu)
                history.append(float(sse + reg_user * (bu * bu).sum()
                                     + reg_item * (bi * bi).sum()))
        return Baseline(method, mu, bu, bi, self.uidx, self.iidx, history, self.ws,
                        reg_user, reg_item)

    def recommend_users(self, top: int):
        """For every user (dense order): top items as (item ids, scores)."""
        _, ids, sc = self.recommend_all(top, True)
        return ids, sc

    def recommend_items(self, top: int):
        _, ids, sc = self.recommend_all(top, False)
        return ids, sc

    def user_factors(self, cache: bool = True):
        return self.uidx.ids(), self.U[:, :self.rank]

    def item_factors(self, cache: bool = True):
        return self.iidx.ids(), self.V[:, :self.rank]
