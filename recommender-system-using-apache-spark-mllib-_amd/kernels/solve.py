"""K2, K2b, K3: the half-sweep solves (csrc/gram_solve.hip and its headers: als_yty,
als_solve_half), the phase bits of als_solve_half and the two-segment schedule of the
sharded engine's pipelined item half-sweep."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from .. import _lib
from .._lib import check, ptr, stream_ptr
from .workspace import Workspace, k_pad
from .schedule import DEFAULT_CHUNK, RatingBlock

MAX_RANK = 128       # k <= 64: gram_solve_kernel; 64 < k <= 128: W1 (one wavefront per system)
# als_solve_half phase bits (include/als_hip.h ALS_PHASE_*)
PHASE_LAUNCH1, PHASE_LAUNCH2, PHASE_PREP, PHASE_RSCALE, PHASE_DUAL, PHASE_RESCUE = 1, 2, 4, 8, 16, 32
PHASE_ALL = 63


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
