"""K5, K12, K14: top-k lists, cosine neighbours and diversified lists (csrc/topk.hip,
csrc/topk_filtered.hip: als_topk, als_topk_filtered; csrc/similar.hip: als_similar,
als_similar_unit_rows; csrc/diversify.hip: als_diversify, als_list_similarity)."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from .._lib import check, ptr, stream_ptr
from .solve import MAX_RANK


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
