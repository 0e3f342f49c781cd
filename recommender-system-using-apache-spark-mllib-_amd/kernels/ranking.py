"""K6, K9, K15: ranking metrics of lists (csrc/rank_metrics.hip: als_rank_metrics;
csrc/rank_positions.hip: als_rank_positions, als_full_rank_metrics;
csrc/list_metrics.hip: als_list_exposure, als_list_concentration, als_list_novelty)."""
from __future__ import annotations

import math

import torch

from .. import _lib
from .. import filters as _filters
from .._lib import check, ptr, stream_ptr
from .workspace import Workspace

LIST_MAX_AT = 256  # als_list_exposure / als_list_novelty: list positions read per row
LIST_METRIC_FIELDS = ("coverage", "gini", "entropy", "effectiveItems", "personalization",
                      "topItemShare", "novelty", "averagePopularity", "longTailShare", "lists",
                      "entries", "skipped")


def _ratio(a, b):
    """a / b, NaN where the denominator is not positive (a mean over nothing)."""
    return a / b if b > 0 else float("nan")


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
    n_lists, at = int(n_lists), int(at)
    pairs = n_lists * (n_lists - 1) // 2
    entropy = conc[4]
    out = {"coverage": _ratio(conc[1], conc[0]), "gini": conc[3], "entropy": entropy,
           "effectiveItems": 2.0 ** entropy if entropy == entropy else nan,
           "personalization": 1.0 - conc[5] / (pairs * at) if pairs > 0 else nan,
           "topItemShare": _ratio(conc[6], n_lists),
           "novelty": nan, "averagePopularity": nan, "longTailShare": nan,
           "lists": n_lists, "entries": int(conc[2]), "skipped": int(skipped)}
    if nov is not None:
        out["novelty"] = _ratio(nov[0], nov[1])
        out["averagePopularity"] = _ratio(nov[2], nov[3])
        if tail:
            out["longTailShare"] = _ratio(nov[4], nov[3])
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
    return {"expectedPercentileRank": _ratio(s[0], s[1]), "meanPercentileRank": _ratio(s[2], s[10]),
            "auc": _ratio(s[3], s[4]), "mrr": _ratio(s[5], s[6]), "rows": int(s[7]),
            "pairs": int(s[8]), "inadmissible": int(s[9])}
