"""Host-side inputs of the filtered top-k (als_topk_filtered, include/als_hip.h).

The reference's product lists, per user, the movies the user has NOT rated
(RecommenderSystem.py:229) among those with more than 75 ratings (R:245).  The
kernel takes the two conditions as
  * per-query-row exclusion ranges: ex_col[ex_begin[r] .. ex_end[r]) = dense rows of
    the other side, ascending within a row, duplicates kept (Spark keeps duplicate
    ratings), and
  * one global allow set as a bitmask over the other side's dense rows.
relevance_lists builds the same range form, de-duplicated, for the relevant sets of the
ranking metrics (als_rank_metrics), and ragged_rows groups the ratings of new rows by
their key for the fold-in (als_fold_in).
Everything here is torch on whatever device the inputs live on (the tests run it on
CPU tensors); nothing launches library code.
"""
from __future__ import annotations

import torch

__all__ = ["pack_allow_bits", "exclusion_lists", "relevance_lists", "ragged_rows",
           "relevance_lists_weighted", "reject_sharded_filters", "reject_sharded_fold_in",
           "reject_sharded_regression", "reject_sharded_full_rank", "reject_sharded_explain",
           "reject_sharded_similar", "reject_sharded_nonnegative", "reject_sharded_diversify",
           "reject_sharded_list_metrics"]


def pack_allow_bits(rows: torch.Tensor, n_v: int) -> torch.Tensor:
    """Dense rows (any integer dtype; entries outside [0, n_v), such as the -1 of an
    unknown id, are dropped; duplicates are fine) -> the allow mask: int32 words holding
    the uint32 bit patterns, bit (j & 31) of word (j >> 5) set for every row j given,
    ceil(n_v / 32) words (at least one, so the mask always has an address)."""
    n_words = max((int(n_v) + 31) // 32, 1)
    rows = rows.reshape(-1).long()
    rows = torch.unique(rows[(rows >= 0) & (rows < int(n_v))])
    words = torch.zeros(n_words, dtype=torch.int64, device=rows.device)
    # distinct bits of one word add up to their OR
    words.index_add_(0, rows >> 5, torch.ones_like(rows) << (rows & 31))
    # the uint32 pattern as int32 (two's complement wrap of bit 31)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def exclusion_lists(q_rows: torch.Tensor, o_rows: torch.Tensor, n_q: int):
    """(query dense row, other-side dense row) pairs -> (begin int64 [n_q], end int64
    [n_q], col int32 [m]): row r's excluded rows are col[begin[r]:end[r]], ascending,
    duplicates kept; pairs with either row negative (an unknown id) are dropped, rows
    without pairs get an empty range.  col has at least one element (a null ex_col with
    non-null ranges is an argument error of the C entry point).
    One sort of a 64-bit (row, col) key: for caller-supplied pair lists; the training
    ratings go through ALSCore's K1-based path instead."""
    q = q_rows.reshape(-1).long()
    o = o_rows.reshape(-1).long()
    if q.numel() != o.numel():
        raise ValueError("exclude: the two id arrays must have the same length")
    ok = (q >= 0) & (q < int(n_q)) & (o >= 0)
    q, o = q[ok], o[ok]
    key = torch.sort((q << 32) | o).values
    col = (key & 0xFFFFFFFF).to(torch.int32)
    ptr = torch.zeros(int(n_q) + 1, dtype=torch.int64, device=q.device)
    if key.numel():
        ptr[1:] = torch.cumsum(torch.bincount(key >> 32, minlength=int(n_q)), 0)
    if col.numel() == 0:
        col = torch.zeros(1, dtype=torch.int32, device=q.device)
    return ptr[:-1].contiguous(), ptr[1:].contiguous(), col.contiguous()


def relevance_lists(q_rows: torch.Tensor, o_rows: torch.Tensor, n_q: int):
    """exclusion_lists with the (row, col) pairs de-duplicated: the relevant sets of
    als_rank_metrics, whose ranges must be STRICTLY ascending (a relevant row counts
    once however often the held-out data names it).  Same inputs and output form."""
    q = q_rows.reshape(-1).long()
    o = o_rows.reshape(-1).long()
    if q.numel() != o.numel():
        raise ValueError("relevant pairs: the two id arrays must have the same length")
    ok = (q >= 0) & (q < int(n_q)) & (o >= 0)
    key = torch.unique((q[ok] << 32) | o[ok])  # sorted, distinct
    return exclusion_lists(key >> 32, key & 0xFFFFFFFF, n_q)


def relevance_lists_weighted(q_rows: torch.Tensor, o_rows: torch.Tensor, vals: torch.Tensor,
                             n_q: int):
    """relevance_lists with a value column carried through (the weights of
    als_full_rank_metrics): (begin, end, col, val f32 aligned with col).  A (row, col) pair
    named more than once keeps its FIRST value in input order (one stable sort)."""
    q = q_rows.reshape(-1).long()
    o = o_rows.reshape(-1).long()
    v = vals.reshape(-1)
    if not (q.numel() == o.numel() == v.numel()):
        raise ValueError("relevant pairs: ids and values must have the same length")
    ok = (q >= 0) & (q < int(n_q)) & (o >= 0)
    key, order = torch.sort((q[ok] << 32) | o[ok], stable=True)
    v = v[ok][order].to(torch.float32)
    first = torch.ones_like(key, dtype=torch.bool)
    first[1:] = key[1:] != key[:-1]
    key, v = key[first], v[first]
    beg, end, col = exclusion_lists(key >> 32, key & 0xFFFFFFFF, n_q)
    if v.numel() == 0:
        v = torch.zeros(1, dtype=torch.float32, device=q.device)
    return beg, end, col, v.contiguous()


def ragged_rows(q_keys: torch.Tensor, o_rows: torch.Tensor, vals: torch.Tensor):
    """Ratings of new rows, (grouping key, other-side dense row, rating) per entry ->
    (keys [m], row_ptr int64 [m + 1], col int32 [n], val f32 [n]): the distinct keys
    ascending, and row r's entries col/val[row_ptr[r]:row_ptr[r + 1]] in input order (one
    stable sort by key; duplicates kept, as Spark keeps duplicate ratings).  Nothing is
    dropped: a -1 in o_rows (an id the model does not know) stays for als_fold_in to
    skip.  Empty input gives m = 0 and row_ptr = [0].  Nothing is read back to the host
    here beyond what torch needs to size the key list."""
    q = q_keys.reshape(-1)
    o = o_rows.reshape(-1)
    v = vals.reshape(-1)
    if not (q.numel() == o.numel() == v.numel()):
        raise ValueError("fold-in: ids, other ids and ratings must have the same length")
    qs, order = torch.sort(q, stable=True)
    keys, counts = torch.unique_consecutive(qs, return_counts=True)
    row_ptr = torch.zeros(keys.numel() + 1, dtype=torch.int64, device=q.device)
    row_ptr[1:] = torch.cumsum(counts, 0)
    return (keys, row_ptr, o[order].to(torch.int32).contiguous(),
            v[order].to(torch.float32).contiguous())


def reject_sharded_fold_in() -> None:
    """The sharded engine carries fold_in / recommend_new with the single-GPU signature
    and refuses them, as it refuses the filters."""
    raise NotImplementedError(
        "fold_in / recommend_new are not supported by the sharded engine (ShardedALS) yet: "
        "fold new rows in on a single-GPU ALSCore (e.g. ALSCore.from_factors over the "
        "gathered factors)")


def reject_sharded_explain() -> None:
    """The sharded engine carries explain with the single-GPU signature and refuses it, as
    it refuses fold_in."""
    raise NotImplementedError(
        "explain is not supported by the sharded engine (ShardedALS) yet: explain scores on "
        "a single-GPU ALSCore (e.g. ALSCore.from_factors over the gathered factors, with "
        "ratings=)")


def reject_sharded_similar() -> None:
    """The sharded engine carries similar / similar_all with the single-GPU signature and
    refuses them, as it refuses explain."""
    raise NotImplementedError(
        "similar / similar_all are not supported by the sharded engine (ShardedALS) yet: "
        "search neighbours on a single-GPU ALSCore (e.g. ALSCore.from_factors over the "
        "gathered factors)")


def reject_sharded_nonnegative() -> None:
    """The sharded engine carries fit's nonnegative flag with the single-GPU signature and
    refuses it, as it refuses the filters and fold-in."""
    raise NotImplementedError(
        "nonnegative=True (the NNLS solver, K13) is not supported by the sharded engine "
        "(ShardedALS) yet: fit nonnegative factors on a single-GPU ALSCore")


def reject_sharded_diversify(sharded_engine: bool = False) -> None:
    """Raises when this process is one rank of a torch.distributed world of more than one
    process: what such a rank holds is the sharded engine, which carries recommend_diverse /
    list_similarity with the single-GPU signature and refuses them (sharded_engine=True: the
    call comes from that engine itself), as it refuses similar."""
    if not sharded_engine:
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            return
    raise NotImplementedError(
        "recommend_diverse / list_similarity are not supported by the sharded engine "
        "(ShardedALS) yet: diversify lists on a single-GPU ALSCore (e.g. ALSCore.from_factors "
        "over the gathered factors)")


def reject_sharded_list_metrics() -> None:
    """The sharded engine carries list_metrics with the single-GPU signature and refuses it,
    as it refuses list_similarity."""
    raise NotImplementedError(
        "list_metrics is not supported by the sharded engine (ShardedALS) yet: measure the "
        "lists on a single-GPU ALSCore (e.g. ALSCore.from_factors over the gathered factors, "
        "with popularity=)")


def reject_sharded_update() -> None:
    """The sharded engine carries add_ratings / refresh / refit with the single-GPU
    signature and refuses them."""
    raise NotImplementedError(
        "add_ratings / refresh / refit are not supported by the sharded engine (ShardedALS) "
        "yet: ratings are added in place on the single-GPU engine, an ALSCore")


def reject_sharded_split() -> None:
    """The sharded engine carries holdout / split with the single-GPU signature and refuses
    them, as it refuses remove_ratings."""
    raise NotImplementedError(
        "holdout / split are not supported by the sharded engine (ShardedALS) yet: the "
        "per-user holdout is made on the single-GPU engine, an ALSCore")


def reject_sharded_remove() -> None:
    """The sharded engine carries remove_ratings / remove_users / remove_items / set_ratings
    with the single-GPU signature and refuses them, as it refuses add_ratings."""
    raise NotImplementedError(
        "remove_ratings / remove_users / remove_items / set_ratings are not supported by the "
        "sharded engine (ShardedALS) yet: ratings are removed and replaced in place on the "
        "single-GPU engine, an ALSCore")


def reject_sharded_rating_stats() -> None:
    """The sharded engine carries rating_stats / global_stats / top_rated / fit_baseline with
    the single-GPU signature and refuses them, as it refuses list_metrics."""
    raise NotImplementedError(
        "rating_stats / global_stats / top_rated / fit_baseline are not supported by the "
        "sharded engine (ShardedALS) yet: rating statistics and bias baselines run on the "
        "single-GPU engine, an ALSCore built on the same ratings")


def reject_sharded_co_rated() -> None:
    """The sharded engine carries co_rated / co_rated_all with the single-GPU signature and
    refuses them, as it refuses rating_stats."""
    raise NotImplementedError(
        "co_rated / co_rated_all are not supported by the sharded engine (ShardedALS) yet: "
        "co-rated neighbours run on the single-GPU engine, an ALSCore built on the same "
        "ratings")


def reject_sharded_regression() -> None:
    """The sharded engine carries regression_metrics with the single-GPU signature and
    refuses it, as it refuses rank_metrics."""
    raise NotImplementedError(
        "regression_metrics is not supported by the sharded engine (ShardedALS) yet: use "
        "rmse() there, or evaluate on a single-GPU ALSCore (e.g. ALSCore.from_factors over "
        "the gathered factors)")


def reject_sharded_full_rank() -> None:
    """The sharded engine carries full_rank_metrics with the single-GPU signature and
    refuses it, as it refuses rank_metrics."""
    raise NotImplementedError(
        "full_rank_metrics is not supported by the sharded engine (ShardedALS) yet: evaluate "
        "full rankings on a single-GPU ALSCore (e.g. ALSCore.from_factors over the gathered "
        "factors)")


def reject_sharded_objective() -> None:
    """The sharded engine carries objective and fit's objective_every / tol with the
    single-GPU signature and refuses them, as it refuses rank_metrics."""
    raise NotImplementedError(
        "objective / objective_every= / tol= are not supported by the sharded engine "
        "(ShardedALS) yet: evaluate the training objective on a single-GPU ALSCore built on "
        "the same ratings")


def reject_sharded_filters(exclude, candidates) -> None:
    """The sharded engine's recommend_all / recommend_subset accept the two keywords and
    refuse them: filtered serving runs on the single-GPU engine only so far."""
    if exclude is not None or candidates is not None:
        raise NotImplementedError(
            "exclude= / candidates= are not supported by the sharded engine (ShardedALS) yet: "
            "serve filtered recommendations from a single-GPU ALSCore (e.g. "
            "ALSCore.from_factors over the gathered factors)")
