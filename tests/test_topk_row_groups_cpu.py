"""CPU side of tests/test_gpu_topk_row_groups.py: what that file's bars rest on, without a
GPU.

* The GPU file lets the 1e-5 tie rule excuse at most 0.5 % of a case's sampled positions.
  Here each case's V and a 1,500-row Q of the same distribution show how many positions
  random data of these shapes puts inside the tie window at all: at most 0.15 % have the
  next fp64 score within 1e-5 max(1, |s|), so at most twice that (the neighbour above or
  below) can be excused by ties, and a kernel that scrambles near-equal scores wholesale
  fails the cap.
* The sampled rows hold the launch seam, the tail and every all-zero row.
* topk_split_rg's threshold (two row groups from 262,144 query rows), read through
  als_topk_workspace_bytes: the key-log slab doubles there.
* The vectorised sample check agrees with the row-by-row one and rejects what it must.
"""
import numpy as np
import pytest

from als_mi355x import _lib
from helpers import (K5RG_BIG_ROWS, K5RG_COPIES, K5RG_FILTERED, K5RG_MIN_ROWS, K5RG_NQ, K5RG_NV,
                     K5RG_RANKS, K5RG_SLICE_ROWS, K5RG_SPLIT, K5RG_TIE, K5RG_TOPS,
                     K5RG_WINDOW_CAP, K5RG_ZERO_ROWS, k5rg_items, k5rg_sample_rows, k5rg_scores,
                     k5rg_window_share, topk_ranking_check, topk_ref_ranking, topk_sample_check)

_SCORES = {}


def _scores(rank):
    """fp64 scores of 1,500 N(0, 1) query rows against the case's V, once per rank."""
    if rank not in _SCORES:
        Vm, copies = k5rg_items(rank)
        Q = np.random.default_rng(6000 + rank).standard_normal((1500, rank)).astype(np.float32)
        planted = np.zeros(K5RG_NV, bool)
        planted[copies] = True
        planted[K5RG_TIE[1]] = True
        _SCORES[rank] = (k5rg_scores(Q, Vm, copies), planted)
    return _SCORES[rank]


@pytest.mark.parametrize("rank", K5RG_RANKS)
def test_items_hold_the_planted_rows(rank):
    Vm, copies = k5rg_items(rank)
    assert Vm.shape == (K5RG_NV, rank) and Vm.dtype == np.float32
    assert len(copies) == K5RG_COPIES == len(np.unique(copies)) and K5RG_COPIES > max(K5RG_TOPS)
    assert (Vm[copies] == Vm[copies[0]]).all()
    lo, hi = K5RG_TIE
    assert (Vm[lo] == Vm[hi]).all() and hi - lo > 2 * 384 and lo not in copies and hi not in copies
    # scattered: copies in the first and in the last (ragged) tile of every class
    assert copies[0] < 192 and copies[-1] >= 6 * 192
    # no other exact duplicate rows
    assert len(np.unique(Vm, axis=0)) == K5RG_NV - (K5RG_COPIES - 1) - 1
    assert k5rg_items(rank)[0] is Vm  # built once


@pytest.mark.parametrize("top", K5RG_TOPS)
@pytest.mark.parametrize("rank", K5RG_RANKS)
def test_tie_window_share_is_far_below_the_cap(rank, top):
    S, planted = _scores(rank)
    share = k5rg_window_share(S, top, planted)
    assert share <= K5RG_WINDOW_CAP, share


def test_sample_rows():
    rows = k5rg_sample_rows()
    assert np.array_equal(rows, np.unique(rows)) and rows[0] == 0 and rows[-1] == K5RG_NQ - 1
    have = set(rows.tolist())
    assert set(range(512)) <= have                                    # blocks 0 and 1, both groups
    assert set(range(K5RG_SLICE_ROWS - 256, K5RG_SLICE_ROWS + 257)) <= have  # the launch seam
    assert set(range(K5RG_NQ - 400, K5RG_NQ)) <= have                 # the ragged last block
    assert 1500 < len(rows) <= 512 + 513 + 400 + 300
    assert set(K5RG_ZERO_ROWS) <= have and set(K5RG_BIG_ROWS) <= have
    # all-zero rows in group 0 and in group 1 of a 256-row block, and the very last row
    groups = {(r % 256) // 128 for r in K5RG_ZERO_ROWS}
    assert groups == {0, 1} and K5RG_NQ - 1 in K5RG_ZERO_ROWS
    # the last block: group 0 full, two rows of group 1
    assert K5RG_NQ % 256 == 130 and (K5RG_NQ + 255) // 256 == 1025
    # both one-group calls stay below the two-group threshold and hold a planted maximum
    assert K5RG_SPLIT < K5RG_MIN_ROWS and K5RG_NQ - K5RG_SPLIT < K5RG_MIN_ROWS
    assert K5RG_BIG_ROWS[0] < K5RG_SPLIT <= K5RG_BIG_ROWS[1]
    assert set(K5RG_FILTERED) <= {(k, t) for k in K5RG_RANKS for t in K5RG_TOPS}


@pytest.mark.parametrize("rank,keys", [(24, 448), (40, 384), (100, 384)])
def test_two_row_groups_start_at_262144_rows(rank, keys):
    """Key logs at top 20 (tk_log_cap keys of 8 bytes — 32 + one tile of 384 rows in 64-key
    steps at NK = 1, the 384 minimum at NK = 2, 4 — per query row of one launch's 512
    blocks): 128-row blocks below the threshold, 256-row blocks from it on; nothing else
    in the workspace depends on n_q."""
    ws = _lib.lib().als_topk_workspace_bytes
    slab = 512 * 128 * keys * 8
    below, at = ws(K5RG_MIN_ROWS - 1, K5RG_NV, rank, 20), ws(K5RG_MIN_ROWS, K5RG_NV, rank, 20)
    assert at - below == slab
    assert ws(K5RG_NQ, K5RG_NV, rank, 20) == at and ws(512 * 128, K5RG_NV, rank, 20) == below
    assert below - ws(K5RG_MIN_ROWS - 1, K5RG_NV, rank, 10) == slab  # (register lists: no logs)


def test_sample_check_agrees_with_the_row_check_and_rejects():
    rank, top = 24, 17
    S, planted = _scores(rank)
    S = S[:200]
    adm = np.ones(S.shape, bool)
    ref_i, ref_s = topk_ref_ranking(S, adm, top)
    idx, sc = ref_i.astype(np.int32), ref_s.astype(np.float32)
    res = topk_sample_check(idx, sc, S, top, skip=planted)
    assert res["excused"] == 0 and res["positions"] == 200 * top and res["max_score_err"] < 1e-6
    assert topk_ranking_check(idx, sc, S, adm, top) == 0
    # two neighbours swapped: far apart in score -> rejected by both; a duplicate likewise
    gap = ref_s[:, 0] - ref_s[:, 1]
    r = int(np.argmax(gap))
    bad = idx.copy()
    bad[r, [0, 1]] = bad[r, [1, 0]]
    for check in (lambda: topk_sample_check(bad, sc, S, top), lambda: topk_ranking_check(bad, sc, S, adm, top)):
        with pytest.raises(AssertionError):
            check()
    dup = idx.copy()
    dup[r, 1] = dup[r, 0]
    with pytest.raises(AssertionError):
        topk_sample_check(dup, sc, S, top)
    # a swap inside the tie window is excused and counted, by both alike
    S2 = S.copy()
    S2[r, ref_i[r, 1]] = S2[r, ref_i[r, 0]] * (1 - 2e-6)
    i2, s2 = topk_ref_ranking(S2, adm, top)
    sw = i2.astype(np.int32)
    sw[r, [0, 1]] = sw[r, [1, 0]]
    assert topk_sample_check(sw, s2.astype(np.float32), S2, top)["excused"] == 2
    assert topk_ranking_check(sw, s2.astype(np.float32), S2, adm, top) == 2
    # open slots (fewer admissible rows than top) must be -1 / -inf
    few = np.zeros(S.shape, bool)
    few[:, :5] = True
    i3, s3 = topk_ref_ranking(S, few, top)
    assert topk_sample_check(i3.astype(np.int32), s3.astype(np.float32), S, top, adm=few)["positions"] == 1000
    i3 = i3.astype(np.int32)
    i3[0, 5] = 7
    with pytest.raises(AssertionError):
        topk_sample_check(i3, s3.astype(np.float32), S, top, adm=few)
