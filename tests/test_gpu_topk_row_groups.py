"""K5 (als_topk, als_topk_filtered) at two row groups per workgroup, and at the tile,
block and rank edges of one group.

1. Two row groups.  csrc/topk.hip's topk_split_rg gives register lists (top <= 16) and
   key logs (16 < top <= 128) two row groups (256 query rows per 8-wave workgroup) from
   262,144 query rows on.  262,144 + 130 rows (1,025 blocks, the last with two rows in
   group 1; three launches on the key-log path) against 1,159 V rows (several tiles and a
   ragged last one in every class), ranks 24 / 40 / 100 (NK = 1, 2, 4) x tops 8, 11, 16, 17,
   64, 99, 128 (one per TOPR class), and six filtered twins.  Per case:
   (a) a sample of rows (helpers.k5rg_sample_rows) against the fp64 ranking under the
       project's rule — indices identical except where fp64 scores tie within
       1e-5 max(1, |s|), scores at rtol = atol = 1e-5 — with the planted exact ties decided
       by index and all-zero rows listing 0 .. top - 1;
   (b) every row on the device: indices in [0, n_v) and distinct, scores non-increasing;
   (c) every row bit for bit against the one-group kernels: the same Q as two calls of
       fewer than 262,144 rows each (a listed pair carries its exact
       split-f16 score, whose arithmetic does not depend on the grouping; ties by index).
   The tie rule may excuse at most 0.5 % of a case's sampled positions (outside the planted
   copies); test_topk_row_groups_cpu.py shows that ties alone cannot reach that.
2. One row group: ranks 1, 31, 33, 63, 65, 127 x tops 10, 20, 200 (register list, key log,
   LDS list) over n_v = 1, 15, 16, 17, VT - 1, VT, VT + 1, 2 VT, 2 VT + 1 (VT = the class's
   tile rows) at 129 query rows, against the same fp64 ranking.

Figures go to $ALS_TEST_REPORT (helpers.report); profiles/k5_row_groups.json holds one run.
"""
import numpy as np
import pytest
import torch

from als_mi355x import engine as E
from als_mi355x import filters as F
from helpers import (K5RG_BIG, K5RG_BIG_ROWS, K5RG_EXCUSED_CAP, K5RG_FILTERED, K5RG_NQ, K5RG_NV,
                     K5RG_RANKS, K5RG_SPLIT, K5RG_TIE, K5RG_TOPS, K5RG_ZERO_ROWS, k5rg_items,
                     k5rg_sample_rows, k5rg_scores, report, topk_ranking_check, topk_sample_check)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(M, rank, extra=0):
    out = torch.zeros((M.shape[0], E.ld_for(rank) + extra), device=DEV)
    out[:, :rank] = torch.as_tensor(np.array(M)).to(DEV)  # (a copy: the shared cases are read-only)
    return out


def _same_bits(a_i, a_s, b_i, b_s):
    return torch.equal(a_i, b_i) and torch.equal(a_s.view(torch.int32), b_s.view(torch.int32))


# ------------------------------------------------------------------ 1. two row groups
_RG_CASES = {}


def _rg_case(rank):
    if rank not in _RG_CASES:
        g = torch.Generator(device=DEV)
        g.manual_seed(9000 + rank)
        Qd = torch.randn((K5RG_NQ, E.ld_for(rank)), device=DEV, generator=g).clamp_(-5.75, 5.75)
        Qd[:, rank:] = 0.0
        Qd[list(K5RG_BIG_ROWS), 0] = K5RG_BIG
        Qd[list(K5RG_ZERO_ROWS)] = 0.0
        Vm, copies = k5rg_items(rank)
        rows = k5rg_sample_rows()
        rows_d = torch.as_tensor(rows, device=DEV)
        Qs = Qd[rows_d, :rank].cpu().numpy()
        planted = np.zeros(K5RG_NV, bool)
        planted[copies] = True
        _RG_CASES[rank] = dict(rank=rank, Qd=Qd, Vd=_dev(Vm, rank), Vm=Vm, copies=copies,
                               planted=planted, rows=rows, rows_d=rows_d,
                               S=k5rg_scores(Qs, Vm, copies),
                               zero=np.nonzero(np.isin(rows, K5RG_ZERO_ROWS))[0])
    return _RG_CASES[rank]


@pytest.fixture(scope="module")
def rg_case():
    """Per rank, built once, shared and left unchanged: Q on the device (seeded N(0, 1),
    clamped below the planted 6.0 so that value is max |Q| of the call and of each half;
    the all-zero rows), V, the sampled rows and their fp64 scores."""
    yield _rg_case
    _RG_CASES.clear()


def _every_row(idx, sc, n_v):
    """(b): test_gpu_big's three assertions, on every row."""
    assert bool((idx >= 0).all()) and bool((idx < n_v).all())
    assert bool((sc[:, :-1] >= sc[:, 1:]).all())
    srt = torch.sort(idx, dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all())


def _planted_ties(c, idx):
    """The copies a row lists are the lowest-index ones, in index order and adjacent (one
    score); the tie pair has the lower index first.  Returns rows listing a copy / both of
    the pair."""
    copies, planted = c["copies"], c["planted"]
    with_copies = with_pair = 0
    for r in np.setdiff1d(np.arange(idx.shape[0]), c["zero"]):
        got = idx[r]
        pos = np.nonzero(planted[got])[0]
        np.testing.assert_array_equal(got[pos], copies[:len(pos)], err_msg=f"sample row {r}")
        if len(pos):
            assert pos[-1] - pos[0] == len(pos) - 1, (r, pos)
            with_copies += 1
        lst = got.tolist()
        if K5RG_TIE[0] in lst and K5RG_TIE[1] in lst:
            assert lst.index(K5RG_TIE[1]) == lst.index(K5RG_TIE[0]) + 1, (r, lst)
            with_pair += 1
    return with_copies, with_pair


@pytest.mark.parametrize("top", K5RG_TOPS)
@pytest.mark.parametrize("rank", K5RG_RANKS)
def test_two_row_groups(rg_case, rank, top):
    c = rg_case(rank)
    Qd, Vd, n_q, n_v = c["Qd"], c["Vd"], K5RG_NQ, K5RG_NV
    idx, sc = E.topk_rows(Qd, n_q, Vd, n_v, rank, top)
    # (a) the sample against fp64
    si, ss = idx[c["rows_d"]].cpu().numpy(), sc[c["rows_d"]].cpu().numpy()
    res = topk_sample_check(si, ss, c["S"], top, skip=c["planted"])
    with_copies, with_pair = _planted_ties(c, si)
    assert with_copies > 20 and with_pair > 0
    assert len(c["zero"]) == len(K5RG_ZERO_ROWS)
    for j in c["zero"]:
        assert si[j].tolist() == list(range(top)) and (ss[j] == 0).all(), c["rows"][j]
    # (b) every row
    _every_row(idx, sc, n_v)
    # (c) every row against the one-group kernels
    a_i, a_s = E.topk_rows(Qd[:K5RG_SPLIT], K5RG_SPLIT, Vd, n_v, rank, top)
    b_i, b_s = E.topk_rows(Qd[K5RG_SPLIT:], n_q - K5RG_SPLIT, Vd, n_v, rank, top)
    one_i, one_s = torch.cat([a_i, b_i]), torch.cat([a_s, b_s])
    same = _same_bits(idx, sc, one_i, one_s)
    res.update(excused_share=res["excused"] / res["positions"], bit_identical_to_one_group=same,
               rows_listing_copies=with_copies, rows_listing_the_tie_pair=with_pair)
    print(f"k5_row_groups[rank={rank},top={top}]: {res}")
    report(f"k5_row_groups[rank={rank},top={top}]", res)
    if not same:
        diff = ((idx != one_i) | (sc.view(torch.int32) != one_s.view(torch.int32))).any(1)
        assert False, f"rows differing from the one-group kernels: {torch.nonzero(diff)[:10, 0].tolist()}"
    assert res["excused"] <= K5RG_EXCUSED_CAP * res["positions"], res


@pytest.mark.parametrize("rank,top", K5RG_FILTERED)
def test_two_row_groups_filtered(rg_case, rank, top):
    c = rg_case(rank)
    Qd, Vd, n_q, n_v = c["Qd"], c["Vd"], K5RG_NQ, K5RG_NV
    u_i, u_s = E.topk_rows(Qd, n_q, Vd, n_v, rank, top)
    _every_row(u_i, u_s, n_v)
    # row r excludes its unfiltered top-3 and {r % n_v}; half the V rows allowed
    ex = torch.cat([u_i[:, :3].long(), (torch.arange(n_q, device=DEV) % n_v)[:, None]], 1)
    ex = torch.sort(ex, dim=1).values
    beg = torch.arange(n_q, device=DEV, dtype=torch.int64) * 4
    allow = np.random.default_rng(rank + top).random(n_v) < 0.5
    bits = F.pack_allow_bits(torch.as_tensor(np.nonzero(allow)[0]).to(DEV), n_v)
    idx, sc = E.topk_rows_filtered(Qd, n_q, Vd, n_v, rank, top, beg, beg + 4,
                                   ex.reshape(-1).to(torch.int32).contiguous(), bits)
    si, ss = idx[c["rows_d"]].cpu().numpy(), sc[c["rows_d"]].cpu().numpy()
    adm = np.repeat(allow[None, :], len(c["rows"]), 0)
    np.put_along_axis(adm, ex[c["rows_d"]].cpu().numpy(), False, 1)
    excused = topk_ranking_check(si, ss, c["S"], adm, top, skip=c["planted"])
    assert int(allow.sum()) - 4 >= top  # every list is full
    for r in np.setdiff1d(np.arange(len(si)), c["zero"]):  # the copies listed: the lowest-index
        got = si[r][c["planted"][si[r]]]                    # admissible ones, in index order
        np.testing.assert_array_equal(got, c["copies"][adm[r, c["copies"]]][:len(got)])
    for j in c["zero"]:  # an all-zero row: its first `top` admissible rows, score 0
        np.testing.assert_array_equal(si[j], np.nonzero(adm[j])[0][:top])
        assert (ss[j] == 0).all()
    # every row: valid, distinct, non-increasing; pairs listed by both calls: one score
    _every_row(idx, sc, n_v)
    step = 1 << 16
    for r0 in range(0, n_q, step):
        n = min(step, n_q - r0)
        dense = torch.full((n, n_v), -1, dtype=torch.int64, device=DEV)  # -1: not listed
        dense.scatter_(1, u_i[r0:r0 + n].long(), u_s[r0:r0 + n].view(torch.int32).long() & 0xFFFFFFFF)
        was = dense.gather(1, idx[r0:r0 + n].long())
        now = sc[r0:r0 + n].view(torch.int32).long() & 0xFFFFFFFF
        assert bool(((was < 0) | (was == now)).all()), r0
        assert bool((was >= 0).any())
    res = topk_sample_check(si, ss, c["S"], top, adm=adm, skip=c["planted"])  # (for the figures)
    assert res["excused"] == excused
    res["excused_share"] = excused / res["positions"]
    print(f"k5_row_groups[filtered,rank={rank},top={top}]: {res}")
    report(f"k5_row_groups[filtered,rank={rank},top={top}]", res)
    assert excused <= K5RG_EXCUSED_CAP * res["positions"], res


# ------------------------------------------------------------------ 2. edges at one group
# V rows per tile, (NK, list class): csrc/topk_sweep.h tk_vt — 384 / NK (192 at NK = 4) with
# register lists and key logs, 64 / NK with LDS lists.  A change there must change this.
TILE_ROWS = {(1, "reg"): 384, (2, "reg"): 192, (4, "reg"): 192,
             (1, "lds"): 64, (2, "lds"): 32, (4, "lds"): 16}
EDGE_NQ = 129   # one 128-row block + 1 (8 waves); two 64-row blocks + 1 (LDS lists)
EDGE_ZERO_ROW = 70


def _edge_case(rank, n_v):
    rng = np.random.default_rng(1000 * rank + n_v)
    Q = rng.standard_normal((EDGE_NQ, rank)).astype(np.float32)
    Q[EDGE_ZERO_ROW] = 0.0
    Vm = rng.standard_normal((n_v, rank)).astype(np.float32)
    S = Q.astype(np.float64) @ Vm.astype(np.float64).T
    if n_v >= 2:  # an exact tie, first row = last row
        Vm[n_v - 1] = Vm[0]
        S[:, n_v - 1] = S[:, 0]
    return Q, Vm, S


@pytest.mark.parametrize("top", [10, 20, 200])
@pytest.mark.parametrize("rank", [1, 31, 33, 63, 65, 127])
def test_tile_and_rank_edges(rank, top):
    nk = 1 if rank <= 32 else (2 if rank <= 64 else 4)
    vt = TILE_ROWS[(nk, "lds" if top > 128 else "reg")]
    out = {}
    for n_v in (1, 15, 16, 17, vt - 1, vt, vt + 1, 2 * vt, 2 * vt + 1):
        Q, Vm, S = _edge_case(rank, n_v)
        Qd, Vd = _dev(Q, rank), _dev(Vm, rank)
        idx_d, sc_d = E.topk_rows(Qd, EDGE_NQ, Vd, n_v, rank, top)
        idx, sc = idx_d.cpu().numpy(), sc_d.cpu().numpy()
        try:
            res = topk_sample_check(idx, sc, S, top)
        except AssertionError as e:
            raise AssertionError(f"n_v = {n_v}: {e}") from e
        n = min(top, n_v)
        assert idx[EDGE_ZERO_ROW, :n].tolist() == list(range(n)), n_v
        assert (sc[EDGE_ZERO_ROW, :n] == 0).all(), n_v
        for r in range(EDGE_NQ):  # the tie: row 0 right before row n_v - 1
            lst = idx[r].tolist()
            if n_v >= 2 and r != EDGE_ZERO_ROW and 0 in lst and n_v - 1 in lst:
                assert lst.index(n_v - 1) == lst.index(0) + 1, (n_v, r, lst)
        if n_v >= 2 and n_v <= top:
            assert all(0 in idx[r] and n_v - 1 in idx[r] for r in range(EDGE_NQ))
        out[n_v] = res
        if rank in (31, 65) and n_v == vt + 1:
            # rows stored 8 floats apart from the tight layout, zero padding
            w_i, w_s = E.topk_rows(_dev(Q, rank, 8), EDGE_NQ, _dev(Vm, rank, 8), n_v, rank, top)
            assert _same_bits(idx_d, sc_d, w_i, w_s), n_v
    worst = {"max_score_err": max(v["max_score_err"] for v in out.values()),
             "excused": sum(v["excused"] for v in out.values()),
             "positions": sum(v["positions"] for v in out.values())}
    print(f"k5_edges[rank={rank},top={top}]: {worst}")
    report(f"k5_edges[rank={rank},top={top}]", worst)
