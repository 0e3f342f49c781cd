"""Edge grid of the three kernels built on csrc/row_system.h: fold-in (K7, als_fold_in),
explain (K11, als_explain) and the nonnegative rows (K13, als_nnls_rows), against the fp64
references the parity tests of each kernel already use (oracle.als_oracle.half_sweep over the
known entries, tests/explain_ref.py, tests/nnls_ref.py).  The case builders live in
tests/helpers.py (rowk_*); tests/test_row_kernel_edges_cpu.py pins them without a GPU.

  §1  every rank of K2K3_RANKS (a full and a near-empty last rank block, all four NB) x the
      row lengths around the 32-rating batch, with an unknown column alone in the last batch,
      a whole batch unknown, a row's only known entry or only positive rating alone in its
      last batch, and rows with a zero right-hand side;
  §2  65,600 rows at rank 8: designed (first row -> second row) pairs of one workgroup, each
      second row bit-identical to the same row as a workgroup's first, plus the failed
      pivot in either position (K7, K11);
  §3  K13's task boundaries inside a batch (chunk 33 and 1) and every branch of the short
      workspace.

Bars: the project's 1e-4 per row (per contribution vector and score for K11), exact n_used,
exact zeros in the padding columns and in the rows with a zero right-hand side, status 0;
K13 also x >= 0 and KKT <= 4 x the reference's (test_gpu_nnls.py's third bar).  Measured
maxima (MI355X): profiles/row_kernel_edges.json.
"""
import numpy as np
import pytest
import torch

import nnls_ref as NR
from als_mi355x import _lib, engine as E
from helpers import (K2K3_RANKS, ROWK2_RANK, ROWK3_CHUNKS, ROWK3_RANKS, ROWK_ALPHA,
                     ROWK_MAX_BLOCKS, ROWK_N_SRC, ROWK_PIVOT_RANK, ROWK_REG, ROWK_TOP_N,
                     explain_check_slots, explain_reference, fold_in_oracle, nnls_slot_bytes,
                     nnls_task_counts, ragged_csr, ragged_ptr, rel_row_errs, report, rowk3_case,
                     rowk_failed_pivot_case, rowk_grid_case, rowk_grid_refs,
                     rowk_second_row_case, rowk_second_row_case_nnls, rowk_zero_rhs_rows,
                     small_rows_systems)

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = ROWK_N_SRC
B = ROWK_MAX_BLOCKS
MODES = pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
SOURCES = pytest.mark.parametrize("signed", [True, False], ids=["signed", "abs"])


# ------------------------------------------------------------------ one call of each kernel
def _t(a, dtype):
    return torch.tensor(np.asarray(a)).to(DEV, dtype).contiguous()   # (a copy: a may be read-only)


def _dev(M):
    k = M.shape[1]
    out = torch.zeros((M.shape[0], E.ld_for(k)), dtype=torch.float32, device=DEV)
    out[:, :k] = torch.tensor(M).to(DEV)
    return out


def _yty(Y, k, implicit, ws):
    return E.compute_yty(_dev(Y), N, k, ws) if implicit else None


def _fold(csr, Y, k, reg, implicit):
    """(X [n, ld_for(k)], n_used, status word) of one als_fold_in call."""
    ptr, col, val = csr
    ws = E.Workspace(torch.device(DEV))
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    X, n_used = E.fold_in_rows(_t(ptr, torch.int64), _t(col, torch.int32), _t(val, torch.float32),
                               _dev(Y), N, k, reg, implicit, ROWK_ALPHA, _yty(Y, k, implicit, ws),
                               status, ws)
    torch.cuda.synchronize()
    return X.cpu().numpy(), n_used.cpu().numpy(), int(status.item())


def _explain(csr, targets, Y, k, reg, implicit, top_n):
    """(score [T], pos [T, top_n], contrib [T, top_n], n_used, status, G): G is the [k, k]
    Gram the call was given (als_yty's, unpacked; None when explicit).  als_yty sums in fp32
    (~1e-7 relative, include/als_hip.h at als_gram_dot_f64), and a contribution
    wb (z . y_j) of a row with one positive rating can cancel to 1e-4 of |z| |y_j|: the
    reference of an implicit call is therefore given the same Gram as the kernel, which
    takes it as an input (against Y^T Y in fp64 the contribution error measured 1.4e-4 at
    rank 65 and 5.6e-4 over 65,600 rank-8 rows of 1-3 entries, 6e-8 when explicit)."""
    ptr, col, val = csr
    tptr, tg = targets
    ws = E.Workspace(torch.device(DEV))
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    yty = _yty(Y, k, implicit, ws)
    G = None
    if implicit:
        p = yty.cpu().numpy().astype(np.float64)
        i, j = np.tril_indices(k)
        G = np.zeros((k, k))
        G[i, j] = G[j, i] = p[i * (i + 1) // 2 + j]
    sc, pos, con, n_used = E.explain_rows(
        _t(ptr, torch.int64), _t(col, torch.int32), _t(val, torch.float32), _dev(Y), N, k, reg,
        implicit, ROWK_ALPHA, yty, _t(tptr, torch.int64), _t(tg, torch.int32), top_n, status, ws)
    torch.cuda.synchronize()
    return (sc.cpu().numpy(), pos.cpu().numpy(), con.cpu().numpy(), n_used.cpu().numpy(),
            int(status.item()), G)


def _nnls(csr, Y, k, implicit, chunk=E.DEFAULT_CHUNK):
    """(X [n, ld_for(k) + 4] prefilled with 7.0, n_used, iterations) of one als_nnls_rows
    call through the engine wrapper (a workspace of exactly als_nnls_workspace_bytes)."""
    ptr, col, val = csr
    ws = E.Workspace(torch.device(DEV))
    X = torch.full((len(ptr) - 1, E.ld_for(k) + 4), 7.0, dtype=torch.float32, device=DEV)
    X, n_used, it = E.nnls_rows(_t(ptr, torch.int64), _t(col, torch.int32),
                                _t(val, torch.float32), _dev(Y), N, k, ROWK_REG, implicit,
                                ROWK_ALPHA, _yty(Y, k, implicit, ws), ws, chunk, X=X, iters=True)
    torch.cuda.synchronize()
    return X.cpu().numpy(), n_used.cpu().numpy(), it.cpu().numpy()


def _tail(csr, first):
    """The rows [first, n) of a CSR as a call of their own."""
    ptr, col, val = csr
    return ptr[first:] - ptr[first], col[ptr[first]:], val[ptr[first]:]


# ------------------------------------------------------------------ §1: rank x length
@MODES
@pytest.mark.parametrize("k", K2K3_RANKS)
def test_grid_fold_in(k, implicit):
    c = rowk_grid_case(k, implicit)
    ref, n_ref = rowk_grid_refs(k, implicit)["fold"]
    rows = list(c["rows"])
    X, n_used, status = _fold(ragged_csr(rows), c["Y"], k, ROWK_REG, implicit)
    errs = rel_row_errs(X[:, :k], ref)
    print(f"row edges fold_in k={k} implicit={implicit}: max rel row err {errs.max():.3e} at "
          f"row {int(errs.argmax())} of lengths {[len(r[0]) for r in rows]}")
    report(f"row_edges[fold_in,rank={k},{'implicit' if implicit else 'explicit'}]",
           {"max_rel_err": float(errs.max()), "worst_length": len(rows[int(errs.argmax())][0])})
    assert status == 0
    np.testing.assert_array_equal(n_used, n_ref)
    assert (X[:, k:] == 0).all()
    zero = rowk_zero_rhs_rows(c)
    assert (len(zero) >= 2 if implicit else not zero) and (X[zero] == 0).all()
    assert errs.max() < 1e-4, errs
    # an unknown entry, or a whole batch of them, adds nothing: the same bits without them
    names = list(c["trimmed"])
    Xt, nt, st = _fold(ragged_csr([c["trimmed"][m] for m in names]), c["Y"], k, ROWK_REG, implicit)
    assert st == 0
    for j, name in enumerate(names):
        row = c["special"][name]
        assert Xt[j].tobytes() == X[row].tobytes(), name
        assert nt[j] == n_used[row]


@MODES
@pytest.mark.parametrize("k", K2K3_RANKS)
def test_grid_explain(k, implicit):
    """17 targets per row (two target batches, the second with one live group), then 1."""
    c = rowk_grid_case(k, implicit)
    refs = rowk_grid_refs(k, implicit)
    rows = list(c["rows"])
    csr = ragged_csr(rows)
    zero = set(rowk_zero_rhs_rows(c))
    # an explicit b that cancels exactly (rank 1: the sources are +-1): the factor is zero and
    # the score's own scale ||x|| ||y_t|| with it
    flat = {r for r in range(len(rows)) if r not in zero and not refs["fold"][0][r].any()}
    assert not flat or k == 1
    worst_c = worst_s = 0.0
    for name in ("targets17", "targets1"):
        sc, pos, con, n_used, status, G = _explain(csr, ragged_ptr(c[name]), c["Y"], k, ROWK_REG,
                                                   implicit, ROWK_TOP_N)
        ref = refs["explain" + name[7:]]       # (well separated: asserted when it was built)
        if implicit:
            ref = explain_reference(rows, c[name], c["Y"], ROWK_REG, implicit, ROWK_ALPHA, yty=G)
        assert status == 0
        np.testing.assert_array_equal(n_used, refs["fold"][1])
        # a zero right-hand side: every weight is 0, so scores and contributions are exactly 0
        z = np.array([s for s, x in enumerate(ref) if x[0] in zero], np.int64)
        assert (sc[z] == 0).all() and (con[z] == 0).all()
        for s, (r, t, s_ref, p_ref, c_ref) in enumerate(ref):
            if r in flat:   # the sum of the contributions, to the fp32 rounding of its terms
                n = min(ROWK_TOP_N, len(p_ref))
                np.testing.assert_array_equal(pos[s, :n], p_ref[:n])
                assert np.linalg.norm(con[s, :n] - c_ref[:n]) <= 1e-4 * np.linalg.norm(c_ref[:n])
                assert abs(sc[s] - s_ref) <= 2.0 ** -22 * np.abs(c_ref).sum()
        keep = np.array([s for s, x in enumerate(ref) if x[0] not in zero and x[0] not in flat])
        e_c, e_s = explain_check_slots([ref[s] for s in keep], rows, c["Y"], k, ROWK_REG, implicit,
                                       ROWK_ALPHA, sc[keep], pos[keep], con[keep], ROWK_TOP_N)
        worst_c, worst_s = max(worst_c, e_c), max(worst_s, e_s)
        if name == "targets17":
            full = (sc, pos, con, np.concatenate([[0], np.cumsum([len(t) for t in c[name]])]))
    print(f"row edges explain k={k} implicit={implicit}: max rel contribution err {worst_c:.3e}, "
          f"max score err {worst_s:.3e}")
    report(f"row_edges[explain,rank={k},{'implicit' if implicit else 'explicit'}]",
           {"max_contrib_err": float(worst_c), "max_score_err": float(worst_s)})
    assert worst_c < 1e-4 and worst_s < 1e-4
    # the rows with unknown entries again without them: the same bits, positions shifted
    sc, pos, con, tptr = full
    names = list(c["trimmed"])
    tg = [c["targets17"][c["special"][m]] for m in names]
    sc2, pos2, con2, _, st, _ = _explain(ragged_csr([c["trimmed"][m] for m in names]),
                                         ragged_ptr(tg), c["Y"], k, ROWK_REG, implicit, ROWK_TOP_N)
    assert st == 0
    for j, name in enumerate(names):
        row = c["special"][name]
        cols = rows[row][0]
        kept = np.nonzero((cols >= 0) & (cols < N))[0]
        a = slice(int(tptr[row]), int(tptr[row + 1]))
        b = slice(17 * j, 17 * j + 17)
        assert sc2[b].tobytes() == sc[a].tobytes(), name
        assert con2[b].tobytes() == con[a].tobytes(), name
        np.testing.assert_array_equal(np.where(pos2[b] >= 0, kept[np.maximum(pos2[b], 0)], -1),
                                      pos[a], err_msg=name)


@MODES
@pytest.mark.parametrize("k", K2K3_RANKS)
def test_grid_nnls(k, implicit):
    c = rowk_grid_case(k, implicit)
    A, b, used, ref = rowk_grid_refs(k, implicit)["nnls"]
    rows = list(c["rows"])
    X, n_used, it = _nnls(ragged_csr(rows), c["Y"], k, implicit)
    errs = rel_row_errs(X[:, :k], ref)
    yard = max(NR.kkt(A[r], b[r], ref[r]) for r in range(len(rows)))
    got = max(NR.kkt(A[r], b[r], X[r, :k]) for r in range(len(rows)))
    print(f"row edges nnls k={k} implicit={implicit}: max rel row err {errs.max():.3e} at row "
          f"{int(errs.argmax())}; kkt GPU {got:.3e} reference {yard:.3e}; iterations {it.tolist()}")
    report(f"row_edges[nnls,rank={k},{'implicit' if implicit else 'explicit'}]",
           {"max_rel_err": float(errs.max()), "worst_length": len(rows[int(errs.argmax())][0]),
            "kkt_ratio": float(got / yard)})
    assert (X[:, :k] >= 0).all()
    assert (X[:, k:] == 0).all() and not (X == 7.0).any()
    np.testing.assert_array_equal(n_used, used)
    zero = rowk_zero_rhs_rows(c)
    assert (X[zero] == 0).all() and (it[zero] == 0).all()
    assert errs.max() <= 1e-4, errs
    assert yard > 0 and got <= 4 * yard
    names = list(c["trimmed"])
    Xt, nt, itt = _nnls(ragged_csr([c["trimmed"][m] for m in names]), c["Y"], k, implicit)
    for j, name in enumerate(names):
        row = c["special"][name]
        assert Xt[j].tobytes() == X[row].tobytes(), name
        assert nt[j] == n_used[row] and itt[j] == it[row]


# ------------------------------------------------------------------ §2: a workgroup's second row
def _check_small_explain(cols, vals, lens, Y, reg, implicit, tg, sc, pos, con, top_n, yty=None):
    """The rows of a few entries with one target each (sc / pos / con: their slots) against
    a vectorised fp64 solve; returns (max contribution error, max score error).  A row whose
    factor is zero (implicit, no positive rating) must score exactly 0."""
    Yd = Y.astype(np.float64)
    A, wb, Yj, m = small_rows_systems(cols, vals, lens, Y, reg, implicit, ROWK_ALPHA, yty)
    z = np.linalg.solve(A, Yd[tg][:, :, None])[:, :, 0]
    c = np.where(m, wb * np.einsum("nja,na->nj", Yj, z), -np.inf)
    order = np.argsort(-c, axis=1, kind="stable")        # ties: the earlier entry first
    c_ord = np.take_along_axis(c, order, 1)
    live = np.isfinite(c_ord)
    top = np.abs(np.where(m, c, 0.0)).max(1)
    gap = np.abs(np.diff(np.where(live, c_ord, 0.0), axis=1))
    both = live[:, 1:] & live[:, :-1]
    assert (~both | (gap == 0) | (gap >= 1e-9 * top[:, None])).all()   # the order is decided
    width = cols.shape[1]
    assert top_n <= width
    np.testing.assert_array_equal(pos, np.where(live, order, -1)[:, :top_n])
    want_c = np.where(live, c_ord, 0.0)[:, :top_n]
    e_c = (np.linalg.norm(con - want_c, axis=1)
           / np.maximum(np.linalg.norm(want_c, axis=1), 1e-300)).max()
    x = np.linalg.solve(A, np.einsum("nj,nja->na", wb, Yj)[:, :, None])[:, :, 0]
    den = np.linalg.norm(x, axis=1) * np.linalg.norm(Yd[tg], axis=1)
    assert (sc[den == 0] == 0).all()
    s_ref = np.where(m, c, 0.0).sum(1)
    e_s = (np.abs(sc - s_ref)[den > 0] / den[den > 0]).max()
    return float(e_c), float(e_s)


@MODES
def test_second_row_fold_in(implicit):
    k = ROWK2_RANK
    c = rowk_second_row_case(implicit)
    csr = (c["ptr"], c["col"], c["val"])
    X, n_used, status = _fold(csr, c["Y"], k, ROWK_REG, implicit)
    assert status == 0
    A, wb, Yj, _ = small_rows_systems(c["cols3"], c["vals3"], c["lens3"], c["Y"], ROWK_REG,
                                      implicit, ROWK_ALPHA)
    ref = np.linalg.solve(A, np.einsum("nj,nja->na", wb, Yj)[:, :, None])[:, :, 0]
    n_ref = np.asarray(c["lens3"]).copy()
    idx = sorted(c["designed"])
    ref[idx], n_ref[idx] = fold_in_oracle([c["designed"][i] for i in idx], c["Y"], ROWK_REG,
                                          implicit, ROWK_ALPHA)
    errs = rel_row_errs(X[:, :k], ref)
    print(f"second row fold_in implicit={implicit}: max rel row err {errs.max():.3e}; designed "
          f"{ {name: [float(errs[i]) for i in p] for name, p in c['pairs'].items()} }")
    report(f"row_edges[fold_in,second_row,{'implicit' if implicit else 'explicit'}]",
           {"max_rel_err": float(errs.max())})
    np.testing.assert_array_equal(n_used, n_ref)
    assert (X[n_ref == 0] == 0).all()
    assert errs.max() < 1e-4
    # every second row: the same bits as in a call where it is its workgroup's first row
    X2, n2, st2 = _fold(_tail(csr, B), c["Y"], k, ROWK_REG, implicit)
    assert st2 == 0
    assert X2.tobytes() == X[B:].tobytes() and n2.tobytes() == n_used[B:].tobytes()


@MODES
def test_second_row_explain(implicit):
    k, top_n = ROWK2_RANK, 3
    c = rowk_second_row_case(implicit)
    csr = (c["ptr"], c["col"], c["val"])
    tptr, tg = ragged_ptr(c["targets"])
    sc, pos, con, n_used, status, G = _explain(csr, (tptr, tg), c["Y"], k, ROWK_REG, implicit,
                                               top_n)
    assert status == 0
    idx = sorted(c["designed"])
    filler = np.ones(c["n"], bool)
    filler[idx] = False
    n_ref = np.asarray(c["lens3"]).copy()
    n_ref[idx] = fold_in_oracle([c["designed"][i] for i in idx], c["Y"], ROWK_REG, implicit,
                                ROWK_ALPHA)[1]
    np.testing.assert_array_equal(n_used, n_ref)
    sl = tptr[:-1][filler]
    e_c, e_s = _check_small_explain(c["cols3"][filler], c["vals3"][filler], c["lens3"][filler],
                                    c["Y"], ROWK_REG, implicit, c["tg"][filler], sc[sl], pos[sl],
                                    con[sl], top_n, yty=G)
    # the designed rows, through the reference of the parity tests
    rows = [c["designed"][i] for i in idx]
    tgs = [c["targets"][i] for i in idx]
    ref = explain_reference(rows, tgs, c["Y"], ROWK_REG, implicit, ROWK_ALPHA, yty=G)
    slots = np.concatenate([np.arange(tptr[i], tptr[i + 1]) for i in idx])
    zero = {r for r, (cc, v) in enumerate(rows)
            if implicit and not (np.asarray(v)[(cc >= 0) & (cc < N)] > 0).any()}
    z = slots[[s for s, x in enumerate(ref) if x[0] in zero]]
    assert (sc[z] == 0).all() and (con[z] == 0).all()
    keep = [s for s, x in enumerate(ref) if x[0] not in zero]
    d_c, d_s = explain_check_slots([ref[s] for s in keep], rows, c["Y"], k, ROWK_REG, implicit,
                                   ROWK_ALPHA, sc[slots[keep]], pos[slots[keep]],
                                   con[slots[keep]], top_n)
    print(f"second row explain implicit={implicit}: fillers contribution err {e_c:.3e}, score "
          f"err {e_s:.3e}; designed rows {d_c:.3e}, {d_s:.3e}")
    report(f"row_edges[explain,second_row,{'implicit' if implicit else 'explicit'}]",
           {"max_contrib_err": max(e_c, float(d_c)), "max_score_err": max(e_s, float(d_s))})
    assert max(e_c, d_c) < 1e-4 and max(e_s, d_s) < 1e-4
    a, b = c["pairs"]["no_targets_then_17"]
    assert tptr[a + 1] == tptr[a] and tptr[b + 1] - tptr[b] == 17
    # every second row as a first row: the same bits
    t2 = (tptr[B:] - tptr[B], tg[tptr[B]:])
    sc2, pos2, con2, n2, st2, _ = _explain(_tail(csr, B), t2, c["Y"], k, ROWK_REG, implicit, top_n)
    assert st2 == 0
    s0 = int(tptr[B])
    assert sc2.tobytes() == sc[s0:].tobytes() and pos2.tobytes() == pos[s0:].tobytes()
    assert con2.tobytes() == con[s0:].tobytes() and n2.tobytes() == n_used[B:].tobytes()


@MODES
def test_second_row_nnls(implicit):
    k = ROWK2_RANK
    c = rowk_second_row_case_nnls(implicit)
    csr = (c["ptr"], c["col"], c["val"])
    assert np.diff(c["ptr"]).max() < E.DEFAULT_CHUNK       # no chunking in either call
    X, n_used, it = _nnls(csr, c["Y"], k, implicit)
    pool_ref = NR.solve_rows(*ragged_csr(c["pool"]), c["Y"], ROWK_REG, implicit, ROWK_ALPHA)
    ref = pool_ref[c["which"]]
    n_ref = np.array([len(p[0]) for p in c["pool"]])[c["which"]]
    idx = sorted(c["designed"])
    rows = [c["designed"][i] for i in idx]
    ptr_d, col_d, val_d = ragged_csr(rows)
    ref[idx] = NR.solve_rows(ptr_d, col_d, val_d, c["Y"], ROWK_REG, implicit, ROWK_ALPHA)
    n_ref[idx] = NR.systems(ptr_d, col_d, val_d, c["Y"], ROWK_REG, implicit, ROWK_ALPHA)[2]
    errs = rel_row_errs(X[:, :k], ref)
    print(f"second row nnls implicit={implicit}: max rel row err {errs.max():.3e}; designed "
          f"{ {name: [float(errs[i]) for i in p] for name, p in c['pairs'].items()} }")
    report(f"row_edges[nnls,second_row,{'implicit' if implicit else 'explicit'}]",
           {"max_rel_err": float(errs.max())})
    assert (X[:, :k] >= 0).all() and (X[:, k:] == 0).all()
    np.testing.assert_array_equal(n_used, n_ref)
    first, _ = c["pairs"]["zero_rhs_then_ordinary"]
    assert (X[first] == 0).all() and it[first] == 0 and n_used[first] == 25
    first, _ = c["pairs"]["unknown_then_ordinary"]
    assert (X[first] == 0).all() and it[first] == 0 and n_used[first] == 0
    assert errs.max() <= 1e-4
    for name, (_, second) in c["pairs"].items():
        if name != "ordinary_then_empty":
            assert np.linalg.norm(ref[second]) > 0, name    # an ordinary row, solved
    X2, n2, it2 = _nnls(_tail(csr, B), c["Y"], k, implicit)
    assert X2.tobytes() == X[B:].tobytes() and n2.tobytes() == n_used[B:].tobytes()
    assert it2.tobytes() == it[B:].tobytes()


def _pivot_refs(c):
    A, wb, Yj, _ = small_rows_systems(c["cols"], c["vals"], c["lens"], c["Y"], 0.0, False, 1.0)
    good = np.ones(c["n"], bool)
    good[list(c["failing"])] = False
    return A, wb, Yj, good


def test_failed_pivot_in_either_position_fold_in():
    """Explicit, reg = 0, rank 4: (failed pivot -> ordinary) in workgroup 0 and (ordinary ->
    failed pivot) in workgroup 1.  The word names one of the two; they read as zeros; every
    other row is solved."""
    c = rowk_failed_pivot_case()
    k = ROWK_PIVOT_RANK
    X, n_used, status = _fold((c["ptr"], c["col"], c["val"]), c["Y"], k, 0.0, False)
    assert status in [r + 1 for r in c["failing"]]
    np.testing.assert_array_equal(n_used, c["lens"])
    assert (X[list(c["failing"])] == 0).all()
    A, wb, Yj, good = _pivot_refs(c)
    ref = np.linalg.solve(A[good], np.einsum("nj,nja->na", wb, Yj)[good][:, :, None])[:, :, 0]
    errs = rel_row_errs(X[good, :k], ref)
    print(f"failed pivot fold_in: other rows max rel row err {errs.max():.3e}, status {status}")
    report("row_edges[fold_in,failed_pivot]", {"max_rel_err": float(errs.max())})
    assert errs.max() < 1e-4


def test_failed_pivot_in_either_position_explain():
    c = rowk_failed_pivot_case()
    k, top_n, n = ROWK_PIVOT_RANK, 3, c["n"]
    sc, pos, con, n_used, status, _ = _explain((c["ptr"], c["col"], c["val"]),
                                               (np.arange(n + 1), c["tg"]), c["Y"], k, 0.0, False,
                                               top_n)
    assert status in [r + 1 for r in c["failing"]]
    np.testing.assert_array_equal(n_used, c["lens"])
    bad = list(c["failing"])
    assert (sc[bad] == 0).all() and (pos[bad] == -1).all() and (con[bad] == 0).all()
    good = np.ones(n, bool)
    good[bad] = False
    e_c, e_s = _check_small_explain(c["cols"][good], c["vals"][good], c["lens"][good], c["Y"], 0.0,
                                    False, c["tg"][good], sc[good], pos[good], con[good], top_n)
    print(f"failed pivot explain: other rows contribution err {e_c:.3e}, score err {e_s:.3e}, "
          f"status {status}")
    report("row_edges[explain,failed_pivot]", {"max_contrib_err": e_c, "max_score_err": e_s})
    assert e_c < 1e-4 and e_s < 1e-4


# ------------------------------------------------------------------ §3: tasks and the short workspace
@pytest.mark.parametrize("chunk", ROWK3_CHUNKS)
@MODES
@SOURCES
@pytest.mark.parametrize("k", ROWK3_RANKS)
def test_nnls_task_boundaries_inside_a_batch(k, signed, implicit, chunk):
    """chunk = 33 and 1: no task but a row's first starts on a 32-rating batch boundary."""
    c = rowk3_case(k, signed, implicit, chunk)
    csr = ragged_csr(list(c["rows"]))
    Xc, nc, _ = _nnls(csr, c["Y"], k, implicit, chunk=chunk)
    Xw, nw, _ = _nnls(csr, c["Y"], k, implicit, chunk=4096)
    e_ref = rel_row_errs(Xc[:, :k], c["ref"])
    e_one = rel_row_errs(Xc[:, :k], Xw[:, :k])
    tag = f"rank={k},{'signed' if signed else 'abs'},{'implicit' if implicit else 'explicit'}"
    print(f"nnls tasks {tag} chunk={chunk}: vs reference {e_ref.max():.3e}, chunk {chunk} vs "
          f"4096 {e_one.max():.3e} (lengths {c['lens']})")
    report(f"row_edges[nnls,tasks,{tag},chunk={chunk}]",
           {"max_rel_err": float(e_ref.max()), "chunked_vs_whole": float(e_one.max())})
    np.testing.assert_array_equal(nc, nw)
    want = list(c["lens"])
    want[-1] = 160
    assert nc.tolist() == want
    assert (Xc[:, :k] >= 0).all() and (Xc[:, k:] == 0).all()
    assert e_ref.max() <= 1e-4
    assert e_one.max() <= 1e-6
    X2, n2, _ = _nnls(csr, c["Y"], k, implicit, chunk=chunk)
    assert Xc.tobytes() == X2.tobytes() and nc.tobytes() == n2.tobytes()


def _nnls_raw(csr, Y, k, implicit, chunk, slots):
    """als_nnls_rows with a workspace of the per-row arrays plus exactly `slots` task slots.
    Returns (rc, X [n, ld_for(k)], n_used)."""
    L = _lib.lib()
    ptr, col, val = csr
    n = len(ptr) - 1
    ws = E.Workspace(torch.device(DEV))
    yty = _yty(Y, k, implicit, ws)
    nbytes = int(L.als_nnls_workspace_bytes(n, 0, k, chunk)) + slots * nnls_slot_bytes(k)
    w = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    Yd = _dev(Y)
    X = torch.full((n, E.ld_for(k)), 7.0, dtype=torch.float32, device=DEV)
    n_used = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    a = (_t(ptr, torch.int64), _t(col, torch.int32), _t(val, torch.float32))
    rc = L.als_nnls_rows(_lib.ptr(a[0]), _lib.ptr(a[1]), _lib.ptr(a[2]), n, _lib.ptr(Yd), N,
                         Yd.shape[1], k, float(ROWK_REG), int(implicit), float(ROWK_ALPHA),
                         _lib.ptr(yty), chunk, _lib.ptr(X), X.shape[1], _lib.ptr(n_used), 0,
                         _lib.ptr(w), nbytes, _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, X.cpu().numpy(), n_used.cpu().numpy()


@MODES
@SOURCES
@pytest.mark.parametrize("k", ROWK3_RANKS)
def test_nnls_short_workspace(k, signed, implicit):
    """S = 0: every long row is summed serially.  S = the first long row's slots: that row
    goes through its slots, the later ones serially.  S + 1: the next row's tasks fit only
    partly, so it goes serially as a whole.  S = T: every long row through its slots, the
    bits of the engine's call."""
    chunk = 33
    c = rowk3_case(k, signed, implicit, chunk)
    csr = ragged_csr(list(c["rows"]))
    tasks = nnls_task_counts(c["lens"], chunk)
    total = sum(tasks)
    first = next(t for t in tasks if t)
    assert 0 < first < first + 1 < total
    Xe, ne, _ = _nnls(csr, c["Y"], k, implicit, chunk=chunk)
    Xe = Xe[:, :E.ld_for(k)]
    worst = {}
    for S in (0, first, first + 1, total):
        rc, X, n_used = _nnls_raw(csr, c["Y"], k, implicit, chunk, S)
        assert rc == 0, (S, _lib.lib().als_last_error())
        e_full = rel_row_errs(X[:, :k], Xe[:, :k])
        e_ref = rel_row_errs(X[:, :k], c["ref"])
        worst[S] = (float(e_full.max()), float(e_ref.max()))
        np.testing.assert_array_equal(n_used, ne)
        assert (X[:, :k] >= 0).all() and (X[:, k:] == 0).all()
        assert e_full.max() <= 1e-6, (S, e_full)
        assert e_ref.max() <= 1e-4, (S, e_ref)
        if S == total:
            assert X.tobytes() == Xe.tobytes()
    tag = f"rank={k},{'signed' if signed else 'abs'},{'implicit' if implicit else 'explicit'}"
    print(f"nnls short workspace {tag}: slots -> (vs full workspace, vs reference) {worst}")
    report(f"row_edges[nnls,short_workspace,{tag}]",
           {f"slots={S}": {"vs_full": a, "max_rel_err": b} for S, (a, b) in worst.items()})
