"""CPU side of the K7 / K11 / K13 edge grid (tests/test_gpu_edges_row_kernels.py): the case
builders of tests/helpers.py (rowk_*) and the references, pinned without a GPU."""
import numpy as np
import pytest

import nnls_ref as NR
from als_mi355x import _lib
from helpers import (K2K3_RANKS, ROWK2_N, ROWK2_RANK, ROWK3_CHUNKS, ROWK3_MARGIN, ROWK3_RANKS,
                     ROWK_ALPHA, ROWK_BATCH, ROWK_IMPLICIT_ROWS, ROWK_LENGTHS, ROWK_MAX_BLOCKS,
                     ROWK_N_SRC, ROWK_PIVOT_RANK, ROWK_REG, ROWK_UNKNOWN_ROWS, fold_in_oracle,
                     known_entries, nnls_slot_bytes, nnls_solve_order, nnls_task_counts,
                     nnls_wall_margin, ragged_csr, rel_row_errs, rowk3_case, rowk3_lengths,
                     rowk_failed_pivot_case, rowk_grid_case, rowk_grid_lengths, rowk_grid_refs,
                     rowk_second_row_case, rowk_second_row_case_nnls, rowk_zero_rhs_rows,
                     small_rows_systems)
from oracle import c_oracle as C

N = ROWK_N_SRC
B = ROWK_MAX_BLOCKS
MODES = pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
CPU_REF_RANKS = (1, 16, 33, 65, 128)   # the references themselves: one rank per NB and k = 1


# ---------------------------------------------------------------- §1: the grid
@MODES
@pytest.mark.parametrize("rank", K2K3_RANKS)
def test_grid_rows_are_as_stated(rank, implicit):
    c = rowk_grid_case(rank, implicit)
    rows, at = c["rows"], c["special"]
    lens = [len(r[0]) for r in rows]
    want = [d for d in ROWK_LENGTHS + (rank - 1, rank, rank + 1) if d >= 1]
    assert c["lengths"] == rowk_grid_lengths(rank) == want and lens[:len(want)] == want
    for d in (31, 32, 33, 63, 64, 65):     # every length around one and two full batches
        assert d in want
    assert ROWK_BATCH == 32
    for cols, vals in rows[:len(want)]:    # the grid rows: distinct known ids, half stars
        assert len(np.unique(cols)) == len(cols) and cols.min() >= 0 and cols.max() < N
        assert vals.dtype == np.float32 and np.all(vals * 2 == np.round(vals * 2))
        assert not cols.flags.writeable and not vals.flags.writeable
    allv = np.concatenate([v for _, v in rows[:len(want)]])
    if implicit:
        assert (allv > 0).any() and (allv < 0).any() and (allv == 0).any()
        ex = np.concatenate([v for _, v in rowk_grid_case(rank, False)["rows"][:len(want)]])
        np.testing.assert_array_equal(allv, ex - np.float32(2.5))
    else:
        assert allv.min() >= 0.5 and allv.max() <= 5.0
    # the special rows: the stated property at the stated position
    names = [m for m, _ in ROWK_UNKNOWN_ROWS + (ROWK_IMPLICIT_ROWS if implicit else ())]
    assert sorted(at) == sorted(names) and len(rows) == len(want) + len(names)
    for name, d in ROWK_UNKNOWN_ROWS + (ROWK_IMPLICIT_ROWS if implicit else ()):
        assert len(rows[at[name]][0]) == d, name

    def unknown(name):
        cols = rows[at[name]][0]
        return np.nonzero((cols < 0) | (cols >= N))[0].tolist()

    assert unknown("unknown_at_32") == [32] and rows[at["unknown_at_32"]][0][32] == -1
    assert unknown("nsrc_at_64") == [64] and rows[at["nsrc_at_64"]][0][64] == N
    assert unknown("unknown_batch") == list(range(32, 64))
    assert unknown("known_last") == list(range(32))
    for name, _ in ROWK_UNKNOWN_ROWS:
        cols, vals = rows[at[name]]
        ok = (cols >= 0) & (cols < N)
        np.testing.assert_array_equal(c["trimmed"][name][0], cols[ok])
        np.testing.assert_array_equal(c["trimmed"][name][1], vals[ok])
    if implicit:
        for name, d in ROWK_IMPLICIT_ROWS:
            v = rows[at[name]][1]
            assert unknown(name) == [] and (v[:-1] <= 0).all() and (v < 0).any()
            if name.startswith("last_positive"):
                assert v[-1] > 0 and (d - 1) % 32 == 0    # alone in the row's last batch
            else:
                assert v[-1] <= 0
        # (a short row whose few ratings happen to be <= 0 has a zero right-hand side too)
        zero = rowk_zero_rhs_rows(c)
        assert {at["nonpositive_33"], at["nonpositive_65"]} <= set(zero)
        assert at["last_positive_33"] not in zero and at["last_positive_65"] not in zero
        for i in zero:
            assert not (known_entries([rows[i]], N)[0][1] > 0).any()
    else:
        assert rowk_zero_rhs_rows(c) == []
    # K11's targets: 17 with a -1, n_src, a rated item and a repeat; 1 known one
    for (cols, _), t17, t1 in zip(rows, c["targets17"], c["targets1"]):
        assert len(t17) == 17 and t17[0] == -1 and t17[4] == N and t17[3] == t17[2]
        assert t17[1] in cols and len(t1) == 1 and 0 <= t1[0] < N
    assert np.allclose(np.linalg.norm(c["Y"].astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert c["Y"].shape == (N, rank) and not c["Y"].flags.writeable


@MODES
@pytest.mark.parametrize("rank", CPU_REF_RANKS)
def test_numpy_and_c_oracle_agree_on_the_grid(rank, implicit):
    """oracle.als_oracle.half_sweep (the GPU test's reference) and the C restatement of
    Spark's packed dspr + dppsv arithmetic are two fp64 computations rounded to fp32.
    tests/test_oracle.py holds them to 1e-9 per row on planted data, i.e. to the same fp32
    bits in every row; the bar here is that same 1e-9 (measured on these rows: 0.0 at every
    rank and mode)."""
    c = rowk_grid_case(rank, implicit)
    ref, n_used = rowk_grid_refs(rank, implicit)["fold"]
    known = known_entries(c["rows"], N)
    np.testing.assert_array_equal(n_used, [len(k[0]) for k in known])
    assert (n_used > 0).all()
    Xc, st = C.half_sweep(*ragged_csr(known), c["Y"], ROWK_REG, implicit, ROWK_ALPHA, threads=2)
    assert st.max() == 0
    errs = rel_row_errs(Xc, ref)
    print(f"numpy vs C oracle on the row-kernel grid rank={rank} implicit={implicit}: "
          f"{errs.max():.3e}")
    assert errs.max() < 1e-9
    zero = rowk_zero_rhs_rows(c)
    assert (ref[zero] == 0).all()
    if rank > 1:   # (at rank 1 the sources are +-1 and an explicit b can cancel exactly)
        assert (np.linalg.norm(np.delete(ref, zero, 0), axis=1) > 0).all()
    # the trimmed rows are the same rows to the reference
    for name, _ in ROWK_UNKNOWN_ROWS:
        r1, n1 = fold_in_oracle([c["trimmed"][name]], c["Y"], ROWK_REG, implicit, ROWK_ALPHA)
        assert r1[0].tobytes() == ref[c["special"][name]].tobytes()
        assert n1[0] == n_used[c["special"][name]]


@MODES
@pytest.mark.parametrize("rank", (16, 65))
def test_grid_references_of_explain_and_nnls(rank, implicit):
    """The explain slots are well separated (asserted when they are built) and sum to the
    reference's score; the NNLS rows are nonnegative, within 1e-5 of KKT, and agree with the
    Cholesky reference wherever that one is nonnegative itself."""
    c = rowk_grid_case(rank, implicit)
    refs = rowk_grid_refs(rank, implicit)
    n_t = {"explain17": 17, "explain1": 1}
    for name, per_row in n_t.items():
        ref = refs[name]
        assert len(ref) == per_row * len(c["rows"])
        for r, t, s, pos, con in ref:
            if 0 <= t < N:
                assert len(pos) == refs["fold"][1][r] and abs(con.sum() - s) <= 1e-12 * max(
                    1.0, np.abs(con).sum())
                assert (np.diff(con) <= 0).all()
            else:
                assert len(pos) == 0 and s == 0.0
    A, b, used, X = refs["nnls"]
    np.testing.assert_array_equal(used, refs["fold"][1])
    assert (X >= 0).all() and X.dtype == np.float32
    for r in range(len(X)):
        assert NR.kkt(A[r], b[r], X[r]) < 1e-5
    zero = rowk_zero_rhs_rows(c)
    assert (X[zero] == 0).all()
    chol = refs["fold"][0]
    inside = (chol > 0).all(1)
    if inside.any():
        assert rel_row_errs(X[inside], chol[inside]).max() < 1e-5


# ---------------------------------------------------------------- §2: second rows
@MODES
def test_second_row_pairs_of_fold_in_and_explain(implicit):
    c = rowk_second_row_case(implicit)
    n, ptr = c["n"], c["ptr"]
    assert n == ROWK2_N == B + 64 and len(ptr) == n + 1 and c["Y"].shape == (N, ROWK2_RANK)
    deg = np.diff(ptr)
    known = lambda i: known_entries([(c["col"][ptr[i]:ptr[i + 1]], c["val"][ptr[i]:ptr[i + 1]])],
                                    N)[0]
    for name, (a, b) in c["pairs"].items():
        assert 0 <= a < 64 and b == a + B, name          # workgroup a: its first and second row
    p = c["pairs"]
    a, b = p["empty_then_ordinary"]
    assert deg[a] == 0 and deg[b] == 20 and len(known(b)[0]) == 20
    a, b = p["ordinary_then_empty"]
    assert deg[a] == 20 and deg[b] == 0
    a, b = p["long_then_short"]
    assert (deg[a], deg[b]) == (300, 1)
    a, b = p["short_then_long"]
    assert (deg[a], deg[b]) == (1, 300)
    a, b = p["unknown_then_ordinary"]
    assert deg[a] == 5 and len(known(a)[0]) == 0 and len(known(b)[0]) == 20
    a, b = p["nonpositive_then_ordinary"]
    assert deg[a] == 12 and (known(a)[1] < 0).all() and len(known(b)[0]) == 20
    if implicit:   # the ordinary second rows have a positive rating: a nonzero factor
        for name, (a, b) in p.items():
            if name.endswith("ordinary") or name == "no_targets_then_17":
                assert (known(b)[1] > 0).any(), name
    a, b = p["no_targets_then_17"]
    assert len(c["targets"][a]) == 0 and len(c["targets"][b]) == 17 and deg[a] == deg[b] == 20
    # everything else: a filler of 1-3 known entries with one target
    filler = np.ones(n, bool)
    filler[sorted(c["designed"])] = False
    assert len(c["designed"]) == 14 and (deg[filler] == c["lens3"][filler]).all()
    assert deg[filler].min() == 1 and deg[filler].max() == 3
    assert all(len(c["targets"][i]) == 1 for i in np.nonzero(filler)[0][:200])
    i = int(np.nonzero(filler)[0][70000 % filler.sum()])
    np.testing.assert_array_equal(c["col"][ptr[i]:ptr[i + 1]], c["cols3"][i, :deg[i]])
    np.testing.assert_array_equal(c["val"][ptr[i]:ptr[i + 1]], c["vals3"][i, :deg[i]])
    # the vectorised filler systems are the row-wise oracle's
    A, wb, Yj, _ = small_rows_systems(c["cols3"][:50], c["vals3"][:50], c["lens3"][:50], c["Y"],
                                      ROWK_REG, implicit, ROWK_ALPHA)
    x = np.linalg.solve(A, np.einsum("nj,nja->na", wb, Yj)[:, :, None])[:, :, 0]
    rows = [(c["cols3"][j, :c["lens3"][j]], c["vals3"][j, :c["lens3"][j]]) for j in range(50)]
    ref, _ = fold_in_oracle(rows, c["Y"], ROWK_REG, implicit, ROWK_ALPHA)
    assert rel_row_errs(x.astype(np.float32), ref).max() < 1e-6


@MODES
def test_second_row_pairs_of_nnls_in_the_sorted_order(implicit):
    """als_nnls_rows' solve launch walks the rows in a stable sort on descending degree and
    workgroup w takes order[w] and order[w + 65,536]: the designed pairs share a workgroup."""
    c = rowk_second_row_case_nnls(implicit)
    ptr, n = c["ptr"], c["n"]
    deg = np.diff(ptr)
    order = nnls_solve_order(ptr)
    assert sorted(order.tolist()) == list(range(n))
    assert (np.diff(deg[order]) <= 0).all()
    same = np.diff(deg[order]) == 0
    assert (np.diff(order)[same] > 0).all()              # ties in index order
    where = np.empty(n, np.int64)
    where[order] = np.arange(n)
    for name, (a, b) in c["pairs"].items():
        assert where[a] < 64 and where[b] == where[a] + B, name
        assert deg[a] >= deg[b]
    assert order[:5].tolist() == [10, 11, 12, 13, 14]
    assert deg[order[:5]].tolist() == [300, 40, 30, 25, 20]
    assert order[B:B + 63].tolist() == list(range(B + 1, n)) and (deg[B + 1:] == 1).all()
    assert order[-1] == 9 and (deg == 0).sum() == 1
    p = c["pairs"]
    assert p["long_then_short"] == (10, B + 1) and p["ordinary_then_empty"][1] == 9
    assert deg[p["ordinary_then_empty"][0]] == 3
    csr = lambda i: (np.array([0, deg[i]]), c["col"][ptr[i]:ptr[i + 1]], c["val"][ptr[i]:ptr[i + 1]])
    # the first rows leave through the exits they are named after
    A, b, used = NR.systems(*csr(p["unknown_then_ordinary"][0]), c["Y"], ROWK_REG, implicit,
                            ROWK_ALPHA)
    assert used[0] == 0
    for name in ("zero_rhs_then_ordinary",) + (("nonpositive_then_ordinary",) if implicit else ()):
        A, b, used = NR.systems(*csr(p[name][0]), c["Y"], ROWK_REG, implicit, ROWK_ALPHA)
        info = {}
        assert used[0] > 0 and (b == 0).all()
        assert (NR.nnls_solve(A[0], b[0], info) == 0).all() and info["iters"] == 0
    # ... and every designed second row but the empty one has a nonzero solution
    for name, (a, b2) in p.items():
        x = NR.solve_rows(*csr(b2), c["Y"], ROWK_REG, implicit, ROWK_ALPHA)
        assert (np.linalg.norm(x) > 0) == (name != "ordinary_then_empty"), name
    # the fillers are the pool's rows
    for i in (0, 15, 40000, B):
        cols, vals = c["pool"][c["which"][i]]
        np.testing.assert_array_equal(c["col"][ptr[i]:ptr[i + 1]], cols)
        np.testing.assert_array_equal(c["val"][ptr[i]:ptr[i + 1]], vals)


def test_failed_pivot_case_fillers_are_positive_definite():
    c = rowk_failed_pivot_case()
    assert c["n"] == ROWK2_N and c["Y"].shape == (N, ROWK_PIVOT_RANK)
    assert c["failing"] == (0, B + 1)        # first row of workgroup 0, second of workgroup 1
    good = np.ones(c["n"], bool)
    good[list(c["failing"])] = False
    assert (c["lens"][good] == 6).all() and c["lens"][list(c["failing"])].tolist() == [2, 2]
    srt = np.sort(c["cols"], axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all()             # 6 distinct items
    A, _, _, _ = small_rows_systems(c["cols"], c["vals"], c["lens"], c["Y"], 0.0, False, 1.0)
    ev = np.linalg.eigvalsh(A)
    ratio = ev[:, 0] / ev[:, -1]
    print(f"failed pivot case: smallest filler eigenvalue ratio {ratio[good].min():.3e}")
    assert (ratio[good] > 1e-6).all()
    # the two short rows: A of rank 2 at rank 4, reg = 0
    assert (np.abs(ev[list(c["failing"]), :2]) < 1e-12 * ev[list(c["failing"]), -1:]).all()
    assert np.diff(c["ptr"]).tolist() == c["lens"].tolist()


# ---------------------------------------------------------------- §3: tasks and the workspace
def test_task_lengths_and_counts():
    assert rowk3_lengths(33) == [32, 33, 34, 66, 67, 98, 200]
    assert rowk3_lengths(1) == [0, 1, 2, 2, 3, 2, 40, 200]
    assert nnls_task_counts(rowk3_lengths(33), 33) == [0, 0, 2, 2, 3, 3, 7]
    assert nnls_task_counts(rowk3_lengths(1), 1) == [0, 0, 2, 2, 3, 2, 40, 200]
    for chunk in ROWK3_CHUNKS:
        for d, t in zip(rowk3_lengths(chunk), nnls_task_counts(rowk3_lengths(chunk), chunk)):
            assert t == (int(np.ceil(d / chunk)) if d > chunk else 0)
    # chunk = 33: every task of a row but its first starts inside a 32-rating batch
    assert all((j * 33) % 32 for j in range(1, 7))
    assert nnls_slot_bytes(16) == 8 * (2 * 256 + 2) and nnls_slot_bytes(128) == 8 * (37 * 256 + 2)
    assert nnls_slot_bytes(17) == nnls_slot_bytes(32) == 8 * (4 * 256 + 2)


@MODES
@pytest.mark.parametrize("signed", [True, False], ids=["signed", "abs"])
@pytest.mark.parametrize("rank", ROWK3_RANKS)
def test_task_rows_do_not_sit_on_a_wall_decision(rank, signed, implicit):
    """A and b perturbed by 1e-13 relative move nnls_ref's solution by less than 1e-8: the
    1e-6 bar between two summation orders of the Gram is one the reference alone keeps."""
    for chunk in ROWK3_CHUNKS:
        c = rowk3_case(rank, signed, implicit, chunk)
        assert [len(r[0]) for r in c["rows"]] == rowk3_lengths(chunk)
        cols = c["rows"][-1][0]
        assert (cols[::5] == -1).all() and (np.delete(cols, np.arange(0, 200, 5)) >= 0).all()
        ptr, col, val = ragged_csr(list(c["rows"]))
        A, b, used = NR.systems(ptr, col, val, c["Y"], ROWK_REG, implicit, ROWK_ALPHA)
        assert used[-1] == 160
        for j in range(len(b)):
            if used[j]:
                m = nnls_wall_margin(A[j], b[j], seed=j)
                assert m == c["margins"][j] and m < ROWK3_MARGIN, (chunk, j, m)
        print(f"task rows rank={rank} signed={signed} implicit={implicit} chunk={chunk}: worst "
              f"margin {max(c['margins']):.2e}, {c['redrawn']} rows redrawn")
        assert (c["ref"] >= 0).all()


@pytest.mark.parametrize("k", ROWK3_RANKS)
def test_workspace_short_of_the_per_row_arrays_is_refused(k):
    """als_nnls_workspace_bytes(n, 0, k, chunk) is the per-row arrays plus 256 spare bytes,
    less than one slot: one byte short of the arrays is ALS_EWORKSPACE on the host."""
    L = _lib.lib()
    n, chunk = 7, 33
    arrays = int(L.als_nnls_workspace_bytes(n, 0, k, chunk)) - 256
    assert arrays > 0 and 256 < nnls_slot_bytes(k)
    two_slots = int(L.als_nnls_workspace_bytes(n, 33, k, chunk)) - int(
        L.als_nnls_workspace_bytes(n, 0, k, chunk))   # nnz / chunk = 1: one row, one task more
    assert 0 <= two_slots - 2 * nnls_slot_bytes(k) < 256  # rounded up by the arena
    ld = (k + 3) // 4 * 4
    rc = L.als_nnls_rows(16, 16, 16, n, 16, 1, ld, k, 0.1, 0, 1.0, 0, chunk, 16, ld, 0, 0, 16,
                         arrays - 1, 0)
    assert rc == -2 and L.als_last_error()
