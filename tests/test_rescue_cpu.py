"""CPU side of the fp64 rescue tests (tests/test_gpu_rescue64.py): the placement of the rescue
list restated against als_solve_workspace_bytes, the conditioning that makes the GPU file's
2^-23 bar a derived one, the exact failure of rescue_ref.failing_case, and the references."""
import os
import re

import numpy as np
import pytest

from als_mi355x import _lib
from oracle import als_oracle as O
from helpers import K2K3_REG, k2k3_grid_case, k2k3_special_rows, rel_row_errs
import rescue_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "recommender-system-using-apache-spark-mllib-_amd", "csrc")


def test_constants_match_the_kernel():
    cfg = open(os.path.join(CSRC, "solve_config.h")).read()
    res = open(os.path.join(CSRC, "rescue64.h")).read()
    assert int(re.search(r"constexpr int kRescueGrid = (\d+);", cfg).group(1)) == R.RESCUE_GRID
    assert int(re.search(r"constexpr int kRescueBatch = (\d+);", res).group(1)) == R.RESCUE_BATCH
    assert R.BAR == 2.0 ** -23 and R.COND_BAR == 2.0 ** -30


# ---------------------------------------------------------------- list_region
@pytest.mark.parametrize("n_src", [0, 1, 1024, 1025, 70001])
@pytest.mark.parametrize("rank", [1, 16, 17, 32, 33, 64, 65, 128])
def test_list_region_placement(rank, n_src):
    """With the byte count als_solve_workspace_bytes returns, and with a larger buffer (a
    workspace that grew for an earlier call), the list lies wholly above the 256 B of scale
    words + the C-layout YtY table + the partial slots, wholly below the split table, and
    is 256-byte aligned."""
    L = _lib.lib()
    kp = L.als_k_pad(rank)
    table = R.align256(4 * kp * (n_src + 1))
    front0 = L.als_solve_workspace_bytes(rank, 0, 0, 0) - R.align256(4 * kp) - 256
    assert front0 >= 256
    for n_rows in (0, 1, 63, 64, 65, 137, 100000):
        for n_chunks in (0, 1, 7, 300):
            need = L.als_solve_workspace_bytes(rank, n_chunks, n_src, n_rows)
            # what the size function puts in front of the list: its total minus the list,
            # the table and the 256 B of alignment slack (the layout comment above
            # als_solve_workspace_bytes)
            front = need - R.align256(4 * n_rows) - table - 256
            assert front % 256 == 0 and front >= front0 and (front > front0) == (n_chunks > 0)
            for slack in (0, 4, 100, 256, 4096 + 12):
                ws_bytes = need + slack
                off = R.list_region(ws_bytes, rank, n_src, n_rows, kp)
                t_off = R.table_offset(ws_bytes, n_src, kp)
                assert off % 256 == 0 and t_off % 256 == 0
                assert off >= front
                assert off + 4 * n_rows <= t_off
                assert t_off + 4 * kp * (n_src + 1) <= ws_bytes


def test_list_region_rejects_a_wrong_k_pad():
    for rank, kp in ((16, 32), (17, 16), (64, 128), (65, 64), (0, 16)):
        with pytest.raises(ValueError):
            R.list_region(1 << 20, rank, 10, 10, kp)
    with pytest.raises(ValueError):
        R.list_region(1 << 20, 16, 10, -1, 16)


# ---------------------------------------------------------------- conditioning of the inputs
def _assert_conditioned(rank, conds):
    assert np.isfinite(conds).all()
    assert R.cond_term(rank, conds) <= R.COND_BAR, (rank, float(conds.max()))


@pytest.mark.parametrize("rank,mode", R.GRID_CASES)
def test_grid_systems_are_well_conditioned(rank, mode):
    """(a), (b): rank * cond * 2^-53 <= 2^-30 for every row, so the fp64 term of the error
    bound stays three orders of magnitude below the fp32 cast."""
    _, conds = R.grid_refs(rank, mode)
    assert len(conds) == len(k2k3_grid_case(rank, R.GRID_MODES[mode][0])["indptr"]) - 1
    assert len(conds) > R.RESCUE_GRID  # workgroups walk several rows each
    _assert_conditioned(rank, conds)


@pytest.mark.parametrize("rank", R.SPECIAL_RANKS)
def test_special_systems_are_well_conditioned(rank):
    _assert_conditioned(rank, R.special_refs(rank)[1])


@pytest.mark.parametrize("rank", R.GUARD_RANKS)
def test_guard_systems_are_well_conditioned(rank):
    """(e): the ratings' scale does not reach A, and the anchor's system is y y^T + 0.1 I."""
    X, conds = R.guard_refs(rank)
    g = R.guard_case(rank)
    assert len(conds) == g["anchor"] + 1 == len(g["indptr"]) - 1
    _assert_conditioned(rank, conds)
    # the reference scales exactly with the ratings
    rows = [0, len(conds) // 2, g["anchor"] - 1, g["anchor"]]
    direct = R.exact_ref(g["indptr"], g["indices"], g["vals"], g["Y"], R.REG, rows=rows)
    assert R.row_errs(direct, X[rows]).max() <= 1e-13
    assert g["vals"][g["indptr"][g["anchor"]]] == 1.0 and np.diff(g["indptr"])[g["anchor"]] == 1
    assert np.abs(np.delete(g["vals"], g["indptr"][g["anchor"]])).max() <= 5 * R.GUARD_SCALE


def test_references_use_the_regparam_of_the_abi():
    """als_solve_half takes regParam as a C float: the kernel's lambda is (double)(float)0.1,
    2^-26 off 0.1, and the references use the same value."""
    assert R.REG == float(np.float32(K2K3_REG)) != K2K3_REG
    assert abs(R.REG - K2K3_REG) / K2K3_REG <= 2.0 ** -26
    assert R.abi_reg(0.0) == 0.0 and R.abi_reg(0.5) == 0.5


@pytest.mark.parametrize("rank,dual", R.GUARD_CASES)
def test_guard_unlisted_rows_yardstick(rank, dual):
    """(e): the rows the guards keep on the fp32-grade path (the anchor; with the dual path
    on, the rows of <= dual_limit ratings) are held to 8 x the fp32 textbook solve's error on
    the same rows; pinned to (0, 1.25e-5] here so that bar is neither vacuous nor looser than
    the project's 1e-4."""
    g = R.guard_case(rank)
    dual_rows, unlisted = R.guard_unlisted(rank, dual)
    assert g["anchor"] in unlisted and len(unlisted) == len(set(dual_rows) | {g["anchor"]})
    assert (len(dual_rows) > 0) == (dual and rank > 32)
    e = R.guard_textbook_errs(rank, unlisted)
    assert len(e) == len(unlisted) and 0 < e.max() <= 1.25e-5
    assert R.YARDSTICK_FACTOR * e.max() <= 1e-4


@pytest.mark.parametrize("rank", R.FAIL_RANKS)
def test_failing_case_full_rows_are_well_conditioned(rank):
    """(d): the rows that are solved there (the failing ones are singular by construction and
    are compared with exact zeros, not with a solution)."""
    f = R.failing_case(rank)
    conds = R.system_conds(f["indptr"], f["indices"], f["vals"], f["Y"], 0.0, rows=f["full"])
    assert conds.max() <= 16.0
    _assert_conditioned(rank, conds)


# ---------------------------------------------------------------- exact failure
@pytest.mark.parametrize("rank", R.FAIL_RANKS)
def test_failing_case_fails_exactly(rank):
    """A literal fp64 replay of the kernel's factorisation meets dd == 0.0 at the stated
    column (>= 1: the break in the middle) for the stated rows and no non-positive pivot
    for the others, whose solution is exact and exactly representable in fp32."""
    f = R.failing_case(rank)
    deg = np.diff(f["indptr"])
    assert deg.min() >= 1 and f["indices"].min() >= 0 and f["indices"].max() < f["n_src"]
    assert len(deg) == R.FAIL_ROWS and f["Y"].shape == (f["n_src"], rank)
    assert ((f["Y"] != 0).sum(1) == 1).all() and np.array_equal(f["Y"], np.round(f["Y"]))
    A, b = R.systems(f["indptr"], f["indices"], f["vals"], f["Y"], 0.0)
    assert np.array_equal(A, np.round(A)) and A.max() <= 16
    for t in range(R.FAIL_ROWS):
        jc = R.cholesky_replay(A[t])
        assert jc == f["fail_col"][t], (t, jc)
        if R.failing_row(t):
            assert jc >= 1 and A[t][jc, jc] == 0.0 and t in f["failing"]
        else:
            assert jc == -1 and t in f["full"]
    assert sorted(set(f["fail_col"][f["failing"]])) == sorted(set(R.fail_columns(rank)))
    X = f["X"]
    assert np.isnan(X[f["failing"]]).all() and np.isfinite(X[f["full"]]).all()
    full = f["full"]
    assert np.array_equal(np.einsum("nab,nb->na", A[full], X[full]), b[full])  # exact
    assert np.array_equal(X[full].astype(np.float32).astype(np.float64), X[full])
    assert np.array_equal(R.exact_ref(f["indptr"], f["indices"], f["vals"], f["Y"], 0.0,
                                      rows=full), X[full])
    # rows that span more than one 32-rating batch at the larger ranks
    assert rank < 33 or deg[full].min() > R.RESCUE_BATCH


def test_failing_and_full_rows_alternate_within_a_workgroup():
    """Every row listed in order: workgroup w walks w, w + 64, w + 128, and both a failing
    row before a full-rank one and the reverse occur in one workgroup."""
    kinds = [R.failing_row(t) for t in range(R.FAIL_ROWS)]
    for w in range(R.RESCUE_GRID):
        walk = kinds[w::R.RESCUE_GRID]
        assert len(walk) == 3 and walk[0] != walk[1] != walk[2]
    assert kinds[0] and not kinds[1]


def test_cholesky_replay_is_a_cholesky():
    rng = np.random.default_rng(1)
    M = rng.standard_normal((40, 9))
    A = M.T @ M
    assert R.cholesky_replay(A) == -1
    A[:, 4] = A[4, :] = 0.0
    assert R.cholesky_replay(A) == 4
    assert R.cholesky_replay(-np.eye(3)) == 0


# ---------------------------------------------------------------- the references
@pytest.mark.parametrize("rank,mode", [(r, m) for r, m in R.GRID_CASES if r in (1, 16, 33, 64, 65, 128)])
def test_exact_ref_agrees_with_the_oracle(rank, mode):
    """exact_ref (fp64, an LU solve) against O.half_sweep (Cholesky, rounded to fp32): they
    agree to fp32 rounding, 2^-24 per entry and so per row."""
    implicit, alpha = R.GRID_MODES[mode]
    c = k2k3_grid_case(rank, implicit)
    X, _ = R.grid_refs(rank, mode)
    assert X.dtype == np.float64 and X.shape == (len(c["indptr"]) - 1, rank)
    Xo = O.half_sweep(c["indptr"], c["indices"], c["vals"], c["Y"], R.REG, implicit, alpha)
    e = R.row_errs(Xo, X)
    assert e.max() <= 2.0 ** -24 * (1 + 1e-6), float(e.max())
    assert rank == 1 or e.max() > 0  # X is not the rounded array itself
    assert rel_row_errs(X.astype(np.float32), Xo).max() <= 2.0 ** -23


@pytest.mark.parametrize("rank", R.SPECIAL_RANKS)
def test_special_refs(rank):
    s = k2k3_special_rows(rank)
    X, _ = R.special_refs(rank)
    for kind in ("nonpositive", "zero"):
        assert np.all(X[s["rows"][kind]] == 0.0)
    last = s["rows"]["last_positive"]
    assert np.linalg.norm(X[last], axis=1).min() > 0
    deg = np.diff(s["indptr"])
    alone = [r for r in last if deg[r] % R.RESCUE_BATCH == 1 and deg[r] > 1]
    assert sorted(deg[alone]) == [33, 65, 129]  # the positive rating alone in the last batch
    Xo = O.half_sweep(s["indptr"], s["indices"], s["vals"], s["Y"], R.REG, True, R.SPECIAL_ALPHA)
    assert R.row_errs(Xo, X).max() <= 2.0 ** -24 * (1 + 1e-6)


def test_packed_yty_layout():
    Y = k2k3_grid_case(3, True)["Y"]
    p = R.packed_yty(Y, 16)
    G = O.yty(Y)
    assert len(p) == 136 and np.isnan(p[6:]).all()
    assert p[:6].tolist() == [G[0, 0], G[1, 0], G[1, 1], G[2, 0], G[2, 1], G[2, 2]]


def test_row_errs_is_absolute_where_the_reference_is_zero():
    e = R.row_errs(np.array([[3.0, 4.0], [1.0, 0.0]]), np.array([[0.0, 0.0], [2.0, 0.0]]))
    assert e.tolist() == [5.0, 0.5]
