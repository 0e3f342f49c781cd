"""GPU parity tests of the fp64 rescue solve (csrc/rescue64.h, rescue64_kernel) on its own,
held to an fp64-grade bar.

Every guard of the K2/K3 kernels sends its difficult rows here, and test_gpu_edges_k2_k3.py
keeps the kernel out on purpose (zero rescued rows), so the rescue is driven directly: after
one sizing call (PHASE_PREP | PHASE_RSCALE: the workspace has its final size, the two count
words are zero) the destination table is prefilled with 7.0, the source table's columns
[rank, ld) are set to NaN (the kernel reads columns [0, k) only), the rows to solve are
written on the list with rescue_ref.write_list, and als_solve_half runs PHASE_RESCUE alone.
ld is ld_for(rank) + 4, so every rank has padding columns.  Implicit calls get the exact
fp64 YtY (rescue_ref.packed_yty), NaN in its padded entries.

Bar: per listed row ||x - ref|| / ||ref|| <= 2^-23 against rescue_ref.exact_ref (fp64, no
rounding to fp32), absolute where ref is zero.  Derived in rescue_ref's docstring: the one
fp32 cast is 2^-24, the fp64 part is held below 2^-30 by the conditioning of every case
(test_rescue_cpu.py), and the reference takes regParam as the ABI carries it, a C float.  A
row above the bar is a finding; the bar is not fitted to a measurement.

  (a) the K2/K3 degree grid (degrees 1 .. 1024 around every multiple of 32, three rows each),
      every rank of K2K3_RANKS, explicit and implicit alpha 4 / 40, every row listed (more
      than kRescueGrid = 64: workgroups walk several rows and reuse their LDS), in ascending
      and in shuffled order: identical bits.
  (b) every third row listed: the others keep their 7.0 bit for bit; a count of 0.
  (c) implicit rows without a positive rating (exactly 0) and with one positive rating alone
      in the last 32-rating batch.
  (d) rescue_ref.failing_case: a pivot of exactly 0.0 in the middle of the factorisation,
      failing and full-rank rows alternating within each workgroup.
  (e) the explicit guards fill the list themselves (ratings 2^-30 of the launch's largest).
      Finding, kept as the code has it: the dual path (rank >= 33, rows of <= dual_limit
      ratings) does not flag such rows and does not need to.  Its window test is on the Gram's
      diagonal only (dual_solve.h: "ratings are not split here"): the ratings enter as the
      fp32 right-hand side of the n x n system, the solve is linear in them, and z is split
      with a scale of its own per row, so a row's relative error does not depend on the size
      of its ratings.  With the dual path on, those rows are therefore absent from the list
      and are held to the fp32-grade path's two bars against the same reference (1e-4, and 8 x
      the fp32 textbook solve's error on the same rows, as test_gpu_edges_k2_k3.py has them),
      so a dual path that went wrong at small ratings would show; with it off (dual=False)
      they are primal light rows and must be listed like every other row.  The anchor row
      carries the launch's largest rating and is never listed (the same two bars).
"""
import numpy as np
import pytest
import torch

import als_mi355x.engine as E
from helpers import K2K3_REG, k2k3_grid_case, k2k3_special_rows, report
import rescue_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = 128


def _t(x, dtype):
    return torch.as_tensor(np.array(x)).to(DEV, dtype)  # a copy: the shared cases are read-only


class Rig:
    """One CSR block on the device (users = destination rows), ready for rescue-only calls:
    the common procedure of the module docstring up to the sizing call."""

    def __init__(self, case, rank, reg, implicit=False, alpha=1.0):
        core = E.ALSCore(case["dst"], case["src"], case["r"], device=DEV, chunk=CHUNK)
        self.block = ub = core.user_block
        np.testing.assert_array_equal(ub.row_ptr.cpu().numpy(), case["indptr"])
        np.testing.assert_array_equal(ub.col.cpu().numpy(), case["indices"])
        np.testing.assert_array_equal(ub.val.cpu().numpy(), case["vals"])
        self.rank, self.reg, self.implicit, self.alpha = rank, reg, implicit, alpha
        self.n_rows = ub.n_light + ub.n_heavy
        self.n_src = core.n_items
        assert self.n_rows == len(case["indptr"]) - 1 and self.n_src == len(case["Y"])
        self.ld = E.ld_for(rank) + 4
        self.Y = torch.zeros((self.n_src, self.ld), dtype=torch.float32, device=DEV)
        self.Y[:, :rank] = _t(case["Y"], torch.float32)
        self.Y_nan = self.Y.clone()
        self.Y_nan[:, rank:] = float("nan")
        self.X = torch.full((self.n_rows, self.ld), 7.0, dtype=torch.float32, device=DEV)
        self.core, self.status = core, core.status
        self.yty = _t(R.packed_yty(case["Y"], E.k_pad(rank)), torch.float64) if implicit else None
        self.ws = E.Workspace(DEV)
        self._call(self.Y, E.PHASE_PREP | E.PHASE_RSCALE)
        assert R.count_words(self.ws) == (0, 0)
        self.ws_bytes = self.ws.buf.numel()

    def _call(self, Y, phases):
        E.solve_half(self.block, Y, self.X, self.rank, self.reg, self.implicit, self.alpha,
                     self.yty, self.status, self.ws, phases)

    def rescue(self, rows):
        """Prefill, list `rows`, run PHASE_RESCUE alone.  Returns (X [n, ld] host, status)."""
        self.X.fill_(7.0)
        self.status.zero_()
        R.write_list(self.ws, rows, self.rank, self.n_src, self.n_rows)
        assert R.count_words(self.ws) == (len(rows), 0)
        self._call(self.Y_nan, E.PHASE_RESCUE)
        torch.cuda.synchronize()
        assert self.ws.buf.numel() == self.ws_bytes  # the sizing call sized it
        return self.X.cpu().numpy(), int(self.status.item())


def _assert_bar(name, X, ref, rows, rank, conds, deg, extra=None):
    e = R.row_errs(X[rows, :rank], ref[rows])
    worst = int(np.asarray(rows)[e.argmax()])
    out = dict(max_rel_err=float(e.max()), bar=R.BAR, worst_row=worst, worst_degree=int(deg[worst]),
               rank_cond_eps=R.cond_term(rank, conds[rows]), list_length=len(rows),
               **(extra or {}))
    print(f"{name}: {out}")
    report(name, out)
    assert e.max() <= R.BAR, (float(e.max()), worst)
    return e


# ---------------------------------------------------------------- (a) the degree grid
@pytest.mark.parametrize("rank,mode", R.GRID_CASES)
def test_degree_grid_every_row_listed(rank, mode):
    """Row lengths around every multiple of kRescueBatch = 32 (tail batches of 1, 31, 32
    ratings), every rank (packed_ij at every triangle size), lists longer than the grid."""
    implicit, alpha = R.GRID_MODES[mode]
    case = k2k3_grid_case(rank, implicit)
    ref, conds = R.grid_refs(rank, mode)
    rig = Rig(case, rank, K2K3_REG, implicit, alpha)
    rows = np.arange(rig.n_rows)
    assert len(rows) > R.RESCUE_GRID
    X1, st1 = rig.rescue(rows)
    words1 = R.count_words(rig.ws)
    X2, st2 = rig.rescue(np.random.default_rng(100 + rank).permutation(rows))
    deg = np.diff(case["indptr"])
    _assert_bar(f"rescue64[grid,rank={rank},{mode}]", X1, ref, rows, rank, conds, deg)
    assert np.all(X1[:, rank:] == 0.0), "padding columns [rank, ld) must be exactly 0"
    assert np.array_equal(X1.view(np.uint32), X2.view(np.uint32)), \
        f"list order changed rows {np.nonzero((X1 != X2).any(1))[0][:10]}"
    assert words1 == (0, 0) and R.count_words(rig.ws) == (0, 0)
    assert st1 == 0 and st2 == 0


# ---------------------------------------------------------------- (b) a partial list
@pytest.mark.parametrize("rank,mode", R.PARTIAL_CASES)
def test_partial_list_leaves_other_rows_alone(rank, mode):
    implicit, alpha = R.GRID_MODES[mode]
    case = k2k3_grid_case(rank, implicit)
    ref, conds = R.grid_refs(rank, mode)
    rig = Rig(case, rank, K2K3_REG, implicit, alpha)
    rows = np.arange(0, rig.n_rows, 3)
    X, st = rig.rescue(rows)
    _assert_bar(f"rescue64[partial,rank={rank},{mode}]", X, ref, rows, rank, conds,
                np.diff(case["indptr"]))
    assert st == 0 and R.count_words(rig.ws) == (0, 0)
    assert np.all(X[rows, rank:] == 0.0)
    others = np.setdiff1d(np.arange(rig.n_rows), rows)
    seven = np.float32(7.0).view(np.uint32)
    assert np.all(X[others].view(np.uint32) == seven), "a row that was not listed was written"
    # a count of 0 writes nothing and leaves both words zero
    X0, st0 = rig.rescue(np.zeros(0, np.int64))
    assert np.all(X0.view(np.uint32) == seven) and st0 == 0
    assert R.count_words(rig.ws) == (0, 0)


# ---------------------------------------------------------------- (c) implicit special rows
@pytest.mark.parametrize("rank", R.SPECIAL_RANKS)
def test_implicit_special_rows(rank):
    """numExplicits = 0 and a zero right-hand side: exactly 0.0.  One positive rating alone
    in the last batch of a row of 33, 65 and 129 ratings: what a count of positive ratings
    taken from the wrong batches, or a right-hand side missing its tail, gets wrong."""
    s = k2k3_special_rows(rank)
    ref, conds = R.special_refs(rank)
    rig = Rig(s, rank, K2K3_REG, True, R.SPECIAL_ALPHA)
    rows = np.arange(rig.n_rows)
    X, st = rig.rescue(rows)
    deg = np.diff(s["indptr"])
    e = _assert_bar(f"rescue64[special,rank={rank}]", X, ref, rows, rank, conds, deg)
    assert st == 0 and R.count_words(rig.ws) == (0, 0)
    assert np.all(X[:, rank:] == 0.0)
    for kind in ("nonpositive", "zero"):
        assert np.all(ref[s["rows"][kind]] == 0.0)
        assert np.all(X[s["rows"][kind]] == 0.0), kind
    last = s["rows"]["last_positive"]
    assert {33, 65} <= set(deg[last].tolist())
    assert np.linalg.norm(ref[last], axis=1).min() > 0 and e[last].max() <= R.BAR


# ---------------------------------------------------------------- (d) the failure path
@pytest.mark.parametrize("rank", R.FAIL_RANKS)
def test_failed_pivot_mid_factorisation(rank):
    """reg = 0, one-hot integer sources: the failing rows' pivot is exactly 0.0 at a column
    >= 1 (test_rescue_cpu.py replays it), the full-rank rows' A is diagonal and their
    solution exact.  The two kinds alternate within every workgroup's walk, so fail_s and
    the LDS image must be fresh for the row after a failed one."""
    f = R.failing_case(rank)
    rig = Rig(f, rank, 0.0)
    rows = np.arange(rig.n_rows)
    X, st = rig.rescue(rows)
    failing, full = f["failing"], f["full"]
    report(f"rescue64[failing,rank={rank}]",
           dict(status=st, failing_rows=len(failing), list_length=len(rows),
                max_abs_err_full_rows=float(np.abs(X[full, :rank] - f["X"][full]).max()),
                rank_cond_eps=rank * 16.0 * 2.0 ** -53))
    assert st - 1 in failing, st
    assert np.all(X[failing] == 0.0), "a failed row must be zero in all ld columns"
    assert np.array_equal(X[full, :rank], f["X"][full].astype(np.float32))
    assert np.all(X[full, rank:] == 0.0)
    assert R.count_words(rig.ws) == (0, 0)
    with pytest.raises(RuntimeError, match=rf"Cholesky failed .* dense row {st - 1}\b"):
        rig.core.check_status()


# ---------------------------------------------------------------- (e) the guards fill the list
@pytest.mark.parametrize("rank,dual", R.GUARD_CASES)
def test_explicit_guards_fill_the_list(rank, dual):
    """Every rating 2^-30 of the anchor's: the primal light rows (launch 1) and the heavy
    rows (launch 2) miss the rating window and must be listed, each exactly once; the list is
    read where rescue_ref.list_region says it is, which checks that helper against the
    product.  The dual-path rows: see the module docstring."""
    g = R.guard_case(rank)
    ref, conds = R.guard_refs(rank)
    core = E.ALSCore(g["dst"], g["src"], g["r"], device=DEV, chunk=CHUNK)
    ub = core.user_block
    np.testing.assert_array_equal(ub.row_ptr.cpu().numpy(), g["indptr"])
    np.testing.assert_array_equal(ub.col.cpu().numpy(), g["indices"])
    np.testing.assert_array_equal(ub.val.cpu().numpy(), g["vals"])
    core.init_factors(rank, seed=3)
    core.V[:, :rank] = _t(g["Y"], torch.float32)
    n_rows, n_src, anchor = ub.n_light + ub.n_heavy, core.n_items, g["anchor"]
    deg = np.diff(g["indptr"])
    assert n_rows == anchor + 1 and ub.n_heavy == int((deg > CHUNK).sum()) > 0
    dual_rows, unlisted = R.guard_unlisted(rank, dual)
    assert len(dual_rows) == (ub.n_dual(rank) if dual else 0)
    assert (anchor in dual_rows) == (dual and E.dual_limit(rank) > 0)
    e_textbook = R.guard_textbook_errs(rank, unlisted)
    expected = np.setdiff1d(np.arange(n_rows), unlisted)
    assert (deg[expected] <= CHUNK).any() and (deg[expected] > CHUNK).any()

    core.U.fill_(7.0)
    core.status.zero_()
    a = (ub, core.V, core.U, rank, K2K3_REG, False, 1.0, None, core.status, core.ws)
    E.solve_half(*a, E.PHASE_ALL & ~E.PHASE_RESCUE, dual=dual)
    listed = R.read_list(core.ws, rank, n_src, n_rows)
    assert R.count_words(core.ws) == (len(listed), 0)
    assert len(listed) == len(expected) and np.array_equal(np.sort(listed), expected), \
        (np.setdiff1d(expected, listed)[:10], np.setdiff1d(listed, expected)[:10])
    U0 = core.U.cpu().numpy()
    assert np.all(U0[expected] == 7.0), "a listed row was written before the rescue"
    ld = core.V.shape[1]
    if ld > rank:
        core.V[:, rank:] = float("nan")
    E.solve_half(*a, E.PHASE_RESCUE, dual=dual)
    torch.cuda.synchronize()
    assert R.count_words(core.ws) == (0, 0)
    core.check_status()
    U = core.U.cpu().numpy()
    assert not np.any(U == 7.0), "a destination entry was never written"
    assert np.all(U[:, rank:] == 0.0)
    e_fp32 = R.row_errs(U[unlisted, :rank], ref[unlisted])
    _assert_bar(f"rescue64[guards,rank={rank},dual={int(dual)}]", U, ref, expected, rank, conds,
                deg, dict(dual_rows=len(dual_rows), heavy_rows=ub.n_heavy,
                     unlisted_rows_max_rel_err=float(e_fp32.max()),
                     unlisted_rows_textbook_max_rel_err=float(e_textbook.max())))
    # the fp32-grade path's own bars (test_gpu_edges_k2_k3.py): 1e-4, and 8 x the fp32
    # textbook solve of the same rows (<= 4.8e-6 here, test_rescue_cpu.py)
    assert e_fp32.max() <= 1e-4, float(e_fp32.max())
    assert e_fp32.max() <= R.YARDSTICK_FACTOR * e_textbook.max(), \
        (float(e_fp32.max()), float(e_textbook.max()))
