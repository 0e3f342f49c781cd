"""GPU edge parity tests for the K2/K3 solve kernels (csrc/gram_solve.hip) at exact task
lengths and at the ranks just inside every instantiation, against the fp64 oracle.

The Gram loops change behaviour with the task length n = pe - pb: 32-rating MFMA steps
(nsteps = ceil(n / 32), the ratings past the end pointing at the zero row or carrying
column -1), 64-rating staging blocks prefetched one block ahead (rhs partials folded on
odd steps and once after the loop), two steps in flight on the explicit rank 65-128 path,
the implicit refinement's second pass in batches of 64 with its count of ratings > 0, and
the light / heavy boundary (n == chunk is a light row, n == chunk + 1 a heavy row whose
last task holds one rating).  Random masks meet these lengths only by chance; here every
destination row has a stated degree (helpers.degree_rows):

  * the degree grid K2K3_DEGREES (+ rank - 1, rank, rank + 1, each three times) x ranks
    1, 3, 15, 16 | 17, 31, 32 | 33, 47, 63, 64 | 65, 97, 127, 128 x chunk 128 and 512 x
    explicit (dual on / off) and implicit (alpha 4 and 40);
  * implicit rows with no positive rating, all-zero ratings, and one positive rating in
    the row's last position;
  * the production task lengths (chunk_for: 4096 / 16384) around the light / heavy
    boundary, and two-segment schedules whose early segment has 0 .. 130 of 130 ratings.

Bars.  (1) per row ||x - ref|| / ||ref|| <= 1e-4, the project's K2/K3 bar.  (2) per case
max GPU error <= 8 x max error of the fp32 textbook solve of the same rows
(helpers.fp32_textbook_half_sweep: the split-f16 product carries ~2^-21 against 2^-24 for
an fp32 product; test_k2k3_edges_cpu.py pins the yardstick to (0, 1.25e-5]).  (3) zero
rows in the fp64 rescue list after the launches: a rescued row is the reference's own
arithmetic and would hide a broken fp32 tail (unit-norm factors at regParam 0.1 miss all
three rescue tests: trace(G) / (lambda n) = 10, operands at the launch maximum, fp64
pivot spreads <= 11 of 32 explicit and < 4 of 8 implicit, test_k2k3_edges_cpu.py).  The
rescue kernel itself is held to its own, fp64-grade bar on these same inputs in
test_gpu_rescue64.py.  The destination table is prefilled with 7.0: the
padding columns [rank, ld) must come back exactly 0 and no 7.0 may survive.
"""
import numpy as np
import pytest
import torch

import als_mi355x.engine as E
from oracle import als_oracle as O
from helpers import (K2K3_N_SRC, K2K3_RANKS, K2K3_REG, degree_rows, fp32_textbook_half_sweep,
                     k2k3_grid_case, k2k3_grid_refs, k2k3_special_rows, rel_row_errs, report,
                     unit_source_factors)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAUNCHES = E.PHASE_ALL & ~E.PHASE_RESCUE
YARDSTICK_FACTOR = 8.0  # 2^-21 / 2^-24


def _t(x, dtype):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV, dtype)


def _exact_rel_errs(x, ref):
    """Per-row ||x - ref|| / ||ref|| with no floor; absolute where ref is zero."""
    x = np.asarray(x, np.float64)
    ref = np.asarray(ref, np.float64)
    nr = np.linalg.norm(ref, axis=1)
    e = np.linalg.norm(x - ref, axis=1) / np.where(nr > 0, nr, 1.0)
    e[nr == 0] = np.linalg.norm(x[nr == 0], axis=1)
    return e


def _rescue_count(core):
    torch.cuda.synchronize()
    return int(core.ws.buf[8:12].view(torch.int32).item())


def _core_of(case, rank, chunk):
    """ALSCore of (dst = users, src = items) whose user block is the case's CSR, the item
    factors set to the case's Y."""
    core = E.ALSCore(case["dst"], case["src"], case["r"], device=DEV, chunk=chunk)
    ub = core.user_block
    np.testing.assert_array_equal(ub.row_ptr.cpu().numpy(), case["indptr"])
    np.testing.assert_array_equal(ub.col.cpu().numpy(), case["indices"])
    np.testing.assert_array_equal(ub.val.cpu().numpy(), case["vals"])
    core.init_factors(rank, seed=3)
    core.V[:, :rank] = _t(case["Y"], torch.float32)
    return core


def _solve_users(core, rank, implicit, alpha, dual=True):
    """One user half-sweep into a table prefilled with 7.0, the fp64 rescue held back
    until its list has been counted.  Returns (U [n, rank], rows the launches flagged)."""
    ub = core.user_block
    yty = E.compute_yty(core.V, core.n_items, rank, core.ws_yty) if implicit else None
    core.U.fill_(7.0)
    core.status.zero_()
    E.solve_half(ub, core.V, core.U, rank, K2K3_REG, implicit, alpha, yty, core.status, core.ws,
                 LAUNCHES, dual=dual)
    rescued = _rescue_count(core)
    E.solve_half(ub, core.V, core.U, rank, K2K3_REG, implicit, alpha, yty, core.status, core.ws,
                 E.PHASE_RESCUE, dual=dual)
    assert _rescue_count(core) == 0
    core.check_status()
    U = core.U.cpu().numpy()
    assert np.all(U[:, rank:] == 0.0), "padding columns [rank, ld) must be exactly 0"
    if rescued == 0:
        assert not np.any(U == 7.0), "a destination entry was never written"
    return U[:, :rank], rescued


def _check(name, U, rescued, X_ref, e_textbook, deg, extra=None):
    e = rel_row_errs(U, X_ref)
    ratio = float(e.max() / e_textbook.max())
    per_degree = {str(int(d)): float(f"{e[deg == d].max():.3g}") for d in np.unique(deg)}
    print(f"{name}: max err {e.max():.3g} (deg {int(deg[e.argmax()])}), textbook "
          f"{e_textbook.max():.3g}, ratio {ratio:.3g}, rescued {rescued}")
    report(name, dict(max_rel_err=float(e.max()), worst_degree=int(deg[e.argmax()]),
                      textbook_max_rel_err=float(e_textbook.max()), yardstick_ratio=ratio,
                      rescued_rows=rescued, per_degree=per_degree, **(extra or {})))
    assert rescued == 0, f"{rescued} rows went to the fp64 rescue"
    assert e.max() <= 1e-4, (float(e.max()), int(deg[e.argmax()]))
    assert e.max() <= YARDSTICK_FACTOR * e_textbook.max(), (ratio, int(deg[e.argmax()]))


# ---------------------------------------------------------------- 1. the degree grid
_CORES = {}


def _grid_core(rank, implicit, chunk):
    key = (rank, implicit)
    if key not in _CORES:
        _CORES[key] = _core_of(k2k3_grid_case(rank, implicit), rank, chunk)
    core = _CORES[key]
    core.rechunk(chunk)
    return core


MODES = {"explicit_dual": (False, 1.0, True), "explicit_primal": (False, 1.0, False),
         "implicit_a4": (True, 4.0, True), "implicit_a40": (True, 40.0, True)}
GRID = [(rank, mode) for rank in K2K3_RANKS for mode in MODES
        if mode != "explicit_primal" or E.dual_limit(rank) > 0]  # below rank 33: no dual path


@pytest.mark.parametrize("chunk", [128, 512])
@pytest.mark.parametrize("rank,mode", GRID)
def test_degree_grid(rank, mode, chunk):
    """Every degree of the grid through every instantiation: CN = 1 (ranks 1-16), CN = 2
    (17-32), CN = 4 (33-64) and the one-wavefront kernels (65-128).  At chunk 128 every
    degree >= 129 is a heavy row whose last task has 1, 31, 32, 33, 63, 64, 65 ... ratings
    or exactly full tasks (256, 384, 512, 1024); at chunk 512 the same degrees are light
    rows of 1-16 steps and 1-8 staging blocks, and 513, 769, 1024 are the chunk + 1 and
    full-task cases.  No row may reach the fp64 rescue."""
    implicit, alpha, dual = MODES[mode]
    case = k2k3_grid_case(rank, implicit)
    X_ref, e_tb = k2k3_grid_refs(rank, implicit, alpha)
    core = _grid_core(rank, implicit, chunk)
    ub = core.user_block
    deg = np.diff(case["indptr"])
    assert ub.chunk == chunk and ub.n_heavy == int((deg > chunk).sum())
    assert ub.n_light == int((deg <= chunk).sum()) and (deg == chunk + 1).sum() >= 3
    if not implicit:
        assert ub.n_dual(rank) == int((deg <= E.dual_limit(rank)).sum()) * (E.dual_limit(rank) > 0)
    U, rescued = _solve_users(core, rank, implicit, alpha, dual)
    _check(f"k2k3_edges[grid,rank={rank},chunk={chunk},{mode}]", U, rescued, X_ref, e_tb, deg)


# ---------------------------------------------------------------- 2. special implicit rows
@pytest.mark.parametrize("chunk", [64, 512])
@pytest.mark.parametrize("rank", [16, 32, 64, 128])
def test_implicit_rows_without_positive_ratings(rank, chunk):
    """Implicit rows the random data meets only by chance (helpers.k2k3_special_rows),
    degrees 1, 32, 33, 64, 65, 129, alpha 4; at chunk 64 the rows of 65 and 129 ratings are
    heavy rows whose last task is their last rating alone.  Rows with no rating > 0 have
    numExplicits = 0 (no lambda n term) and a zero right-hand side: the solution is
    exactly zero, as the oracle's.  The rows whose only positive rating is their last are
    what a short count of ratings > 0 (or a right-hand side missing its last block) would
    get wrong: per row against the oracle, no norm floor."""
    s = k2k3_special_rows(rank)
    alpha = 4.0
    X_ref = O.half_sweep(s["indptr"], s["indices"], s["vals"], s["Y"], K2K3_REG, True, alpha)
    core = _core_of(s, rank, chunk)
    deg = np.diff(s["indptr"])
    assert core.user_block.n_heavy == int((deg > chunk).sum())
    U, rescued = _solve_users(core, rank, True, alpha)
    assert int(core.status.item()) == 0
    e = _exact_rel_errs(U, X_ref)
    out = {"rescued_rows": rescued}
    for kind, rows in s["rows"].items():
        out[kind] = {str(int(deg[r])): float(e[r]) for r in rows}
    out["other_rows_max"] = float(np.delete(e, sum(s["rows"].values(), [])).max())
    print(f"k2k3_edges[special,rank={rank},chunk={chunk}]: {out}")
    report(f"k2k3_edges[special,rank={rank},chunk={chunk}]", out)
    assert rescued == 0
    for kind in ("nonpositive", "zero"):
        rows = s["rows"][kind]
        assert np.all(X_ref[rows] == 0.0)
        assert np.all(U[rows] == 0.0), (kind, np.abs(U[rows]).max(axis=1))
    assert np.linalg.norm(X_ref[s["rows"]["last_positive"]], axis=1).min() > 0
    assert e.max() <= 1e-4, (float(e.max()), int(deg[e.argmax()]))


# ---------------------------------------------------------------- 3. production task lengths
@pytest.mark.parametrize("implicit", [False, True])
@pytest.mark.parametrize("rank", [16, 64, 128])
def test_production_chunk_boundary(rank, implicit):
    """The light / heavy boundary and a one-rating last task at the task lengths the fits
    use (chunk_for: 4096, 16384 for explicit rank 128): rows of chunk - 1, chunk (the
    longest fp32 sum one task holds, light), chunk + 1 (twice: 2 chunk + 1 does not fit
    n_src = chunk + 40), chunk + 33 and n_src ratings."""
    chunk = E.chunk_for(rank, implicit)
    assert chunk == (16384 if rank == 128 and not implicit else 4096)
    n_src, alpha = chunk + 40, 4.0
    degrees = [chunk - 1, chunk, chunk + 1, chunk + 33]
    degrees.append(2 * chunk + 1 if 2 * chunk + 1 <= n_src else chunk + 1)
    dst, src, r = degree_rows(degrees, n_src, seed=rank, ratings="signed" if implicit else "stars")
    indptr, indices, vals = O.csr_build(dst, src, r, len(degrees) + 1)
    case = dict(dst=dst, src=src, r=r, indptr=indptr, indices=indices, vals=vals,
                Y=unit_source_factors(n_src, rank, seed=4000 + rank))
    args = (indptr, indices, vals, case["Y"], K2K3_REG, implicit, alpha)
    X_ref = O.half_sweep(*args)
    e_tb = rel_row_errs(fp32_textbook_half_sweep(*args, yty=O.yty(case["Y"]) if implicit else None),
                        X_ref)
    assert 0 < YARDSTICK_FACTOR * e_tb.max() <= 1e-4
    core = _core_of(case, rank, chunk)
    ub = core.user_block
    assert (ub.n_light, ub.n_heavy, ub.n_chunks) == (2, 4, 8)
    U, rescued = _solve_users(core, rank, implicit, alpha)
    _check(f"k2k3_edges[production,rank={rank},chunk={chunk},imp={int(implicit)}]", U, rescued,
           X_ref, e_tb, np.diff(indptr))


SEGMENT_EARLY = (0, 1, 32, 33, 64, 65, 129, 130)


def _two_segment_ratings(rank, implicit, n_src, cut, n):
    """(early, dst, src, r): two rows of n ratings per entry of SEGMENT_EARLY, the first
    early[j] of them from source ids below `cut`, plus one row rating every source id."""
    rng = np.random.default_rng(100 + rank)
    early = list(SEGMENT_EARLY) * 2
    src = [np.concatenate([rng.choice(cut, e, replace=False),
                           cut + rng.choice(n_src - cut, n - e, replace=False)]) for e in early]
    src.append(np.arange(n_src))  # every source id rated: dense ids = ids, early ones first
    dst = np.repeat(np.arange(len(src)), [len(s) for s in src]).astype(np.int32)
    src = np.concatenate(src).astype(np.int32)
    r = (rng.integers(1, 11, len(src)) / 2 - (2.5 if implicit else 0.0)).astype(np.float32)
    return early, dst, src, r


@pytest.mark.parametrize("implicit", [False, True])
@pytest.mark.parametrize("rank", [16, 64, 128])
def test_two_segment_edges(rank, implicit):
    """The two-segment schedule (solve_half_split, chunk 64) on rows of 130 ratings whose
    early segment has 0, 1, 32, 33, 64, 65, 129, 130 of them: an empty early and an empty
    late segment, segments of exactly one task and of one task plus one rating.  The not
    yet arrived source rows hold NaN during the early call.  Against the one-call solve
    and the fp64 oracle, with test_two_segment_half_sweep's bars."""
    n_src, cut, n, chunk, alpha = 512, 256, 130, 64, 2.0
    early, dst, src, r = _two_segment_ratings(rank, implicit, n_src, cut, n)
    core = E.ALSCore(dst, src, r, device=DEV, chunk=chunk)
    assert core.iidx.n == n_src and core.uidx.n == len(early) + 1
    core.init_factors(rank, seed=7)
    core.V[:, :rank] = _t(unit_source_factors(n_src, rank, seed=5000 + rank), torch.float32)
    ub = core.user_block
    rp, col = ub.row_ptr.cpu().numpy(), ub.col.cpu().numpy()
    seg = rp[:-1] + np.array(early + [cut])
    assert (col[np.arange(len(col)) < np.repeat(seg, np.diff(rp))] < cut).all()
    assert (col[np.arange(len(col)) >= np.repeat(seg, np.diff(rp))] >= cut).all()
    sched = E.split_schedule(ub, _t(seg, torch.int64), cut, chunk=chunk)
    # tasks: ceil(e / 64) early and ceil((130 - e) / 64) late per row, 4 + 4 of the full row
    assert sched.early[3] == 2 * sum(-(-e // chunk) for e in SEGMENT_EARLY) + cut // chunk
    assert sched.late[3] == 2 * sum(-(-(n - e) // chunk) for e in SEGMENT_EARLY) + cut // chunk
    yty = E.compute_yty(core.V, n_src, rank, core.ws_yty) if implicit else None
    core.status.zero_()
    E.solve_half(ub, core.V, core.U, rank, K2K3_REG, implicit, alpha, yty, core.status, core.ws,
                 dual=False)
    U1 = core.U[:, :rank].cpu().numpy()
    Y0 = core.V[:, :rank].cpu().numpy()
    ws = E.Workspace(DEV)
    Us = torch.full_like(core.U, 7.0)
    held = core.V[cut:].clone()
    core.V[cut:] = float("nan")
    E.solve_half_split(ub, sched, "early", core.V, Us, rank, K2K3_REG, implicit, alpha, yty,
                       core.status, ws)
    core.V[cut:] = held
    E.solve_half_split(ub, sched, "late", core.V, Us, rank, K2K3_REG, implicit, alpha, yty,
                       core.status, ws)
    torch.cuda.synchronize()
    core.check_status()
    Us = Us.cpu().numpy()
    assert np.all(Us[:, rank:] == 0.0) and not np.any(Us == 7.0)
    X_ref = O.half_sweep(rp, col, ub.val.cpu().numpy(), Y0, K2K3_REG, implicit, alpha)
    e_one = _exact_rel_errs(Us[:, :rank], U1)
    e_ref = _exact_rel_errs(Us[:, :rank], X_ref)
    by_early = {str(e): float(max(e_ref[j], e_ref[j + len(SEGMENT_EARLY)]))
                for j, e in enumerate(SEGMENT_EARLY)}
    print(f"k2k3_edges[two_segment,rank={rank},imp={int(implicit)}]: vs one call "
          f"{e_one.max():.3g}, vs oracle {e_ref.max():.3g} {by_early}")
    report(f"k2k3_edges[two_segment,rank={rank},imp={int(implicit)}]",
           {"vs_one_call": float(e_one.max()), "vs_oracle": float(e_ref.max()),
            "vs_oracle_by_early_ratings": by_early, "early_tasks": sched.early[3],
            "late_tasks": sched.late[3]})
    assert e_ref.max() <= (1e-5 if implicit and rank <= 64 else 1e-4), float(e_ref.max())
    assert e_one.max() <= 1e-4, float(e_one.max())
