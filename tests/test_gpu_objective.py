"""The training objective on the GPU (K10: als_objective_side, als_gram_dot_f64,
ALSCore.objective, fit's objective_every / tol, the ml / mllib surfaces) against the numpy fp64
reference tests/objective_ref.py.

Bars.  Kernel against reference: |got - want| <= 1e-12 * scale, scale = the sum of the
absolute values of everything added — at most ~1e4 fp64 terms, each good to an ulp (1.1e-16),
on identical fp32 inputs.  Grams: 1e-13 relative to sum_rows |f_a f_b| per entry (the products
of two fp32 values are exact in fp64; at most 1000 additions).  The invariant: a half-sweep
solves every row's normal equations, so L_after <= L_before (1 + 1e-9): the solver's row
solution is off by a small delta, the excess delta^T A delta is second order in it, and the
fp64 evaluation noise is ~1e-13.  The CPU oracle's own half-sweeps lower L by at least 0.5 % at
every step of this protocol (tests/test_objective_cpu.py), far inside that bound.
"""
import functools
import types

import numpy as np
import pytest
import torch

import objective_ref as R
from als_mi355x import engine as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
RANKS = (1, 16, 17, 33, 64, 65, 128)
N_U, N_I = 37, 23
MODES = ((False, 1.0), (True, 0.01), (True, 40.0))   # (implicit, alpha)


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype).contiguous()


def _table(F):
    """An fp32 [n, k] host table as the engine stores it: [n, ld_for(k)], padding zero."""
    n, k = F.shape
    T = torch.zeros((n, E.ld_for(k)), dtype=torch.float32, device=DEV)
    T[:, :k] = _dev(F, torch.float32)
    return T


def _ws():
    return E.Workspace(torch.device(DEV))


@functools.lru_cache(maxsize=None)
def small_problem():
    """37 x 23, ~300 ratings with r < 0, r = 0, a duplicate pair, and user 0 all <= 0; every
    user and item rated (dense row = id)."""
    rng = np.random.default_rng(7)
    u = np.concatenate([np.arange(N_U), rng.integers(0, N_U, 263)])
    i = np.concatenate([np.arange(N_I), rng.integers(0, N_I, 277)])
    r = rng.integers(-4, 11, 300).astype(np.float32) / 2
    r[u == 0] = -np.abs(r[u == 0])
    u, i, r = np.append(u, u[-1]), np.append(i, i[-1]), np.append(r, np.float32(1.5))
    assert (r < 0).any() and (r == 0).any() and not (r[u == 0] > 0).any()
    return u.astype(np.int32), i.astype(np.int32), r


@functools.lru_cache(maxsize=None)
def small_core():
    return E.ALSCore(*small_problem(), device=DEV)


def _set_factors(core, rank, seed):
    rng = np.random.default_rng(seed)
    U = rng.normal(0, 0.5, (core.n_users, rank)).astype(np.float32)
    V = rng.normal(0, 0.5, (core.n_items, rank)).astype(np.float32)
    core.init_factors(rank, U0=U)
    core.V[:, :rank] = _dev(V, torch.float32)
    return U, V


def _close(got, want, what):
    tol = 1e-12 * want["scale"]
    for key in ("objective", "data", "reg", "scale"):
        print(f"K10 {what} {key}: got {got[key]!r} want {want[key]!r} tol {tol:.3e}")
        assert abs(got[key] - want[key]) <= tol, (what, key, got[key], want[key], tol)
    assert (got["n"], got["n_positive"]) == (want["n"], want["n_positive"]), what
    assert sorted(got) == sorted(want)


# ------------------------------------------------------------------ kernel vs reference
@pytest.mark.parametrize("rank", RANKS)
def test_objective_matches_reference(rank):
    core = small_core()
    u, i, r = small_problem()
    U, V = _set_factors(core, rank, seed=rank)
    for implicit, alpha in MODES:
        got = core.objective(0.1, implicit, alpha)
        _close(got, R.objective(u, i, r, U, V, 0.1, implicit, alpha), f"k={rank} {implicit} {alpha}")
        assert core.objective(0.1, implicit, alpha) == got      # bit-identical second call
    assert R.objective(u, i, r, U, V, 0.1, True, 40.0)["n_positive"] < len(r)


def test_padding_columns_are_masked_in_the_rating_pass():
    core = small_core()
    u, i, r = small_problem()
    U, V = _set_factors(core, 17, seed=3)
    want = core.objective(0.1, True, 40.0)
    core.U[:, 17:] = float("nan")
    core.V[:, 17:] = 1e30
    assert core.objective(0.1, True, 40.0) == want
    core.U[:, 17:] = 0
    core.V[:, 17:] = 0


# ------------------------------------------------------------------ span edges
def _lens_to_rows(lens):
    return np.repeat(np.arange(len(lens)), lens)


def _span_cases():
    S = E.objective_span()
    light = [3, 1, 7, 2, 5]
    return S, {
        "heavy row of 3S+5": light + [3 * S + 5] + light,
        "row ends on a boundary": [5, S - 5, 9, 4],
        "row starts on a boundary": [S - 2, 2, S // 2, 6],
        "rows cut at every group": [S // 16] * 16 + [1],
        "nnz = S": [S - 10, 10],
        "nnz = S - 1": [S - 11, 10],
        "nnz = S + 1": [S - 10, 11],
        "one rating": [1],
        # empty rows: equal row_ptr entries under the binary search, and the row walk's
        # `while (ee >= next ...)` stepping over more than one row (X rows are scaled apart
        # below, so a mis-stepped row shows in reg)
        "three empty rows first": [0, 0, 0] + light + [S, 4],
        "empty rows on a group and on a span boundary": [S // 16, 0, 0, 5, S - S // 16 - 5,
                                                         0, 0, 0, 7],
        "empty rows last": [5, S - 5, 9, 0, 0],
        "S - 1, two empty rows, 1": [S - 1, 0, 0, 1],
    }


def _check_span_cases(cases, rank, implicit, alpha):
    ws = _ws()
    for name, lens in cases.items():
        rng = np.random.default_rng(len(lens) + sum(lens))
        rows = _lens_to_rows(lens)
        n_r, n_c = len(lens), 29
        cols = rng.integers(0, n_c, len(rows))
        cols[: min(n_c, len(rows))] = np.arange(min(n_c, len(rows)))
        n_c = int(cols.max()) + 1
        vals = rng.integers(-2, 11, len(rows)).astype(np.float32) / 2
        X = rng.normal(0, 0.5, (n_r, rank)).astype(np.float32)
        Y = rng.normal(0, 0.5, (n_c, rank)).astype(np.float32)
        if 0 in lens:                      # row j scaled by 1 + j: every |x_j|^2 its own size
            X *= (1 + np.arange(n_r, dtype=np.float32))[:, None]
        Xd, Yd = _table(X), _table(Y)
        got = {}
        # the side whose rows are `rows`, then the transposed side (rows = cols)
        for side, (a, b, A, B, Ad, Bd, n_a, n_b) in {
                "row side": (rows, cols, X, Y, Xd, Yd, n_r, n_c),
                "col side": (cols, rows, Y, X, Yd, Xd, n_c, n_r)}.items():
            ptr, c, v = R.csr(a, b, vals, n_a)
            blk = types.SimpleNamespace(row_ptr=_dev(ptr, torch.int64), col=_dev(c, torch.int32),
                                        val=_dev(v, torch.float32), nnz=len(v), n_rows=n_a)
            out = E.objective_side(blk, Ad, Bd, n_b, rank, implicit, alpha, ws).tolist()
            want = R.side(a, b, vals, A, B, implicit, alpha)
            tol = 1e-12 * (want[1] + want[2])
            print(f"K10 span {name} / {side} k={rank}: got {out} want {want} tol {tol:.3e}")
            assert out[3:] == want[3:], (name, side)
            for g, w_ in zip(out[:3], want[:3]):
                assert abs(g - w_) <= tol, (name, side, out, want)
            again = E.objective_side(blk, Ad, Bd, n_b, rank, implicit, alpha, ws).tolist()
            assert again == out, (name, side)
            reg_only = E.objective_side(blk, Ad, None, n_b, rank, implicit, alpha, ws).tolist()
            assert reg_only == [0.0, 0.0] + out[2:], (name, side)
            got[side] = out
        # both sides hold the same ratings: the data term agrees
        tol = 1e-12 * got["row side"][1]
        assert abs(got["row side"][0] - got["col side"][0]) <= tol, name


@pytest.mark.parametrize("rank,implicit,alpha", [(17, False, 1.0), (17, True, 40.0),
                                                 (128, True, 0.01)])
def test_span_edges_on_both_sides(rank, implicit, alpha):
    S, cases = _span_cases()
    assert S % 16 == 0
    _check_span_cases(cases, rank, implicit, alpha)


@pytest.mark.parametrize("implicit", [False, True])
def test_more_than_256_partial_blocks(implicit):
    """257 S + 1 ratings: 258 blocks of partials, the last holding one rating, so the strided
    loop of the final sum (sum_partials_kernel) makes a second pass for threads 0 and 1."""
    S = E.objective_span()
    lens = [S // 4 + 3] * 1000
    lens.append(257 * S + 1 - sum(lens))
    assert lens[-1] > 0 and sum(lens) == 257 * S + 1
    _check_span_cases({"nnz = 257 S + 1": lens}, 8, implicit, 40.0 if implicit else 1.0)


@pytest.mark.parametrize("rank,implicit,alpha", [(17, False, 1.0), (128, True, 40.0)])
def test_out_of_range_columns_add_no_data_term(rank, implicit, alpha):
    """col = -1, n_cols and INT32_MAX at 5 % of the ratings: no data term and no read of Y
    (include/als_hip.h), while the rating still counts in n, n_positive and reg: the kernel
    counts before the range test.  Only the side whose columns they are can hold them (a CSR
    has no row outside its range)."""
    S = E.objective_span()
    rng = np.random.default_rng(rank)
    lens = rng.integers(1, 90, 40)
    lens[7] = S + 11
    rows = _lens_to_rows(lens)
    n_r, n_c = len(lens), 29
    cols = rng.integers(0, n_c, len(rows))
    hit = rng.random(len(rows))
    bad = hit < 0.05
    cols[bad] = np.array([-1, n_c, 2 ** 31 - 1])[rng.integers(0, 3, int(bad.sum()))]
    cols[:3] = (-1, n_c, 2 ** 31 - 1)               # a group's first gathers
    cols[-1] = 2 ** 31 - 1
    vals = rng.integers(-2, 11, len(rows)).astype(np.float32) / 2
    X = rng.normal(0, 0.5, (n_r, rank)).astype(np.float32)
    X *= (1 + np.arange(n_r, dtype=np.float32))[:, None]
    Y = rng.normal(0, 0.5, (n_c, rank)).astype(np.float32)
    ptr, c, v = R.csr(rows, cols, vals, n_r)
    blk = types.SimpleNamespace(row_ptr=_dev(ptr, torch.int64), col=_dev(c, torch.int32),
                                val=_dev(v, torch.float32), nnz=len(v), n_rows=n_r)
    ws = _ws()
    out = E.objective_side(blk, _table(X), _table(Y), n_c, rank, implicit, alpha, ws).tolist()
    want = R.side(rows, cols, vals, X, Y, implicit, alpha, n_cols=n_c)
    ok = (cols >= 0) & (cols < n_c)
    dropped = R.side(rows[ok], cols[ok], vals[ok], X, Y, implicit, alpha)
    kept = R.side(rows, np.where(ok, cols, 0), vals, X, Y, implicit, alpha)
    assert want[:2] == dropped[:2] and want[2:] == kept[2:] and want[3] > dropped[3]
    tol = 1e-12 * (want[1] + want[2])
    print(f"K10 out-of-range cols k={rank}: got {out} want {want} tol {tol:.3e}")
    assert out[3:] == want[3:]                      # n, n_positive: every rating
    for g, w_ in zip(out[:3], want[:3]):            # data, scale: without them; reg: with
        assert abs(g - w_) <= tol, (out, want)
    assert abs(out[2] - dropped[2]) > 1e3 * tol     # reg without them is another number
    assert E.objective_side(blk, _table(X), _table(Y), n_c, rank, implicit, alpha, ws).tolist() == out


# ------------------------------------------------------------------ Gram kernel alone
@pytest.mark.parametrize("n", [1, 15, 16, 17, 1000])
def test_gram_f64_matches_numpy(n):
    ws = _ws()
    for rank in RANKS:
        rng = np.random.default_rng(1000 * n + rank)
        A = rng.normal(0, 1, (n, rank)).astype(np.float32)
        B = rng.normal(0, 1, (max(n // 2, 1), rank)).astype(np.float32)
        Ad, Bd = _table(A), _table(B)
        Ad[:, rank:] = float("nan")       # garbage past k in one table: masked, not assumed 0
        if Ad.shape[1] > rank + 1:
            Ad[:, rank + 1:] = 1e30
        dot, ga, gb = E.gram_dot(Ad, n, Bd, B.shape[0], rank, ws, grams=True)
        dot2, ga2, gb2 = E.gram_dot(Ad, n, Bd, B.shape[0], rank, ws, grams=True)
        assert torch.equal(ga, ga2) and torch.equal(gb, gb2) and torch.equal(dot, dot2)
        A64, B64 = A.astype(np.float64), B.astype(np.float64)
        absA, absB = np.abs(A64).T @ np.abs(A64), np.abs(B64).T @ np.abs(B64)
        for G, F64, absG in ((ga, A64, absA), (gb, B64, absB)):
            err = np.abs(G.cpu().numpy() - F64.T @ F64) / absG
            print(f"K10 gram n={n} k={rank}: worst error / sum|f_a f_b| = {err.max():.3e}")
            assert err.max() <= 1e-13, (n, rank, err.max())
        want = float(((A64.T @ A64) * (B64.T @ B64)).sum())
        # each Gram entry is good to 1e-13 of its absolute sum; the k^2 products add ulps
        tol = 1e-12 * float((absA * absB).sum())
        assert abs(float(dot.item()) - want) <= tol, (n, rank, float(dot.item()), want, tol)


# ------------------------------------------------------------------ the invariant
@functools.lru_cache(maxsize=None)
def grouped_core():
    return E.ALSCore(*R.grouped_problem(), device=DEV)


def _alternate(core, rank, implicit, iterations=3):
    """L at the start and after every half-sweep from the protocol's fixed U0."""
    core.init_factors(rank, U0=R.grouped_start(core.n_users, rank))
    core.status.zero_()
    L = [core.objective(0.1, implicit, 1.0)["objective"]]
    for _ in range(iterations):
        core.half_sweep_items(0.1, implicit, 1.0)
        L.append(core.objective(0.1, implicit, 1.0)["objective"])
        core.half_sweep_users(0.1, implicit, 1.0)
        L.append(core.objective(0.1, implicit, 1.0)["objective"])
    core.check_status()
    return L


@pytest.mark.parametrize("implicit", [False, True])
@pytest.mark.parametrize("rank", [8, 48, 128])
def test_half_sweeps_never_raise_the_objective(rank, implicit):
    L = _alternate(grouped_core(), rank, implicit)
    ratios = [b / a for a, b in zip(L, L[1:])]
    print(f"K10 invariant k={rank} implicit={implicit}: L = {L}; worst L_after / L_before - 1 = "
          f"{max(ratios) - 1:.3e}; first half-sweep ratio {ratios[0]:.4f}")
    for a, b in zip(L, L[1:]):
        assert b <= a * (1 + 1e-9), (rank, implicit, L)
    assert L[1] < 0.5 * L[0], (rank, implicit, L[:2])


# ------------------------------------------------------------------ fit bookkeeping
@pytest.mark.parametrize("implicit", [False, True])
def test_fit_history_equals_the_manual_alternation(implicit):
    core = grouped_core()
    rank = 48
    U0 = R.grouped_start(core.n_users, rank)
    manual = _alternate(core, rank, implicit)[2::2]          # after each full iteration
    core.fit(rank, 3, 0.1, implicit, 1.0, U0=U0, objective_every=1)
    assert core.iterations_run == 3
    assert core.objective_history == list(zip((1, 2, 3), manual))      # bit for bit
    u, i, r = R.grouped_problem()
    want = R.objective(u, i, r, core.U[:, :rank].cpu().numpy(), core.V[:, :rank].cpu().numpy(),
                       0.1, implicit, 1.0)
    got = core.objective(0.1, implicit, 1.0)
    _close(got, want, f"after fit implicit={implicit}")
    assert got["objective"] == core.objective_history[-1][1]
    # observing does not perturb the fit
    Uo, Vo = core.U.clone(), core.V.clone()
    core.fit(rank, 3, 0.1, implicit, 1.0, U0=U0)
    assert core.objective_history == [] and core.iterations_run == 3
    assert torch.equal(core.U, Uo) and torch.equal(core.V, Vo)


def test_fit_period_and_tol():
    core = grouped_core()
    U0 = R.grouped_start(core.n_users, 8)
    core.fit(8, 5, 0.1, U0=U0, objective_every=2)
    assert [it for it, _ in core.objective_history] == [2, 4, 5]
    sparse = list(core.objective_history)
    every = list(core.fit(8, 5, 0.1, U0=U0, objective_every=1).objective_history)
    assert [it for it, _ in every] == [1, 2, 3, 4, 5]
    assert sparse == [p for p in every if p[0] in (2, 4, 5)]
    core.fit(8, 20, 0.1, U0=U0, tol=0.5)             # no step after the first halves L
    assert core.iterations_run == 2 < 20
    assert core.objective_history == every[:2]
    core.fit(8, 5, 0.1, U0=U0, tol=0.0)              # L still falls: runs to the end
    assert core.iterations_run == 5 and core.objective_history == every
    with pytest.raises(ValueError):
        core.fit(8, 1, 0.1, objective_every=-1)
    with pytest.raises(ValueError):
        core.fit(8, 1, 0.1, tol=-1.0)


def test_tol_stop_still_writes_the_due_checkpoint(tmp_path):
    from als_mi355x import checkpoint as C
    core = grouped_core()
    U0 = R.grouped_start(core.n_users, 8)
    core.fit(8, 20, 0.1, U0=U0, tol=0.5, checkpoint_dir=str(tmp_path), checkpoint_interval=2)
    assert core.iterations_run == 2
    st = C.load(str(tmp_path))
    assert st.iteration == 2
    assert np.array_equal(st.U, core.U[:, :8].cpu().numpy())
    # resumed: the list starts at the first evaluated iteration after the checkpoint
    core.fit(8, 4, 0.1, U0=U0, objective_every=1, checkpoint_dir=str(tmp_path),
             checkpoint_interval=10, resume=True)
    assert [it for it, _ in core.objective_history] == [3, 4]


def test_objective_needs_the_training_blocks():
    core = grouped_core()
    core.fit(8, 1, 0.1, seed=1)
    uids, U = core.user_factors()
    iids, V = core.item_factors()
    served = E.ALSCore.from_factors(uids, U, iids, V)
    assert served.objective_history == []
    with pytest.raises(ValueError, match="ratings"):
        served.objective(0.1)


# ------------------------------------------------------------------ public surfaces
def _frame():
    import pandas as pd
    u, i, r = R.grouped_problem()
    return pd.DataFrame({"user": u, "item": i, "rating": r})


@pytest.mark.parametrize("implicit", [False, True])
def test_ml_surface(implicit, tmp_path):
    from als_mi355x.ml.recommendation import ALS, ALSModel
    als = ALS(rank=8, maxIter=4, regParam=0.1, implicitPrefs=implicit, seed=3)
    model = als.setObjectiveHistory(1).fit(_frame())
    hist = model.objectiveHistory
    assert model.objectiveIterations == [1, 2, 3, 4] and len(hist) == 4
    assert all(b <= a for a, b in zip(hist, hist[1:])), hist
    obj = model.trainingObjective()
    assert obj["objective"] == hist[-1] and obj["n"] == 4000
    plain = ALS(rank=8, maxIter=4, regParam=0.1, implicitPrefs=implicit, seed=3).fit(_frame())
    assert plain.objectiveHistory == [] and plain.trainingObjective() == obj
    stopped = als.copy().setObjectiveHistory(1, tol=0.9).fit(_frame())
    assert stopped.objectiveIterations == [1, 2] and stopped.engine.iterations_run == 2
    model.save(str(tmp_path / "m"))
    back = ALSModel.load(str(tmp_path / "m"))
    assert back.objectiveHistory == [] and back.objectiveIterations == []
    with pytest.raises(ValueError, match="ratings"):
        back.trainingObjective()


def test_mllib_surface(tmp_path):
    from als_mi355x.mllib.recommendation import ALS, MatrixFactorizationModel
    u, i, r = R.grouped_problem()
    model = ALS.trainImplicit(list(zip(u.tolist(), i.tolist(), r.tolist())), 8, iterations=2,
                              lambda_=0.1, alpha=1.0, seed=3)
    got = model.trainingObjective(0.1, implicit=True, alpha=1.0)
    core = model.engine
    want = R.objective(u, i, r, core.U[:, :8].cpu().numpy(), core.V[:, :8].cpu().numpy(), 0.1,
                       True, 1.0)
    _close(got, want, "mllib implicit")
    model.save(None, str(tmp_path / "m"))
    with pytest.raises(ValueError, match="ratings"):
        MatrixFactorizationModel.load(None, str(tmp_path / "m")).trainingObjective(0.1)
