"""GPU tests of the update path (K17 als_csr_merge, ALSCore.add_ratings / refresh / refit and
the public surfaces over them).

Shapes come from T = als_csr_merge_tile(): about 40 rows per side with user-row lengths 1,
T - 1, T, T + 1, 2T + 3, ... (update_ref.row_lengths) and batches of 1 to ~80 ratings
(update_ref.CASES, held to the oracle's csr_build on the concatenation by test_update_cpu.py).
The bar for everything made of ratings is bit equality with a fresh ALSCore on the
concatenation; factor rows are compared bitwise with the row kernels' own output and within
the project's 1e-4 per-row bar with the numpy oracles.
"""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import nnls_ref
import update_ref as UR
from als_mi355x import engine as E
from helpers import fold_in_oracle, planted, rel_row_err, rel_row_errs, report

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
REG = 0.1


def _T():
    return E.csr_merge_tile()


def _cat(a, b):
    return tuple(np.concatenate([x, y]) for x, y in zip(a, b))


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _assert_same_ratings(core, fresh):
    """Everything made of the ratings, bit for bit: id maps, CSR sides, schedules, nnz."""
    assert core.nnz == fresh.nnz
    for name in ("uidx", "iidx"):
        a, b = getattr(core, name), getattr(fresh, name)
        assert (a.n, a.offset, a.id_space) == (b.n, b.offset, b.id_space), name
        assert torch.equal(a.map, b.map) and torch.equal(a.uniq, b.uniq), name
        assert a.map.dtype == b.map.dtype == torch.int32 and a.uniq.dtype == torch.int32
    for name in ("user_block", "item_block"):
        a, b = getattr(core, name), getattr(fresh, name)
        used = {"light_rows": a.n_light, "heavy_rows": a.n_heavy, "chunk_row": a.n_chunks,
                "chunk_begin": a.n_chunks, "chunk_end": a.n_chunks}   # the rest is allocation
        for f in dataclasses.fields(E.RatingBlock):
            x, y = getattr(a, f.name), getattr(b, f.name)
            if isinstance(x, torch.Tensor):
                n = used.get(f.name)
                if n is not None:
                    x, y = x[:n], y[:n]
                assert x.dtype == y.dtype and x.shape == y.shape, (name, f.name)
                assert torch.equal(_bits(x), _bits(y)), (name, f.name)
            else:
                assert x == y, (name, f.name, x, y)


# ---------------------------------------------------------------- blocks are K1's, bit for bit
@pytest.mark.parametrize("name", UR.CASES)
def test_add_ratings_gives_the_blocks_of_a_fresh_core(name):
    """Cases (a)-(g), each before any fit (i)."""
    old, add = UR.case(name, _T())
    core = E.ALSCore(*old)
    info = core.add_ratings(*add)
    assert core.rank == 0 and core.U is None
    _assert_same_ratings(core, E.ALSCore(*_cat(old, add)))
    assert info["added"] == len(add[0])
    for side, s in (("users", 0), ("items", 1)):
        new = np.setdiff1d(add[s], old[s])
        assert info[f"new_{side}"].cpu().numpy().tolist() == new.tolist()
        idx = core.uidx if s == 0 else core.iidx
        want = idx.rows_of(torch.as_tensor(np.unique(add[s]), device=DEV)).cpu().numpy()
        assert info[f"touched_{side}"].cpu().numpy().tolist() == want.tolist()


def test_two_adds_in_sequence_and_an_empty_one():
    """(h): two batches one after the other against one concatenation; an empty batch is a
    no-op."""
    T = _T()
    old, a1 = UR.case("b_new_both", T)
    _, a2 = UR.case("c_negative", T)
    core = E.ALSCore(*old)
    core.add_ratings(*a1)
    before = (core.user_block, core.uidx)
    info = core.add_ratings(a1[0][:0], a1[1][:0], a1[2][:0])
    assert info["added"] == 0 and core.user_block is before[0] and core.uidx is before[1]
    core.add_ratings(*(torch.as_tensor(x, device=DEV) for x in a2))      # device arrays too
    _assert_same_ratings(core, E.ALSCore(*_cat(_cat(old, a1), a2)))
    # the rows touched by either batch, in the final numbering, are kept for refresh
    tu = core.uidx.rows_of(torch.as_tensor(np.unique(np.concatenate([a1[0], a2[0]])), device=DEV))
    assert core._touched[0].tolist() == tu.tolist()
    with pytest.raises(ValueError, match="same length"):
        core.add_ratings([1, 2], [1], [1.0])


# ---------------------------------------------------------------- factors and caches
def _fitted_then_added(seed, rank=6):
    old, add = UR.case("b_new_both", _T())
    core = E.ALSCore(*old)
    core.fit(rank, 3, REG, seed=2)
    core.recommend_all(3, exclude="train")        # fills the exclusion cache with the old pairs
    before = dict(U=core.U.clone(), V=core.V.clone(), uids=core.uidx.ids().clone(),
                  iids=core.iidx.ids().clone())
    uid, iid = np.unique(old[0]), np.unique(old[1])
    # the new users of the case: one rated a known item only, one a new item only, one both
    before["known_only"], before["new_only"], before["both"] = uid[-1] + 1, uid[2] + 1, uid[0] - 1
    for key in ("known_only", "both"):
        sel = add[0] == before[key]
        before["fold_" + key] = core.fold_in(add[0][sel], add[1][sel], add[2][sel], reg=REG)[1]
    info = core.add_ratings(*add, seed=seed)
    return old, add, core, before, info


def test_factors_move_and_new_rows_get_factors():
    old, add, core, b, info = _fitted_then_added(seed=7)
    k = core.rank
    assert core.U.shape == (core.n_users, E.ld_for(k)) and core.V.shape[0] == core.n_items
    # old rows keep their bits at their new positions
    assert torch.equal(_bits(core.U[core.uidx.rows_of(b["uids"])]), _bits(b["U"]))
    assert torch.equal(_bits(core.V[core.iidx.rows_of(b["iids"])]), _bits(b["V"]))
    row = lambda uid: int(core.uidx.rows_of(torch.tensor([uid], device=DEV)))
    # a new user who rated only known items: the bits fold_in gave before the growth; one who
    # also rated a new item: that rating is left out, as fold_in leaves out an unknown item
    for key in ("known_only", "both"):
        assert torch.equal(_bits(core.U[row(b[key]), :k]), _bits(b["fold_" + key][0])), key
        assert float(core.U[row(b[key]), :k].abs().max()) > 0
    # a new user who rated only new items: a unit-norm row, never zero
    x = core.U[row(b["new_only"]), :k].double()
    assert abs(float(x.norm()) - 1.0) < 1e-6
    assert core.U.shape[1] > k                   # rank 6: the padding columns stay zero
    assert float(core.U[:, k:].abs().sum()) == 0 and float(core.V[:, k:].abs().sum()) == 0
    # every new item has factors (its raters all have rows by then)
    new_i = core.iidx.rows_of(info["new_items"])
    assert bool((core.V[new_i, :k].abs().amax(1) > 0).all())
    # same seed, same rows; another seed, another Gaussian row
    _, _, again, _, _ = _fitted_then_added(seed=7)
    assert torch.equal(_bits(again.U), _bits(core.U)) and torch.equal(_bits(again.V), _bits(core.V))
    _, _, other, _, _ = _fitted_then_added(seed=8)
    y = other.U[row(b["new_only"]), :k].double()
    assert abs(float(y.norm()) - 1.0) < 1e-6 and not torch.equal(x, y)
    assert torch.equal(_bits(other.U[row(b["known_only"])]), _bits(core.U[row(b["known_only"])]))


def test_caches_statistics_and_objective_follow_the_batch():
    old, add, core, b, info = _fitted_then_added(seed=7)
    fresh = E.ALSCore(*_cat(old, add))
    _assert_same_ratings(core, fresh)
    # train exclusion: no added pair is listed any more (the cache held the old pairs)
    keys, ids, sc = (x.cpu().numpy() for x in core.recommend_all(core.n_items, exclude="train"))
    for u, i in zip(add[0], add[1]):
        r = int(np.searchsorted(keys, u))
        assert keys[r] == u and i not in ids[r][np.isfinite(sc[r])]
    for a, f in zip(core.train_exclusion(True), fresh.train_exclusion(True)):
        assert torch.equal(a, f)
    # statistics
    for side in (False, True):
        got, want = core.rating_stats(side), fresh.rating_stats(side)
        assert torch.equal(got["ids"], want["ids"]) and torch.equal(got["count"], want["count"])
        assert int(got["count"].sum()) == len(old[0]) + len(add[0])
        assert torch.equal(core.popularity(side), fresh.popularity(side))
    assert core.fingerprint() == fresh.fingerprint()
    assert core.fingerprint()["nnz"] == len(old[0]) + len(add[0])
    # the objective of the same factors is the fresh core's, bit for bit (K10 is reproducible)
    fresh.rank, fresh.U, fresh.V = core.rank, core.U.clone(), core.V.clone()
    assert core.objective(REG) == fresh.objective(REG)
    assert core.objective(REG, True, 2.0) == fresh.objective(REG, True, 2.0)


# ---------------------------------------------------------------- refresh
def _rows_of(block, rows):
    rp, col, val = (x.cpu().numpy() for x in (block.row_ptr, block.col, block.val))
    return [(col[rp[r]:rp[r + 1]], val[rp[r]:rp[r + 1]]) for r in rows.tolist()]


@pytest.mark.parametrize("mode", ["explicit", "implicit", "nonnegative"])
@pytest.mark.parametrize("rank", [8, 64])
def test_refresh_solves_the_touched_rows_and_nothing_else(rank, mode):
    implicit, nonneg, alpha = mode == "implicit", mode == "nonnegative", 0.5
    old, add = UR.case("b_new_both", _T())
    core = E.ALSCore(*old)
    core.fit(rank, 2, REG, implicit, alpha, seed=4, nonnegative=nonneg)
    core.add_ratings(*add)
    U0, V0 = core.U.clone(), core.V.clone()
    tu, ti = core._touched
    assert 0 < tu.numel() < core.n_users and 0 < ti.numel() < core.n_items
    assert core.refresh() is core
    ws = E.Workspace(core.device)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)

    def solve(block, rows, Y, n_src):
        csr = E.gather_rows(block.row_ptr, block.col, block.val, rows)
        yty = E.compute_yty(Y, n_src, rank, E.Workspace(core.device)) if implicit else None
        if nonneg:
            return E.nnls_rows(*csr, Y, n_src, rank, REG, implicit, alpha, yty, ws)[0]
        return E.fold_in_rows(*csr, Y, n_src, rank, REG, implicit, alpha, yty, status, ws)[0]

    def oracle(block, rows, Y):
        rr = _rows_of(block, rows)
        if nonneg:
            from helpers import ragged_csr
            return nnls_ref.solve_rows(*ragged_csr(rr), Y, REG, implicit, alpha)
        return fold_in_oracle(rr, Y, REG, implicit, alpha)[0]

    for F, F0, t, block, Y, n_src, side in (
            (core.U, U0, tu, core.user_block, V0, core.n_items, "users"),
            (core.V, V0, ti, core.item_block, core.U, core.n_users, "items")):
        keep = torch.ones(F.shape[0], dtype=torch.bool, device=DEV)
        keep[t] = False
        assert torch.equal(_bits(F[keep]), _bits(F0[keep])), f"untouched {side} moved"
        assert torch.equal(_bits(F[t]), _bits(solve(block, t, Y, n_src))), side
        assert not torch.equal(F[t], F0[t])
        errs = rel_row_errs(F[t, :rank].cpu().numpy(),
                            oracle(block, t, Y[:, :rank].cpu().numpy()))
        report(f"refresh_{side}_k{rank}_{mode}", float(errs.max()))
        assert errs.max() < 1e-4, errs
        if nonneg:
            assert float(F[t].min()) >= 0
    assert int(status.item()) == 0
    # other parameters than the fit's can be asked for, and sweeps repeats the pair of solves
    core.refresh(reg=2 * REG, sweeps=2)
    assert not torch.equal(core.U[tu], solve(core.user_block, tu, V0, core.n_items))
    with pytest.raises(ValueError, match="sweeps"):
        core.refresh(sweeps=0)


def test_refresh_needs_a_fit_or_a_reg():
    old, add = UR.case("f_one", _T())
    core = E.ALSCore(*old)
    core.add_ratings(*add)
    with pytest.raises(ValueError, match="factors"):
        core.refresh(reg=REG)
    with pytest.raises(ValueError, match="factors"):
        core.refit(1)


# ---------------------------------------------------------------- refit
def test_refit_is_a_fit_from_the_current_user_factors():
    old, add = UR.case("b_new_both", _T())
    core = E.ALSCore(*old)
    core.fit(8, 3, REG, seed=2)
    core.add_ratings(*add)
    U_start = core.U[:, :8].clone()
    assert core.refit(2) is core and core.iterations_run == 2
    fresh = E.ALSCore(*_cat(old, add))
    fresh.fit(8, 2, REG, U0=U_start)
    eu = rel_row_err(core.U[:, :8].cpu().numpy(), fresh.U[:, :8].cpu().numpy())
    ev = rel_row_err(core.V[:, :8].cpu().numpy(), fresh.V[:, :8].cpu().numpy())
    report("refit_vs_fresh_fit", max(eu, ev))
    assert max(eu, ev) <= 1e-4
    assert core._touched is None                       # a fit re-solves every row
    with pytest.raises(ValueError, match="current"):
        core.refit(1, U0=U_start)
    core.refit(1, reg=0.5, objective_every=1)          # overrides and observers pass through
    assert len(core.objective_history) == 1 and core._fit_params["reg"] == 0.5


def test_warm_beats_cold():
    """helpers.planted's seeded rank-8 300 x 200 set, fitted 10 iterations, then a 2 % batch
    (update_ref.warm_cold_data): one warm iteration on the merged data ends below one cold
    iteration.  The numpy oracle on the same input (oracle.als_oracle.train, lambda 0.1, its
    own seeded start): 6215.29 after the warm iteration against 34456.53 after the cold one
    (6271.62 before it); only the inequality is asserted."""
    old, add = UR.warm_cold_data()
    assert 0.015 * len(old[0]) < len(add[0]) < 0.025 * len(old[0])
    core = E.ALSCore(*old)
    core.fit(8, 10, REG, seed=1)
    info = core.add_ratings(*add)
    assert info["new_users"].numel() == info["new_items"].numel() == 0
    core.refit(1, objective_every=1)
    warm = core.objective_history[-1][1]
    cold_core = E.ALSCore(*_cat(old, add))
    cold_core.fit(8, 1, REG, seed=1, objective_every=1)
    cold = cold_core.objective_history[-1][1]
    report("warm_objective", warm)
    report("cold_objective", cold)
    assert warm < cold


# ---------------------------------------------------------------- public surfaces
def _trips(t):
    return list(zip(t[0].tolist(), t[1].tolist(), t[2].tolist()))


@pytest.mark.parametrize("mode", ["refit", "refresh", "none"])
def test_mllib_model_update(mode):
    from als_mi355x.mllib.recommendation import ALS, Rating
    old, add = UR.case("b_new_both", _T())
    model = ALS.train(_trips(old), 8, iterations=3, lambda_=REG, seed=5)
    eng = model.engine
    U0, old_rows_ids = eng.U.clone(), eng.uidx.ids().clone()
    batch = _trips(add)
    batch[0] = Rating(*batch[0])                       # tuples and Ratings alike
    assert model.update(batch, 2, mode=mode) is model and model.engine is eng
    _assert_same_ratings(eng, E.ALSCore(*_cat(old, add)))
    new_user = int(np.setdiff1d(add[0], old[0])[0])
    assert np.isfinite(model.predict(new_user, int(old[1][0])))
    moved = eng.U[eng.uidx.rows_of(old_rows_ids)]
    touched_old = torch.isin(old_rows_ids, torch.as_tensor(np.unique(add[0]), device=DEV).int())
    if mode == "none":
        assert torch.equal(moved, U0)
    elif mode == "refresh":
        assert torch.equal(moved[~touched_old], U0[~touched_old])
        assert not torch.equal(moved[touched_old], U0[touched_old])
    else:
        assert eng.iterations_run == 2 and not torch.equal(moved[~touched_old], U0[~touched_old])


@pytest.mark.parametrize("mode", ["refit", "refresh", "none"])
def test_ml_model_update(mode):
    from als_mi355x.ml.recommendation import ALS
    old, add = UR.case("b_new_both", _T())
    frame = lambda t: {"u": t[0], "m": t[1], "r": t[2]}
    est = ALS(rank=8, maxIter=3, regParam=REG, userCol="u", itemCol="m", ratingCol="r", seed=5)
    model = est.setObjectiveHistory(1).fit(frame(old))
    assert model.objectiveIterations == [1, 2, 3]
    eng = model.engine
    U_pre, V_pre, ids_pre = eng.U.clone(), eng.V.clone(), eng.uidx.ids().clone()
    assert model.update(frame(add), maxIter=2, mode=mode) is model
    _assert_same_ratings(eng, E.ALSCore(*_cat(old, add)))
    assert len(model.userFactors) == eng.n_users == len(np.unique(_cat(old, add)[0]))
    if mode == "refit":
        # the history follows the refit, which is a fit from the U add_ratings left
        assert model.objectiveIterations == [1, 2]
        h = model.objectiveHistory
        assert h[1] <= h[0] and h[1] == model.trainingObjective()["objective"]
        twin = E.ALSCore(*old)
        twin.fit(8, 0, REG, U0=U_pre[:, :8])
        twin.V = V_pre.clone()
        twin.add_ratings(*add, seed=5)
        fresh = E.ALSCore(*_cat(old, add))
        fresh.fit(8, 2, REG, U0=twin.U[:, :8])
        assert rel_row_err(eng.U[:, :8].cpu().numpy(), fresh.U[:, :8].cpu().numpy()) <= 1e-4
    else:
        assert model.objectiveIterations == [1, 2, 3]
        moved = eng.U[eng.uidx.rows_of(ids_pre)]
        touched = torch.isin(ids_pre, torch.as_tensor(np.unique(add[0]), device=DEV).int())
        assert torch.equal(moved[~touched], U_pre[~touched])
        assert torch.equal(moved[touched], U_pre[touched]) == (mode == "none")


def test_personal_recommendations_update():
    """The reference's twelve personal ratings (tests/golden/personal_ratings.json, movie ids
    folded onto a 200-movie catalogue; the repeat that makes stays a duplicate rating) added
    to a model that has never seen user 0, against personal_recommendations on a model
    refitted from the union with the same U0."""
    from als_mi355x import personal
    from als_mi355x.mllib.recommendation import ALS, MatrixFactorizationModel
    n_items, min_ratings = 200, 24
    u, m, r = planted(300, n_items, density=0.08, seed=11)
    u = u + 1                                          # user 0 is new
    gold = json.load(open(os.path.join(HERE, "golden", "personal_ratings.json")))
    rated = [(0, mv % n_items, float(x)) for _, mv, x in gold["my_rated_movies"]]
    assert len(rated) == 12
    movies = [(j, f"m{j}") for j in range(n_items)] + [(10 ** 6, "never seen")]
    model = ALS.train(_trips((u, m, r)), 8, iterations=3, lambda_=REG, seed=5)
    eng = model.engine
    # the expectation first: the same add on a twin core gives the U0 of the fresh fit
    twin = E.ALSCore(u, m, r)
    twin.fit(8, 0, REG, U0=eng.U[:, :8])
    twin.V = eng.V.clone()
    ru, rm, rr = (np.asarray(x) for x in zip(*rated))
    twin.add_ratings(ru, rm, rr)
    union = (np.concatenate([u, ru]), np.concatenate([m, rm]), np.concatenate([r, rr]))
    fresh = E.ALSCore(*union)
    fresh.fit(8, 2, REG, U0=twin.U[:, :8])
    counts = personal.movie_counts_and_averages(_trips(union))
    want = personal.personal_recommendations(MatrixFactorizationModel(fresh), 0, rated, movies,
                                             counts, min_count=min_ratings, num=20)
    got = personal.personal_recommendations_update(model, 0, rated, movies, num=20,
                                                   min_ratings=min_ratings, iterations=2)
    assert len(got) == 20 and eng.nnz == len(u) + 12
    assert [t for _, t, _ in got] == [t for _, t, _ in want]
    np.testing.assert_allclose([p for p, _, _ in got], [p for p, _, _ in want], rtol=1e-5, atol=0)
    rated_m = {mv for _, mv, _ in rated}
    cnt = np.bincount(union[1], minlength=n_items)
    assert 0 < (cnt > min_ratings).sum() < n_items     # the filter bites
    for p, title, n in got:
        mid = int(title[1:])
        assert mid not in rated_m and n == cnt[mid] > min_ratings
    assert [p for p, _, _ in got] == sorted((p for p, _, _ in got), reverse=True)
    # the engine's own counts include the batch: a rated movie's count went up by its ratings
    stats = eng.rating_stats(False)
    assert stats["count"].cpu().numpy().tolist() == cnt[stats["ids"].cpu().numpy()].tolist()
    assert personal.personal_recommendations_update(model, 0, [], movies, min_ratings=10 ** 6) == []
