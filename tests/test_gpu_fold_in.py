"""Fold-in (K7, als_fold_in) on the GPU: kernel parity against the fp64 oracle, padding,
determinism, the status word, fold-in against training, the serving-only core,
recommend_new and the public surfaces.

Oracle: oracle.als_oracle.half_sweep over the rows' ratings with the unknown items removed
(rows left without a rating are not given to it: their result is defined as zero).  The
error is the per-row relative 2-norm smoke() uses, and the bar is the project's 1e-4.
Measured maxima (MI355X) per rank, explicit / implicit: see DESIGN.md section K7.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from als_mi355x import engine as E
from helpers import fold_in_oracle, ragged_csr, rel_row_errs, report

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
N_ITEMS = 200
REG = 0.1
ALPHA = 40.0
RANKS = (1, 8, 17, 33, 64, 100, 128)


# ------------------------------------------------------------------ helpers
def _factors(k, seed=0):
    rng = np.random.default_rng(1000 + 7 * k + seed)
    return (rng.standard_normal((N_ITEMS, k)) / np.sqrt(k)).astype(np.float32)


def _dev(M, ld=None, fill=0.0):
    k = M.shape[1]
    out = torch.full((M.shape[0], ld or E.ld_for(k)), fill, dtype=torch.float32, device=DEV)
    out[:, :k] = torch.as_tensor(M).to(DEV)
    return out


def _rows(k, seed=0):
    """The rows of one parity call as (cols, vals) lists: lengths 0, 1, 2, k - 1, k, k + 1,
    300 (5000 too at k = 128), one row of one repeated item, one mixing valid entries with
    col = -1 and col = n_src."""
    rng = np.random.default_rng(50 + k + seed)
    lens = [0, 1, 2, k - 1, k, k + 1, 300] + ([5000] if k == 128 else [])
    rows = []
    for n in lens:
        rows.append((rng.integers(0, N_ITEMS, n), rng.integers(1, 6, n)))
    rows.append((np.full(40, 17), rng.integers(1, 6, 40)))
    mixed = rng.integers(0, N_ITEMS, 30)
    mixed[::3] = -1
    mixed[1::3] = N_ITEMS
    rows.append((mixed, rng.integers(1, 6, 30)))
    return rows


_csr = ragged_csr
_oracle = fold_in_oracle   # (X_ref [n, k] with zero rows where nothing is used, n_used [n])


def _run(rows, V, k, reg, implicit, alpha=ALPHA, ld=None, fill=0.0):
    """One als_fold_in call over `rows` against V stored with leading dimension ld, its
    padding columns holding `fill` (als_yty, unlike K7, needs zeros there: the Gram
    always comes from the zero-padded copy)."""
    ptr, col, val = _csr(rows)
    t = lambda a, d: torch.as_tensor(a).to(DEV, d).contiguous()
    ws = E.Workspace(torch.device(DEV))
    Vd = _dev(V, ld, fill)
    yty = E.compute_yty(_dev(V), N_ITEMS, k, ws) if implicit else None
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    X, n_used = E.fold_in_rows(t(ptr, torch.int64), t(col, torch.int32), t(val, torch.float32), Vd,
                               N_ITEMS, k, reg, implicit, alpha, yty, status, ws)
    torch.cuda.synchronize()
    return X, n_used.cpu().numpy(), int(status.item())


@functools.lru_cache(maxsize=None)
def _parity_case(k, implicit):
    V, rows = _factors(k), _rows(k)
    ref, n_ref = _oracle(rows, V, REG, implicit, ALPHA)
    return V, rows, ref, n_ref


# ------------------------------------------------------------------ kernel
@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
@pytest.mark.parametrize("k", RANKS)
def test_kernel_parity(k, implicit):
    V, rows, ref, n_ref = _parity_case(k, implicit)
    X, n_used, status = _run(rows, V, k, REG, implicit)
    assert status == 0
    X = X.cpu().numpy()
    np.testing.assert_array_equal(n_used, n_ref)
    full = n_ref > 0
    errs = rel_row_errs(X[full, :k], ref[full])
    print(f"fold_in parity k={k} implicit={implicit}: max rel row err {errs.max():.3e} "
          f"(row lengths {[len(c) for c, _ in rows]})")
    report(f"fold_in_parity[k={k},implicit={implicit}]", float(errs.max()))
    assert (X[~full] == 0).all()          # the length-0 row (and k - 1 = 0 at k = 1): exactly zero
    assert not full[0] and len(rows[0][0]) == 0
    assert (X[:, k:] == 0).all()
    assert errs.max() < 1e-4, errs


@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
@pytest.mark.parametrize("k", (1, 17, 33, 64))
def test_padding_columns_never_reach_a_result(k, implicit):
    V, rows, _, _ = _parity_case(k, implicit)
    ld = (k + 4 + 3) // 4 * 4
    assert ld >= k + 4
    Xz, nz, sz = _run(rows, V, k, REG, implicit, ld=ld, fill=0.0)
    Xn, nn, sn = _run(rows, V, k, REG, implicit, ld=ld, fill=float("nan"))
    assert sz == sn == 0
    assert torch.equal(Xz, Xn) and not torch.isnan(Xn).any()
    np.testing.assert_array_equal(nz, nn)
    assert Xn.shape[1] == E.ld_for(k) and (Xn[:, k:] == 0).all()
    # the tight layout gives the same bits as the padded one
    Xt, _, _ = _run(rows, V, k, REG, implicit)
    assert torch.equal(Xt, Xz)


@pytest.mark.parametrize("k,implicit", [(33, False), (128, True)])
def test_two_calls_are_bit_identical(k, implicit):
    V, rows, _, _ = _parity_case(k, implicit)
    a = _run(rows, V, k, REG, implicit)
    b = _run(rows, V, k, REG, implicit)
    assert torch.equal(a[0], b[0]) and (a[1] == b[1]).all()


def test_failed_pivot_sets_status_and_raises():
    """Explicit, reg = 0, k = 8: a row with 3 ratings has a rank-3 A.  The word names it,
    the other rows of the call are solved, and ALSCore.fold_in raises."""
    k = 8
    V = _factors(k, seed=3)
    rng = np.random.default_rng(9)
    rows = [(rng.choice(N_ITEMS, 20, replace=False), rng.integers(1, 6, 20)) for _ in range(5)]
    rows.insert(2, (np.array([5, 70, 131]), np.array([4, 2, 5])))
    X, n_used, status = _run(rows, V, k, 0.0, False)
    assert status == 3                         # row + 1 of the only failing row
    good = [0, 1, 3, 4, 5]
    ref, _ = _oracle([rows[r] for r in good], V, 0.0, False, 1.0)
    errs = rel_row_errs(X.cpu().numpy()[good, :k], ref)
    print(f"fold_in status case: other rows max rel row err {errs.max():.3e}")
    assert errs.max() < 1e-4
    np.testing.assert_array_equal(n_used, [len(c) for c, _ in rows])

    core = E.ALSCore.from_factors(np.arange(3), _factors(k, seed=4)[:3], np.arange(N_ITEMS), V)
    ids = np.concatenate([np.full(len(c), 10 + r) for r, (c, _) in enumerate(rows)])
    cols = np.concatenate([c for c, _ in rows])
    vals = np.concatenate([v for _, v in rows]).astype(np.float32)
    with pytest.raises(RuntimeError, match="Cholesky"):
        core.fold_in(ids, cols, vals, reg=0.0)
    keys, Xc, nu = core.fold_in(ids, cols, vals, reg=REG)   # the same rows are fine with reg > 0
    assert keys.tolist() == [10 + r for r in range(len(rows))]
    ref, _ = _oracle(rows, V, REG, False, 1.0)
    assert rel_row_errs(Xc.cpu().numpy(), ref).max() < 1e-4


# ------------------------------------------------------------------ against training
def _smoke_ratings(seed=0):
    rng = np.random.default_rng(seed)
    n_u, n_i = 300, N_ITEMS
    mask = rng.random((n_u, n_i)) < 0.08
    mask[np.arange(n_u), rng.integers(0, n_i, n_u)] = True
    mask[rng.integers(0, n_u, n_i), np.arange(n_i)] = True
    u, i = np.nonzero(mask)
    r = np.clip(np.round(3.5 + rng.normal(0, 1, len(u))), 1, 5).astype(np.float32)
    return u.astype(np.int32), i.astype(np.int32), r


@pytest.fixture(scope="module")
def fitted():
    """(ml ALSModel, u, i, r) fitted on the smoke-shaped data: 300 x 200, 8 % dense, rank 8,
    5 iterations, lambda 0.1.  Never modified by a test."""
    import pandas as pd

    from als_mi355x.ml.recommendation import ALS
    u, i, r = _smoke_ratings()
    model = ALS(rank=8, maxIter=5, regParam=REG, seed=5).fit(
        pd.DataFrame({"user": u, "item": i, "rating": r}))
    return model, u, i, r


def test_fold_in_reproduces_the_last_user_half_sweep(fitted):
    """A fit ends with the user half-sweep against the final V, so folding every training
    user's own ratings in gives the fitted U back: both are within 1e-4 of one oracle row."""
    model, u, i, r = fitted
    core = model.engine
    keys, X, n_used = core.fold_in(u, i, r, reg=REG)
    assert torch.equal(keys, core.user_factor_ids())
    np.testing.assert_array_equal(n_used.cpu().numpy(), np.bincount(u, minlength=300))
    errs = rel_row_errs(X.cpu().numpy(), core.U[:, :8].cpu().numpy())
    print(f"fold_in vs fitted U: max rel row err {errs.max():.3e}")
    assert errs.max() < 2e-4


def test_fold_in_items_reproduces_an_item_half_sweep():
    """user_side=False, by recomputing: one more item half-sweep of a fitted core (V from
    its final U, als_solve_half) against every item's ratings folded in over the same U."""
    from als_mi355x.mllib.recommendation import ALS
    u, i, r = _smoke_ratings(seed=1)
    core = ALS.train(np.stack([u, i, r], 1), 8, iterations=5, lambda_=REG, seed=5).engine
    core.half_sweep_items(REG)
    core.check_status()
    keys, X, _ = core.fold_in(i, u, r, reg=REG, user_side=False)
    assert torch.equal(keys, core.iidx.ids())
    errs = rel_row_errs(X.cpu().numpy(), core.V[:, :8].cpu().numpy())
    print(f"fold_in items vs item half-sweep: max rel row err {errs.max():.3e}")
    assert errs.max() < 2e-4


def _new_users(seed=21, n=50, first=1000):
    """n new users (ids from `first`) with 5 to 40 ratings each of the model's items."""
    rng = np.random.default_rng(seed)
    us, its, rs = [], [], []
    for j in range(n):
        m = int(rng.integers(5, 41))
        us.append(np.full(m, first + j))
        its.append(rng.choice(N_ITEMS, m, replace=False))
        rs.append(rng.integers(1, 6, m))
    return (np.concatenate(us).astype(np.int32), np.concatenate(its).astype(np.int32),
            np.concatenate(rs).astype(np.float32))


def test_serving_only_core_folds_in_the_same_bits(fitted, tmp_path):
    import pandas as pd

    from als_mi355x.ml.recommendation import ALSModel
    model, *_ = fitted
    model.save(str(tmp_path / "m"))
    loaded = ALSModel.load(str(tmp_path / "m"))
    assert loaded.engine.user_block is None      # serving only: no ratings, cannot fit
    nu, ni, nr = _new_users()
    df = pd.DataFrame({"user": nu, "item": ni, "rating": nr})
    a, b = model.foldInUsers(df), loaded.foldInUsers(df)
    assert list(a.columns) == ["id", "features"] and len(a) == 50
    np.testing.assert_array_equal(a["id"].to_numpy(), b["id"].to_numpy())
    assert np.array_equal(np.stack(a["features"].to_list()), np.stack(b["features"].to_list()))
    # the same rows turned round: new items (ids from 500) rated by users the model knows
    df = pd.DataFrame({"user": nu - 1000, "item": ni + 500, "rating": nr})
    a, b = model.foldInItems(df), loaded.foldInItems(df)
    np.testing.assert_array_equal(a["id"].to_numpy(), np.unique(ni + 500))
    assert np.abs(np.stack(a["features"].to_list())).max() > 0
    assert np.array_equal(np.stack(a["features"].to_list()), np.stack(b["features"].to_list()))


# ------------------------------------------------------------------ recommend_new
@pytest.fixture(scope="module")
def served(fitted):
    """New users' ratings (plus one user who rated unknown items only), the candidate
    set, the folded rows and the fp64 scores X_new V^T."""
    model, *_ = fitted
    core = model.engine
    nu, ni, nr = _new_users()
    ghost = 5000                                   # every item unknown to the model
    nu = np.concatenate([nu, np.full(3, ghost)]).astype(np.int32)
    ni = np.concatenate([ni, [10 ** 6, 10 ** 6 + 1, -4]]).astype(np.int32)
    nr = np.concatenate([nr, [5, 4, 3]]).astype(np.float32)
    cand = np.sort(np.random.default_rng(2).choice(N_ITEMS, 120, replace=False))
    keys, X, n_used = core.fold_in(nu, ni, nr, reg=REG)
    S = X.double().cpu().numpy() @ core.V[:, :8].double().cpu().numpy().T
    return dict(core=core, u=nu, i=ni, r=nr, cand=cand, keys=keys.cpu().numpy(), S=S,
                n_used=n_used.cpu().numpy(), ghost=ghost)


def _check_lists(sv, keys, ids, sc, exclude_rated, top=10):
    keys, ids, sc = (np.asarray(x.cpu().numpy() if torch.is_tensor(x) else x) for x in (keys, ids, sc))
    assert sv["ghost"] not in keys and len(keys) == 50
    np.testing.assert_array_equal(keys, sv["keys"][sv["n_used"] > 0])
    for key, row_ids, row_sc in zip(keys, ids, sc):
        row = int(np.nonzero(sv["keys"] == key)[0][0])
        rated = set(sv["i"][sv["u"] == key].tolist())
        assert np.isfinite(row_sc).all() and len(set(row_ids.tolist())) == top
        assert set(row_ids.tolist()) <= set(sv["cand"].tolist())
        if not exclude_rated:
            continue
        assert not (set(row_ids.tolist()) & rated)
        s = sv["S"][row]
        np.testing.assert_allclose(row_sc, s[row_ids], rtol=1e-5, atol=0)
        adm = np.zeros(N_ITEMS, bool)
        adm[sv["cand"]] = True
        adm[list(rated)] = False
        best = np.sort(s[adm])[::-1][:top]
        np.testing.assert_allclose(np.sort(row_sc)[::-1], best, rtol=1e-5, atol=0)
        assert (np.diff(row_sc) <= 0).all()


def test_recommend_new(served):
    sv = served
    out = sv["core"].recommend_new(sv["u"], sv["i"], sv["r"], 10, reg=REG, candidates=sv["cand"])
    assert out[1].shape == out[2].shape == (50, 10)
    _check_lists(sv, *out, exclude_rated=True)
    out = sv["core"].recommend_new(sv["u"], sv["i"], sv["r"], 10, reg=REG, candidates=sv["cand"],
                                   exclude_rated=False)
    _check_lists(sv, *out, exclude_rated=False)


def test_public_surfaces_agree_with_the_engine(fitted, served):
    import pandas as pd

    from als_mi355x.mllib.recommendation import MatrixFactorizationModel
    model, *_ = fitted
    sv = served
    keys, ids, sc = (x.cpu().numpy() for x in sv["core"].recommend_new(
        sv["u"], sv["i"], sv["r"], 10, reg=REG, candidates=sv["cand"]))
    df = pd.DataFrame({"user": sv["u"], "item": sv["i"], "rating": sv["r"]})
    recs = model.recommendForNewUsers(df, 10, candidates=sv["cand"])
    assert list(recs.columns) == ["user", "recommendations"]
    np.testing.assert_array_equal(recs["user"].to_numpy(), keys)
    for row, lst in enumerate(recs["recommendations"]):
        assert [a for a, _ in lst] == ids[row].tolist()
        assert [b for _, b in lst] == [float(x) for x in sc[row]]
    mf = MatrixFactorizationModel(sv["core"])
    got = mf.recommendProductsForNewUsers(np.stack([sv["u"], sv["i"], sv["r"]], 1), 10, REG,
                                          candidates=sv["cand"])
    assert [k for k, _ in got] == keys.tolist()
    for row, (k, lst) in enumerate(got):
        assert all(x.user == k for x in lst)
        assert [x.product for x in lst] == ids[row].tolist()
        assert [x.rating for x in lst] == [float(x) for x in sc[row]]
    feats = mf.foldInUsers(np.stack([sv["u"], sv["i"], sv["r"]], 1), REG)
    assert [k for k, _ in feats] == sv["keys"].tolist()
    both = mf.recommendProductsForNewUsers(np.stack([sv["u"], sv["i"], sv["r"]], 1), 10, REG,
                                           candidates=sv["cand"], exclude_rated=False)
    assert len(both) == 50 and all(len(lst) == 10 for _, lst in both)


def test_personal_recommendations_fold_in(fitted):
    """The reference's 12 personal ratings (tests/golden/personal_ratings.json; movie ids
    folded onto this model's 200 items, the repeat that makes is kept as a duplicate
    rating) served without the retrain of R:218."""
    from als_mi355x import personal
    model, *_ = fitted
    gold = json.load(open(os.path.join(HERE, "golden", "personal_ratings.json")))
    rated = [(u, m % N_ITEMS, r) for u, m, r in gold["my_rated_movies"]]
    assert len(rated) == 12
    movies = [(m, f"m{m}") for m in range(N_ITEMS)] + [(10 ** 6, "never seen")]
    counts = {m: (50 + m, 3.0) if m % 2 else 50 + m for m in range(N_ITEMS)}  # both forms
    top = personal.personal_recommendations_fold_in(model, rated, movies, counts, REG)
    assert len(top) == 20
    preds = [p for p, _, _ in top]
    assert preds == sorted(preds, reverse=True)
    assert all(n > 75 for _, _, n in top)
    assert all(isinstance(p, float) and isinstance(t, str) and isinstance(n, int) for p, t, n in top)
    u, m, r = (np.asarray(x) for x in zip(*rated))
    _, X, _ = model.engine.fold_in(u, m, r.astype(np.float32), reg=REG)
    s = (X.double().cpu().numpy() @ model.engine.V[:, :8].double().cpu().numpy().T)[0]
    rated_m = {int(x) for x in m}
    for p, title, n in top:
        mid = int(title[1:])
        assert mid not in rated_m and n == 50 + mid
        assert abs(p - s[mid]) <= 1e-5 * abs(s[mid])
    adm = np.array([50 + j > 75 and j not in rated_m for j in range(N_ITEMS)])
    np.testing.assert_allclose(preds, np.sort(s[adm])[::-1][:20], rtol=1e-5, atol=0)
    assert personal.personal_recommendations_fold_in(model, rated, movies, counts, REG,
                                                     min_count=10 ** 6) == []
