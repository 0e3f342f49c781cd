"""Explain (K11, als_explain) on the GPU: kernel parity against the fp64 reference
(tests/explain_ref.py), list order, the sum invariant, agreement with K7, the status word,
determinism, the grid stride, trained users against predict() and the public surfaces.

Errors, per (row, target): ||c - c_ref||_2 / ||c_ref||_2 over the contribution vector (the
whole of it for rows of <= 32 entries at top_n = 32, the listed head otherwise) and
|score - score_ref| / (||x_ref|| ||y_t||); the bar is the project's 1e-4 (as K7).  Measured
maxima (MI355X): see DESIGN.md section K11.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import explain_ref as R
from als_mi355x import engine as E
from helpers import explain_check_slots, explain_reference, ragged_csr, ragged_ptr, report

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
N_ITEMS = 200
REG = 0.1
ALPHA = 40.0
RANKS = (1, 8, 17, 33, 64, 100, 128)
TOPS = (1, 10, 32)
N_TARGETS = (1, 16, 17, 0, 17, 1, 16, 17, 16)   # per row of _rows: 0, 1, 16 and 17 all occur


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
    """(cols, vals) per row: lengths 0, 1, 2, k - 1, k, k + 1 and 300, one row of 40 entries
    of one item with ratings 1-5 (exact ties), one mixing valid cols with -1 and n_src (and,
    among the valid ones, a rating of 0 and a negative one: implicit contributions of 0)."""
    rng = np.random.default_rng(50 + k + seed)
    rows = []
    for n in (0, 1, 2, k - 1, k, k + 1, 300):
        rows.append((rng.integers(0, N_ITEMS, n), rng.integers(1, 6, n)))
    rows.append((np.full(40, 17), rng.integers(1, 6, 40)))
    mixed = rng.integers(0, N_ITEMS, 30)
    mixed[::3] = -1
    mixed[1::3] = N_ITEMS
    vals = rng.integers(1, 6, 30)
    vals[2], vals[5] = 0, -2
    rows.append((mixed, vals))
    return rows


def _targets(rows, counts, seed=0):
    """Ragged targets: counts[r] per row.  A list of 16 or more holds a -1, n_src, an item
    the row rated (when it has one) and a repeated target."""
    rng = np.random.default_rng(77 + seed)
    out = []
    for (c, _), n in zip(rows, counts):
        tg = rng.integers(0, N_ITEMS, n)
        if n >= 16:
            known = np.asarray(c)[(np.asarray(c) >= 0) & (np.asarray(c) < N_ITEMS)]
            tg[0], tg[4] = -1, N_ITEMS
            if len(known):
                tg[1] = known[0]
            tg[3] = tg[2]
        out.append(tg)
    return out


_csr = ragged_csr
_ragged = ragged_ptr
_reference = explain_reference   # per slot (row, target, score, pos, contrib), the full list


def _run(rows, targets, V, k, reg, implicit, top_n, alpha=ALPHA, ld=None, fill=0.0, fold=False):
    """One als_explain call: (score [T], pos [T, top_n], contrib [T, top_n], n_used, status)
    as numpy; fold=True appends als_fold_in's X of the same rows."""
    ptr, col, val = _csr(rows)
    tptr, tg = _ragged(targets)
    t = lambda a, d: torch.as_tensor(a).to(DEV, d).contiguous()
    ws = E.Workspace(torch.device(DEV))
    Vd = _dev(V, ld, fill)
    yty = E.compute_yty(_dev(V), N_ITEMS, k, ws) if implicit else None
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    args = (t(ptr, torch.int64), t(col, torch.int32), t(val, torch.float32), Vd, N_ITEMS, k, reg,
            implicit, alpha, yty)
    sc, pos, con, n_used = E.explain_rows(*args, t(tptr, torch.int64), t(tg, torch.int32), top_n,
                                          status, ws)
    torch.cuda.synchronize()
    out = (sc.cpu().numpy(), pos.cpu().numpy(), con.cpu().numpy(), n_used.cpu().numpy(),
           int(status.item()))
    if fold:
        st2 = torch.zeros(1, dtype=torch.int32, device=DEV)
        X, _ = E.fold_in_rows(*args, st2, ws)
        out += (X.cpu().numpy()[:, :k],)
    return out


@functools.lru_cache(maxsize=None)
def _parity_case(k, implicit):
    """(V, rows, targets, reference slots); the reference is computed once and never
    modified.  Asserts, on the reference alone, that every list's order is decided by the
    values: no two consecutive contributions closer than 1e-9 max|c| unless equal."""
    V, rows = _factors(k), _rows(k)
    targets = _targets(rows, N_TARGETS)
    ref = _reference(rows, targets, V, REG, implicit, ALPHA)
    for r, t, _, pos, con in ref:
        assert R.well_separated(con, pos), (k, implicit, r, t)
    return V, rows, targets, ref


_check_slots = explain_check_slots   # -> (max contribution error, max score error)


# ------------------------------------------------------------------ kernel
@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
@pytest.mark.parametrize("k", RANKS)
def test_kernel_parity(k, implicit):
    """Y is stored with ld > k and 7.5 in the padding; every top_n of TOPS."""
    V, rows, targets, ref = _parity_case(k, implicit)
    assert sorted(set(N_TARGETS)) == [0, 1, 16, 17]
    ld = (k + 4 + 3) // 4 * 4
    n_ref = [int(((np.asarray(c) >= 0) & (np.asarray(c) < N_ITEMS)).sum()) for c, _ in rows]
    worst_c = worst_s = 0.0
    for top_n in TOPS:
        sc, pos, con, n_used, status = _run(rows, targets, V, k, REG, implicit, top_n, ld=ld,
                                            fill=7.5)
        assert status == 0
        np.testing.assert_array_equal(n_used, n_ref)
        e_c, e_s = _check_slots(ref, rows, V, k, REG, implicit, ALPHA, sc, pos, con, top_n)
        worst_c, worst_s = max(worst_c, e_c), max(worst_s, e_s)
    print(f"explain parity k={k} implicit={implicit}: max rel contribution err {worst_c:.3e}, "
          f"max score err {worst_s:.3e}")
    report(f"explain_parity_contrib[k={k},implicit={implicit}]", worst_c)
    report(f"explain_parity_score[k={k},implicit={implicit}]", worst_s)
    assert worst_c < 1e-4 and worst_s < 1e-4


@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
def test_repeated_item_ties_come_in_ascending_position(implicit):
    k = 17
    V, rows, targets, ref = _parity_case(k, implicit)
    _, pos, con, _, _ = _run(rows, targets, V, k, REG, implicit, 32)
    row = 7
    vals = np.asarray(rows[row][1])
    assert len(set(rows[row][0].tolist())) == 1 and len(vals) == 40
    slots = [s for s, x in enumerate(ref) if x[0] == row and len(x[3])]
    assert slots
    for s in slots:
        p, c = pos[s], con[s]
        assert (np.diff(c) <= 0).all()
        for a, b in zip(range(31), range(1, 32)):
            if vals[p[a]] == vals[p[b]]:
                assert c[a] == c[b] and p[a] < p[b]      # bit-equal, earlier entry first


@pytest.mark.parametrize("k,implicit", [(8, False), (33, True), (128, False)])
def test_listed_contributions_sum_to_the_score(k, implicit):
    """Rows of <= 32 entries at top_n = 32 list everything: the fp32 contributions sum to
    the fp32 score within 32 * 2^-23 * sum|c|."""
    V, rows, targets, ref = _parity_case(k, implicit)
    sc, pos, con, _, _ = _run(rows, targets, V, k, REG, implicit, 32)
    seen = 0
    for s, (r, _, _, p_ref, _) in enumerate(ref):
        if 0 < len(rows[r][0]) <= 32 and len(p_ref):
            c = con[s].astype(np.float64)
            assert abs(c.sum() - float(sc[s])) <= 32 * 2.0 ** -23 * np.abs(c).sum()
            seen += 1
    assert seen > 20


@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
@pytest.mark.parametrize("k", (8, 64, 128))
def test_score_agrees_with_fold_in(k, implicit):
    """score = y_t . x with x from als_fold_in on the same inputs: two fp64 computations
    rounded to fp32, within 2^-22 of ||x|| ||y_t||."""
    V, rows, targets, ref = _parity_case(k, implicit)
    sc, _, _, _, _, X = _run(rows, targets, V, k, REG, implicit, 10, fold=True)
    Vd, X = V.astype(np.float64), X.astype(np.float64)
    worst = 0.0
    for s, (r, t, _, p_ref, _) in enumerate(ref):
        if len(p_ref):
            worst = max(worst, abs(sc[s] - X[r] @ Vd[t])
                        / (np.linalg.norm(X[r]) * np.linalg.norm(Vd[t])))
    print(f"explain vs fold_in k={k} implicit={implicit}: {worst:.3e}")
    assert worst <= 2.0 ** -22


def test_failed_pivot_sets_status_and_spares_the_other_rows():
    """Explicit, reg = 0, k = 8: a row with 3 ratings has a rank-3 A.  The word names it, its
    slots read as empty, and the other rows of the call are explained as usual."""
    k = 8
    V = _factors(k, seed=3)
    rng = np.random.default_rng(9)
    rows = [(rng.choice(N_ITEMS, 20, replace=False), rng.integers(1, 6, 20)) for _ in range(5)]
    rows.insert(2, (np.array([5, 70, 131]), np.array([4, 2, 5])))
    targets = [rng.integers(0, N_ITEMS, 2) for _ in rows]
    sc, pos, con, n_used, status = _run(rows, targets, V, k, 0.0, False, 10)
    assert status == 3
    assert (sc[4:6] == 0).all() and (pos[4:6] == -1).all() and (con[4:6] == 0).all()
    np.testing.assert_array_equal(n_used, [len(c) for c, _ in rows])
    good = [0, 1, 3, 4, 5]
    ref = _reference([rows[r] for r in good], [targets[r] for r in good], V, 0.0, False, 1.0)
    keep = np.array([s for s in range(12) if s // 2 != 2])
    for r, t, _, p, c in ref:
        assert R.well_separated(c, p)
    e_c, e_s = _check_slots(ref, [rows[r] for r in good], V, k, 0.0, False, 1.0, sc[keep],
                            pos[keep], con[keep], 10)
    print(f"explain status case: other rows contribution err {e_c:.3e}, score err {e_s:.3e}")
    assert e_c < 1e-4 and e_s < 1e-4


@pytest.mark.parametrize("k,implicit", [(33, False), (128, True)])
def test_two_calls_are_bit_identical(k, implicit):
    V, rows, targets, _ = _parity_case(k, implicit)
    a = _run(rows, targets, V, k, REG, implicit, 10)
    b = _run(rows, targets, V, k, REG, implicit, 10)
    for x, y in zip(a[:4], b[:4]):
        assert x.tobytes() == y.tobytes()


def test_grid_stride_rows_past_65536():
    """Rank 8, 65,600 rows of 1-3 entries, one target each, top_n = 2: the only shape where
    a workgroup takes a second row.  Every row against a vectorised fp64 reference."""
    k, n, top_n = 8, 65600, 2
    V = _factors(k, seed=5)
    Vd = V.astype(np.float64)
    rng = np.random.default_rng(123)
    lens = rng.integers(1, 4, n)
    cols = rng.integers(0, N_ITEMS, (n, 3))
    vals = rng.integers(1, 6, (n, 3)).astype(np.float64)
    tg = rng.integers(0, N_ITEMS, n)
    m = np.arange(3)[None, :] < lens[:, None]
    Yj = Vd[cols] * m[:, :, None]
    A = np.einsum("nja,njb->nab", Yj, Yj) + (REG * lens)[:, None, None] * np.eye(k)
    z = np.linalg.solve(A, Vd[tg][:, :, None])[:, :, 0]
    c = np.where(m, vals * np.einsum("nja,na->nj", Yj, z), -np.inf)
    order = np.argsort(-c, axis=1, kind="stable")        # ties: the earlier entry first
    c_ord = np.take_along_axis(c, order, 1)
    s_ref = np.where(m, c, 0.0).sum(1)
    top = np.abs(np.where(m, c, 0.0)).max(1)
    gap = np.abs(np.diff(np.where(np.isfinite(c_ord), c_ord, 0.0), axis=1))
    both = np.isfinite(c_ord[:, 1:]) & np.isfinite(c_ord[:, :-1])
    assert (~both | (gap == 0) | (gap >= 1e-9 * top[:, None])).all()
    rows_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=rows_ptr[1:])
    t = lambda a, d: torch.as_tensor(a).to(DEV, d).contiguous()
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    sc, pos, con, n_used = E.explain_rows(
        t(rows_ptr, torch.int64), t(cols[m], torch.int32), t(vals[m], torch.float32), _dev(V),
        N_ITEMS, k, REG, False, 1.0, None, t(np.arange(n + 1), torch.int64), t(tg, torch.int32),
        top_n, status, E.Workspace(torch.device(DEV)))
    torch.cuda.synchronize()
    sc, pos, con = sc.cpu().numpy(), pos.cpu().numpy(), con.cpu().numpy()
    assert int(status.item()) == 0
    np.testing.assert_array_equal(n_used.cpu().numpy(), lens)
    want_pos = np.where(np.isfinite(c_ord[:, :top_n]), order[:, :top_n], -1)
    want_c = np.where(np.isfinite(c_ord[:, :top_n]), c_ord[:, :top_n], 0.0)
    np.testing.assert_array_equal(pos, want_pos)
    scale = np.maximum(np.linalg.norm(want_c, axis=1), 1e-300)
    e_c = (np.linalg.norm(con - want_c, axis=1) / scale).max()
    x = np.linalg.solve(A, np.einsum("nja,nj->na", Yj, vals * m)[:, :, None])[:, :, 0]
    e_s = (np.abs(sc - s_ref) / (np.linalg.norm(x, axis=1) * np.linalg.norm(Vd[tg], axis=1))).max()
    print(f"explain grid stride: contribution err {e_c:.3e}, score err {e_s:.3e}")
    assert e_c < 1e-4 and e_s < 1e-4


# ------------------------------------------------------------------ trained users
def _train_ratings(seed=0):
    """300 x 200, 6,000 distinct (user, item) pairs, ratings 1-5."""
    rng = np.random.default_rng(seed)
    cell = rng.choice(300 * N_ITEMS, 6000, replace=False)
    r = np.clip(np.round(3.5 + rng.normal(0, 1, 6000)), 1, 5).astype(np.float32)
    return (cell // N_ITEMS).astype(np.int32), (cell % N_ITEMS).astype(np.int32), r


@pytest.fixture(scope="module")
def fitted():
    """(ml ALSModel, u, i, r): explicit, rank 8, 5 iterations.  Never modified by a test."""
    import pandas as pd

    from als_mi355x.ml.recommendation import ALS
    u, i, r = _train_ratings()
    model = ALS(rank=8, maxIter=5, regParam=REG, seed=5).fit(
        pd.DataFrame({"user": u, "item": i, "rating": r}))
    return model, u, i, r


def _pairs_of(u, seed=3, n=200):
    rng = np.random.default_rng(seed)
    return rng.choice(np.unique(u), n).astype(np.int32), rng.integers(0, N_ITEMS, n).astype(np.int32)


@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
def test_trained_users_scores_are_the_predictions(implicit):
    """ALSCore.explain with ratings=None on pairs of trained users reproduces predict()
    within the project's per-row bar, |score - predict| <= 1e-4 ||x_u|| ||y_i|| (Cauchy-
    Schwarz over the per-row 1e-4).  It holds because iterate() solves the users last: U is
    the solution of exactly the normal equations explain rebuilds from the final V."""
    u, i, r = _train_ratings(seed=1)
    alpha = 2.0 if implicit else 1.0
    core = E.ALSCore(u, i, r)
    core.fit(8, 5, REG, implicit=implicit, alpha=alpha, seed=5)
    pu, pi = _pairs_of(u)
    uu, ii, sc, ids, rat, con, n = core.explain(pu, pi, 10, reg=REG, implicit=implicit,
                                                alpha=alpha)
    np.testing.assert_array_equal(uu.cpu().numpy(), pu)       # all known, input order
    np.testing.assert_array_equal(ii.cpu().numpy(), pi)
    pred = core.predict(pu, pi).cpu().numpy()
    known = ~np.isnan(pred)
    assert known.sum() > 150
    U = core.U[:, :8].double().cpu().numpy()[core.uidx.rows_of(uu).cpu().numpy()]
    Vt = core.V[:, :8].double().cpu().numpy()[core.iidx.rows_of(ii).cpu().numpy()]
    bound = 1e-4 * np.linalg.norm(U, axis=1) * np.linalg.norm(Vt, axis=1)
    err = np.abs(sc.cpu().numpy().astype(np.float64) - pred)
    print(f"explain vs predict implicit={implicit}: max err / bound "
          f"{(err[known] / bound[known]).max():.3e}")
    assert (err[known] <= bound[known]).all()
    assert np.isnan(sc.cpu().numpy()[~known]).all() and (n.cpu().numpy()[~known] == 0).all()
    # the lists name what the user rated, with the rating given
    n, ids, rat = n.cpu().numpy(), ids.cpu().numpy(), rat.cpu().numpy()
    for p in np.nonzero(known)[0][:40]:
        mine = {(int(a), float(b)) for a, b in zip(i[u == pu[p]], r[u == pu[p]])}
        assert n[p] == min(10, len(mine))
        assert {(int(a), float(b)) for a, b in zip(ids[p, :n[p]], rat[p, :n[p]])} <= mine
        assert (ids[p, n[p]:] == -1).all()


def test_items_side_and_grouping(fitted):
    """user_side=False explains item rows against U; pairs come back in input order."""
    model, u, i, r = fitted
    core = model.engine
    pu, pi = _pairs_of(u, seed=8, n=50)
    uu, ii, sc, ids, rat, con, n = (x.cpu().numpy() for x in core.explain(
        pu, pi, 5, reg=REG, user_side=False))
    rated_items = np.isin(pi, i)
    np.testing.assert_array_equal(uu, pu[rated_items])
    np.testing.assert_array_equal(ii, pi[rated_items])
    U = core.U[:, :8].cpu().numpy()
    for p in range(0, len(uu), 7):
        cols = core.uidx.rows_of(torch.as_tensor(u[i == ii[p]]).to(DEV)).cpu().numpy()
        (s, pos, c), = R.explain_row(cols, r[i == ii[p]], U, [int(core.uidx.rows_of(
            torch.as_tensor(uu[p:p + 1]).to(DEV)).item())], REG, False, 1.0)
        m = min(5, len(pos))
        assert n[p] == m and abs(float(sc[p]) - s) <= 1e-5 * max(abs(s), 1e-3)
        np.testing.assert_array_equal(ids[p, :m], u[i == ii[p]][pos[:m]])
        np.testing.assert_allclose(con[p, :m], c[:m], rtol=1e-5, atol=1e-7)


# ------------------------------------------------------------------ surfaces
def test_ml_and_mllib_surfaces(fitted):
    import pandas as pd

    from als_mi355x.mllib.recommendation import MatrixFactorizationModel
    model, u, i, r = fitted
    pu, pi = _pairs_of(u, seed=4, n=30)
    pu[0] = 10 ** 6                                  # a user the model does not know: dropped
    eng = [x.cpu().numpy() for x in model.engine.explain(pu, pi, 5, reg=REG)]
    df = model.explainRecommendations(pd.DataFrame({"user": pu, "item": pi}), 5)
    assert list(df.columns) == ["user", "item", "prediction", "contributions"]
    assert len(df) == 29 and 10 ** 6 not in df["user"].to_numpy()
    np.testing.assert_array_equal(df["user"].to_numpy(), eng[0])
    np.testing.assert_array_equal(df["prediction"].to_numpy(), eng[2])
    for p, lst in enumerate(df["contributions"]):
        assert len(lst) == eng[6][p] <= 5
        assert [a for a, _, _ in lst] == eng[3][p, :len(lst)].tolist()
        assert [c for _, _, c in lst] == [float(x) for x in eng[5][p, :len(lst)]]
        assert all(isinstance(a, int) and isinstance(b, float) for a, b, _ in lst)
    got = MatrixFactorizationModel(model.engine).explain(np.stack([pu, pi], 1), REG, 5)
    assert len(got) == 29
    for p, (a, b, s, lst) in enumerate(got):
        assert (a, b) == (int(eng[0][p]), int(eng[1][p]))
        assert s == float(eng[2][p]) or np.isnan(s)
        assert lst == df["contributions"][p]


def test_loaded_model_explains_from_given_ratings(fitted, tmp_path):
    """A saved and loaded model holds no ratings: it refuses ratings=None and, given the
    users' ratings, returns the live model's contributions."""
    import pandas as pd

    from als_mi355x.ml.recommendation import ALSModel
    model, u, i, r = fitted
    model.save(str(tmp_path / "m"))
    loaded = ALSModel.load(str(tmp_path / "m"))
    pu, pi = _pairs_of(u, seed=6, n=40)
    pairs = pd.DataFrame({"user": pu, "item": pi})
    with pytest.raises(ValueError, match="ratings"):
        loaded.explainRecommendations(pairs, 10)
    sel = np.isin(u, pu)
    mine = pd.DataFrame({"user": u[sel], "item": i[sel], "rating": r[sel]})
    a = model.explainRecommendations(pairs, 10)
    b = loaded.explainRecommendations(pairs, 10, ratings=mine)
    assert len(a) == len(b) == 40
    # the training block keeps a user's ratings in input order, as ragged_rows does
    np.testing.assert_array_equal(a["prediction"].to_numpy(), b["prediction"].to_numpy())
    assert a["contributions"].tolist() == b["contributions"].tolist()


def test_personal_explanations(fitted):
    """The reference's 12 personal ratings (tests/golden/personal_ratings.json, movie ids
    folded onto this model's 200 items): titles instead of ids, and predictions equal to
    what the fold-in serves."""
    from als_mi355x import personal
    model, *_ = fitted
    gold = json.load(open(os.path.join(HERE, "golden", "personal_ratings.json")))
    rated = [(u, m % N_ITEMS, r) for u, m, r in gold["my_rated_movies"]]
    movies = [(m, f"m{m}") for m in range(N_ITEMS)]
    counts = {m: 100 for m in range(N_ITEMS)}
    top = personal.personal_recommendations_fold_in(model, rated, movies, counts, REG)
    want = [int(t[1:]) for _, t, _ in top]
    out = personal.personal_explanations(model, rated, movies, want + [10 ** 6], REG, num=5)
    assert [t for t, _, _ in out] == [f"m{m}" for m in want]   # the unknown movie is absent
    rated_titles = {f"m{m}": float(r) for _, m, r in rated}
    for (p, _, _), (title, pred, lst) in zip(top, out):
        assert abs(pred - p) <= 1e-5 * max(abs(p), 1.0)
        assert len(lst) == 5 and all(isinstance(t, str) for t, _, _ in lst)
        assert all(t in rated_titles for t, _, _ in lst)
        cs = [c for _, _, c in lst]
        assert cs == sorted(cs, reverse=True)
