"""Filtered top-k (als_topk_filtered) on the GPU: kernel parity against a numpy ranking,
bit-exactness against the unfiltered kernel, sliced launches, edge rows, and the
exclude= / candidates= keywords of the public surfaces.

Reference ranking: fp64 Q @ V.T, inadmissible entries (excluded, not allowed, NaN) set
to -inf, ranked by (score descending, index ascending).  Tolerances are those of
test_gpu_kernels.test_topk_parity: an index may differ from the reference only where the
fp64 scores tie within 1e-5 relative, scores are compared at rtol = atol = 1e-5.
"""
import functools

import numpy as np
import pytest
import torch

from als_mi355x import engine as E
from als_mi355x import filters as F
from helpers import topk_ranking_check as _check  # the reference ranking of the docstring
from oracle import als_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------ helpers
def _dev(M, rank):
    out = torch.zeros((M.shape[0], E.ld_for(rank)), device=DEV)
    out[:, :rank] = torch.as_tensor(M).to(DEV)
    return out


def _ex_arrays(lists):
    """Per-row python lists -> (begin, end, col) device tensors (each list sorted here)."""
    lens = np.array([len(x) for x in lists], np.int64)
    end = np.cumsum(lens)
    beg = end - lens
    col = np.concatenate([np.sort(np.asarray(x, np.int64)) for x in lists] + [np.zeros(1, np.int64)])
    t = lambda a, d: torch.as_tensor(a).to(DEV, d).contiguous()
    return t(beg, torch.int64), t(end, torch.int64), t(col, torch.int32)


def _admissible(n_q, n_v, lists, allow):
    adm = np.ones((n_q, n_v), bool)
    if lists is not None:
        for r, x in enumerate(lists):
            adm[r, np.asarray(x, np.int64)] = False
    if allow is not None:
        adm &= np.asarray(allow, bool)[None, :]
    return adm


def _bits(allow):
    return None if allow is None else F.pack_allow_bits(
        torch.as_tensor(np.nonzero(allow)[0]).to(DEV), len(allow))


def _run(Qd, n_q, Vd, n_v, rank, top, lists, allow):
    ex = _ex_arrays(lists) if lists is not None else (None, None, None)
    idx, sc = E.topk_rows_filtered(Qd, n_q, Vd, n_v, rank, top, *ex, _bits(allow))
    torch.cuda.synchronize()
    return idx.cpu().numpy(), sc.cpu().numpy()


# ------------------------------------------------------------------ 1. parity grid
@functools.lru_cache(maxsize=None)
def _grid_case(rank, n_q, n_v):
    """N(0, 1) factors with one exact tie, a per-row exclusion list of seven kinds and three
    allow masks; n_v >= 5 (the small sizes serve test_gpu_buffer_bounds.py)."""
    rng = np.random.default_rng(100 + rank)
    Q = rng.standard_normal((n_q, rank)).astype(np.float32)
    Vm = rng.standard_normal((n_v, rank)).astype(np.float32)
    lo, hi = (10, 20) if n_v > 20 else (1, n_v - 1)
    Vm[lo] = Vm[hi]  # exact tie: the lower index first; hi alone where lo is excluded
    top50, _ = O.topk(Q, Vm, min(50, n_v))
    lists = []
    for r in range(n_q):
        kind = r % 7
        if kind == 0:
            x = []
        elif kind == 1:
            x = list(top50[r])                                   # the row's own unfiltered top-50
        elif kind == 2:
            x = list(np.delete(np.arange(n_v), rng.choice(n_v, 3, replace=False)))  # all but 3
        elif kind == 3:
            x = list(range(n_v))                                 # everything
        elif kind == 4:
            x = list(rng.integers(0, n_v, 40)) * 2 + [int(top50[r][0])] * 3  # duplicates
        elif kind == 5:
            x = [0, n_v - 1] + list(rng.choice(np.arange(1, n_v - 1), min(25, n_v - 2),
                                               replace=False))
        else:
            x = [lo] + list(top50[r][:3])                        # lo excluded: hi stands alone
        lists.append([int(v) for v in x])
    S = Q.astype(np.float64) @ Vm.astype(np.float64).T
    allows = {"none": None, "half": rng.random(n_v) < 0.5, "five": np.zeros(n_v, bool)}
    allows["five"][[j for j in (3, 10, 20, 777, n_v - 1) if j < n_v]] = True
    return Q, Vm, S, lists, allows


def _grid(rank):
    return _grid_case(rank, 333, 1500)


@pytest.mark.parametrize("allow", ["none", "half", "five"])
@pytest.mark.parametrize("rank,top", [(10, 10), (64, 16), (64, 20), (128, 100), (64, 200)])
def test_filtered_parity_grid(rank, top, allow):
    Q, Vm, S, lists, allows = _grid(rank)
    n_q, n_v = S.shape
    a = allows[allow]
    idx, sc = _run(_dev(Q, rank), n_q, _dev(Vm, rank), n_v, rank, top, lists, a)
    adm = _admissible(n_q, n_v, lists, a)
    _check(idx, sc, S, adm, top)
    for r in range(n_q):  # the exact tie 10 / 20 (20 alone where 10 is excluded: _check)
        lst = list(idx[r])
        if 10 in lst and 20 in lst:
            assert lst.index(10) < lst.index(20)


# ------------------------------------------------------------------ 2. bit-exact
@pytest.mark.parametrize("rank", [10, 128])
def test_filtered_lists_are_the_unfiltered_ranking_restricted(rank):
    """n_v = 250 at top = 256: the unfiltered call yields every row's full ranking; each
    filtered list must be its first `top` admissible entries, indices and score bits."""
    rng = np.random.default_rng(rank)
    n_q, n_v = 150, 250
    Q = rng.standard_normal((n_q, rank)).astype(np.float32)
    Vm = rng.standard_normal((n_v, rank)).astype(np.float32)
    Vm[7] = Vm[200]
    Qd, Vd = _dev(Q, rank), _dev(Vm, rank)
    full_i, full_s = E.topk_rows(Qd, n_q, Vd, n_v, rank, 256)
    full_i, full_s = full_i.cpu().numpy(), full_s.cpu().numpy()
    assert (full_i[:, :n_v] >= 0).all() and (full_i[:, n_v:] == -1).all()
    lists = [[int(v) for v in rng.choice(n_v, int(rng.integers(0, 120)), replace=False)]
             for _ in range(n_q)]
    allow = rng.random(n_v) < 0.6
    adm = _admissible(n_q, n_v, lists, allow)
    for top in (10, 20, 200):
        idx, sc = _run(Qd, n_q, Vd, n_v, rank, top, lists, allow)
        for r in range(n_q):
            keep = adm[r, full_i[r, :n_v]]
            want_i = full_i[r, :n_v][keep][:top]
            want_s = full_s[r, :n_v][keep][:top]
            n = len(want_i)
            np.testing.assert_array_equal(idx[r, :n], want_i)
            np.testing.assert_array_equal(sc[r, :n].view(np.int32), want_s.view(np.int32))
            assert (idx[r, n:] == -1).all() and np.isneginf(sc[r, n:]).all()


# ------------------------------------------------------------------ 3. no filter
@pytest.mark.parametrize("rank,top", [(10, 10), (64, 20), (64, 200)])
def test_all_filters_null_is_topk_rows(rank, top):
    Q, Vm, _, _, _ = _grid(rank)
    Qd, Vd = _dev(Q, rank), _dev(Vm, rank)
    a_i, a_s = E.topk_rows(Qd, len(Q), Vd, len(Vm), rank, top)
    b_i, b_s = E.topk_rows_filtered(Qd, len(Q), Vd, len(Vm), rank, top, None, None, None, None)
    assert torch.equal(a_i, b_i) and torch.equal(a_s.view(torch.int32), b_s.view(torch.int32))


# ------------------------------------------------------------------ 4. many tiles
@pytest.mark.parametrize("top", [10, 50])
def test_filtered_many_tiles(top):
    rank, n_v, n_q = 64, 20011, 261
    rng = np.random.default_rng(n_v + top)
    Q = rng.standard_normal((n_q, rank)).astype(np.float32)
    Vm = rng.standard_normal((n_v, rank)).astype(np.float32)
    Vm *= (1.0 + 3.0 * (np.arange(n_v) % 97 == 0))[:, None].astype(np.float32)  # strong items
    top30, _ = O.topk(Q, Vm, 30)
    lists = [[int(v) for v in np.concatenate([top30[r], rng.integers(0, n_v, 200)])]
             for r in range(n_q)]
    idx, sc = _run(_dev(Q, rank), n_q, _dev(Vm, rank), n_v, rank, top, lists, None)
    S = Q.astype(np.float64) @ Vm.astype(np.float64).T
    _check(idx, sc, S, _admissible(n_q, n_v, lists, None), top)


# ------------------------------------------------------------------ 5. sliced launches
def test_sliced_launches_offset_the_exclusion_ranges():
    """70,000 query rows at top 20 run as two launches of the key-log kernel (65,536 rows
    each at most): the second launch must read ITS rows' exclusion ranges.  The same rows
    of the unfiltered call are checked against the oracle as well."""
    rank, top, n_q, n_v = 16, 20, 70000, 2000
    rng = np.random.default_rng(5)
    Q = rng.standard_normal((n_q, rank)).astype(np.float32)
    Vm = rng.standard_normal((n_v, rank)).astype(np.float32)
    Qd, Vd = _dev(Q, rank), _dev(Vm, rank)
    u_i, u_s = E.topk_rows(Qd, n_q, Vd, n_v, rank, top)
    rows = np.unique(np.concatenate([np.arange(64), np.arange(65536, 65664),
                                     rng.choice(n_q, 200, replace=False)]))
    S = Q[rows].astype(np.float64) @ Vm.astype(np.float64).T
    ref_i, ref_s = O.topk(Q[rows], Vm, top)
    ui, us = u_i.cpu().numpy()[rows], u_s.cpu().numpy()[rows]
    _check(ui, us, S, np.ones(S.shape, bool), top)           # unfiltered, sliced, vs numpy
    np.testing.assert_allclose(us, ref_s, rtol=1e-5, atol=1e-5)  # ... and vs the oracle
    for j in range(len(rows)):
        for p in np.nonzero(ui[j] != ref_i[j])[0]:  # only where fp64 scores tie within 1e-5
            assert abs(S[j, ui[j, p]] - ref_s[j, p]) <= 1e-5 * max(1, abs(ref_s[j, p]))
    # row r excludes its unfiltered top-5 and {r % n_v}: six entries per row, sorted
    ex = torch.cat([u_i[:, :5].long(), (torch.arange(n_q, device=DEV) % n_v)[:, None]], 1)
    ex = torch.sort(ex, dim=1).values
    beg = torch.arange(n_q, device=DEV, dtype=torch.int64) * 6
    idx, sc = E.topk_rows_filtered(Qd, n_q, Vd, n_v, rank, top, beg, beg + 6,
                                   ex.reshape(-1).to(torch.int32).contiguous(), None)
    idx, sc = idx.cpu().numpy()[rows], sc.cpu().numpy()[rows]
    exh = ex.cpu().numpy()
    adm = np.ones(S.shape, bool)
    for j, r in enumerate(rows):
        adm[j, exh[r]] = False
    _check(idx, sc, S, adm, top)


@pytest.mark.parametrize("top", [10, 20])
def test_two_row_groups_per_workgroup(top):
    """262,144 query rows: register lists and key logs run with two row groups per
    workgroup, so group 1's rows (128 .. 255 of every 256) index their own exclusion
    ranges.  Row r excludes its unfiltered top-3 and {r % n_v}; half the V rows allowed."""
    rank, n_q, n_v = 8, 262144, 96
    rng = np.random.default_rng(top)
    Q = rng.standard_normal((n_q, rank)).astype(np.float32)
    Vm = rng.standard_normal((n_v, rank)).astype(np.float32)
    Qd, Vd = _dev(Q, rank), _dev(Vm, rank)
    u_i, _ = E.topk_rows(Qd, n_q, Vd, n_v, rank, top)
    ex = torch.cat([u_i[:, :3].long(), (torch.arange(n_q, device=DEV) % n_v)[:, None]], 1)
    ex = torch.sort(ex, dim=1).values
    beg = torch.arange(n_q, device=DEV, dtype=torch.int64) * 4
    allow = rng.random(n_v) < 0.5
    idx, sc = E.topk_rows_filtered(Qd, n_q, Vd, n_v, rank, top, beg, beg + 4,
                                   ex.reshape(-1).to(torch.int32).contiguous(), _bits(allow))
    rows = np.unique(np.concatenate([np.arange(0, 512), np.arange(n_q - 300, n_q),
                                     rng.choice(n_q, 300, replace=False)]))
    idx, sc, exh = idx.cpu().numpy()[rows], sc.cpu().numpy()[rows], ex.cpu().numpy()[rows]
    S = Q[rows].astype(np.float64) @ Vm.astype(np.float64).T
    adm = np.repeat(allow[None, :], len(rows), 0)
    np.put_along_axis(adm, exh, False, 1)
    _check(idx, sc, S, adm, top)


# ------------------------------------------------------------------ 6. edge rows
@pytest.mark.parametrize("rank,top", [(10, 10), (64, 20), (10, 200)])
def test_zero_query_rows_and_mask_word_boundaries(rank, top):
    """An all-zero query row lists its first `top` admissible rows by index with score 0
    (indices 0..4 excluded, a sparse allow mask with bits 31, 32 and n_v - 1 set, n_v not
    a multiple of 32); the other rows rank under the same mask."""
    rng = np.random.default_rng(rank + top)
    n_q, n_v = 70, 1003
    Q = rng.standard_normal((n_q, rank)).astype(np.float32)
    Q[[3, 17, 69]] = 0.0
    Vm = rng.standard_normal((n_v, rank)).astype(np.float32)
    allow = np.zeros(n_v, bool)
    allow[::9] = True
    allow[[2, 31, 32, n_v - 1]] = True
    lists = [[0, 1, 2, 3, 4] if r % 2 else [] for r in range(n_q)]
    idx, sc = _run(_dev(Q, rank), n_q, _dev(Vm, rank), n_v, rank, top, lists, allow)
    S = Q.astype(np.float64) @ Vm.astype(np.float64).T
    adm = _admissible(n_q, n_v, lists, allow)
    _check(idx, sc, S, adm, top)
    for r in (3, 17, 69):
        want = np.nonzero(adm[r])[0][:top]
        np.testing.assert_array_equal(idx[r, :len(want)], want)
        assert (sc[r, :len(want)] == 0).all()
    assert 31 in idx[3] and 32 in idx[3] and 0 not in idx[3] and 2 not in idx[3]
    # only the three boundary bits: every non-zero row lists exactly those rows
    only = np.zeros(n_v, bool)
    only[[31, 32, n_v - 1]] = True
    idx, sc = _run(_dev(Q, rank), n_q, _dev(Vm, rank), n_v, rank, top, None, only)
    _check(idx, sc, S, _admissible(n_q, n_v, None, only), top)
    assert sorted(idx[0, :3].tolist()) == [31, 32, n_v - 1] and (idx[:, 3:] == -1).all()


@pytest.mark.parametrize("rank,top", [(10, 10), (64, 20), (10, 200)])
def test_nan_row_of_v_is_never_listed(rank, top):
    rng = np.random.default_rng(7 * rank + top)
    n_q, n_v = 50, 300
    Q = rng.standard_normal((n_q, rank)).astype(np.float32)
    Vm = rng.standard_normal((n_v, rank)).astype(np.float32)
    Vm[64, rank // 2] = np.nan  # allowed, never excluded
    allow = rng.random(n_v) < 0.7
    allow[64] = True
    lists = [[int(v) for v in rng.choice(np.delete(np.arange(n_v), 64), 30, replace=False)]
             for _ in range(n_q)]
    idx, sc = _run(_dev(Q, rank), n_q, _dev(Vm, rank), n_v, rank, top, lists, allow)
    assert not (idx == 64).any() and not np.isnan(sc).any()
    S = Q.astype(np.float64) @ Vm.astype(np.float64).T
    _check(idx, sc, S, _admissible(n_q, n_v, lists, allow), top)


# ------------------------------------------------------------------ 7. surfaces
GAP = 2  # ids = GAP x dense row (every user and item occurs in helpers.planted)


@pytest.fixture(scope="module")
def fitted():
    import pandas as pd

    from als_mi355x.ml.recommendation import ALS
    from helpers import planted
    u, i, r = planted(200, 120, density=0.12, seed=11, dup=40, id_gap=GAP)
    df = pd.DataFrame({"user": u, "item": i, "rating": r})
    model = ALS(rank=8, maxIter=3, regParam=0.1, seed=3).fit(df)
    core = model.engine
    U = core.U[:, :8].cpu().numpy().astype(np.float64)
    V = core.V[:, :8].cpu().numpy().astype(np.float64)
    return model, df, U, V, U @ V.T


def _lists_of_df(recs, key):
    return {int(k): ([a for a, _ in v], [b for _, b in v])
            for k, v in zip(recs[key], recs["recommendations"])}


def _check_recs(got, S, adm, top, gap=GAP):
    """got: id -> (listed ids, scores); S / adm indexed by dense row = id / gap."""
    for key, (ids, scs) in got.items():
        r = key // gap
        n = min(top, int(adm[r].sum()))
        idx = np.full((1, top), -1)
        sc = np.full((1, top), -np.inf, np.float32)
        assert len(ids) == n, (key, len(ids), n)
        idx[0, :n] = np.asarray(ids, np.int64) // gap
        sc[0, :n] = scs
        _check(idx, sc, S[r:r + 1], adm[r:r + 1], top)


def test_exclude_train_on_the_ml_surface(fitted):
    model, df, U, V, S = fitted
    n_u, n_i = S.shape
    adm = np.ones(S.shape, bool)
    adm[df["user"].to_numpy() // GAP, df["item"].to_numpy() // GAP] = False
    recs = model.recommendForAllUsers(10, exclude="train")
    got = _lists_of_df(recs, "user")
    assert len(got) == n_u
    trained = set(zip(df["user"].tolist(), df["item"].tolist()))
    assert not any((u, it) in trained for u, (ids, _) in got.items() for it in ids)
    _check_recs(got, S, adm, 10)
    # unfiltered lists do contain training pairs: the keyword is what removes them
    plain = _lists_of_df(model.recommendForAllUsers(10), "user")
    assert any((u, it) in trained for u, (ids, _) in plain.items() for it in ids)
    # candidates= restricts the ids listed; with the exclusion on top
    cand = [int(x) * GAP for x in range(0, n_i, 3)] + [10 ** 6]  # an unknown id is dropped
    adm_c = adm.copy()
    adm_c[:, [j for j in range(n_i) if j % 3]] = False
    got = _lists_of_df(model.recommendForAllUsers(10, exclude="train", candidates=cand), "user")
    assert all(it in set(cand) for ids, _ in got.values() for it in ids)
    _check_recs(got, S, adm_c, 10)
    # the Arrays form: empty slots keep score -inf
    keys, ids, sc = model.recommendForAllUsersArrays(50, candidates=cand[:7])
    assert ids.shape == (n_u, 50) and bool(torch.isinf(sc[:, 7:]).all())
    assert bool(torch.isfinite(sc[:, :7]).all())
    # the item side: users per item, training pairs excluded
    got = _lists_of_df(model.recommendForAllItems(10, exclude="train"), "item")
    _check_recs(got, S.T, adm.T, 10)
    got = _lists_of_df(model.recommendForItemSubset({"item": [0, 4, 10 ** 6]}, 10, exclude=df),
                       "item")
    assert sorted(got) == [0, 4]
    _check_recs(got, S.T, adm.T, 10)


def test_subset_with_explicit_pairs_and_unknown_ids(fitted):
    import pandas as pd
    model, df, U, V, S = fitted
    ex = pd.DataFrame({"user": [0, 0, 0, 6, 6, 10 ** 6, 8], "item": [0, 2, 2, 4, 10 ** 6, 4, 6]})
    adm = np.ones(S.shape, bool)
    adm[0, [0, 1]] = False
    adm[3, 2] = False
    adm[4, 3] = False
    got = _lists_of_df(model.recommendForUserSubset({"user": [6, 0, 8, 0, 999999]}, 12, exclude=ex),
                       "user")
    assert sorted(got) == [0, 6, 8]
    _check_recs(got, S, adm, 12)


def test_mllib_forms(fitted):
    from als_mi355x.mllib.recommendation import MatrixFactorizationModel
    model, df, U, V, S = fitted
    mf = MatrixFactorizationModel(model.engine)
    adm = np.ones(S.shape, bool)
    adm[df["user"].to_numpy() // GAP, df["item"].to_numpy() // GAP] = False
    cand_items = [int(x) * GAP for x in range(0, S.shape[1], 2)]
    adm_c = adm.copy()
    adm_c[:, 1::2] = False
    rs = mf.recommendProducts(4, 10, exclude="train", candidates=cand_items)
    assert all(x.user == 4 for x in rs)
    _check_recs({4: ([x.product for x in rs], [x.rating for x in rs])}, S, adm_c, 10)
    rs = mf.recommendUsers(6, 10, exclude=list(zip(df["user"].tolist(), df["item"].tolist())))
    assert all(x.product == 6 for x in rs)
    _check_recs({6: ([x.user for x in rs], [x.rating for x in rs])}, S.T, adm.T, 10)
    allp = dict(mf.recommendProductsForUsers(10, exclude="train"))
    _check_recs({k: ([x.product for x in v], [x.rating for x in v]) for k, v in allp.items()},
                S, adm, 10)
    allu = dict(mf.recommendUsersForProducts(10, exclude="train", candidates=[0, 2, 4, 6]))
    adm_u = adm.T.copy()
    adm_u[:, 4:] = False
    _check_recs({k: ([x.user for x in v], [x.rating for x in v]) for k, v in allu.items()},
                S.T, adm_u, 10)


def test_reloaded_model_has_no_training_pairs(fitted, tmp_path):
    from als_mi355x.ml.recommendation import ALSModel
    model, df, U, V, S = fitted
    model.save(str(tmp_path / "m"))
    loaded = ALSModel.load(str(tmp_path / "m"))
    with pytest.raises(ValueError, match="saved factors"):
        loaded.recommendForAllUsers(10, exclude="train")
    a = model.recommendForAllUsersArrays(10, exclude="train")
    b = loaded.recommendForAllUsersArrays(10, exclude=df)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_one_call_equals_the_personal_flow(fitted):
    """RecommenderSystem.py:229-247 as one call: exclude = the user's rated pairs,
    candidates = the movies with more than `min_count` ratings."""
    import pandas as pd

    from als_mi355x import personal
    model, df, U, V, S = fitted
    user, min_count = 0, 20
    triples = list(zip(df["user"].tolist(), df["item"].tolist(), df["rating"].tolist()))
    counts = personal.movie_counts_and_averages(triples)
    rated = [t for t in triples if t[0] == user]
    movies = [(int(m) * GAP, f"m{int(m) * GAP}") for m in range(S.shape[1])] + [(10 ** 6, "never seen")]
    want = personal.personal_recommendations(model, user, rated, movies, counts, min_count, 20)
    popular = [m for m, (c, _) in counts.items() if c > min_count]
    assert 20 <= len(popular) < S.shape[1]
    recs = model.recommendForUserSubset(
        {"user": [user]}, 20, exclude=pd.DataFrame({"user": [t[0] for t in rated],
                                                    "item": [t[1] for t in rated]}),
        candidates=popular)
    ids, scs = _lists_of_df(recs, "user")[user]
    assert len(ids) == len(want) == 20
    np.testing.assert_allclose(scs, [p for p, _, _ in want], rtol=1e-5, atol=1e-5)
    for p, (it, (pred, title, n)) in enumerate(zip(ids, want)):
        if f"m{it}" != title:  # only where the predictions tie within 1e-5
            assert abs(S[user // GAP, it // GAP] - pred) <= 1e-5 * max(1, abs(pred)), p
        assert counts[it][0] > min_count and (user, it) not in {(a, b) for a, b, _ in rated}
