"""Diversified lists (K14, als_diversify / als_list_similarity) on the GPU.

The greedy picks are checked by diversify_ref.check_greedy, which replays the kernel's own
picks against fp64 values (tolerance 2e-5, derived in diversify_ref.py); ILS against the fp64
reference at atol 1e-5.  lam = 1 must reproduce the live prefix of the pool exactly.
"""
import functools

import numpy as np
import pytest
import torch

import diversify_ref as R
from als_mi355x import _lib, engine as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_V = 1200


def _dev(M, rank, fill=float("nan")):
    """[n, ld > rank] on the device, the padding columns NaN."""
    out = torch.full((M.shape[0], E.ld_for(rank) + 4), fill, device=DEV)
    out[:, :rank] = torch.as_tensor(np.array(M, np.float32)).to(DEV)
    return out.contiguous()


@functools.lru_cache(maxsize=None)
def _table(rank, n=N_V):
    """N(0, 1) plus a shared direction: cosines spread over about (-0.2, 0.9)."""
    rng = np.random.default_rng(300 + rank)
    V = rng.standard_normal((n, rank)) + 2.0 * rng.random((n, 1))
    V = V.astype(np.float32)
    V.setflags(write=False)
    return V


def _pools(V, rank, n_q, m, seed=0):
    """Score-descending pools as K5 lists them, from random user vectors (host fp64 -> f32)."""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((n_q, rank)) + 0.5
    S = (Q @ V[:, :rank].astype(np.float64).T).astype(np.float32)
    idx = np.argsort(-S, axis=1, kind="stable")[:, :m].astype(np.int32)
    return idx, np.take_along_axis(S, idx, 1)


def _run(idx, sc, V, rank, top, lam, Vd=None):
    Vd = _dev(V, rank) if Vd is None else Vd
    oi, os_, ils = E.diversify_rows(torch.as_tensor(idx).to(DEV), torch.as_tensor(sc).to(DEV), Vd,
                                    len(V), rank, top, lam)
    torch.cuda.synchronize()
    return oi.cpu().numpy(), os_.cpu().numpy(), ils.cpu().numpy()


def _ils(idx, V, rank, Vd=None):
    Vd = _dev(V, rank) if Vd is None else Vd
    out = E.list_similarity_rows(torch.as_tensor(np.asarray(idx, np.int32)).to(DEV), Vd, len(V),
                                 rank)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(idx, sc, V, rank, top, lam):
    oi, os_, ils = _run(idx, sc, V, rank, top, lam)
    want = R.check_greedy(idx, sc, V, rank, lam, oi, os_, top)
    np.testing.assert_allclose(ils, want, rtol=0, atol=R.ILS_ATOL, equal_nan=True)
    return oi, os_, ils


# every value of each axis appears; not the full product
GRID = [  # rank, m, top, lam, n_q
    (1, 1, 1, 0.3, 1), (1, 65, 10, 0.0, 70), (3, 2, 2, 0.7, 70), (3, 100, 10, 0.3, 1),
    (8, 63, 63, 0.0, 70), (8, 64, 10, 0.7, 300), (8, 256, 10, 0.3, 70), (33, 65, 65, 0.7, 70),
    (33, 64, 1, 1.0, 1), (64, 100, 100, 0.3, 70), (64, 256, 256, 0.7, 1), (64, 2, 1, 0.0, 300),
    (65, 63, 10, 0.3, 70), (65, 256, 10, 1.0, 70), (128, 64, 64, 0.0, 70),
    (128, 256, 256, 0.3, 1), (128, 100, 1, 0.7, 300), (128, 1, 1, 1.0, 70)]


@pytest.mark.parametrize("rank,m,top,lam,n_q", GRID)
def test_greedy_and_ils_grid(rank, m, top, lam, n_q):
    V = _table(rank)
    idx, sc = _pools(V, rank, n_q, m, seed=m + top)
    oi, os_, _ = _check(idx, sc, V, rank, top, lam)
    assert (oi[:, 0] == idx[:, 0]).all()      # step 0 is the best-scored slot at any lam
    a, b, c = _run(idx, sc, V, rank, top, lam)
    d, e, f = _run(idx, sc, V, rank, top, lam)
    assert a.tobytes() == d.tobytes() and b.tobytes() == e.tobytes() and c.tobytes() == f.tobytes()


@pytest.mark.parametrize("rank,m", [(8, 64), (64, 128), (128, 256), (33, 50)])
def test_lam_one_is_the_live_prefix_exactly(rank, m):
    V = _table(rank)
    idx, sc = _pools(V, rank, 70, m, seed=5)
    idx, sc = idx.copy(), sc.copy()
    idx[3, m // 2:] = -1                      # a filtered row: -1 / -inf tail
    sc[3, m // 2:] = -np.inf
    sc[4, 1:] = sc[4, 0]                      # all scores equal: ties keep the slot order
    for top in sorted({1, min(10, m), m}):
        oi, os_, ils = _run(idx, sc, V, rank, top, 1.0)
        live = min(top, m // 2)
        np.testing.assert_array_equal(oi[3, :live], idx[3, :live])
        assert (oi[3, live:] == -1).all() and np.isneginf(os_[3, live:]).all()
        keep = np.arange(70) != 3
        np.testing.assert_array_equal(oi[keep], idx[keep, :top])
        assert os_[keep].tobytes() == sc[keep, :top].tobytes()
        pre = idx[:, :top].copy()
        pre[3, live:] = -1
        prefix_ils = _ils(pre, V, rank)
        assert np.array_equal(np.isnan(ils), np.isnan(prefix_ils))
        np.testing.assert_allclose(ils, prefix_ils, rtol=0, atol=1e-12, equal_nan=True)
        np.testing.assert_allclose(prefix_ils, R.list_similarity(pre, V, rank), rtol=0,
                                   atol=R.ILS_ATOL, equal_nan=True)


def test_dead_slots_in_the_middle_and_short_rows():
    rank, m = 8, 100
    V = _table(rank)
    idx, sc = _pools(V, rank, 6, m, seed=9)
    idx, sc = idx.copy(), sc.copy()
    idx[0, [0, 5, 70]] = -1                   # dead by index (the best slot among them)
    sc[0, [3, 64]] = [np.nan, np.inf]         # dead by score
    idx[1, 10:40] = N_V + np.arange(30)       # idx >= n_v is dead
    idx[1, 50] = np.iinfo(np.int32).max
    idx[2, :] = -1                            # no live slot
    sc[2, :] = -np.inf
    idx[3, 1:] = -1                           # one live slot
    sc[3, 1:] = -np.inf
    idx[4, :99] = -1                          # one live slot, the last
    sc[5, 2:] = -np.inf                       # two live slots
    for top, lam in ((10, 0.3), (100, 0.7), (100, 0.0)):
        oi, os_, ils = _check(idx, sc, V, rank, top, lam)
        assert oi[0, 0] == idx[0, 1]
        assert (oi[2] == -1).all() and np.isneginf(os_[2]).all() and np.isnan(ils[2])
        assert oi[3, 0] == idx[3, 0] and (oi[3, 1:] == -1).all() and np.isnan(ils[3])
        assert oi[4, 0] == idx[4, 99] and np.isnan(ils[4])
        assert (oi[5, :2] == idx[5, :2]).all() and (oi[5, 2:] == -1).all() and \
            np.isfinite(ils[5])
        assert (oi[1] < N_V).all()


def test_degenerate_candidates():
    rank = 8
    V = np.array(_table(rank)[:64])
    V[5] = 0                                  # zero norm
    V[6, 3] = np.inf                          # a non-finite entry
    V[7, 0] = np.nan
    V[20] = V[10]                             # identical vectors at different indices
    idx = np.array([[10, 20, 5, 6, 7, 30, 31, 32, 33, 34]], np.int32)
    sc = np.linspace(5, 4, 10).astype(np.float32)[None, :]
    oi, os_, ils = _check(idx, sc, V, rank, 10, 0.5)
    assert sorted(oi[0].tolist()) == sorted(idx[0].tolist())       # all still pickable
    lst = oi[0].tolist()
    assert lst[0] == 10 and lst.index(20) > lst.index(5)           # the twin is picked late
    np.testing.assert_allclose(ils, R.mmr(idx, sc, V, rank, 10, 0.5)[2], atol=R.ILS_ATOL)
    # cosine 0 with everything: a list of the three rows without a direction has ILS 0
    assert _ils(np.array([[5, 6, 7]]), V, rank)[0] == 0.0
    # all scores equal in a row: rel = 1 for all, still a valid greedy run
    eq = np.full((1, 10), 2.5, np.float32)
    oi, _, _ = _check(idx, eq, V, rank, 10, 0.3)
    assert oi[0, 0] == 10
    oi1, os1, _ = _run(idx, eq, V, rank, 10, 1.0)
    np.testing.assert_array_equal(oi1, idx)


@pytest.mark.parametrize("m", [2, 10, 64, 65, 256])
def test_list_similarity_against_the_reference(m):
    for rank in (3, 64, 128):
        V = _table(rank)
        rng = np.random.default_rng(m + rank)
        idx = rng.integers(0, N_V, (40, m)).astype(np.int32)
        idx[rng.random((40, m)) < 0.2] = -1
        idx[0] = -1
        idx[1, 1:] = N_V
        idx[2] = 7                                                 # duplicates: cosine 1
        got = _ils(idx, V, rank)
        want = R.list_similarity(idx, V, rank)
        assert np.isnan(got[0]) and np.isnan(got[1]) and abs(got[2] - 1) <= 1e-6
        np.testing.assert_allclose(got, want, rtol=0, atol=R.ILS_ATOL, equal_nan=True)


def test_noop_and_bad_arguments_through_ctypes():
    L = _lib.lib()
    V = _dev(_table(8)[:10], 8)
    idx = torch.zeros((2, 4), dtype=torch.int32, device=DEV)
    sc = torch.zeros((2, 4), device=DEV)
    oi = torch.full((2, 4), 77, dtype=torch.int32, device=DEV)
    os_ = torch.full((2, 4), 77.0, device=DEV)
    ils = torch.full((2,), 77.0, dtype=torch.float64, device=DEV)
    p = E.ptr

    def call(n_q=2, m=4, top=4, lam=0.5, k=8):
        return L.als_diversify(p(V), 10, V.shape[1], k, p(idx), p(sc), n_q, m, top, lam, p(oi),
                               p(os_), p(ils), E.stream_ptr(V.device))
    assert call(n_q=0) == 0
    assert call(top=5) == -1 and call(lam=1.5) == -1 and call(lam=float("nan")) == -1
    assert call(m=257) == -4 and call(k=129) == -4
    assert L.als_list_similarity(p(V), 10, V.shape[1], 8, p(idx), 0, 4, p(ils), 0) == 0
    assert L.als_list_similarity(p(V), 10, V.shape[1], 8, p(idx), 2, 257, p(ils), 0) == -4
    torch.cuda.synchronize()
    assert (oi == 77).all() and (os_ == 77).all() and (ils == 77).all()   # nothing launched
    e_i, e_s, e_l = E.diversify_rows(idx[:0], sc[:0], V, 10, 8, 2, 0.5)
    assert tuple(e_i.shape) == (0, 2) and e_l.numel() == 0


# ------------------------------------------------------------------ engine and surfaces
GAP = 2


@pytest.fixture(scope="module")
def fitted():
    import pandas as pd

    from als_mi355x.ml.recommendation import ALS
    from helpers import planted
    u, i, r = planted(200, 120, density=0.12, seed=11, dup=40, id_gap=GAP)
    df = pd.DataFrame({"user": u, "item": i, "rating": r})
    model = ALS(rank=8, maxIter=3, regParam=0.1, seed=3).fit(df)
    return model, df


def _np(*xs):
    return [x.cpu().numpy() for x in xs]


def test_recommend_diverse_is_k5_then_k14_whatever_the_chunking(fitted):
    model, _ = fitted
    core = model.engine
    cand = np.arange(0, 240, GAP)[:70]                            # fewer than the pool of 100
    kw = dict(exclude="train", candidates=cand)
    keys, ids, sc, ils = _np(*core.recommend_diverse(10, pool=100, trade_off=0.6, **kw))
    assert keys.tolist() == core.uidx.ids().cpu().tolist() and ids.shape == (200, 10)
    pi, ps = E.topk_rows_filtered(core.U, core.n_users, core.V, core.n_items, 8, 100,
                                  *core._filter_args("train", cand, True))
    assert bool((pi[:, 70:] == -1).all())                         # the -1 / -inf tail
    wi, ws, wl = E.diversify_rows(pi, ps, core.V, core.n_items, 8, 10, 0.6)
    np.testing.assert_array_equal(ids, E.ids_of(core.iidx.ids(), wi).cpu().numpy())
    assert sc.tobytes() == ws.cpu().numpy().tobytes()
    assert ils.tobytes() == wl.cpu().numpy().tobytes()
    V = core.V[:, :8].cpu().numpy()
    R.check_greedy(pi.cpu().numpy(), ps.cpu().numpy(), V, 8, 0.6, wi.cpu().numpy(), ws.cpu().numpy(),
                   10)
    for chunk in (64, 100):
        got = _np(*core.recommend_diverse(10, pool=100, trade_off=0.6, chunk_rows=chunk, **kw))
        for a, b in zip(got, (keys, ids, sc, ils)):
            assert a.tobytes() == b.tobytes(), chunk
    # the subset: unknown dropped, distinct ascending; the rows of the full run
    want = [4, 0, 398, 4, 7, 10 ** 6]
    for chunk in (None, 2):
        k2, i2, s2, l2 = _np(*core.recommend_diverse(10, ids=want, pool=100, trade_off=0.6,
                                                     chunk_rows=chunk, **kw))
        assert k2.tolist() == [0, 4, 398]
        rows = [0, 2, 199]
        np.testing.assert_array_equal(i2, ids[rows])
        assert s2.tobytes() == sc[rows].tobytes() and l2.tobytes() == ils[rows].tobytes()
    # the item side, the default pool (min(256, max(4 top, 50)) capped at the 200 users)
    k3, i3, s3, l3 = core.recommend_diverse(60, False)
    assert tuple(i3.shape) == (120, 60) and l3.dtype == torch.float64
    p3 = E.topk_rows(core.V, core.n_items, core.U, core.n_users, 8, 200)
    w3 = E.diversify_rows(*p3, core.U, core.n_users, 8, 60, 0.7)
    assert torch.equal(s3, w3[1]) and torch.equal(i3, E.ids_of(core.uidx.ids(), w3[0]))


def test_from_factors_core_serves_diverse_lists(fitted):
    model, _ = fitted
    core = model.engine
    bare = E.ALSCore.from_factors(core.uidx.ids(), core.U[:, :8], core.iidx.ids(), core.V[:, :8])
    a = _np(*core.recommend_diverse(5, trade_off=0.4, candidates=[0, 2, 4, 6, 8, 10, 12]))
    b = _np(*bare.recommend_diverse(5, trade_off=0.4, candidates=[0, 2, 4, 6, 8, 10, 12]))
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    with pytest.raises(ValueError, match="ratings"):
        bare.recommend_diverse(5, exclude="train")
    lists = [[0, 2, 4], [6, 6, 10 ** 6], [7, 8, 9]]              # 7, 9, 10^6 unknown
    got = bare.list_similarity(lists).cpu().numpy()
    V = core.V[:, :8].cpu().numpy()
    want = R.list_similarity(np.array([[0, 1, 2], [3, 3, -1], [-1, 4, -1]]), V, 8)
    np.testing.assert_allclose(got, want, atol=R.ILS_ATOL, equal_nan=True)
    assert np.isnan(got[2]) and abs(got[1] - 1) <= 1e-6


def test_ml_and_mllib_surfaces(fitted, tmp_path):
    import pandas as pd

    from als_mi355x.ml.recommendation import ALSModel
    from als_mi355x.mllib.recommendation import MatrixFactorizationModel
    model, df = fitted
    core = model.engine
    keys, ids, sc, ils = _np(*core.recommend_diverse(7, trade_off=0.5, exclude="train"))
    got = model.recommendForAllUsersDiverse(7, 0.5, exclude="train")
    assert list(got.columns) == ["user", "recommendations", "intraListSimilarity"]
    assert list(got["user"]) == keys.tolist()
    for r, lst in enumerate(got["recommendations"]):
        n = int(np.isfinite(sc[r]).sum())
        assert [a for a, _ in lst] == ids[r, :n].tolist()
        assert [np.float32(b) for _, b in lst] == sc[r, :n].tolist()
    np.testing.assert_array_equal(got["intraListSimilarity"].to_numpy(), ils)
    sub = model.recommendForUserSubsetDiverse(pd.DataFrame({"user": [398, 4, 7]}), 7, 0.5,
                                              exclude="train")
    assert list(sub["user"]) == [4, 398]
    assert sub["recommendations"][0] == got["recommendations"][2]
    items = model.recommendForAllItemsDiverse(5, 0.5, pool=30)
    isub = model.recommendForItemSubsetDiverse(pd.DataFrame({"item": [6, 0]}), 5, 0.5, pool=30)
    assert list(items.columns) == ["item", "recommendations", "intraListSimilarity"]
    assert isub["recommendations"][1] == items["recommendations"][3]
    # tradeOff = 1 is the plain list, and intraListSimilarity of the plain lists is the
    # reference's
    plain = model.recommendForAllUsers(7)
    one = model.recommendForAllUsersDiverse(7, 1.0)
    assert list(one["recommendations"]) == list(plain["recommendations"])
    V = core.V[:, :8].cpu().numpy()
    rows = np.array([[a // GAP for a, _ in lst] for lst in plain["recommendations"]])
    scored = model.intraListSimilarity(plain)
    assert list(scored.columns) == ["user", "intraListSimilarity"]
    np.testing.assert_allclose(scored["intraListSimilarity"].to_numpy(),
                               R.list_similarity(rows, V, 8), atol=R.ILS_ATOL)
    np.testing.assert_allclose(one["intraListSimilarity"].to_numpy(),
                               scored["intraListSimilarity"].to_numpy(), atol=1e-12)
    # mllib
    mf = MatrixFactorizationModel(core)
    lst, v = mf.recommendProductsDiverse(4, 7, 0.5, exclude="train")
    assert [(x.product, x.rating) for x in lst] == got["recommendations"][2] and v == ils[2]
    assert mf.recommendProductsDiverse(4, 7, 1.0)[0] == mf.recommendProducts(4, 7)
    everyone = mf.recommendProductsForUsersDiverse(7, 0.5, exclude="train")
    assert [k for k, _, _ in everyone] == keys.tolist() and everyone[2][1] == lst
    with pytest.raises(KeyError):
        mf.recommendProductsDiverse(7, 5)
    # a reloaded model serves the same lists; only exclude="train" needs the ratings
    model.save(str(tmp_path / "m"))
    loaded = ALSModel.load(str(tmp_path / "m"))
    again = loaded.recommendForAllUsersDiverse(7, 1.0)
    assert list(again["recommendations"]) == list(plain["recommendations"])
    with pytest.raises(ValueError, match="ratings"):
        loaded.recommendForAllUsersDiverse(7, 0.5, exclude="train")


def test_planted_clusters_end_to_end():
    from als_mi355x.ml.recommendation import ALSModel, _Params
    V, u = R.planted_clusters()
    U = np.stack([u, u[::-1].copy()])
    core = E.ALSCore.from_factors([0, 1], U, np.arange(40), V)
    model = ALSModel(core, dict(_Params._defaults))
    cluster = lambda lst: [a // 10 for a, _ in lst]
    plain = model.recommendForAllUsersDiverse(8, 1.0, pool=40)
    half = model.recommendForAllUsersDiverse(8, 0.5, pool=40)
    assert cluster(plain["recommendations"][0]) == [0] * 8
    assert sorted(cluster(half["recommendations"][0])[:4]) == [0, 1, 2, 3]
    assert half["intraListSimilarity"][0] < 0.4 < plain["intraListSimilarity"][0]
    want = R.mmr(*R.pool_of(u, V, 8, 40), V, 8, 8, 0.5)
    assert [a for a, _ in half["recommendations"][0]] == want[0][0].tolist()
    np.testing.assert_allclose(half["intraListSimilarity"][0], want[2][0], atol=R.ILS_ATOL)


def test_personal_fold_in_with_a_trade_off(fitted):
    from als_mi355x import personal
    model, df = fitted
    rated = [(10 ** 6, 0, 5.0), (10 ** 6, 2, 4.0), (10 ** 6, 4, 1.0), (10 ** 6, 6, 3.0)]
    movies = [(m, f"movie {m}") for m in range(0, 240, GAP)]
    counts = personal.movie_counts_and_averages(df[["user", "item", "rating"]].to_numpy())
    plain = personal.personal_recommendations_fold_in(model, rated, movies, counts, 0.1,
                                                      min_count=5, num=10)
    same = personal.personal_recommendations_fold_in(model, rated, movies, counts, 0.1,
                                                     min_count=5, num=10, trade_off=1.0)
    assert plain == same and len(plain) == 10
    div = personal.personal_recommendations_fold_in(model, rated, movies, counts, 0.1,
                                                    min_count=5, num=10, trade_off=0.3)
    assert len(div) == 10 and div[0] == plain[0] and len({t for _, t, _ in div}) == 10
    assert not {"movie 0", "movie 2", "movie 4", "movie 6"} & {t for _, t, _ in div}
