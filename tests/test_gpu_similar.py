"""Cosine neighbour search (K12, als_similar) on the GPU: parity against the fp64 reference
of similar_ref.py, bitwise independence from the slice count and from power-of-two scaling,
the never-listed rules, the unit copy + K5 route against the same contract, and the public
surfaces.

Tolerance (similar_ref.check): an index may differ from the reference only where the fp64
scores tie within 1e-5; scores at rtol = atol = 1e-5.  The fp32 dot of k <= 128 terms errs
by at most k 2^-24 ~ 7.6e-6 of |q||t| in the worst order, the norms add ~1e-7.
"""
import functools

import numpy as np
import pytest
import torch

import similar_ref as R
from als_mi355x import engine as E
from als_mi355x import filters as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 1500
ZERO, NAN, INF = 70, 80, 90   # planted rows without a direction


def _dev(M, rank, fill=0.0):
    out = torch.full((M.shape[0], E.ld_for(rank)), fill, device=DEV)
    out[:, :rank] = torch.as_tensor(np.array(M, np.float32)).to(DEV)
    return out.contiguous()


def _bits(allow):
    return None if allow is None else F.pack_allow_bits(
        torch.as_tensor(np.nonzero(allow)[0]).to(DEV), len(allow))


def _i32(a):
    return None if a is None else torch.as_tensor(np.asarray(a, np.int32)).to(DEV)


def _run(Q, T, rank, top, self_rows=None, allow=None, slices=0, Qd=None, Td=None):
    idx, sc = E.similar_rows(_dev(Q, rank) if Qd is None else Qd, len(Q),
                             _dev(T, rank) if Td is None else Td, len(T), rank, top,
                             _i32(self_rows), _bits(allow), slices)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), sc.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _table(rank, n=N):
    rng = np.random.default_rng(200 + rank)
    T = rng.standard_normal((n, rank)).astype(np.float32)
    T[10] = T[20]            # an exact tie: the lower index first
    T[30] = 3 * T[40]        # cosine 1 across different norms
    T[50] = -T[60]           # cosine -1: last, still listed when top >= n - 1
    T[ZERO] = 0
    T[NAN, rank // 2] = np.nan
    T[INF, 0] = np.inf
    allows = {"none": None, "half": rng.random(n) < 0.5, "five": np.zeros(n, bool)}
    allows["five"][[3, 10, 20, 777, n - 1]] = True
    T.setflags(write=False)
    return T, allows


QROWS = [10, 30, 50, 7] + list(range(100, 136))   # 40 queries: the planted rows first


# ------------------------------------------------------------------ 1. parity grid
@pytest.mark.parametrize("allow", ["none", "half", "five"])
@pytest.mark.parametrize("n_q", [1, 16, 17, 40])
@pytest.mark.parametrize("top", [1, 10, 100, 256])
@pytest.mark.parametrize("rank", [10, 33, 64, 128])
def test_parity_grid(rank, top, n_q, allow):
    T, allows = _table(rank)
    rows = np.array(QROWS[:n_q])
    Q = T[rows]
    a = allows[allow]
    idx, sc = _run(Q, T, rank, top, rows, a)
    R.check(idx, sc, R.cosine(Q, T), R.admissible(Q, T, rows, a), top)
    if a is None:
        assert idx[0, 0] == 20 and abs(sc[0, 0] - 1) <= 1e-6      # query 10: its twin, at 1
        if n_q > 1:
            assert idx[1, 0] == 40 and abs(sc[1, 0] - 1) <= 1e-6  # 3 x row 40
    for r in range(n_q):                                          # exact tie 10 / 20
        lst = list(idx[r])
        if 10 in lst and 20 in lst:
            assert lst.index(10) + 1 == lst.index(20)


def test_opposite_row_ranks_last_but_is_listed():
    rank, n = 10, 200
    T, _ = _table(rank)
    T = T[:n]
    rows = np.array([50, 60])
    idx, sc = _run(T[rows], T, rank, n - 1, rows)
    adm = R.admissible(T[rows], T, rows)
    R.check(idx, sc, R.cosine(T[rows], T), adm, n - 1)
    m = int(adm[0].sum())                     # n - 1 minus the three rows without a direction
    assert m == n - 4
    assert idx[0, m - 1] == 60 and abs(sc[0, m - 1] + 1) <= 1e-6 and idx[0, m] == -1
    assert idx[1, m - 1] == 50 and abs(sc[1, m - 1] + 1) <= 1e-6


# ------------------------------------------------------------------ 2. padding columns
@pytest.mark.parametrize("rank", [10, 33])
def test_padding_columns_are_never_read(rank):
    T, _ = _table(rank)
    rows = np.array(QROWS[:17])
    Q = T[rows]
    clean = _run(Q, T, rank, 10, rows)
    rng = np.random.default_rng(5)
    Td, Qd = _dev(T, rank), _dev(Q, rank)
    pad = E.ld_for(rank) - rank
    assert pad > 0
    Td[:, rank:] = torch.as_tensor(rng.standard_normal((N, pad)) * 1e3).to(DEV)
    Qd[:, rank:] = torch.as_tensor(rng.standard_normal((17, pad)) * 1e3).to(DEV)
    Td[::3, rank:] = float("nan")
    Qd[::2, rank:] = float("nan")
    Td[1::3, -1] = float("inf")
    dirty = _run(Q, T, rank, 10, rows, Qd=Qd, Td=Td)
    np.testing.assert_array_equal(clean[0], dirty[0])
    np.testing.assert_array_equal(clean[1].view(np.int32), dirty[1].view(np.int32))


# ------------------------------------------------------------------ 3. slices
@pytest.mark.parametrize("top", [10, 256])
@pytest.mark.parametrize("rank", [33, 128])
def test_slices_give_bitwise_identical_lists(rank, top):
    n = 5000
    T, _ = _table(rank, n)
    rows = np.array(QROWS[:17])
    Q = T[rows]
    Td, Qd = _dev(T, rank), _dev(Q, rank)
    base = _run(Q, T, rank, top, rows, slices=1, Qd=Qd, Td=Td)
    R.check(base[0], base[1], R.cosine(Q, T), R.admissible(Q, T, rows), top)
    for s in (3, 7, 0, 100):        # 100: the two-stage merge
        got = _run(Q, T, rank, top, rows, slices=s, Qd=Qd, Td=Td)
        np.testing.assert_array_equal(base[0], got[0], err_msg=f"slices={s}")
        np.testing.assert_array_equal(base[1].view(np.int32), got[1].view(np.int32))


# ------------------------------------------------------------------ 4. edges
def test_small_table_leaves_open_slots():
    rng = np.random.default_rng(9)
    T = rng.standard_normal((5, 10)).astype(np.float32)
    rows = np.array([0, 4])
    idx, sc = _run(T[rows], T, 10, 10, rows)
    R.check(idx, sc, R.cosine(T[rows], T), R.admissible(T[rows], T, rows), 10)
    assert (idx[:, 4:] == -1).all() and np.isneginf(sc[:, 4:]).all() and (idx[:, :4] >= 0).all()


def test_zero_and_nan_queries_get_empty_lists():
    rank = 33
    T, _ = _table(rank)
    Q = T[[ZERO, NAN, INF, 5]].copy()
    idx, sc = _run(Q, T, rank, 10, [-1, -1, -1, -1])
    assert (idx[:3] == -1).all() and np.isneginf(sc[:3]).all()
    assert idx[3, 0] == 5                      # the live query next to them is untouched
    R.check(idx, sc, R.cosine(Q, T), R.admissible(Q, T), 10)


def test_allow_mask_word_boundaries():
    rank = 64
    T, _ = _table(rank)
    allow = np.zeros(N, bool)
    allow[[31, 32, N - 1]] = True
    rows = np.array([31, 5, N - 1])
    idx, sc = _run(T[rows], T, rank, 10, rows, allow)
    R.check(idx, sc, R.cosine(T[rows], T), R.admissible(T[rows], T, rows, allow), 10)
    assert set(idx[0, :2]) == {32, N - 1} and idx[0, 2] == -1
    assert set(idx[1, :3]) == {31, 32, N - 1} and idx[1, 3] == -1


@pytest.mark.parametrize("rank", [10, 128])
def test_power_of_two_scaling_changes_nothing(rank):
    """Powers of two pass exactly through dot, norm and quotient: a norm taken from the
    wrong row or the wrong columns would show."""
    T, _ = _table(rank)
    rows = np.array(QROWS[:17])
    rng = np.random.default_rng(3)
    et = np.ldexp(1.0, rng.integers(-12, 13, N)).astype(np.float32)
    eq = np.ldexp(1.0, rng.integers(-12, 13, len(rows))).astype(np.float32)
    a = _run(T[rows], T, rank, 100, rows)
    b = _run(T[rows] * eq[:, None], T * et[:, None], rank, 100, rows)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1].view(np.int32), b[1].view(np.int32))


def test_without_self_exclusion_the_row_itself_comes_first():
    rank = 64
    T, _ = _table(rank)
    rows = np.array([7, 20, 40, 123])
    idx, sc = _run(T[rows], T, rank, 5, -np.ones(4))
    np.testing.assert_array_equal(idx[[0, 1, 3], 0], [7, 10, 123])  # 10 = 20's twin: an exact
    assert np.abs(sc[:, 0] - 1).max() <= 1e-6                       # tie, the lower index first
    assert idx[1, 1] == 20 and set(idx[2, :2]) == {30, 40}          # 30 = 3 x 40, rounded
    assert abs(sc[2, 1] - 1) <= 1e-6
    R.check(idx, sc, R.cosine(T[rows], T), R.admissible(T[rows], T), 5)
    idx2, _ = _run(T[rows], T, rank, 5, None)                    # a null self_rows: the same
    np.testing.assert_array_equal(idx, idx2)


# ------------------------------------------------------------------ 5. the two routes
@pytest.mark.parametrize("allow", ["none", "half"])
@pytest.mark.parametrize("rank,top", [(33, 10), (128, 100)])
def test_the_two_routes_keep_one_contract(rank, top, allow):
    T, allows = _table(rank)
    a = allows[allow]
    Td = _dev(T, rank)
    rows = np.arange(N)
    S, adm = R.cosine(T, T), R.admissible(T, T, rows, a)
    i1, s1 = E.similar_rows(Td, N, Td, N, rank, top, _i32(rows), _bits(a))
    i2, s2 = E.similar_rows_unit(None, Td, N, rank, top, _bits(a))
    sub = torch.as_tensor(np.array(QROWS)).to(DEV)
    i3, s3 = E.similar_rows_unit(sub, Td, N, rank, top, _bits(a))
    torch.cuda.synchronize()
    R.check(i1.cpu().numpy(), s1.cpu().numpy(), S, adm, top)
    R.check(i2.cpu().numpy(), s2.cpu().numpy(), S, adm, top)
    R.check(i3.cpu().numpy(), s3.cpu().numpy(), S[QROWS], adm[QROWS], top)
    for r in (ZERO, NAN, INF):     # K5 alone would list rows at score 0 here
        assert (i2[r] == -1).all() and torch.isneginf(s2[r]).all()


def test_unit_rows_copy_mask_and_valid():
    rank = 33
    T, allows = _table(rank)
    a = allows["half"]
    Td = _dev(T, rank, fill=float("nan"))            # garbage padding in, zeros out
    Tn, bits, valid = E.unit_rows(Td, N, rank, _bits(a))
    Tn1, bits1, _ = E.unit_rows(Td, N, rank, None)
    torch.cuda.synchronize()
    ok = R.has_direction(T)
    np.testing.assert_array_equal(valid.cpu().numpy().astype(bool), ok)
    want = np.where(ok[:, None], T.astype(np.float64), 0)
    want = want / np.where(ok, np.sqrt((want * want).sum(1)), 1)[:, None]
    got = Tn.cpu().numpy()
    np.testing.assert_allclose(got[:, :rank], want, rtol=0, atol=6e-8)   # one fp32 rounding
    assert (got[:, rank:] == 0).all() and np.array_equal(got, Tn1.cpu().numpy())
    unpack = lambda b: np.unpackbits(b.cpu().numpy().view(np.uint8), bitorder="little")[:N]
    np.testing.assert_array_equal(unpack(bits).astype(bool), a & ok)
    np.testing.assert_array_equal(unpack(bits1).astype(bool), ok)


# ------------------------------------------------------------------ 6. surfaces
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
    U = core.U[:, :8].cpu().numpy()
    V = core.V[:, :8].cpu().numpy()
    return model, df, U, V


def _same_lists(a, b):
    assert list(a.columns) == list(b.columns) and list(a.iloc[:, 0]) == list(b.iloc[:, 0])
    for x, y in zip(a["similar"], b["similar"]):
        assert [i for i, _ in x] == [i for i, _ in y]
        np.testing.assert_allclose([s for _, s in x], [s for _, s in y], rtol=0, atol=1e-6)


def _check_df(df, key, F_, top, allow=None, gap=GAP):
    """df: DataFrame[key, similar]; F_: that side's factors in dense order."""
    n = len(F_)
    t = min(top, n - 1)
    S = R.cosine(F_, F_)
    assert list(df.columns) == [key, "similar"]
    for k, lst in zip(df[key], df["similar"]):
        r = int(k) // gap
        adm = R.admissible(F_[r:r + 1], F_, [r], allow)
        m = min(t, int(adm.sum()))
        assert len(lst) == m, (k, len(lst), m)
        idx = np.full((1, t), -1)
        sc = np.full((1, t), -np.inf, np.float32)
        idx[0, :m] = np.asarray([a for a, _ in lst], np.int64) // gap
        sc[0, :m] = [b for _, b in lst]
        R.check(idx, sc, S[r:r + 1], adm, t)


def test_similar_items_and_users_surfaces(fitted, tmp_path):
    import pandas as pd

    from als_mi355x.ml.recommendation import ALSModel
    model, df, U, V = fitted
    want = [4, 0, 238, 4, 7, 10 ** 6]                    # 7 and 10^6 are unknown: dropped
    got = model.similarItems(pd.DataFrame({"item": want}), 10)
    assert list(got["item"]) == [0, 4, 238]
    _check_df(got, "item", V, 10)
    got_ids = model.similarItems(np.array(want), 10)     # plain ids instead of a dataset
    _same_lists(got_ids, got)
    assert model.similarItems(4, 3)["similar"][0] == got["similar"][1][:3]
    users = model.similarUsers(pd.DataFrame({"user": [2, 398, 3]}), 7)
    assert list(users["user"]) == [2, 398]
    _check_df(users, "user", U, 7)
    everything = model.similarItemsForAllItems(5)
    assert list(everything["item"]) == list(range(0, 240, GAP))
    _check_df(everything, "item", V, 5)
    # candidates restrict the neighbours, not the queries
    cand = list(range(0, 60, GAP))
    allow = np.zeros(120, bool)
    allow[:30] = True
    far = model.similarItems([200, 4], 10, candidates=cand + [10 ** 6])
    assert list(far["item"]) == [4, 200]
    _check_df(far, "item", V, 10, allow)
    assert all(a < 60 for lst in far["similar"] for a, _ in lst)
    _check_df(model.similarItemsForAllItems(10, candidates=cand), "item", V, 10, allow)
    # a reloaded model holds the factors and nothing else: the same lists
    model.save(str(tmp_path / "m"))
    loaded = ALSModel.load(str(tmp_path / "m"))
    _same_lists(loaded.similarItems(np.array(want), 10), got)
    _same_lists(loaded.similarUsers([2, 398], 7), users)
    _same_lists(loaded.similarItemsForAllItems(5), everything)


def test_similar_products_and_movies(fitted):
    from als_mi355x import personal
    from als_mi355x.mllib.recommendation import MatrixFactorizationModel
    model, df, U, V = fitted
    mf = MatrixFactorizationModel(model.engine)
    ref = model.similarItems([4], 10)["similar"][0]
    assert mf.similarProducts(4, 10) == ref
    assert mf.similarUsers(2, 7) == model.similarUsers([2], 7)["similar"][0]
    assert all(a in (0, 2, 6) for a, _ in mf.similarProducts(4, 10, candidates=[0, 2, 4, 6]))
    assert len(mf.similarProducts(4, 10, candidates=[0, 2, 4, 6])) == 3   # 4 itself never
    with pytest.raises(KeyError):
        mf.similarProducts(7, 10)
    movies = [(m, f"movie {m}") for m in range(0, 240, GAP) if m != 6]    # 6 has no title
    out = personal.similar_movies(model, [4, 7, 0], movies, num=5)
    assert [name for name, _ in out] == ["movie 0", "movie 4"]
    assert [n for n, _ in out[1][1]] == [f"movie {a}" if a != 6 else "6" for a, _ in ref[:5]]
    np.testing.assert_allclose([s for _, s in out[1][1]], [s for _, s in ref[:5]])
    # min_ratings: neighbours among the movies with MORE than that many ratings
    triples = df[["user", "item", "rating"]].to_numpy()
    counts = personal.movie_counts_and_averages(triples)
    cut = int(np.median([c for c, _ in counts.values()]))
    popular = {m for m, (c, _) in counts.items() if c > cut}
    assert 0 < len(popular) < 120
    out = personal.similar_movies(model, [4], movies, num=8, min_ratings=cut, ratings=triples)
    allow = np.array([GAP * r in popular for r in range(120)])
    name_of = {f"movie {m}": m for m in range(0, 240, GAP)}
    name_of["6"] = 6
    lst = [(name_of[nm], s) for nm, s in out[0][1]]
    assert all(m in popular for m, _ in lst)
    import pandas as pd
    _check_df(pd.DataFrame({"item": [4], "similar": [lst]}), "item", V, 8, allow)
    with pytest.raises(ValueError):
        personal.similar_movies(model, [4], movies, min_ratings=3)
