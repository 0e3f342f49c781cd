"""K16 on the GPU: als_row_moments / als_bias_update / als_baseline_predict against the numpy
fp64 reference (baseline_ref.py), then the engine, ml, mllib and personal surfaces.

Shapes are the ones where the sweep can go wrong, not a workload's: with T = the task length and
R = the rows per workgroup the library reports — one row of one rating; rows of 0, 1, T - 1, T,
T + 1 and 3 T + 5 ratings in one block; one heavy row before and after 300 empty rows; R k - 1
and R k + 1 rows; no ratings at all; columns -1 and n_cols beside valid ones under a gather
table whose entries all differ.

Tolerances, u = 2^-53, per row and for the total, n the ratings and e_j the terms summed:
  half-star data   every fp64 sum is exact: n, sum, min, max equal the reference bit for bit
  sum              |sum - ref| <= 2 n u sum |e_j|   (any order of n - 1 additions errs by at most
                   (n - 1) u sum |e_j|; the reference's pairwise sum by less; together < 2 n u ..)
  M2               |M2 - ref| <= 4 n u sum e_j^2
  bias             |b - ref| <= 2 n u sum |e_j| / (damping + n): the sum's bound over the
                   denominator (the division's own rounding is below it), step by step with the
                   device's previous tables fed to the reference
"""
import numpy as np
import pandas as pd
import pytest
import torch

import baseline_ref as BR
from als_mi355x import _lib, datasets, personal
from als_mi355x import engine as E
from als_mi355x.ml.evaluation import RegressionEvaluator
from als_mi355x.ml.recommendation import ALS, BaselinePredictor
from als_mi355x.ml.tuning import ParamGridBuilder, TrainValidationSplit
from als_mi355x.mllib.recommendation import ALS as MLlibALS
from als_mi355x.mllib.recommendation import BaselineModel as MLlibBaseline

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = BR.U53


@pytest.fixture(scope="module")
def TR():
    L = _lib.lib()
    return int(L.als_rating_stats_task()), int(L.als_rating_stats_group_rows())


@pytest.fixture(scope="module")
def ws():
    return E.Workspace(torch.device(DEV))


def _dev(side):
    rp, c, v = side
    return (torch.as_tensor(rp, device=DEV), torch.as_tensor(c, device=DEV),
            torch.as_tensor(v, device=DEV))


def _device_moments(side, n_cols, ws, other=None, offset=0.0):
    o = None if other is None else torch.as_tensor(np.asarray(other, np.float64), device=DEV)
    mom, total = E.row_moments(_dev(side), n_cols, ws, other=o, offset=offset)
    torch.cuda.synchronize()
    return mom.cpu().numpy(), total.cpu().numpy()


def _assert_moments(got, want, exact: bool, what=""):
    (mom, total), (rmom, rtotal, a, q) = got, want
    for g, r, sa, sq in ((mom, rmom, a[:-1], q[:-1]), (total[None], rtotal[None], a[-1:], q[-1:])):
        n = r[:, 0]
        np.testing.assert_array_equal(g[:, 0], n, err_msg=f"{what} n")
        for f in (3, 4):   # min, max: exact, NaN for an empty row
            np.testing.assert_array_equal(g[:, f], r[:, f], err_msg=f"{what} field {f}")
        if exact:
            np.testing.assert_array_equal(g[:, 1], r[:, 1], err_msg=f"{what} sum")
            with np.errstate(invalid="ignore", divide="ignore"):
                np.testing.assert_array_equal(g[:, 1] / g[:, 0], r[:, 1] / n)
        err = np.abs(g[:, 1] - r[:, 1])
        assert (err <= 2 * n * U * sa).all(), (what, "sum", err.max())
        err = np.abs(g[:, 2] - r[:, 2])
        assert (err <= 4 * n * U * sq).all(), (what, "M2", err.max(), (4 * n * U * sq).max())
        assert (g[n == 0][:, :3] == 0).all()


def _shapes(T, R):
    return {
        "one": [1],
        "edges": [0, 1, T - 1, T, T + 1, 3 * T + 5],
        "heavy_first": [4 * T + 3] + [0] * 300,
        "heavy_last": [0] * 300 + [4 * T + 3],
        "below_group": [3, 0, 5, 1] * (R // 2) + [2] * (R - 1),      # 3 R - 1 rows
        "above_group": [3, 0, 5, 1] * (R // 2) + [2] * (R + 1),      # 3 R + 1 rows
        "unaligned_starts": [1, T + 2, 3, 2 * T + 1, 2, T + 3],      # tasks begin inside a quad
        "no_ratings": [0] * 5,
    }


SHAPES = ["one", "edges", "heavy_first", "heavy_last", "below_group", "above_group",
          "unaligned_starts", "no_ratings"]


@pytest.mark.parametrize("shape", SHAPES)
def test_half_star_moments_are_exact(shape, TR, ws):
    lengths = _shapes(*TR)[shape]
    rng = np.random.default_rng(len(shape))
    side = BR.csr_from_lengths(lengths, 50, rng, "half")
    got = _device_moments(side, 50, ws)
    _assert_moments(got, BR.row_moments(*side, 50), exact=True, what=shape)
    # two calls give identical bytes
    again = _device_moments(side, 50, ws)
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()


@pytest.mark.parametrize("shape", ["edges", "heavy_first", "above_group", "unaligned_starts"])
def test_gather_with_columns_outside_the_table(shape, TR, ws):
    """other: distinct multiples of 1/4 (a wrong gather shows, and the sums stay exact);
    columns -1 and n_cols among the valid ones take 0 from it."""
    lengths = _shapes(*TR)[shape]
    rng = np.random.default_rng(7 + len(shape))
    n_cols = 211
    side = BR.csr_from_lengths(lengths, n_cols, rng, "half")
    nnz = len(side[1])
    side[1][rng.choice(nnz, nnz // 7, replace=False)] = -1
    side[1][rng.choice(nnz, nnz // 7, replace=False)] = n_cols
    side[1][[0, nnz - 1]] = [n_cols, -1]
    other = (rng.permutation(n_cols) - 100) * 0.25
    got = _device_moments(side, n_cols, ws, other, 1.5)
    _assert_moments(got, BR.row_moments(*side, n_cols, other, 1.5), exact=True, what=shape)
    again = _device_moments(side, n_cols, ws, other, 1.5)
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()


@pytest.mark.parametrize("shape", ["edges", "heavy_last", "below_group"])
def test_wide_ratings_meet_the_summation_bounds(shape, TR, ws):
    lengths = _shapes(*TR)[shape]
    rng = np.random.default_rng(11 + len(shape))
    side = BR.csr_from_lengths(lengths, 64, rng, "wide")
    other = rng.normal(0.0, 300.0, 64)
    _assert_moments(_device_moments(side, 64, ws), BR.row_moments(*side, 64), False, shape)
    _assert_moments(_device_moments(side, 64, ws, other, -2.25),
                    BR.row_moments(*side, 64, other, -2.25), False, shape + " gather")


def test_m2_of_shifted_ratings_is_not_the_textbook_formula(TR, ws):
    """1e4 + N(0, 1): M2 within 1e-9 of the two-pass value, per row and in total
    (test_rating_stats_cpu.py shows the two-pass value is good to 1e-12 and that
    sum e^2 - sum^2 / n misses 1e-9)."""
    T, _ = TR
    rng = np.random.default_rng(21)
    side = BR.csr_from_lengths([3 * T + 5, 700, T, 40], 8, rng, "shifted")
    mom, total = _device_moments(side, 8, ws)
    rmom, rtotal, _, _ = BR.row_moments(*side, 8)
    print("M2 relative errors", np.abs(mom[:, 2] - rmom[:, 2]) / rmom[:, 2],
          abs(total[2] - rtotal[2]) / rtotal[2])
    assert (np.abs(mom[:, 2] - rmom[:, 2]) <= 1e-9 * rmom[:, 2]).all()
    assert abs(total[2] - rtotal[2]) <= 1e-9 * rtotal[2]
    e = side[2].astype(np.float64)
    assert abs(BR.textbook_m2(e) - rtotal[2]) > 1e-9 * rtotal[2]


def test_misaligned_tables_give_the_same_bits(TR, ws):
    """col / val 4 bytes past a 16-byte boundary take the 4-byte loads: same numbers."""
    T, _ = TR
    rng = np.random.default_rng(4)
    side = BR.csr_from_lengths([5, 2 * T + 9, 0, 33], 20, rng, "wide")
    other = torch.as_tensor(rng.normal(0, 1, 20), device=DEV)
    rp, c, v = _dev(side)
    nnz = len(side[1])
    c1 = torch.zeros(nnz + 1, dtype=torch.int32, device=DEV)[1:]
    v1 = torch.zeros(nnz + 1, dtype=torch.float32, device=DEV)[1:]
    c1.copy_(c), v1.copy_(v)
    assert c1.data_ptr() % 16 == 4 and c.data_ptr() % 16 == 0
    a = E.row_moments((rp, c, v), 20, ws, other=other, offset=0.5)
    a = (a[0].clone(), a[1].clone())
    b = E.row_moments((rp, c1, v1), 20, ws, other=other, offset=0.5)
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes()
    assert a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()


def test_bias_update_and_predict_kernels(ws):
    rng = np.random.default_rng(2)
    side = BR.csr_from_lengths([0, 3, 1, 40, 0, 7], 9, rng, "half")
    mom, _ = E.row_moments(_dev(side), 9, ws, offset=3.0)
    rmom = BR.row_moments(*side, 9, None, 3.0)[0]
    for damping in (0.0, 2.5, 25.0):
        b = E.bias_update(mom, damping).cpu().numpy()
        np.testing.assert_array_equal(b, BR.bias_update(rmom, damping))   # exact sums: exact
    n_u, n_i = 6, 9
    bu = rng.normal(0, 1, n_u)
    bi = rng.normal(0, 1, n_i)
    urow = rng.integers(-1, n_u + 1, 1000).astype(np.int32)
    irow = rng.integers(-1, n_i + 1, 1000).astype(np.int32)
    tb = lambda x: None if x is None else torch.as_tensor(x, device=DEV)
    for u_tab, i_tab in ((bu, bi), (None, bi), (bu, None), (None, None)):
        pred, known = E.baseline_predict_rows(tb(urow), tb(irow), 3.53, tb(u_tab), tb(i_tab),
                                              n_u, n_i)
        rp, rk = BR.predict_sized(urow, irow, 3.53, u_tab, n_u, i_tab, n_i)
        np.testing.assert_array_equal(pred.cpu().numpy(), rp)
        np.testing.assert_array_equal(known.cpu().numpy(), rk)


# ---------------------------------------------------------------- the engine
@pytest.fixture(scope="module")
def small():
    """200 users x 80 items, 5000 half-star ratings, ids offset so dense rows != ids."""
    u, i, r = datasets.synthetic(200, 80, 5000, seed=3, half_stars=True, device="cpu")
    u, i, r = u.numpy().astype(np.int32) * 3 + 7, i.numpy().astype(np.int32) * 2 + 11, r.numpy()
    core = E.ALSCore(u, i, r)
    uid, iid = np.unique(u), np.unique(i)
    us = BR.csr_from_triples(np.searchsorted(uid, u), np.searchsorted(iid, i), r, len(uid))
    it = BR.csr_from_triples(np.searchsorted(iid, i), np.searchsorted(uid, u), r, len(iid))
    return dict(u=u, i=i, r=r, core=core, uid=uid, iid=iid, us=us, it=it)


def _sorted_side(block):
    """The engine's CSR side on the host (the order inside a row is the engine's own)."""
    return (block.row_ptr.cpu().numpy(), block.col.cpu().numpy(), block.val.cpu().numpy())


def test_rating_stats_global_stats_and_top_rated(small):
    core = small["core"]
    for user_side, ids, side, n_cols in ((False, small["iid"], small["it"], len(small["uid"])),
                                         (True, small["uid"], small["us"], len(small["iid"]))):
        st = {k: v.cpu().numpy() for k, v in core.rating_stats(user_side=user_side).items()}
        mom = BR.row_moments(*side, n_cols)[0]
        np.testing.assert_array_equal(st["ids"], ids)
        np.testing.assert_array_equal(st["count"], mom[:, 0].astype(np.int64))
        assert st["count"].dtype == np.int64
        np.testing.assert_array_equal(st["mean"], mom[:, 1] / mom[:, 0])
        np.testing.assert_array_equal(st["min"], mom[:, 3])
        np.testing.assert_array_equal(st["max"], mom[:, 4])
        np.testing.assert_allclose(st["std"], np.sqrt(mom[:, 2] / mom[:, 0]), rtol=1e-12)
        with np.errstate(invalid="ignore", divide="ignore"):
            want = np.where(mom[:, 0] > 1, np.sqrt(mom[:, 2] / (mom[:, 0] - 1)), np.nan)
        np.testing.assert_allclose(st["std_sample"], want, rtol=1e-12, equal_nan=True)
    g = core.global_stats()
    r = small["r"].astype(np.float64)
    assert g["count"] == len(r) and g["mean"] == r.sum() / len(r)
    assert g["min"] == r.min() and g["max"] == r.max()
    assert g["std"] == pytest.approx(r.std(), rel=1e-12)
    mom = BR.row_moments(*small["it"], 1)[0]
    for num, min_count, damping in ((10, 0, 0.0), (200, 60, 0.0), (15, 40, 5.0), (0, 0, 0.0)):
        ids, means, counts = (x.cpu().numpy() for x in core.top_rated(num, min_count, False,
                                                                      damping))
        want = BR.top_rated(small["iid"], mom[:, 0], mom[:, 1], num, min_count, damping)
        assert ids.tolist() == [t[0] for t in want]
        assert means.tolist() == [t[1] for t in want]
        assert counts.tolist() == [t[2] for t in want] and (counts > min_count).all()


def test_bias_fit_step_by_step(small, ws):
    """Every update against the reference fed with the device's own previous table, then
    fit_baseline as a whole: the same bits as the hand loop, and its history against the
    objective of the device's tables."""
    core = small["core"]
    n_u, n_i, N = core.n_users, core.n_items, core.nnz
    reg_u, reg_i, sweeps = 10.0, 25.0, 4
    ib, ub = core.item_block, core.user_block
    it, us = _sorted_side(ib), _sorted_side(ub)
    _, total = E.row_moments(ib, n_u, ws)
    t = total.tolist()
    mu = t[1] / t[0]
    assert mu == small["r"].astype(np.float64).sum() / N
    bu = torch.zeros(n_u, dtype=torch.float64, device=DEV)
    bi = torch.zeros(n_i, dtype=torch.float64, device=DEV)
    tables, q_user = [], []
    for _ in range(sweeps):
        for block, side, n_cols, damping, other, out in ((ib, it, n_u, reg_i, bu, bi),
                                                         (ub, us, n_i, reg_u, bi, bu)):
            prev = other.cpu().numpy().copy()
            mom, _ = E.row_moments(block, n_cols, ws, other=other, offset=mu)
            E.bias_update(mom, damping, out=out)
            rmom, _, a, q = BR.row_moments(*side, n_cols, prev, mu)
            want = BR.bias_update(rmom, damping)
            err = np.abs(out.cpu().numpy() - want)
            bound = 2 * rmom[:, 0] * U * a[:-1] / (damping + rmom[:, 0])
            assert (err <= bound).all(), (err.max(), bound.min())
        tables.append((bu.cpu().numpy().copy(), bi.cpu().numpy().copy()))
        q_user.append(q[-1])
    base = core.fit_baseline("bias", reg_u, reg_i, sweeps)
    assert base.mu == mu
    assert base.bu.cpu().numpy().tobytes() == tables[-1][0].tobytes()
    assert base.bi.cpu().numpy().tobytes() == tables[-1][1].tobytes()
    assert len(base.history) == sweeps
    # history: sums of N non-negative fp64 terms on both sides, each term good to a few u of
    # sum e^2 (the M2 bound above): 16 N u (sum e^2 + the penalty) covers device and reference
    prev = None
    for j, (tbu, tbi) in enumerate(tables):
        want = BR.objective(us, mu, tbu, tbi, reg_u, reg_i)
        tol = 16 * N * U * (q_user[j] + want)
        print(f"sweep {j + 1}: objective {base.history[j]!r} reference {want!r} tol {tol:.3e}")
        assert abs(base.history[j] - want) <= tol
        if prev is not None:
            assert base.history[j] <= prev + tol
        prev = base.history[j]


def test_undamped_item_baseline_is_the_item_mean(small):
    """damping 0, method "item": mu + b_i = the item's mean rating (RecommenderSystem.py:50-58).
    mu + sum (r - mu) / n is the mean exactly; computed, the terms r - mu carry u |e| each, the
    sum (n - 1) u sum |e|, the division u |b| and the last addition u |mean|: inside
    2 u sum |e| + 3 u |mean| with the reference mean's own rounding."""
    core = small["core"]
    base = core.fit_baseline("item", reg_item=0.0)
    assert not base.bu.any() and len(base.history) == 1
    mom, _, a, _ = BR.row_moments(*small["it"], 1, None, base.mu)
    plain = BR.row_moments(*small["it"], 1)[0]
    mean = plain[:, 1] / plain[:, 0]
    got = base.mu + base.bi.cpu().numpy()
    assert (np.abs(got - mean) <= 2 * U * a[:-1] + 3 * U * np.abs(mean)).all()
    for method in ("global", "user"):
        b = core.fit_baseline(method)
        assert not b.bi.any() and (method == "user" or not b.bu.any())
    g = core.fit_baseline("global")
    r = small["r"].astype(np.float64)
    assert g.history[0] == pytest.approx(((r - r.mean()) ** 2).sum(), rel=1e-12)
    with pytest.raises(ValueError, match="from_factors"):
        E.ALSCore.from_factors([1, 2], np.ones((2, 2), np.float32), [1, 2],
                               np.ones((2, 2), np.float32)).fit_baseline()


# ---------------------------------------------------------------- the public surfaces
def _frame(small):
    return pd.DataFrame({"user": small["u"], "item": small["i"], "rating": small["r"]})


def _ref_predict(small, mu, bu, bi, users, items):
    urow = np.searchsorted(small["uid"], users)
    urow = np.where((urow < len(small["uid"])) & (small["uid"][np.minimum(
        urow, len(small["uid"]) - 1)] == users), urow, -1)
    irow = np.searchsorted(small["iid"], items)
    irow = np.where((irow < len(small["iid"])) & (small["iid"][np.minimum(
        irow, len(small["iid"]) - 1)] == items), irow, -1)
    return BR.predict(urow, irow, mu, bu, bi)


def test_baseline_predictor_fit_transform_evaluate(small):
    df = _frame(small)
    model = BaselinePredictor(regUser=10.0, regItem=25.0, maxIter=6).fit(df)
    mu, bu, bi, hist = BR.fit(small["us"], small["it"], "bias", 10.0, 25.0, 6)
    assert model.globalMean == mu
    ub, ibs = model.userBias, model.itemBias
    assert ub["id"].tolist() == small["uid"].tolist() and ibs["id"].tolist() == small["iid"].tolist()
    # one update errs by the step bound of test_bias_fit_step_by_step (below 1e-14 on rows of
    # at most 200 ratings of size <= 5) and an error fed into the next update is damped by
    # n / (damping + n) < 1, so six sweeps of two updates stay below 12 e-14 < 1e-12
    np.testing.assert_allclose(ub["bias"].to_numpy(), bu, rtol=0, atol=1e-12)
    np.testing.assert_allclose(ibs["bias"].to_numpy(), bi, rtol=0, atol=1e-12)
    # the objective of tables 1e-12 apart, each side summed to 16 N u = 9e-12 (see there)
    np.testing.assert_allclose(model.objectiveHistory, hist, rtol=1e-10)
    # known pairs, an unknown user, an unknown item, both unknown
    users = np.array([small["u"][0], small["u"][5], 1, small["u"][9], 2], np.int32)
    items = np.array([small["i"][3], small["i"][8], small["i"][2], 4, 6], np.int32)
    test = pd.DataFrame({"user": users, "item": items,
                         "rating": np.array([4.0, 2.5, 3.0, 5.0, 1.0], np.float32)})
    want, known = _ref_predict(small, mu, bu, bi, users, items)
    assert known.tolist() == [3, 3, 2, 1, 0] and want[4] == np.float32(mu)
    out = model.transform(test)
    got = out["prediction"].to_numpy()
    assert got.dtype == np.float32 and not np.isnan(got).any()
    # fp64 tables agree to 1e-12, so the fp32 roundings are at most one ulp apart
    assert (np.abs(got - want) <= 2.0 ** -23 * np.abs(want)).all()
    assert got[4] == np.float32(model.globalMean)
    nan = model.setColdStartStrategy("nan").transform(test)["prediction"].to_numpy()
    assert np.isnan(nan).tolist() == [False, False, True, True, True]
    assert (nan[:2] == got[:2]).all()
    drop = model.setColdStartStrategy("drop").transform(test)
    assert len(drop) == 2 and (drop["prediction"].to_numpy() == got[:2]).all()
    model.setColdStartStrategy("fallback")
    ev = model.evaluateRegression(test)
    err = test["rating"].to_numpy().astype(np.float64) - got.astype(np.float64)
    assert ev["n"] == 5 and ev["dropped"] == 0
    assert ev["rmse"] == pytest.approx(np.sqrt((err ** 2).mean()), rel=1e-12)
    assert ev["mae"] == pytest.approx(np.abs(err).mean(), rel=1e-12)
    # mllib: the same fit, every pair predicted
    mm = MLlibBaseline.train(list(zip(small["u"].tolist(), small["i"].tolist(),
                                      small["r"].tolist())), iterations=6)
    assert mm.globalMean == mu
    pa = mm.predictAll(list(zip(users.tolist(), items.tolist())))
    assert [(p.user, p.product) for p in pa] == list(zip(users.tolist(), items.tolist()))
    assert [np.float32(p.rating) for p in pa] == got.tolist()
    assert np.float32(mm.predict(int(users[4]), int(items[4]))) == np.float32(mu)


def test_compare_to_baseline_and_model_statistics(small):
    df = _frame(small)
    tr, te = datasets.random_split(len(df), (8, 2), seed=1)
    train, test = df.iloc[tr], df.iloc[te]
    model = ALS(rank=4, maxIter=3, regParam=0.1, seed=1).fit(train)
    cmp_ = model.compareToBaseline(test, regUser=10.0, regItem=25.0, maxIter=5)
    assert cmp_["model"] == model.evaluateRegression(test)
    base = BaselinePredictor(regUser=10.0, regItem=25.0, maxIter=5).fit(train)
    assert cmp_["baseline"] == base.evaluateRegression(test)
    assert cmp_["rmseRatio"] == cmp_["model"]["rmse"] / cmp_["baseline"]["rmse"]
    assert cmp_["baseline"]["dropped"] == 0 and cmp_["baseline"]["n"] == len(test)
    g = model.compareToBaseline(test, method="global")["baseline"]
    r_tr = train["rating"].to_numpy().astype(np.float64)
    r_te = test["rating"].to_numpy().astype(np.float64)
    want = np.sqrt(((r_te - np.float32(r_tr.mean())) ** 2).mean())    # R:172-177
    assert g["rmse"] == pytest.approx(want, rel=1e-12)
    st = model.itemStatistics()
    assert list(st.columns) == ["id", "count", "mean", "stddev", "min", "max"]
    counts = train.assign(rating=train["rating"].astype(np.float64)).groupby("item")["rating"] \
        .agg(["count", "mean", "std", "min", "max"])      # pandas averages a float32 column in fp32
    assert st["id"].tolist() == counts.index.tolist()
    assert st["count"].tolist() == counts["count"].tolist()
    np.testing.assert_allclose(st["mean"], counts["mean"], rtol=1e-14)
    np.testing.assert_allclose(st["stddev"], counts["std"], rtol=1e-9, atol=1e-12, equal_nan=True)
    assert len(model.userStatistics()) == train["user"].nunique()
    top = model.topRatedItems(5, minCount=30)
    assert list(top.columns) == ["id", "mean", "count"] and (top["count"] > 30).all()
    assert top["mean"].is_monotonic_decreasing
    mm = MLlibALS.train(list(zip(train["user"].tolist(), train["item"].tolist(),
                                 train["rating"].tolist())), 4, iterations=2, seed=1)
    ps = mm.productStatistics()
    assert [p[0] for p in ps] == counts.index.tolist()
    assert [p[1] for p in ps] == counts["count"].tolist()
    assert len(mm.userStatistics()) == train["user"].nunique()


def test_highest_rated_movies_equals_the_host_flow(small):
    triples = list(zip(small["u"].tolist(), small["i"].tolist(), small["r"].tolist()))
    movies = [(int(m), f"movie {m}") for m in small["iid"][::-1] if m % 5]   # some untitled
    movies.append((10 ** 6, "never rated"))
    counts = personal.movie_counts_and_averages(triples)
    titles = dict(movies)
    for min_count, num in ((50, 20), (0, 1000), (65, 5)):
        want = sorted(((avg, m, c) for m, (c, avg) in counts.items()
                       if c > min_count and m in titles), key=lambda t: (-t[0], t[1]))[:num]
        want = [(avg, titles[m], c) for avg, m, c in want]
        assert personal.highest_rated_movies(small["core"], movies, min_count, num) == want
    # coarse ratings: many equal averages, ordered by id
    coarse = [(u, m, float(round(r))) for u, m, r in triples if m % 3 == 0]
    cc = personal.movie_counts_and_averages(coarse)
    every = [(m, str(m)) for m in cc]
    want = sorted(((avg, m, c) for m, (c, avg) in cc.items() if c > 0),
                  key=lambda t: (-t[0], t[1]))
    assert personal.highest_rated_movies(coarse, every, 0, 10 ** 6) == \
        [(avg, str(m), c) for avg, m, c in want]


def test_baseline_predictor_under_train_validation_split(small):
    df = _frame(small)
    grid = ParamGridBuilder().addGrid(BaselinePredictor.regItem, [1.0, 400.0]).build()
    tvs = TrainValidationSplit(BaselinePredictor(regUser=5.0, maxIter=5), grid,
                               RegressionEvaluator(labelCol="rating"), trainRatio=0.75, seed=3)
    out = tvs.fit(df)
    tr, va = tvs.split(len(df))
    u, i, r = small["u"], small["i"], small["r"]
    uid, iid = np.unique(u[tr]), np.unique(i[tr])
    sub = dict(uid=uid, iid=iid)
    us = BR.csr_from_triples(np.searchsorted(uid, u[tr]), np.searchsorted(iid, i[tr]), r[tr],
                             len(uid))
    it = BR.csr_from_triples(np.searchsorted(iid, i[tr]), np.searchsorted(uid, u[tr]), r[tr],
                             len(iid))
    want = []
    for reg_item in (1.0, 400.0):
        mu, bu, bi, _ = BR.fit(us, it, "bias", 5.0, reg_item, 5)
        pred, _ = _ref_predict(sub, mu, bu, bi, u[va], i[va])
        want.append(float(np.sqrt(((r[va].astype(np.float64) - pred) ** 2).mean())))
    print("validation rmse: device", out.validationMetrics, "reference", want)
    assert abs(want[0] - want[1]) > 1e-3 * min(want)     # a choice rounding cannot flip
    np.testing.assert_allclose(out.validationMetrics, want, rtol=1e-6)
    best = (1.0, 400.0)[int(np.argmin(want))]
    assert out.bestModel._p["regItem"] == best
    full = BaselinePredictor(regUser=5.0, maxIter=5, regItem=best).fit(df)
    assert out.bestModel.globalMean == full.globalMean
    pd.testing.assert_frame_equal(out.bestModel.itemBias, full.itemBias)
