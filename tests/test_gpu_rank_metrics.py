"""GPU tests of kernel K6 (als_rank_metrics) and the surfaces over it, against the numpy
fp64 restatement of Spark's RankingMetrics in tests/ranking_ref.py.

Synthetic lists, so the hits are under the test's control.  Row r of the pattern:
  0  m = 0 (random list: nothing can hit)
  1  m = 1, an all -1 list: no hits, every value exactly 0
  2  m = 1000 (> at; search depth): the range's first element at position 0, its last at
     position at - 1, ids outside the range between them
  3  m = at, every position a hit: every value exactly 1.0
  4  the SAME range as row 3 (aliased slice): its first half, then a -1 tail
  then r % 8 of 5: m = at + 3 with random hits, 6: valid ids but no hits, 7: random,
  0-4 as above (rows 3 and 4 of every group alias one slice of their own)
The n_q cases are prefixes of one 1030-row pattern per `at`, whose reference is computed
once.  Columns [at, idx_ld) hold a relevant id, so a read past `at` would count as a hit.

Bounds: per-row precision and recall are one correctly rounded fp64 division of two
integers and must equal the reference bit for bit; AP, NDCG and the sums agree within
1e-12 relative (at most 256 fp64 terms at 2^-53 each plus a few ulp of log2, about 3e-14).
"""
import functools

import numpy as np
import pytest
import torch

import ranking_ref as R
from als_mi355x import _lib
from als_mi355x import engine as E

pytestmark = pytest.mark.gpu

N_V = 4096
N_MAX = 1030
ATS = (1, 10, 63, 64, 65, 100, 256)
N_QS = (0, 1, 3, 4, 5, 257, 1030)
RTOL = 1e-12


def pattern_inputs(at, n_max=N_MAX):
    """(lists int32 [n_max, at], begin, end int64 [n_max], col int32, rows): the pattern's
    first n_max rows.  Rows are drawn one after another from one generator, so a shorter
    pattern is a prefix of a longer one."""
    rng = np.random.default_rng(1000 + at)
    lists = np.empty((n_max, at), np.int32)
    begin = np.zeros(n_max, np.int64)
    end = np.zeros(n_max, np.int64)
    cols, off, labels = [], 0, []

    def new_range(lab):
        nonlocal off
        lab = np.sort(np.asarray(lab, np.int32))
        cols.append(lab)
        off += len(lab)
        return off - len(lab), off

    for r in range(n_max):
        kind = r if r < 5 else r % 8
        rnd = rng.integers(0, N_V, at)
        if kind == 0:
            lab, lists[r] = [], rnd
        elif kind == 1:
            lab, lists[r] = [int(rng.integers(0, N_V))], -1
        elif kind == 2:
            lab = np.sort(rng.choice(N_V, 1000, replace=False))
            outside = np.setdiff1d(np.arange(N_V), lab)
            lists[r] = rng.choice(outside, at)
            lists[r, at - 1] = lab[-1]
            lists[r, 0] = lab[0]
        elif kind == 3:
            lab = rng.choice(N_V, at, replace=False)
            lists[r] = rng.permutation(lab)
        elif kind == 4:
            lab = labels[r - 1]                      # the slice of row 3, aliased
            lists[r] = -1
            half = (at + 1) // 2
            lists[r, :half] = rng.permutation(lab)[:half]
        elif kind == 5:
            lab = rng.choice(N_V, at + 3, replace=False)
            lists[r] = np.where(rng.random(at) < 0.3, rng.choice(lab, at), rnd)
        elif kind == 6:
            lab = rng.choice(N_V // 2, 5, replace=False)
            lists[r] = N_V // 2 + rnd // 2           # valid ids, none relevant
        else:
            lab = rng.choice(N_V, int(rng.integers(1, 40)), replace=False)
            lists[r] = np.where(rng.random(at) < 0.2, rng.choice(lab, at), rnd)
        labels.append(np.asarray(lab, np.int64))
        if kind == 4:
            begin[r], end[r] = begin[r - 1], end[r - 1]
        else:
            begin[r], end[r] = new_range(lab)
    col = np.concatenate(cols + [np.zeros(1, np.int32)])
    rows = [(lists[r], labels[r]) for r in range(n_max)]
    return lists, begin, end, col, rows


@functools.lru_cache(maxsize=None)
def pattern(at):
    """pattern_inputs(at) and the per-row reference of its N_MAX rows."""
    lists, begin, end, col, rows = pattern_inputs(at)
    return lists, begin, end, col, rows, R.per_row(rows, at)


def run(idx, at, begin, end, col, per_row=True):
    sums, pr = E.rank_metrics_rows(idx, at, begin, end, col, E.Workspace(idx.device), per_row)
    return sums.cpu().numpy(), (pr.cpu().numpy() if pr is not None else None)


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("at", ATS)
def test_kernel_against_reference(at, pad):
    dev = torch.device("cuda")
    lists, begin, end, col, rows, ref = pattern(at)
    wide = np.empty((N_MAX, at + pad), np.int32)
    wide[:, :at] = lists
    wide[:, at:] = col[np.minimum(begin, len(col) - 1)][:, None]  # a relevant id past `at`
    idx_all = torch.as_tensor(wide, device=dev)
    b_all, e_all = torch.as_tensor(begin, device=dev), torch.as_tensor(end, device=dev)
    c = torch.as_tensor(col, device=dev)
    for n_q in N_QS:
        idx = idx_all[:n_q]
        assert n_q <= 1 or idx.stride(0) == at + pad
        sums, pr = run(idx, at, b_all[:n_q], e_all[:n_q], c)
        want = ref[:n_q]
        has = np.array([len(l) > 0 for _, l in rows[:n_q]], bool)
        assert pr.shape == (n_q, 4)
        # precision, recall: bit for bit
        np.testing.assert_array_equal(pr[:, :2], want[:, :2], err_msg=f"n_q {n_q}")
        # AP, NDCG: 1e-12 relative
        np.testing.assert_allclose(pr[:, 2:], want[:, 2:], rtol=RTOL, atol=0, err_msg=f"n_q {n_q}")
        want_sums = np.array([want[:, j].sum() for j in range(4)]
                             + [float(has.sum()), float((want[:, 0] > 0).sum())])
        np.testing.assert_allclose(sums[:4], want_sums[:4], rtol=RTOL, atol=0,
                                   err_msg=f"n_q {n_q}")
        np.testing.assert_array_equal(sums[4:], want_sums[4:], err_msg=f"n_q {n_q}")
        # exact rows
        for r in range(min(n_q, 5)):
            if r in (0, 1):
                assert (pr[r] == 0.0).all(), (n_q, r, pr[r])
            if r == 3:
                assert (pr[r] == 1.0).all(), (n_q, r, pr[r])
        for r in range(n_q):
            if r >= 5 and r % 8 == 6:
                assert (pr[r] == 0.0).all(), (n_q, r, pr[r])
            if r >= 5 and r % 8 == 3:
                assert (pr[r] == 1.0).all(), (n_q, r, pr[r])
        # a second call, and a call without the per-row output: bit-identical sums
        again, _ = run(idx, at, b_all[:n_q], e_all[:n_q], c)
        lean, none = run(idx, at, b_all[:n_q], e_all[:n_q], c, per_row=False)
        assert none is None
        assert sums.tobytes() == again.tobytes() == lean.tobytes(), n_q


def test_kernel_rejects_bad_lists():
    dev = torch.device("cuda")
    z = torch.zeros(4, dtype=torch.int64, device=dev)
    c = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = E.Workspace(dev)
    with pytest.raises(ValueError):
        E.rank_metrics_rows(torch.zeros((4, 3), dtype=torch.int32, device=dev), 4, z, z, c, ws)
    with pytest.raises(ValueError):
        E.rank_metrics_rows(torch.zeros((4, 3), dtype=torch.int64, device=dev), 3, z, z, c, ws)
    with pytest.raises(_lib.ALSNativeError, match="at"):
        E.rank_metrics_rows(torch.zeros((4, 300), dtype=torch.int32, device=dev), 257, z, z, c, ws)


# ---- Spark's known answers through the public surfaces ----
def _check_spark(m):
    assert m.meanAveragePrecision == pytest.approx(R.SPARK_MAP, abs=1e-6)
    for k, want in R.SPARK_PRECISION.items():
        assert m.precisionAt(k) == pytest.approx(want, abs=1e-9), k
    for k, want in R.SPARK_RECALL.items():
        assert m.recallAt(k) == pytest.approx(want, abs=1e-9), k
    for k, want in R.SPARK_MAP_AT.items():
        assert m.meanAveragePrecisionAt(k) == pytest.approx(want, abs=1e-6), k
    for k, want in R.SPARK_NDCG.items():
        assert m.ndcgAt(k) == pytest.approx(want, abs=1e-6), k
    assert m.ndcgAt(15) == m.ndcgAt(10)
    for k in (1, 4, 15, 200):                # and the reference at full precision
        ref = R.means(R.SPARK_ROWS, k)
        got = dict(precision=m.precisionAt(k), recall=m.recallAt(k),
                   map=m.meanAveragePrecisionAt(k), ndcg=m.ndcgAt(k))
        for name in ref:
            assert got[name] == pytest.approx(ref[name], rel=RTOL, abs=0), (name, k)


def test_mllib_ranking_metrics_known_answers():
    from als_mi355x.mllib.evaluation import RankingMetrics
    _check_spark(RankingMetrics(R.SPARK_ROWS))
    # any int32 id: the same rows under an injective map onto negative and large ids
    def far(ids):
        return [int(x) * 214748364 - 2 ** 31 for x in ids]
    _check_spark(RankingMetrics((far(p), far(l)) for p, l in R.SPARK_ROWS))
    m = RankingMetrics(R.SPARK_ROWS)
    with pytest.raises(ValueError):
        m.precisionAt(257)
    with pytest.raises(ValueError):
        m.ndcgAt(0)
    # duplicate labels count once; a row list longer than k; no rows with labels at all
    assert RankingMetrics([([1, 2, 3], [2, 2, 2])]).recallAt(3) == 1.0
    empty = RankingMetrics([([1, 2], [])])
    assert empty.precisionAt(2) == 0.0 and empty.meanAveragePrecision == 0.0


def test_ml_ranking_evaluator_known_answers():
    import pandas as pd

    from als_mi355x.ml.evaluation import RankingEvaluator
    df = pd.DataFrame({"prediction": [p for p, _ in R.SPARK_ROWS],
                       "label": [l for _, l in R.SPARK_ROWS]})
    assert RankingEvaluator().evaluate(df) == pytest.approx(R.SPARK_MAP, abs=1e-6)
    for name, key, table in (("precisionAtK", "precision", R.SPARK_PRECISION),
                             ("recallAtK", "recall", R.SPARK_RECALL),
                             ("meanAveragePrecisionAtK", "map", R.SPARK_MAP_AT),
                             ("ndcgAtK", "ndcg", R.SPARK_NDCG)):
        for k, want in table.items():
            ev = RankingEvaluator(metricName=name, k=k)
            got = ev.evaluate(df)
            assert got == pytest.approx(want, abs=1e-6), (name, k)
            assert got == pytest.approx(R.means(R.SPARK_ROWS, k)[key], rel=RTOL, abs=0)
    other = {"p": df["prediction"].tolist(), "l": df["label"].tolist()}
    ev = RankingEvaluator(metricName="ndcgAtK", k=5, predictionCol="p", labelCol="l")
    assert ev.evaluate(other) == pytest.approx(R.SPARK_NDCG[5], abs=1e-6)


# ---- end to end: a fitted model against a held-out split ----
def _compare(got, lists, test, known_items, thr):
    rows = R.held_out_rows(lists, test, known_items, thr)
    s = R.sums(rows, 10)
    print({k: got[k] for k in ("precision", "recall", "map", "ndcg", "hitRate", "rows")})
    assert got["rows"] == len(rows) == int(s[4])
    assert got["rows"] >= 0.8 * R.E2E_USERS and got["hitRate"] > 0   # not vacuous
    for j, name in enumerate(("precision", "recall", "map", "ndcg")):
        assert got[name] == pytest.approx(s[j] / len(rows), rel=RTOL, abs=0), name
    assert got["hitRate"] == s[5] / len(rows)
    return rows


@pytest.mark.parametrize("thr", [None, R.E2E_THRESHOLD])
def test_als_model_evaluate_ranking(thr):
    import pandas as pd

    from als_mi355x.ml.recommendation import ALS
    (u, i, r), test = R.e2e_problem()
    model = ALS(rank=R.E2E_RANK, maxIter=R.E2E_ITERS, regParam=R.E2E_REG,
                seed=R.E2E_FIT_SEED).fit(pd.DataFrame({"user": u, "item": i, "rating": r}))
    test_df = pd.DataFrame({"user": test[0], "item": test[1], "rating": test[2]})
    got = model.evaluateRanking(test_df, 10, ratingThreshold=thr, exclude="train")
    known = model.engine.item_factors()[0].cpu().numpy()
    rel = np.isin(test[1], known) & (True if thr is None else test[2] >= thr)
    # the same query users in the same order, so the lists are the kernel's own
    recs = model.recommendForUserSubset(test_df[rel], 10, exclude="train")
    lists = {int(k): [int(a) for a, _ in v] for k, v in zip(recs["user"], recs["recommendations"])}
    _compare(got, lists, test, known, thr)


def test_mllib_model_ranking_metrics_and_per_row():
    from als_mi355x.mllib.recommendation import ALS
    (u, i, r), test = R.e2e_problem()
    model = ALS.train(np.stack([u, i, r], axis=1), R.E2E_RANK, iterations=R.E2E_ITERS,
                      lambda_=R.E2E_REG, seed=R.E2E_FIT_SEED)
    core = model.engine
    known = core.item_factors()[0].cpu().numpy()
    held = np.stack(test, axis=1)
    for thr in (None, R.E2E_THRESHOLD):
        got = model.rankingMetrics(held if thr is not None else held[:, :2], 10, threshold=thr,
                                   exclude="train")
        rel = np.isin(test[1], known) & (True if thr is None else test[2] >= thr)
        keys, ids, sc = core.recommend_subset(test[0][rel], 10, True, exclude="train")
        ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
        lists = {int(k): [int(a) for a, s in zip(ri, rs) if np.isfinite(s)]
                 for k, ri, rs in zip(keys.cpu().numpy(), ids, sc)}
        rows = _compare(got, lists, test, known, thr)
        full = core.rank_metrics(test[0], test[1], 10, ratings=test[2], threshold=thr,
                                 exclude="train", per_row=True)
        assert {k: full[k] for k in got} == got
        np.testing.assert_array_equal(full["keys"].cpu().numpy(), keys.cpu().numpy())
        want = R.per_row(rows, 10)
        pr = full["per_row"].cpu().numpy()
        np.testing.assert_array_equal(pr[:, :2], want[:, :2])
        np.testing.assert_allclose(pr[:, 2:], want[:, 2:], rtol=RTOL, atol=0)
    # no relevant pair at all: NaN means over zero rows
    none = core.rank_metrics([10 ** 6], [3], 10)
    assert none["rows"] == 0 and np.isnan(none["map"]) and np.isnan(none["hitRate"])
    # `at` is capped by the rows of the other side
    capped = core.rank_metrics(test[0], test[1], 256)
    assert capped["rows"] >= 0.8 * R.E2E_USERS
    assert capped["recall"] == 1.0            # all 200 items listed: every relevant one is hit
    with pytest.raises(ValueError):
        core.rank_metrics(test[0], test[1], 257)
