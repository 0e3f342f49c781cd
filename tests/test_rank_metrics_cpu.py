"""CPU tests of the ranking-metrics feature (no GPU, no compute launched).

* The numpy reference (tests/ranking_ref.py) reproduces the hand-derivable figures of
  upstream Spark's RankingMetricsSuite, so the GPU tests compare against a checked ruler.
* filters.relevance_lists against numpy, on CPU tensors.
* als_rank_metrics' argument checks run host-side and return the documented codes (small
  integers stand in for pointers; nothing is dereferenced before the checks).
* The public surfaces validate their parameters, import without a GPU and refuse to run
  without one; the sharded engine refuses the call.
* The end-to-end problem of tests/test_gpu_rank_metrics.py is not vacuous: with
  oracle-fitted factors its split leaves >= 80% of the users a held-out item and some
  list hits one.
"""
import numpy as np
import pytest
import torch

import ranking_ref as R
from als_mi355x import _lib, filters


# ---- the reference against Spark's known answers ----
def test_reference_mean_average_precision():
    assert R.mean_average_precision(R.SPARK_ROWS) == pytest.approx(R.SPARK_MAP, abs=1e-6)


@pytest.mark.parametrize("name,table", [("precision", R.SPARK_PRECISION),
                                        ("recall", R.SPARK_RECALL), ("map", R.SPARK_MAP_AT),
                                        ("ndcg", R.SPARK_NDCG)])
def test_reference_known_answers(name, table):
    for k, want in table.items():
        assert R.means(R.SPARK_ROWS, k)[name] == pytest.approx(want, abs=1e-6), (name, k)


def test_reference_sums_and_counts():
    s = R.sums(R.SPARK_ROWS, 5)
    assert s[4] == 2 and s[5] == 2            # the label-less row is not counted
    assert s[0] == pytest.approx(0.8)
    assert R.row_metrics([-1, -1, 3], [3], 2) == (0.0, 0.0, 0.0, 0.0)  # empty slots never hit
    assert R.row_metrics([7, 8], [7, 8], 2) == (1.0, 1.0, 1.0, 1.0)


# ---- filters.relevance_lists ----
def test_relevance_lists_against_numpy():
    rng = np.random.default_rng(4)
    n_q, n_v = 29, 40
    q = rng.integers(-1, n_q, 800)           # -1: unknown query id
    o = rng.integers(-1, n_v, 800)           # -1: unknown id of the other side
    q[:6], o[:6] = 5, 9                      # duplicates collapse
    q[q == 13] = 14                          # an empty row among non-empty ones
    beg, end, col = filters.relevance_lists(torch.as_tensor(q), torch.as_tensor(o), n_q)
    assert beg.dtype == end.dtype == torch.int64 and col.dtype == torch.int32
    assert beg.shape == end.shape == (n_q,)
    beg, end, col = beg.numpy(), end.numpy(), col.numpy()
    for r in range(n_q):
        want = np.unique(o[(q == r) & (o >= 0)])
        got = col[beg[r]:end[r]]
        np.testing.assert_array_equal(got, want)
        assert (np.diff(got) > 0).all()      # strictly ascending
    assert end[13] == beg[13]
    assert (col[beg[5]:end[5]] == 9).sum() == 1


def test_relevance_lists_empty_and_mismatched():
    beg, end, col = filters.relevance_lists(torch.tensor([-1, 2]), torch.tensor([3, -4]), 4)
    assert beg.tolist() == end.tolist() == [0, 0, 0, 0]
    assert col.numel() >= 1                  # never a null rel_col beside non-null ranges
    with pytest.raises(ValueError):
        filters.relevance_lists(torch.tensor([1]), torch.tensor([1, 2]), 4)


# ---- als_rank_metrics argument rules ----
def _call(idx=16, n_q=1, idx_ld=10, at=10, rb=16, re=16, rc=16, sums=16, per_row=0, ws=16,
          ws_bytes=1 << 20, stream=0):
    return _lib.lib().als_rank_metrics(idx, n_q, idx_ld, at, rb, re, rc, sums, per_row, ws,
                                       ws_bytes, stream)


@pytest.mark.parametrize("over,code", [
    (dict(at=0), -4), (dict(at=-3), -4), (dict(at=257, idx_ld=300), -4),
    (dict(idx_ld=9), -1), (dict(n_q=-1), -1),
    (dict(idx=0), -1), (dict(rb=0), -1), (dict(re=0), -1), (dict(rc=0), -1), (dict(sums=0), -1),
    (dict(ws=8), -1), (dict(ws=24), -1),
    (dict(ws_bytes=16), -2), (dict(ws=0, ws_bytes=0), -2),
    (dict(n_q=10 ** 6, ws_bytes=4096 + 256), -2)])
def test_rank_metrics_argument_errors(over, code):
    L = _lib.lib()
    assert _call(**over) == code
    assert L.als_last_error()                # a message is set


def test_rank_metrics_error_order_and_empty_call():
    # a bad `at` is reported before anything else; n_q = 0 needs no pointer at all
    assert _call(at=300, idx_ld=2, n_q=-1, idx=0, ws=8) == -4
    assert _call(idx=0, n_q=0, rb=0, re=0, rc=0, sums=0, ws=0, ws_bytes=0) == 0
    assert _call(idx=0, n_q=0, at=0, sums=0, ws=0, ws_bytes=0) == -4


def test_rank_metrics_workspace_is_monotone():
    ws = _lib.lib().als_rank_metrics_workspace_bytes
    sizes = [ws(n) for n in (0, 1, 4, 5, 1030, 10 ** 4, 10 ** 6, 10 ** 9)]
    assert sizes == sorted(sizes)
    assert ws(1) < ws(1030) < ws(10 ** 6)
    assert ws(0) > 0 and ws(10 ** 9) < (1 << 20)  # the partials are capped, not O(n_q)


# ---- surfaces ----
def test_evaluation_modules_import_without_gpu():
    from als_mi355x.ml.evaluation import RankingEvaluator
    from als_mi355x.mllib.evaluation import RankingMetrics
    ev = RankingEvaluator()
    assert ev.getMetricName() == "meanAveragePrecision" and ev.getK() == 10
    assert ev.getPredictionCol() == "prediction" and ev.getLabelCol() == "label"
    assert ev.isLargerBetter() is True
    assert ev.setK(3).setMetricName("ndcgAtK").getK() == 3
    assert callable(RankingMetrics.precisionAt)


def test_ranking_evaluator_rejects_bad_params():
    from als_mi355x.ml.evaluation import RankingEvaluator
    for name in ("meanAveragePrecision", "meanAveragePrecisionAtK", "precisionAtK", "ndcgAtK",
                 "recallAtK"):
        assert RankingEvaluator(metricName=name).getMetricName() == name
    with pytest.raises(ValueError, match="metricName"):
        RankingEvaluator(metricName="rmse")
    with pytest.raises(ValueError, match="metricName"):
        RankingEvaluator().setMetricName("precisionAt")
    for k in (0, -1):
        with pytest.raises(ValueError):
            RankingEvaluator(k=k)
        with pytest.raises(ValueError):
            RankingEvaluator().setK(k)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_ranking_metrics_refuses_to_run_without_gpu():
    from als_mi355x.ml.evaluation import RankingEvaluator
    from als_mi355x.mllib.evaluation import RankingMetrics
    with pytest.raises(_lib.ALSNativeError, match="no CPU fallback"):
        RankingMetrics(R.SPARK_ROWS)
    with pytest.raises(_lib.ALSNativeError, match="no CPU fallback"):
        RankingEvaluator().evaluate({"prediction": [[1, 2]], "label": [[2]]})


def test_models_and_sharded_engine_expose_the_call():
    import inspect

    from als_mi355x import distributed as D
    from als_mi355x import engine as E
    from als_mi355x.ml.recommendation import ALSModel
    from als_mi355x.mllib.recommendation import MatrixFactorizationModel
    sig = inspect.signature(E.ALSCore.rank_metrics)
    for kw in ("ratings", "threshold", "user_side", "exclude", "candidates", "per_row"):
        assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY
    assert "ratingThreshold" in inspect.signature(ALSModel.evaluateRanking).parameters
    assert "threshold" in inspect.signature(MatrixFactorizationModel.rankingMetrics).parameters
    with pytest.raises(NotImplementedError, match="sharded"):
        D.ShardedALS.rank_metrics(None, [1], [2], 10, exclude="train")
    d = E.rank_metrics_dict([1.0, 2.0, 3.0, 4.0, 4.0, 2.0], 4)
    assert d == {"precision": 0.25, "recall": 0.5, "map": 0.75, "ndcg": 1.0, "hitRate": 0.5,
                 "rows": 4}
    assert all(np.isnan(v) for k, v in E.rank_metrics_dict([0.0] * 6, 0).items() if k != "rows")


# ---- the end-to-end problem is not vacuous ----
def test_e2e_split_leaves_rows_and_hits():
    from oracle import als_oracle as O
    (u, i, r), test = R.e2e_problem()
    U, V, umap, imap, uids, iids = O.train(u, i, r, R.E2E_RANK, R.E2E_ITERS, R.E2E_REG,
                                           seed=R.E2E_FIT_SEED)
    assert len(uids) == R.E2E_USERS           # every user keeps a training rating
    score = np.asarray(U, np.float64) @ np.asarray(V, np.float64).T
    score[umap[u], imap[i]] = -np.inf         # exclude="train"
    top = np.argsort(-score, axis=1, kind="stable")[:, :10]
    lists = {int(uids[a]): [int(iids[j]) for j in top[a]] for a in range(len(uids))}
    for thr in (None, R.E2E_THRESHOLD):
        rows = R.held_out_rows(lists, test, iids, thr)
        s = R.sums(rows, 10)
        assert s[4] == len(rows)
        print(f"threshold {thr}: rows {len(rows)}, rows with a hit {int(s[5])}")
        assert len(rows) >= 0.8 * R.E2E_USERS, thr
        assert s[5] > 0, thr
