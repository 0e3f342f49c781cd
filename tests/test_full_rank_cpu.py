"""CPU tests of the full-ranking boundary (K9, als_rank_positions / als_full_rank_metrics; no
GPU, no compute launched).

* The header, the library and the ctypes table agree on the new entry points (ABI 9).
* Argument checks run host-side and return the documented codes (small integers stand in
  for pointers; nothing is dereferenced before the checks).
* The numpy oracle against a brute-force argsort, and its band counts.
* engine.full_rank_dict, pure host arithmetic, on hand-worked cases.
* filters.relevance_lists_weighted, parameter handling of FullRankingEvaluator, the tuners'
  _score branch, and the sharded engine's refusal.
"""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import fullrank_ref as F
from als_mi355x import _lib, filters
from als_mi355x import engine as E
from als_mi355x.ml import evaluation as ml_eval
from als_mi355x.ml.evaluation import FullRankingEvaluator, RankingEvaluator
from test_abi import _header_signatures, declared_functions

NAMES = ("als_rank_positions", "als_full_rank_metrics", "als_full_rank_workspace_bytes",
         "als_rank_positions_table")


def _positions(**over):
    a = dict(Q=16, n_q=5, V=16, n_v=9, ld=8, k=8, rel_begin=16, rel_end=16, rel_col=16,
             ex_begin=0, ex_end=0, ex_col=0, allow=0, above=16, tied=16, n_adm=16, ws=0,
             ws_bytes=0, stream=0)
    a.update(over)
    return _lib.lib().als_rank_positions(*a.values())


def _metrics(**over):
    a = dict(above=16, tied=16, n_adm=16, n_q=5, rel_begin=16, rel_end=16, w=0, sums=16,
             per_row=0, ws=16, ws_bytes=1 << 20, stream=0)
    a.update(over)
    return _lib.lib().als_full_rank_metrics(*a.values())


def test_header_library_and_binding_agree():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    hdr = _header_signatures()
    for name in NAMES:
        assert name in declared_functions()
        assert hasattr(raw, name)
        assert hdr[name] == _lib.SIGNATURES[name][1]
    assert _lib.SIGNATURES["als_rank_positions"][0] is ctypes.c_int
    assert _lib.SIGNATURES["als_full_rank_metrics"][0] is ctypes.c_int
    assert _lib.SIGNATURES["als_full_rank_workspace_bytes"][0] is _lib.SZ
    # the filter arguments are als_topk_filtered's four pointers
    assert _lib.SIGNATURES["als_rank_positions"][1][9:13] == [_lib.P] * 4
    assert _lib.ABI_VERSION == 9 == _lib.lib().als_abi_version()  # a compatible addition
    assert E.FULL_RANK_SUMS == F.SUMS and len(E.FULL_RANK_SUMS) == 11


def test_table_size_matches_the_kernel_source():
    src = os.path.join(os.path.dirname(_lib.PRODUCT_LIB), "csrc", "rank_positions.hip")
    m = re.search(r"constexpr int kRpTable = (\d+);", open(src).read())
    assert m and int(m.group(1)) == E.rank_positions_table()
    t = E.rank_positions_table()
    assert t >= 2 and t & (t - 1) == 0 and t <= 4096   # bitonic network, 12 slot bits


@pytest.mark.parametrize("over,code", [
    (dict(k=0), -4), (dict(k=129, ld=132), -4), (dict(ld=6), -1), (dict(ld=4), -1),
    (dict(n_q=-1), -1), (dict(n_v=-1), -1), (dict(n_v=2 ** 31), -1),
    (dict(Q=0), -1), (dict(V=0), -1), (dict(rel_begin=0), -1), (dict(rel_end=0), -1),
    (dict(rel_col=0), -1), (dict(above=0), -1), (dict(tied=0), -1), (dict(n_adm=0), -1),
    (dict(Q=20), -1), (dict(V=24), -1),                      # not 16-byte aligned
    (dict(ex_begin=16), -1), (dict(ex_begin=16, ex_end=16), -1), (dict(ex_col=16), -1)])
def test_positions_argument_errors_before_any_device_call(over, code):
    assert _positions(**over) == code
    assert _lib.lib().als_last_error().startswith(b"als_rank_positions:")


@pytest.mark.parametrize("over,code", [
    (dict(n_q=-1), -1), (dict(above=0), -1), (dict(tied=0), -1), (dict(n_adm=0), -1),
    (dict(rel_begin=0), -1), (dict(rel_end=0), -1), (dict(sums=0), -1),
    (dict(ws=24), -1),                                        # misaligned workspace
    (dict(ws=0), -2), (dict(ws_bytes=8), -2), (dict(n_q=10 ** 9, ws_bytes=1 << 10), -2)])
def test_metrics_argument_errors_before_any_device_call(over, code):
    assert _metrics(**over) == code
    assert _lib.lib().als_last_error().startswith(b"als_full_rank_metrics:")


def test_zero_rows_of_positions_is_a_noop():
    assert _positions(Q=0, n_q=0, V=0, rel_begin=0, rel_end=0, rel_col=0, above=0, tied=0,
                      n_adm=0) == 0
    assert _positions(n_q=0, k=0) == -4          # the rank is checked even then


def test_workspace_size_is_monotone():
    ws = _lib.lib().als_full_rank_workspace_bytes
    sizes = [ws(n) for n in (0, 1, 4, 5, 1000, 10 ** 6)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    assert ws(1000) >= 8 * 11 * 250              # one 11-double partial per block of 4 rows


# ------------------------------------------------------------------ the oracle itself
def test_oracle_matches_brute_force_argsort_without_ties():
    rng = np.random.default_rng(3)
    n_q, n_v, rank = 23, 157, 9
    Q = rng.standard_normal((n_q, rank)).astype(np.float32)
    V = rng.standard_normal((n_v, rank)).astype(np.float32)
    rel = F.random_relevant(rng, n_q, n_v, rng.integers(0, 12, n_q))
    ex = F.random_exclusions(rng, n_q, n_v, rel)
    allow = rng.choice(n_v, 120, replace=False)
    for kw in (dict(), dict(ex=ex), dict(allow=allow), dict(ex=ex, allow=allow)):
        c = F.counts(Q, V, rel, **kw)
        s, _ = F.score_matrix(Q, V)
        assert all(len(np.unique(row)) == n_v for row in s)          # no ties
        assert (c["tied"][c["above"] >= 0] == 0).all()
        np.testing.assert_array_equal(c["above"], F.brute_force(Q, V, rel, **kw))
        ok = c["above"] >= 0
        assert (c["lo"][ok] <= c["above"][ok]).all() and (c["above"][ok] <= c["hi"][ok]).all()
        adm = F.admissible_mask(n_q, n_v, kw.get("ex"), kw.get("allow"))
        np.testing.assert_array_equal(c["n_adm"], adm.sum(1))
    assert (F.counts(Q, V, rel, ex=ex)["above"] == -1).sum() >= sum(
        1 for r in range(n_q) if r % 3 == 0 and len(rel[r]))


def test_oracle_counts_ties_and_nan_rows():
    Q = np.array([[1.0, 0.0]], np.float32)
    V = np.array([[3, 0], [1, 5], [1, -2], [np.nan, 0], [0, 0], [1, 1]], np.float32)
    c = F.counts(Q, V, [np.array([1, 3, 4])])
    assert c["n_adm"].tolist() == [5]                  # the NaN row is not admissible
    assert c["above"].tolist() == [1, -1, 4] and c["tied"].tolist() == [2, -1, 0]


# ------------------------------------------------------------------ full_rank_dict
def _dict_of(above, tied, n_adm, row, w=None):
    ours = E.full_rank_dict(F.sums(above, tied, n_adm, row, w))
    assert ours == pytest.approx(F.metrics(above, tied, n_adm, row, w), nan_ok=True)
    return ours


@pytest.mark.parametrize("pos", range(4))
def test_one_relevant_item_in_each_position(pos):
    d = _dict_of([pos], [0], [4], [0])
    assert d["expectedPercentileRank"] == d["meanPercentileRank"] == pos / 3
    assert d["auc"] == pytest.approx(1 - pos / 3)
    assert d["mrr"] == 1 / (1 + pos)
    assert (d["rows"], d["pairs"], d["inadmissible"]) == (1, 1, 0)


def test_fully_tied_row():
    N, m = 7, 3
    d = _dict_of([0] * m, [N - 1] * m, [N], [0] * m)
    assert d["expectedPercentileRank"] == d["meanPercentileRank"] == 0.5
    assert d["auc"] == pytest.approx(0.5)
    assert d["mrr"] == 1 / (1 + (N - 1) / 2)


def test_every_admissible_item_relevant_has_no_auc():
    d = _dict_of([0, 1, 2], [0, 0, 0], [3], [0, 0, 0])
    assert math.isnan(d["auc"]) and d["meanPercentileRank"] == 0.5 and d["mrr"] == 1.0
    two = _dict_of([0, 1, 2, 1], [0, 0, 0, 0], [3, 4], [0, 0, 0, 1])
    assert two["auc"] == pytest.approx(1 - 1 / 3)      # the second row alone is counted
    assert two["rows"] == 2


def test_single_admissible_item_and_empty_input():
    d = _dict_of([0], [0], [1], [0])
    assert math.isnan(d["expectedPercentileRank"]) and math.isnan(d["meanPercentileRank"])
    assert math.isnan(d["auc"]) and d["mrr"] == 1.0 and d["pairs"] == 1
    z = E.full_rank_dict([0.0] * 11)
    assert all(math.isnan(z[k]) for k in ("expectedPercentileRank", "meanPercentileRank", "auc",
                                          "mrr"))
    assert (z["rows"], z["pairs"], z["inadmissible"]) == (0, 0, 0)
    with pytest.raises(ValueError, match="11 sums"):
        E.full_rank_dict([0.0] * 6)


def test_weights_and_inadmissible_entries():
    above, tied, row = [0, 6, -1, 2], [0, 0, -1, 2], [0, 0, 0, 1]
    d = _dict_of(above, tied, [11, 5], row, w=[3.0, 1.0, 9.0, 2.0])
    assert d["expectedPercentileRank"] == pytest.approx((3 * 0 + 1 * 0.6 + 2 * 0.75) / 6)
    assert d["meanPercentileRank"] == pytest.approx((0.3 + 0.75) / 2)
    assert (d["rows"], d["pairs"], d["inadmissible"]) == (2, 3, 1)
    same = _dict_of(above, tied, [11, 5], row, w=[2.0] * 4)
    plain = _dict_of(above, tied, [11, 5], row)
    assert same["expectedPercentileRank"] == pytest.approx(plain["expectedPercentileRank"])


# ------------------------------------------------------------------ host-side helpers
def test_relevance_lists_weighted_keeps_the_first_rating():
    q = torch.tensor([1, 0, 1, 1, -1, 0, 1])
    o = torch.tensor([5, 2, 3, 5, 1, 2, -1])
    v = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0])
    beg, end, col, val = filters.relevance_lists_weighted(q, o, v, 3)
    b2, e2, c2 = filters.relevance_lists(q, o, 3)
    assert torch.equal(beg, b2) and torch.equal(end, e2) and torch.equal(col, c2)
    assert col.tolist() == [2, 3, 5] and val.tolist() == [2.0, 3.0, 1.0]
    assert val.dtype == torch.float32 and col.dtype == torch.int32
    empty = filters.relevance_lists_weighted(q[:0], o[:0], v[:0], 2)
    assert empty[0].tolist() == [0, 0] and empty[2].numel() == 1 and empty[3].numel() == 1
    with pytest.raises(ValueError, match="same length"):
        filters.relevance_lists_weighted(q, o, v[:2], 3)


# ------------------------------------------------------------------ evaluator
def test_full_ranking_evaluator_params():
    ev = FullRankingEvaluator()
    assert (ev.getMetricName(), ev.getLabelCol(), ev.getWeighted(), ev.getExclude()) \
        == ("expectedPercentileRank", "rating", False, "train")
    ev = FullRankingEvaluator(metricName="auc", labelCol="count", weighted=True, exclude=None)
    assert (ev.getMetricName(), ev.getLabelCol(), ev.getWeighted(), ev.getExclude()) \
        == ("auc", "count", True, None)
    assert ev.setMetricName("mrr").setLabelCol("y").setWeighted(False).setExclude("train") is ev
    assert (ev.getMetricName(), ev.getLabelCol(), ev.getWeighted(), ev.getExclude()) \
        == ("mrr", "y", False, "train")
    assert ev.setParams(metricName="meanPercentileRank", weighted=True) is ev
    assert ev.getMetricName() == "meanPercentileRank" and ev.getWeighted() is True
    with pytest.raises(ValueError, match="metricName given invalid value"):
        FullRankingEvaluator(metricName="ndcgAtK")
    with pytest.raises(ValueError, match="supported: expectedPercentileRank, meanPercentileRank, "
                                         "auc, mrr"):
        ev.setMetricName("AUC")
    with pytest.raises(TypeError):
        ev.setParams(k=10)
    assert "FullRankingEvaluator" in ml_eval.__all__
    assert ml_eval.__all__[:2] == ["RankingEvaluator", "RegressionEvaluator"]
    with pytest.raises(ValueError):                       # the at-k evaluator is unchanged
        RankingEvaluator(metricName="expectedPercentileRank")


@pytest.mark.parametrize("name,larger", [("expectedPercentileRank", False),
                                         ("meanPercentileRank", False), ("auc", True),
                                         ("mrr", True)])
def test_is_larger_better(name, larger):
    assert FullRankingEvaluator(metricName=name).isLargerBetter() is larger


def test_evaluate_without_a_model_raises():
    with pytest.raises(TypeError, match="evaluateFused"):
        FullRankingEvaluator().evaluate({"prediction": [1.0], "rating": [1.0]})


class _StubModel:
    """Stands in for a fitted model: records what the evaluator asks of it."""

    def __init__(self, value):
        self.value, self.calls = value, []

    def transform(self, dataset):
        raise AssertionError("the full-ranking evaluator must not ask for predictions")


def test_tuning_score_sends_the_evaluator_through_evaluate_fused():
    from als_mi355x.ml import tuning

    class Ev(FullRankingEvaluator):
        def evaluateFused(self, model, dataset):
            model.calls.append(dataset)
            return model.value

    stub = _StubModel(0.125)
    assert tuning._score(Ev(), stub, "validation rows") == 0.125
    assert stub.calls == ["validation rows"]


# ------------------------------------------------------------------ sharded engine
def test_sharded_engine_rejects_full_rank_metrics():
    from als_mi355x import distributed as D
    from als_mi355x.engine import ALSCore
    assert D.reject_sharded_full_rank is filters.reject_sharded_full_rank
    eng = D.ShardedALS.__new__(D.ShardedALS)  # no process group needed: it refuses at once
    with pytest.raises(NotImplementedError, match="sharded"):
        eng.full_rank_metrics([1], [2])
    with pytest.raises(NotImplementedError, match="full_rank_metrics"):
        eng.full_rank_metrics([1], [2], ratings=[1.0], weighted=True, exclude="train")
    sharded = inspect.signature(D.ShardedALS.full_rank_metrics)
    single = inspect.signature(ALSCore.full_rank_metrics)
    assert list(sharded.parameters) == list(single.parameters)
    for name, par in single.parameters.items():
        assert sharded.parameters[name].default == par.default
        assert sharded.parameters[name].kind == par.kind
