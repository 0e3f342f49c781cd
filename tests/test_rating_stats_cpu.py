"""CPU tests of K16 (no GPU): the numpy reference against personal.movie_counts_and_averages and
hand-computed cases, the ABI of the new entry points, their host-side argument checks (which
come before any device call), the refusing stubs of the sharded engine, and the properties of
the reference the GPU tests lean on."""
import ctypes
import json
import os

import numpy as np
import pytest

import baseline_ref as BR
from als_mi355x import _lib, filters, personal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("als_rating_stats_task", "als_rating_stats_group_rows", "als_rating_stats_scratch_bytes",
         "als_row_moments", "als_bias_update", "als_baseline_predict")


# ---------------------------------------------------------------- the reference itself
def test_reference_agrees_with_movie_counts_and_averages():
    rng = np.random.default_rng(1)
    n = 4000
    u = rng.integers(0, 300, n)
    m = rng.integers(5, 95, n)
    r = rng.integers(1, 11, n) * 0.5
    want = personal.movie_counts_and_averages(list(zip(u.tolist(), m.tolist(), r.tolist())))
    ids = np.unique(m)
    rows = np.searchsorted(ids, m)
    side = BR.csr_from_triples(rows, u, r, len(ids))
    mom, total, _, _ = BR.row_moments(*side, 300)
    assert len(want) == len(ids)
    for j, a in enumerate(ids):
        assert want[int(a)] == (int(mom[j, 0]), mom[j, 1] / mom[j, 0])
    assert total[0] == n and total[1] == r.sum() and total[3] == r.min() and total[4] == r.max()


def test_reference_on_the_golden_personal_ratings():
    """The reference's own rated movies (twelve one-rating rows): counts and averages."""
    data = json.load(open(os.path.join(ROOT, "tests", "golden", "personal_ratings.json")))
    u, m, r = (np.asarray(c) for c in zip(*data["my_rated_movies"]))
    want = personal.movie_counts_and_averages(list(zip(u.tolist(), m.tolist(), r.tolist())))
    ids = np.unique(m)
    side = BR.csr_from_triples(np.searchsorted(ids, m), np.zeros(len(m), np.int32), r, len(ids))
    mom = BR.row_moments(*side, 1)[0]
    for j, a in enumerate(ids):
        c, avg = want[int(a)]
        assert (c, avg) == (int(mom[j, 0]), mom[j, 1] / mom[j, 0])


def test_hand_computed_moments_bias_and_prediction():
    # rows: [1, 2, 3, 4 | (none) | 5]   columns 0, 1, 0, 7(outside), | 1
    row_ptr = np.array([0, 4, 4, 5])
    col = np.array([0, 1, 0, 7, 1], np.int32)
    val = np.array([1, 2, 3, 4, 5], np.float32)
    mom, total, a, q = BR.row_moments(row_ptr, col, val, 2)
    assert mom[0].tolist() == [4.0, 10.0, 5.0, 1.0, 4.0]
    assert mom[1, :3].tolist() == [0.0, 0.0, 0.0] and np.isnan(mom[1, 3:]).all()
    assert mom[2].tolist() == [1.0, 5.0, 0.0, 5.0, 5.0]
    assert total.tolist() == [5.0, 15.0, 10.0, 1.0, 5.0]
    assert a.tolist() == [10.0, 0.0, 5.0, 15.0] and q.tolist() == [30.0, 0.0, 25.0, 55.0]
    # offset 1 and other = [0.5, -1]: e = [-0.5, 2, 1.5, 3 (col 7: no gather) | 5]
    mom, total, _, _ = BR.row_moments(row_ptr, col, val, 2, other=[0.5, -1.0], offset=1.0)
    assert mom[0].tolist() == [4.0, 6.0, 6.5, -0.5, 3.0]
    assert mom[2].tolist() == [1.0, 5.0, 0.0, 5.0, 5.0]
    assert total[:2].tolist() == [5.0, 11.0]
    assert BR.bias_update(mom, 2.0).tolist() == [1.0, 0.0, 5.0 / 3.0]
    assert BR.bias_update(mom, 0.0).tolist() == [1.5, 0.0, 5.0]
    pred, known = BR.predict([0, -1, 1, -1, 2], [1, 0, -1, -1, 0], 3.0, [0.5, -0.25], [1.0, 2.0])
    assert pred.tolist() == [5.5, 4.0, 2.75, 3.0, 4.0] and known.tolist() == [3, 2, 1, 0, 2]
    assert pred.dtype == np.float32 and known.dtype == np.uint8
    pred, known = BR.predict_sized([0, 1], [0, 5], 3.0, None, 2, [1.0], 1)
    assert pred.tolist() == [4.0, 3.0] and known.tolist() == [3, 1]


def test_top_rated_is_strict_and_breaks_ties_by_id():
    ids, count, total = [7, 3, 9, 4, 5], [2, 2, 5, 1, 0], [8.0, 8.0, 20.0, 5.0, 0.0]
    assert BR.top_rated(ids, count, total, 10) == [(4, 5.0, 1), (3, 4.0, 2), (7, 4.0, 2),
                                                   (9, 4.0, 5)]
    assert BR.top_rated(ids, count, total, 10, min_count=2) == [(9, 4.0, 5)]     # strict >
    assert BR.top_rated(ids, count, total, 10, min_count=1) == [(3, 4.0, 2), (7, 4.0, 2),
                                                                (9, 4.0, 5)]
    assert BR.top_rated(ids, count, total, 2, min_count=1) == [(3, 4.0, 2), (7, 4.0, 2)]
    # damping pulls short rows down: 8 / 7, 20 / 10, 5 / 6
    assert [t[0] for t in BR.top_rated(ids, count, total, 10, damping=5.0)] == [9, 3, 7, 4]


def _planted(rng, n_u, n_i, density):
    mask = rng.random((n_u, n_i)) < density
    mask[np.arange(n_u), rng.integers(0, n_i, n_u)] = True
    mask[rng.integers(0, n_u, n_i), np.arange(n_i)] = True
    u, i = np.nonzero(mask)
    r = np.clip(np.round(2 * (3.4 + rng.normal(0, 0.7, n_u)[u] + rng.normal(0, 0.5, n_i)[i]
                              + rng.normal(0, 0.6, len(u)))) / 2, 0.5, 5.0)
    return u, i, r


def test_alternating_fit_never_raises_its_objective():
    """Each update is the exact minimiser over its table (a line search with the exact step),
    so the reference's history is non-increasing; the one-step methods sit between "global"
    and the alternating fit."""
    rng = np.random.default_rng(5)
    u, i, r = _planted(rng, 60, 40, 0.2)
    us, it = BR.csr_from_triples(u, i, r, 60), BR.csr_from_triples(i, u, r, 40)
    mu, bu, bi, hist = BR.fit(us, it, "bias", 10.0, 25.0, 8)
    assert mu == pytest.approx(r.mean(), rel=1e-15)
    assert len(hist) == 8
    for a, b in zip(hist, hist[1:]):
        assert b <= a * (1 + 1e-14)
    g = BR.fit(us, it, "global")[3][0]
    for method in ("item", "user"):
        h = BR.fit(us, it, method, 10.0, 25.0)[3]
        assert len(h) == 1 and hist[-1] <= h[0] <= g
    assert g == pytest.approx(((r - r.mean()) ** 2).sum(), rel=1e-12)


def test_two_pass_m2_is_stable_where_the_textbook_formula_is_not():
    """The case the GPU test holds to 1e-9: ratings 1e4 + N(0, 1) in fp32.  The two-pass value
    agrees with exact rational arithmetic far inside that tolerance; sum e^2 - sum^2 / n does
    not reach it."""
    from fractions import Fraction
    rng = np.random.default_rng(9)
    _, _, val = BR.csr_from_lengths([3000], 1, rng, "shifted")
    e = val.astype(np.float64)
    fr = [Fraction(float(x)) for x in e]
    mean = sum(fr) / len(fr)
    exact = float(sum((x - mean) ** 2 for x in fr))
    two_pass = BR.row_moments(np.array([0, 3000]), np.zeros(3000, np.int32), val, 1)[0][0, 2]
    assert abs(two_pass - exact) <= 1e-12 * exact
    assert abs(BR.textbook_m2(e) - exact) > 1e-9 * exact


# ---------------------------------------------------------------- ABI
def test_header_prototypes_equal_the_binding_and_abi_is_9():
    from test_abi import _header_signatures
    hdr = _header_signatures()
    for name in NAMES:
        assert hdr[name] == _lib.SIGNATURES[name][1], name
    for name in ("als_row_moments", "als_bias_update", "als_baseline_predict"):
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
    assert _lib.SIGNATURES["als_rating_stats_scratch_bytes"][0] is _lib.SZ
    assert _lib.ABI_VERSION == 9 and _lib.lib().als_abi_version() == 9


def test_new_names_keep_clear_of_the_other_registries():
    for name in NAMES:
        assert not name.endswith("_workspace_bytes") and not name.startswith("als_list_")


def test_task_and_group_constants():
    L = _lib.lib()
    assert L.als_rating_stats_task() >= 64 and L.als_rating_stats_task() % 4 == 0
    assert 1 <= L.als_rating_stats_group_rows() <= 256
    sz = L.als_rating_stats_scratch_bytes
    assert 0 < sz(0, 1) <= sz(10 ** 4, 10) <= sz(10 ** 7, 10) <= sz(10 ** 7, 10 ** 6)
    assert sz(-1, 1) == 0 and sz(1, -1) == 0


def test_host_side_argument_checks_need_no_device():
    L = _lib.lib()
    off = ctypes.c_double(0.0)
    po = ctypes.addressof(off)
    big = 1 << 30
    ok = dict(row_ptr=8, col=16, val=16, nnz=4, n_rows=2, n_cols=3, other=0, offset=po,
              moments=8, total=8, ws=16, ws_bytes=big, stream=0)

    def moments(**over):
        a = dict(ok)
        a.update(over)
        return L.als_row_moments(*a.values())

    for over, code in [(dict(nnz=-1), -1), (dict(n_rows=-1), -1), (dict(n_cols=-1), -1),
                       (dict(moments=0), -1), (dict(total=0), -1), (dict(row_ptr=0), -1),
                       (dict(val=0), -1), (dict(other=8, col=0), -1), (dict(other=4), -1),
                       (dict(ws=0), -2), (dict(ws_bytes=8), -2), (dict(ws=8), -1),
                       (dict(nnz=1 << 40), -4)]:
        assert moments(**over) == code, over
        assert L.als_last_error()
    # n_rows = 0 is valid and does nothing: not even the outputs are looked at
    assert moments(n_rows=0, nnz=0, moments=0, total=0, row_ptr=0, ws=0, ws_bytes=0) == 0
    damp = ctypes.c_double(2.0)
    pd_ = ctypes.addressof(damp)
    assert L.als_bias_update(8, -1, pd_, 8, 0) == -1
    assert L.als_bias_update(8, 3, pd_, 0, 0) == -1
    assert L.als_bias_update(0, 3, pd_, 8, 0) == -1
    assert L.als_bias_update(0, 0, pd_, 0, 0) == 0
    for bad in (-1.0, float("nan"), float("inf")):
        damp.value = bad
        assert L.als_bias_update(8, 3, pd_, 8, 0) == -1
    mu = ctypes.c_double(3.5)
    pm = ctypes.addressof(mu)
    assert L.als_baseline_predict(4, 4, -1, pm, 0, 1, 0, 1, 4, 1, 0) == -1
    assert L.als_baseline_predict(4, 4, 5, pm, 0, -1, 0, 1, 4, 1, 0) == -1
    assert L.als_baseline_predict(4, 4, 5, pm, 0, 1, 0, 1, 0, 1, 0) == -1      # NULL pred
    assert L.als_baseline_predict(4, 4, 5, pm, 0, 1, 0, 1, 4, 0, 0) == -1      # NULL known
    assert L.als_baseline_predict(0, 4, 5, pm, 0, 1, 0, 1, 4, 1, 0) == -1
    assert L.als_baseline_predict(0, 0, 0, pm, 0, 0, 0, 0, 0, 0, 0) == 0       # n = 0
    assert L.als_last_error()


def test_every_rating_stats_size_function_has_a_bounds_case():
    import test_gpu_rating_stats_bounds as BB
    sizers = sorted(n for n in _lib.SIGNATURES
                    if n.startswith("als_rating_stats_") and n.endswith("_bytes"))
    assert sizers == sorted(BB.SCRATCH_CASES) and sizers
    for name, tests in BB.SCRATCH_CASES.items():
        assert tests
        for t in tests:
            assert callable(getattr(BB, t, None)), f"{name}: {t} is not a test of the bounds file"


# ---------------------------------------------------------------- Python layer
def test_sharded_engine_refuses_rating_statistics():
    import inspect

    from als_mi355x.distributed import ShardedALS
    from als_mi355x.engine import ALSCore
    with pytest.raises(NotImplementedError, match="single-GPU engine"):
        filters.reject_sharded_rating_stats()
    for name, args in (("rating_stats", ()), ("global_stats", ()), ("top_rated", (5,)),
                       ("fit_baseline", ())):
        with pytest.raises(NotImplementedError, match="single-GPU engine"):
            getattr(ShardedALS, name)(None, *args)
        assert list(inspect.signature(getattr(ShardedALS, name)).parameters) == \
            list(inspect.signature(getattr(ALSCore, name)).parameters)


def test_a_core_without_ratings_says_so():
    from als_mi355x.engine import ALSCore
    core = ALSCore.__new__(ALSCore)
    core.user_block = core.item_block = None
    for call in (core.rating_stats, core.global_stats, lambda: core.top_rated(3),
                 core.fit_baseline):
        with pytest.raises(ValueError, match="from_factors"):
            call()
    with pytest.raises(ValueError, match="method must be"):
        core.fit_baseline("median")


def test_baseline_predictor_params_and_param_maps():
    from als_mi355x.ml.param import Param
    from als_mi355x.ml.recommendation import ALS, BaselinePredictor
    est = BaselinePredictor(regItem=5.0, userCol="u")
    assert est.getRegItem() == 5.0 and est.getMethod() == "bias" and est.getMaxIter() == 10
    assert est.getColdStartStrategy() == "fallback" and est.getUserCol() == "u"
    assert BaselinePredictor.regItem == Param("BaselinePredictor", "regItem")
    for name in ("regUser", "regItem", "method", "maxIter"):
        assert isinstance(getattr(BaselinePredictor, name), Param)
    cp = est.copy({BaselinePredictor.regItem: 1.0, "method": "item"})
    assert (cp.getRegItem(), cp.getMethod(), est.getRegItem()) == (1.0, "item", 5.0)
    assert est.setRegUser(3.0) is est and est.getOrDefault(BaselinePredictor.regUser) == 3.0
    with pytest.raises(ValueError, match="not a parameter"):
        est.copy({ALS.rank: 4})
    with pytest.raises(TypeError):
        BaselinePredictor(rank=3)
    for bad in (dict(method="median"), dict(regUser=-1.0), dict(maxIter=0),
                dict(coldStartStrategy="zero")):
        with pytest.raises(ValueError):
            BaselinePredictor(**bad).fit({"user": [1], "item": [1], "rating": [1.0]})
