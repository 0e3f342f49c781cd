"""CPU tests of the diversified lists boundary (K14, als_diversify / als_list_similarity; no
GPU, nothing launched).

* The fp64 reference (diversify_ref.py) on a planted case worked by hand: four clusters of
  ten items around e1..e4, a user who likes them in that order.
* The header, the library and the ctypes table agree on the two entry points, ABI still 9.
* Argument errors: ValueError from the binding before the library is touched, and the
  documented codes from the C entry points (small integers stand in for pointers).
* The sharded engine carries recommend_diverse / list_similarity and refuses them.
* personal_recommendations_fold_in(trade_off=None) is the call without the argument.
"""
import inspect
import re

import numpy as np
import pytest
import torch

import diversify_ref as R
from als_mi355x import _lib, engine as E, filters, personal
from test_abi import HEADER, _header_signatures, declared_functions

NAMES = ("als_diversify", "als_list_similarity")


def test_reference_on_the_planted_clusters():
    V, u = R.planted_clusters()
    idx, sc = R.pool_of(u, V, 8, 40)
    cluster = lambda i: np.asarray(i) // 10
    # the pool is cluster 1, then 2, 3, 4 (scores ~1, .9, .8, .7 with noise 1e-3)
    np.testing.assert_array_equal(cluster(idx[0]), np.repeat([0, 1, 2, 3], 10))
    i1, s1, ils1, slots1 = R.mmr(idx, sc, V, 8, 8, 1.0)
    assert (cluster(i1[0]) == 0).all()                      # pure relevance: cluster 1 only
    np.testing.assert_array_equal(i1[0], idx[0, :8])        # = the pool's prefix, exactly
    assert s1.tobytes() == sc[:, :8].tobytes() and slots1 == [list(range(8))]
    assert ils1[0] > 0.999
    # lam = 0.5, by hand: after a pick from cluster 1 its siblings cost 0.5 * ~1 while a
    # cluster-2 item costs 0.5 * ~0 and loses only 0.5 * (rel 1 - rel 2/3): one of each first
    i5, s5, ils5, _ = R.mmr(idx, sc, V, 8, 8, 0.5)
    assert sorted(cluster(i5[0, :4]).tolist()) == [0, 1, 2, 3]
    assert cluster(i5[0, 0]) == 0 and i5[0, 0] == idx[0, 0]
    # ... after which a cluster-1 sibling (0.5 * ~1 - 0.5 * ~1 = ~0) beats a second item of
    # any other cluster (at most 0.5 * 2/3 - 0.5): the last four picks are cluster 1 again
    assert sorted(cluster(i5[0]).tolist()) == [0, 0, 0, 0, 0, 1, 2, 3]
    assert ils5[0] < 0.4 < ils1[0]
    # 10 same-cluster pairs of 28 at cosine ~1; the other 18 are of the order of the noise
    np.testing.assert_allclose(ils5[0], 10 / 28, atol=3e-3)
    # the plain list's ILS from the second entry point's reference
    np.testing.assert_allclose(R.list_similarity(idx[:, :8], V, 8), ils1, atol=1e-12)
    # and the checker accepts the reference's own picks and rejects a wrong one
    R.check_greedy(idx, sc, V, 8, 0.5, i5, s5, 8)
    bad = i5.copy()
    bad[0, 1] = idx[0, 1]                                   # a second cluster-1 item at step 1
    bs = s5.copy()
    bs[0, 1] = sc[0, 1]
    with pytest.raises(AssertionError):
        R.check_greedy(idx, sc, V, 8, 0.5, bad, bs, 8)


def test_reference_dead_slots_ties_and_degenerate_rows():
    V = np.array([[1, 0], [1, 0], [0, 1], [0, 0], [np.inf, 1]], np.float32)
    idx = np.array([[0, 1, -1, 2, 7, 3, 4]], np.int32)
    sc = np.array([[3, 3, 9, 2, 8, 1, np.nan]], np.float32)
    live = R.live_slots(idx[0], sc[0], len(V))
    np.testing.assert_array_equal(live, [1, 1, 0, 1, 0, 1, 0])
    oi, os_, ils, slots = R.mmr(idx, sc, V, 2, 7, 0.5)
    # step 0: slots 0 and 1 tie at rel 1 -> slot 0; then e2 (slot 3: 0.25 - 0) beats the
    # duplicate (slot 1: 0.5 - 0.5) and the zero row (slot 5: 0 - 0); then slot 1 ties with
    # slot 5 at 0 -> the lower slot; the zero row last; three open slots
    assert slots == [[0, 3, 1, 5]]
    np.testing.assert_array_equal(oi[0], [0, 2, 1, 3, -1, -1, -1])
    np.testing.assert_array_equal(os_[0], [3, 2, 3, 1] + [-np.inf] * 3)
    np.testing.assert_allclose(ils[0], 1 / 6)               # one pair of six has cosine 1
    # lam = 1 never forms inf * 0: the live slots in pool order
    oi1, _, _, slots1 = R.mmr(idx, sc, V, 2, 7, 1.0)
    assert slots1 == [[0, 1, 3, 5]]
    # equal scores: rel 1 for all; fewer than two picks: NaN
    _, _, ils2, s2 = R.mmr(np.array([[2, 0]], np.int32), np.array([[5, 5]], np.float32), V, 2, 2,
                           0.3)
    assert s2 == [[0, 1]] and ils2[0] == 0.0
    assert np.isnan(R.mmr(idx[:, :1], sc[:, :1], V, 2, 1, 0.3)[2][0])
    assert np.isnan(R.list_similarity(np.array([[-1, 9, 1]], np.int32), V, 2)[0])
    np.testing.assert_allclose(R.list_similarity(np.array([[0, 1, 2, 4]], np.int32), V, 2),
                               [1 / 6])


def test_header_library_and_binding_agree():
    import ctypes
    raw = ctypes.CDLL(_lib.LIB_PATH)
    hdr = _header_signatures()
    for name in NAMES:
        assert name in declared_functions()
        assert hasattr(raw, name)
        assert hdr[name] == _lib.SIGNATURES[name][1]
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
    assert _lib.ABI_VERSION == 9 == _lib.lib().als_abi_version()
    assert int(re.search(r"#define ALS_ABI_VERSION (\d+)", open(HEADER).read()).group(1)) == 9
    assert E.DIVERSIFY_MAX_POOL == 256


def _mmr(**over):
    a = dict(V=16, n_v=100, ld=64, k=64, idx=16, score=16, n_q=1, m=50, top=10, lam=0.7,
             out_idx=16, out_score=16, out_ils=16, stream=0)
    a.update(over)
    return _lib.lib().als_diversify(*a.values())


def _ils(**over):
    a = dict(V=16, n_v=100, ld=64, k=64, idx=16, n_q=1, m=50, out=16, stream=0)
    a.update(over)
    return _lib.lib().als_list_similarity(*a.values())


@pytest.mark.parametrize("over,code", [
    (dict(k=0), -4), (dict(k=129, ld=132), -4), (dict(m=0, top=0), -4), (dict(m=257), -4),
    (dict(top=0), -1), (dict(top=51), -1), (dict(lam=-0.01), -1), (dict(lam=1.01), -1),
    (dict(lam=float("nan")), -1), (dict(ld=62), -1), (dict(ld=60), -1), (dict(n_v=-1), -1),
    (dict(n_v=2 ** 31), -1), (dict(n_q=-1), -1), (dict(V=0), -1), (dict(V=20), -1),
    (dict(idx=0), -1), (dict(score=0), -1), (dict(out_idx=0), -1), (dict(out_score=0), -1),
    (dict(out_ils=0), -1)])
def test_diversify_argument_errors_before_any_device_call(over, code):
    assert _mmr(**over) == code
    assert b"als_diversify" in _lib.lib().als_last_error()


@pytest.mark.parametrize("over,code", [
    (dict(k=0), -4), (dict(k=129, ld=132), -4), (dict(m=0), -4), (dict(m=257), -4),
    (dict(ld=62), -1), (dict(n_v=-1), -1), (dict(n_q=-1), -1), (dict(V=0), -1),
    (dict(V=24), -1), (dict(idx=0), -1), (dict(out=0), -1)])
def test_list_similarity_argument_errors_before_any_device_call(over, code):
    assert _ils(**over) == code
    assert b"als_list_similarity" in _lib.lib().als_last_error()


def test_zero_rows_is_a_noop():
    assert _mmr(n_q=0, V=0, idx=0, score=0, out_idx=0, out_score=0, out_ils=0) == 0
    assert _ils(n_q=0, V=0, idx=0, out=0) == 0


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name}) before the range checks")


@pytest.mark.parametrize("kw", [
    dict(top=0), dict(top=6), dict(lam=-0.1), dict(lam=1.5), dict(lam=float("nan")),
    dict(rank=0), dict(rank=129), dict(n_v=-1), dict(m=0), dict(m=257), dict(flat=True),
    dict(sc_m=4)])
def test_binding_range_checks_raise_value_error(monkeypatch, kw):
    monkeypatch.setattr(_lib, "lib", lambda: _NoLibrary())
    a = dict(top=3, lam=0.5, rank=8, n_v=6, m=5, flat=False, sc_m=None)
    a.update(kw)
    V = torch.zeros((6, E.ld_for(8)))
    idx = torch.zeros((2, a["m"]), dtype=torch.int32)
    sc = torch.zeros((2, a["sc_m"] or a["m"]))
    if a["flat"]:
        idx, sc = idx.reshape(-1), sc.reshape(-1)
    with pytest.raises(ValueError):
        E.diversify_rows(idx, sc, V, a["n_v"], a["rank"], a["top"], a["lam"])
    if not set(kw) & {"top", "lam", "sc_m"}:
        with pytest.raises(ValueError):
            E.list_similarity_rows(idx, V, a["n_v"], a["rank"])


def _cpu_core(n=5, gap=3):
    core = E.ALSCore.__new__(E.ALSCore)
    core.device = torch.device("cpu")
    core.rank = 4
    ids = torch.arange(n, dtype=torch.int32) * gap
    mp = torch.full((int(ids.max()) + 1,), -1, dtype=torch.int32)
    mp[ids.long()] = torch.arange(n, dtype=torch.int32)
    core.iidx = E.IdIndex(mp, ids, n, 0)
    core.uidx = E.IdIndex(mp.clone(), ids.clone(), n, 0)
    core.U = torch.zeros((n, 4))
    core.V = torch.zeros((n, 4))
    return core


def test_engine_argument_checks_and_unknown_ids_need_no_kernel(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _NoLibrary())
    core = _cpu_core()
    for kw in (dict(top=0), dict(top=3, trade_off=1.2), dict(top=3, trade_off=float("nan")),
               dict(top=3, pool=0), dict(top=3, pool=257), dict(top=3, chunk_rows=0)):
        with pytest.raises(ValueError):
            core.recommend_diverse(**kw)
    keys, ids, sc, ils = core.recommend_diverse(3, ids=[1, 2, 100, -7])   # all unknown
    assert keys.numel() == 0 and tuple(ids.shape) == tuple(sc.shape) == (0, 3)
    assert ils.dtype == torch.float64 and ils.numel() == 0
    _, ids, _, _ = core.recommend_diverse(10, False, ids=[1], pool=20)   # t = min(top, pool, n)
    assert tuple(ids.shape) == (0, 5)
    with pytest.raises(ValueError):
        core.list_similarity([1, 2, 3])
    bare = E.ALSCore.__new__(E.ALSCore)
    bare.U = bare.V = None
    with pytest.raises(ValueError, match="factors"):
        bare.recommend_diverse(3)
    with pytest.raises(ValueError, match="factors"):
        bare.list_similarity([[1, 2]])
    sig = inspect.signature(E.ALSCore.recommend_diverse)
    assert list(sig.parameters) == ["self", "top", "user_side", "ids", "trade_off", "pool",
                                    "exclude", "candidates", "chunk_rows"]
    assert sig.parameters["trade_off"].default == 0.7
    assert sig.parameters["ids"].kind is inspect.Parameter.KEYWORD_ONLY


def test_reject_sharded_diversify_under_a_gloo_group(tmp_path, monkeypatch):
    import torch.distributed as dist
    from als_mi355x import distributed as D
    assert D.reject_sharded_diversify is filters.reject_sharded_diversify
    assert "reject_sharded_diversify" in filters.__all__
    assert filters.reject_sharded_diversify() is None          # no process group
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'rdzv'}", rank=0,
                            world_size=1)
    try:
        assert filters.reject_sharded_diversify() is None      # a world of one: single GPU
        # what a rank of a larger world holds is the sharded engine
        monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 4)
        with pytest.raises(NotImplementedError, match="sharded"):
            filters.reject_sharded_diversify()
        made = {}
        monkeypatch.setattr(D.ShardedALS, "__init__", lambda self, *a, **k: made.update(s=1))
        eng = E.make_engine([1], [2], [3.0])
        assert isinstance(eng, D.ShardedALS) and made
        with pytest.raises(NotImplementedError, match="sharded"):
            eng.recommend_diverse(10, ids=[1], trade_off=0.5)
        with pytest.raises(NotImplementedError, match="sharded"):
            eng.list_similarity([[1, 2]])
    finally:
        monkeypatch.undo()
        dist.destroy_process_group()
    for name in ("recommend_diverse", "list_similarity"):
        sharded = inspect.signature(getattr(D.ShardedALS, name))
        single = inspect.signature(getattr(E.ALSCore, name))
        assert list(sharded.parameters) == list(single.parameters)
        for p in sharded.parameters:
            assert sharded.parameters[p].default == single.parameters[p].default
            assert sharded.parameters[p].kind == single.parameters[p].kind


class _FoldInEngine:
    """Records recommend_new and serves a fixed list: enough for the host side of
    personal_recommendations_fold_in."""

    def __init__(self):
        self.calls = []

    def recommend_new(self, u, m, r, top, **kw):
        self.calls.append((u.tolist(), m.tolist(), r.tolist(), top,
                           {k: (v.tolist() if hasattr(v, "tolist") else v)
                            for k, v in kw.items()}))
        ids = torch.tensor([[30, 10, 20][:top] + [0] * max(0, top - 3)], dtype=torch.int32)
        sc = torch.tensor([[4.5, 4.0, 3.5][:top] + [float("-inf")] * max(0, top - 3)])
        return torch.tensor([7], dtype=torch.int32), ids, sc


def test_personal_fold_in_trade_off_none_is_the_plain_call():
    class Model:
        engine = _FoldInEngine()
    rated = [(7, 1, 5.0), (7, 2, 3.0)]
    movies = [(10, "A"), (20, "B"), (30, "C"), (40, "D")]
    counts = {10: 100, 20: (90, 3.0), 30: 80, 40: 5}
    plain = personal.personal_recommendations_fold_in(Model, rated, movies, counts, 0.1, num=5)
    none = personal.personal_recommendations_fold_in(Model, rated, movies, counts, 0.1, num=5,
                                                     trade_off=None)
    assert plain == none == [(4.5, "C", 80), (4.0, "A", 100), (3.5, "B", 90)]
    assert Model.engine.calls[0] == Model.engine.calls[1]
    assert Model.engine.calls[0][3] == 5 and Model.engine.calls[0][4]["candidates"] == [10, 20, 30]
    sig = inspect.signature(personal.personal_recommendations_fold_in)
    assert sig.parameters["trade_off"].default is None
