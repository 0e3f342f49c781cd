"""K15 on the GPU (als_list_exposure, als_list_concentration, als_list_novelty) against the
numpy fp64 restatement list_metrics_ref.py.

Counts and the integer fields are compared exactly (everything stays far below 2^53); Gini,
entropy and the novelty values at rtol 1e-12, the bar of the K6 tests for fp64 values built
from log2.  Every call runs twice and must give the same bytes.
"""
import functools
import math

import numpy as np
import pytest
import torch

import list_metrics_ref as LR
from als_mi355x import _lib, engine as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL = 1e-12
I32_MIN = np.iinfo(np.int32).min


@functools.lru_cache(maxsize=None)
def _window():
    return E.list_exposure_window() or 4099


def _d(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _lists(n_q, at, n_v, seed, pad=3, zipf=False):
    """idx int32 [n_q, at + pad]: the first `at` columns valid rows, garbage past them."""
    rng = np.random.default_rng(seed)
    if zipf:
        p = 1.0 / np.arange(1, n_v + 1) ** 1.1
        body = rng.permutation(n_v)[rng.choice(n_v, size=(n_q, at), p=p / p.sum())]
    else:
        body = rng.integers(0, n_v, size=(n_q, at))
    idx = np.concatenate([body, rng.integers(-5, 2 ** 31 - 1, size=(n_q, pad))], axis=1)
    return idx.astype(np.int32)


def _exposure(idx, at, n_v, bits=None, view=True):
    """Runs twice (byte-identical), returns (counts, skipped) as numpy / int."""
    full = _d(idx)
    lists = full[:, :at] if view else full
    b = None if bits is None else _d(bits)
    c1, s1 = E.list_exposure_rows(lists, at, n_v, b)
    c2, s2 = E.list_exposure_rows(lists, at, n_v, b)
    torch.cuda.synchronize()
    assert torch.equal(c1, c2) and torch.equal(s1, s2)
    return c1.cpu().numpy(), int(s1.item())


def _w_cases():
    w = _window()
    return [  # n_v, at, n_q: every value of each axis appears once or more
        (1, 10, 70), (31, 1, 5000), (32, 64, 3), (33, 65, 70), (1200, 256, 3),
        (w - 1, 10, 5000), (w, 64, 70), (w + 1, 65, 1), (2 * w + 3, 10, 5000),
        (2 * w + 3, 256, 70)]


@pytest.mark.parametrize("case", range(10))
def test_exposure_equals_bincount(case):
    n_v, at, n_q = _w_cases()[case]
    idx = _lists(n_q, at, n_v, seed=case)
    got, skipped = _exposure(idx, at, n_v)
    want = np.bincount(idx[:, :at].reshape(-1), minlength=n_v)
    assert got.dtype == np.int32 and (got == want).all() and skipped == 0
    assert int(got.sum()) == n_q * at


@pytest.mark.parametrize("n_v", [33, "2w+3"])
def test_exposure_skip_rules_and_mask(n_v):
    n_v = 2 * _window() + 3 if n_v == "2w+3" else n_v
    rng = np.random.default_rng(n_v)
    at, n_q = 10, 300
    idx = _lists(n_q, at, n_v, seed=5)
    hit = rng.random((n_q, at))
    idx[:, :at][hit < 0.1] = -1
    idx[:, :at][(hit >= 0.1) & (hit < 0.15)] = n_v
    idx[:, :at][(hit >= 0.15) & (hit < 0.2)] = I32_MIN
    idx[7, :at] = -1                                  # a row with nothing
    allowed = rng.random(n_v) < 0.6
    bits = LR.pack_bits(allowed).copy()
    if n_v % 32:
        bits[-1] |= np.int32(-1) << np.int32(n_v % 32)   # bits past n_v: ignored
    for b in (None, bits):
        want, want_skipped = LR.exposure(idx, at, n_v, b)
        got, skipped = _exposure(idx, at, n_v, b)
        assert (got == want).all() and skipped == want_skipped
        assert skipped > 0 and (b is None or not got[~allowed].any())


def test_exposure_maximal_contention_and_zipf():
    n_v = 2 * _window() + 3
    same = np.full((5000, 4), 7, np.int32)
    got, skipped = _exposure(same, 4, n_v, view=False)
    assert got[7] == 20000 and int(got.sum()) == 20000 and skipped == 0
    z = _lists(5000, 64, n_v, seed=9, zipf=True)
    got, _ = _exposure(z, 64, n_v)
    want = np.bincount(z[:, :64].reshape(-1), minlength=n_v)
    assert (got == want).all() and want.max() > 50 * np.median(want[want > 0])


def test_exposure_accumulates_and_overwrites():
    n_v, at = _window() + 1, 10
    idx = _lists(701, at, n_v, seed=2)
    idx[::9, 3] = -1
    whole, skipped = _exposure(idx, at, n_v)
    a, b = _d(idx[:300])[:, :at], _d(idx[300:])[:, :at]
    dirty = torch.full((n_v,), 12345, dtype=torch.int32, device=DEV)
    dirty_skip = torch.full((1,), 99, dtype=torch.int64, device=DEV)
    L = _lib.lib()
    rc = L.als_list_exposure(a.data_ptr(), 300, a.stride(0), at, n_v, 0, 0, dirty.data_ptr(),
                             dirty_skip.data_ptr(), 0)
    assert rc == 0
    torch.cuda.synchronize()
    assert (dirty.cpu().numpy() == np.bincount(idx[:300, :at][idx[:300, :at] >= 0],
                                               minlength=n_v)).all()   # overwritten in full
    c, s = E.list_exposure_rows(b, at, n_v, counts=dirty, skipped=dirty_skip)
    assert c is dirty and (c.cpu().numpy() == whole).all() and int(s.item()) == skipped
    # n_q == 0: zeroes unless accumulating
    empty = torch.empty((0, at), dtype=torch.int32, device=DEV)
    c2, _ = E.list_exposure_rows(empty, at, n_v, counts=c.clone())
    assert (c2.cpu().numpy() == whole).all()
    c3, s3 = E.list_exposure_rows(empty, at, n_v)
    assert not c3.any() and int(s3.item()) == 0


# ------------------------------------------------------------------ concentration
def _concentration(counts, bits=None, n_lists=5, at=10):
    c = _d(counts, torch.int32)
    b = None if bits is None else _d(bits)
    ws = E.Workspace(torch.device(DEV))
    o1 = E.list_concentration(c, len(counts), b, n_lists, at, ws).clone()
    o2 = E.list_concentration(c, len(counts), b, n_lists, at, ws)
    torch.cuda.synchronize()
    assert o1.cpu().numpy().tobytes() == o2.cpu().numpy().tobytes()
    return o1.cpu().numpy()


def _assert_concentration(got, want):
    for f in (0, 1, 2, 5, 6):
        assert got[f] == want[f], (f, got[f], want[f])
    for f in (3, 4):
        if math.isnan(want[f]):
            assert math.isnan(got[f]), f
        else:
            np.testing.assert_allclose(got[f], want[f], rtol=RTOL, atol=0)


@pytest.mark.parametrize("n_v", [1, 2, 33, 1200, 70001])
def test_concentration_against_the_reference(n_v):
    rng = np.random.default_rng(n_v)
    p = 1.0 / np.arange(1, n_v + 1) ** 1.05
    counts = rng.permutation(rng.multinomial(40 * n_v + 7, p / p.sum()))
    _assert_concentration(_concentration(counts), LR.concentration(counts))
    # masked catalogue, with counts on rows outside it and bits past n_v set
    in_cat = rng.random(n_v) < 0.5
    in_cat[rng.integers(n_v)] = True
    bits = LR.pack_bits(in_cat).copy()
    if n_v % 32:
        bits[-1] |= np.int32(-1) << np.int32(n_v % 32)
    got = _concentration(counts, bits)
    _assert_concentration(got, LR.concentration(counts, bits))
    assert got[0] == in_cat.sum()
    # all zero: NaN; one non-zero: Gini 1 - 1/n and entropy 0; all equal: Gini 0, entropy log2 n
    z = _concentration(np.zeros(n_v, np.int64))
    assert z[:3].tolist() == [n_v, 0, 0] and np.isnan(z[3:5]).all() and z[5:].tolist() == [0, 0]
    one = np.zeros(n_v, np.int64)
    one[n_v // 2] = 11
    got = _concentration(one)
    _assert_concentration(got, LR.concentration(one))
    assert got[4] == 0.0 and got[5] == 55.0 and got[6] == 11.0
    np.testing.assert_allclose(got[3], 1.0 - 1.0 / n_v, rtol=RTOL, atol=0)
    eq = _concentration(np.full(n_v, 6))
    assert eq[3] == 0.0 and eq[1] == n_v and eq[6] == 6.0
    np.testing.assert_allclose(eq[4], math.log2(n_v), rtol=RTOL, atol=0)


def test_concentration_of_an_empty_catalogue():
    out = torch.full((7,), 5.0, dtype=torch.float64, device=DEV)
    rc = _lib.lib().als_list_concentration(0, 0, 0, 3, 10, out.data_ptr(), 0, 0, 0)
    assert rc == 0
    o = out.cpu().numpy()
    assert o[[0, 1, 2, 5, 6]].tolist() == [0, 0, 0, 0, 0] and np.isnan(o[3:5]).all()


# ------------------------------------------------------------------ novelty
def _novelty(idx, at, n_v, pop, n_pop, bits=None, tail=None):
    lists = _d(idx)[:, :at]
    ws = E.Workspace(torch.device(DEV))
    args = (lists, at, n_v, _d(pop, torch.int32), n_pop, ws,
            None if bits is None else _d(bits), None if tail is None else _d(tail))
    s1, r1 = E.list_novelty_rows(*args, per_row=True)
    s1 = s1.clone()
    s2, r2 = E.list_novelty_rows(*args, per_row=True)
    s3, r3 = E.list_novelty_rows(*args)
    torch.cuda.synchronize()
    assert r3 is None
    for a, b in ((s1, s2), (r1, r2), (s1, s3)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    return s1.cpu().numpy(), r1.cpu().numpy()


@pytest.mark.parametrize("at,n_q", [(1, 70), (10, 5000), (64, 3), (65, 70), (256, 1), (10, 1027)])
def test_novelty_against_the_reference(at, n_q):
    n_v = 1200
    rng = np.random.default_rng(at * 7 + n_q)
    idx = _lists(n_q, at, n_v, seed=at + n_q, zipf=True)
    hit = rng.random((n_q, at))
    idx[:, :at][hit < 0.08] = -1
    idx[:, :at][(hit >= 0.08) & (hit < 0.1)] = n_v
    pop = rng.integers(0, 3000, size=n_v)
    pop[rng.random(n_v) < 0.1] = 0
    if n_q >= 3:
        idx[0, :at] = I32_MIN                            # no valid entry
        idx[2, :at] = np.nonzero(pop == 0)[0][:1]        # only pop = 0 entries
    allowed = rng.random(n_v) < 0.8
    tail = LR.pack_bits(LR.long_tail(pop, n_v, 0.2))
    for bits, t in ((None, tail), (LR.pack_bits(allowed), tail), (None, None)):
        want_s, want_r = LR.novelty(idx, at, n_v, pop, 4321, bits, t)
        got_s, got_r = _novelty(idx, at, n_v, pop, 4321, bits, t)
        assert (np.isnan(got_r) == np.isnan(want_r)).all()
        np.testing.assert_allclose(got_r, want_r, rtol=RTOL, atol=0, equal_nan=True)
        np.testing.assert_allclose(got_s, want_s, rtol=RTOL, atol=0)
        assert got_s[[1, 3, 5, 6]].tolist() == [want_s[i] for i in (1, 3, 5, 6)]
        if t is None:
            assert np.isnan(got_r[:, 2]).all() and got_s[4] == 0.0
    if n_q >= 3:
        assert np.isnan(got_r[0]).all() and math.isnan(got_r[2, 0]) and got_r[2, 1] == 0.0


def test_novelty_of_no_lists_zeroes_the_sums():
    ws = E.Workspace(torch.device(DEV))
    s, r = E.list_novelty_rows(torch.empty((0, 4), dtype=torch.int32, device=DEV), 4, 9,
                               torch.ones(9, dtype=torch.int32, device=DEV), 3, ws, per_row=True)
    assert not s.any() and tuple(r.shape) == (0, 3)


# ------------------------------------------------------------------ status codes
def test_status_codes_of_the_host_checks():
    L = _lib.lib()
    idx = torch.zeros((4, 8), dtype=torch.int32, device=DEV)
    cnt = torch.zeros(16, dtype=torch.int32, device=DEV)
    out = torch.zeros(7, dtype=torch.float64, device=DEV)
    w = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    ip, cp, op, wp = idx.data_ptr(), cnt.data_ptr(), out.data_ptr(), w.data_ptr()

    def expo(n_q=4, ld=8, at=8, n_v=16, i=ip, c=cp):
        return L.als_list_exposure(i, n_q, ld, at, n_v, 0, 0, c, 0, 0)

    def conc(n_v=16, at=8, n_lists=4, c=cp, o=op, ws=wp, nb=w.numel()):
        return L.als_list_concentration(c, n_v, 0, n_lists, at, o, ws, nb, 0)

    def nov(n_q=4, ld=8, at=8, n_v=16, n_pop=5, i=ip, p=cp, o=op, ws=wp, nb=w.numel()):
        return L.als_list_novelty(i, n_q, ld, at, n_v, 0, p, n_pop, 0, o, 0, ws, nb, 0)

    assert expo() == 0 and conc() == 0 and nov() == 0
    for f in (expo, conc, nov):
        assert f(at=0) == -4 and f(at=257) == -4
        assert f(n_v=-1) == -1 and f(n_v=2 ** 31 - 1) == -1
    for f in (expo, nov):
        assert f(n_q=-1) == -1 and f(ld=7) == -1 and f(i=0) == -1
    assert expo(c=0) == -1 and conc(c=0) == -1 and conc(o=0) == -1 and conc(n_lists=-1) == -1
    assert nov(n_pop=0) == -1 and nov(p=0) == -1 and nov(o=0) == -1
    assert conc(ws=wp + 8) == -1 and nov(ws=wp + 8) == -1            # misaligned
    assert conc(nb=64) == -2 and conc(ws=0) == -2 and nov(nb=8) == -2 and nov(ws=0) == -2
    assert L.als_last_error()
    assert expo(n_q=0, i=0) == 0 and nov(n_q=0, i=0, p=0, ws=0, nb=0) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ end to end
GAP = 2


@pytest.fixture(scope="module")
def fitted():
    import pandas as pd

    from als_mi355x.ml.recommendation import ALS
    from helpers import planted
    u, i, r = planted(300, 180, density=0.1, seed=21, dup=30, id_gap=GAP, heavy_items=(3, 50))
    df = pd.DataFrame({"user": u, "item": i, "rating": r})
    return ALS(rank=8, maxIter=3, regParam=0.1, seed=3).fit(df), df


def _rows_of_recs(core, top, **kw):
    keys, ids, sc = core.recommend_all(top, **kw)
    rows = (ids.cpu().numpy() // GAP).astype(np.int32)
    rows[~np.isfinite(sc.cpu().numpy())] = -1
    return rows


def _assert_dict(got, want):
    assert set(want) <= set(got)
    for k, v in want.items():
        if isinstance(v, float) and math.isnan(v):
            assert math.isnan(got[k]), k
        elif k in ("lists", "entries", "skipped", "coverage", "topItemShare", "personalization"):
            assert got[k] == v, (k, got[k], v)
        else:
            np.testing.assert_allclose(got[k], v, rtol=RTOL, atol=0, err_msg=k)


def test_engine_list_metrics_end_to_end(fitted):
    model, df = fitted
    core = model.engine
    n_u, n_i = core.n_users, core.n_items
    pop = np.bincount(df["item"].to_numpy() // GAP, minlength=n_i)
    assert (core.popularity().cpu().numpy() == pop).all()
    want = LR.metrics_dict(_rows_of_recs(core, 10), 10, n_i, None, pop, n_u)
    got = core.list_metrics(top=10)
    _assert_dict(got, want)
    assert got["lists"] == n_u and got["entries"] == 10 * n_u and 0 < got["coverage"] < 1
    # the same lists handed in as ids
    _, ids, _ = core.recommend_all(10)
    _assert_dict(core.list_metrics(ids), want)
    # exclude="train" changes the lists, candidates= the lists and the catalogue
    want = LR.metrics_dict(_rows_of_recs(core, 10, exclude="train"), 10, n_i, None, pop, n_u)
    _assert_dict(core.list_metrics(top=10, exclude="train"), want)
    cand_rows = np.arange(0, n_i, 3)
    cand = cand_rows * GAP
    bits = LR.pack_bits(np.isin(np.arange(n_i), cand_rows))
    want = LR.metrics_dict(_rows_of_recs(core, 10, candidates=cand), 10, n_i, bits, pop, n_u, 0.3)
    got = core.list_metrics(top=10, candidates=cand, head_fraction=0.3)
    _assert_dict(got, want)
    assert got["coverage"] == want["coverage"] and got["skipped"] == 0
    # given lists measured over a narrower catalogue: what is off it is skipped
    got = core.list_metrics(ids, candidates=cand)
    _assert_dict(got, LR.metrics_dict(_rows_of_recs(core, 10), 10, n_i, bits, pop, n_u))
    assert got["skipped"] > 0
    # per row
    got = core.list_metrics(top=10, per_row=True)
    tail = LR.pack_bits(LR.long_tail(pop, n_i, 0.2))
    _, rows = LR.novelty(_rows_of_recs(core, 10), 10, n_i, pop, n_u, None, tail)
    np.testing.assert_allclose(got["per_row"].cpu().numpy(), rows, rtol=RTOL, equal_nan=True)
    assert got["keys"].tolist() == core.uidx.ids().tolist()
    # the item side lists users
    upop = np.bincount(df["user"].to_numpy() // GAP, minlength=n_u)
    keys, uids, sc = core.recommend_all(5, user_side=False)
    want = LR.metrics_dict((uids.cpu().numpy() // GAP).astype(np.int32), 5, n_u, None, upop, n_i)
    _assert_dict(core.list_metrics(top=5, user_side=False), want)


def test_from_factors_core_and_the_public_surfaces(fitted, tmp_path):
    import pandas as pd

    from als_mi355x.ml.recommendation import ALSModel
    from als_mi355x.mllib.evaluation import ListMetrics
    from als_mi355x.mllib.recommendation import MatrixFactorizationModel
    model, df = fitted
    core = model.engine
    full = core.list_metrics(top=10)
    bare = E.ALSCore.from_factors(core.uidx.ids(), core.U[:, :8], core.iidx.ids(), core.V[:, :8])
    got = bare.list_metrics(top=10)
    for k in ("novelty", "averagePopularity", "longTailShare"):
        assert math.isnan(got[k]) and not math.isnan(full[k])
    for k in ("coverage", "gini", "entropy", "personalization", "topItemShare", "entries"):
        assert got[k] == full[k], k
    item_ids, cnt = np.unique(df["item"].to_numpy(), return_counts=True)
    assert bare.list_metrics(top=10, popularity=(item_ids, cnt)) == full
    # ml
    assert model.evaluateListQuality(numItems=10) == full
    recs = model.recommendForAllUsers(10)
    assert model.evaluateListQuality(recs) == full
    ex = model.evaluateListQuality(numItems=10, exclude="train", headFraction=0.3)
    assert ex == core.list_metrics(top=10, exclude="train", head_fraction=0.3) and ex != full
    per = model.listQualityPerRow(recs)
    assert list(per.columns) == ["user", "novelty", "averagePopularity", "longTailShare"]
    want = core.list_metrics(top=10, per_row=True)["per_row"].cpu().numpy()
    np.testing.assert_array_equal(per[["novelty", "averagePopularity", "longTailShare"]]
                                  .to_numpy(), want)
    assert list(per["user"]) == list(recs["user"])
    assert model.listQualityPerRow(numItems=10).equals(per)
    items = model.evaluateListQuality(model.recommendForAllItems(5))
    assert items == core.list_metrics(top=5, user_side=False)
    with pytest.raises(ValueError, match="either recommendations or numItems"):
        model.evaluateListQuality()
    model.save(str(tmp_path / "m"))
    loaded = ALSModel.load(str(tmp_path / "m"))
    assert math.isnan(loaded.evaluateListQuality(numItems=10)["novelty"])
    assert loaded.evaluateListQuality(numItems=10, popularity=(item_ids, cnt)) == full
    assert loaded.listQualityPerRow(recs, popularity=(item_ids, cnt)).equals(per)
    # mllib
    mf = MatrixFactorizationModel(core)
    assert mf.listMetrics(10) == full
    assert mf.listMetrics(10, exclude="train") == core.list_metrics(top=10, exclude="train")
    lists = [[a for a, _ in lst] for lst in recs["recommendations"]]
    lm = ListMetrics(lists, popularity=dict(zip(item_ids.tolist(), cnt.tolist())),
                     numUsers=core.n_users, catalog=item_ids)
    assert lm.toDict() == full and lm.coverage == full["coverage"] and lm.gini == full["gini"]
    anon = ListMetrics(lists)
    assert anon.personalization == full["personalization"] and math.isnan(anon.novelty)
    assert anon.coverage == 1.0                # the catalogue is what the lists name
    with pytest.raises(AttributeError):
        lm.nothing


def _blockbusters(n_users, n_items, density, seed, spread=1.0):
    """Explicit ratings dominated by an item-quality term: every user's plain list is the same
    few best items."""
    rng = np.random.default_rng(seed)
    mask = rng.random((n_users, n_items)) < density
    mask[np.arange(n_users), rng.integers(0, n_items, n_users)] = True
    mask[rng.integers(0, n_users, n_items), np.arange(n_items)] = True
    u, i = np.nonzero(mask)
    q = rng.normal(0, 1, n_items)
    us, vs = rng.normal(0, 0.35, (n_users, 8)), rng.normal(0, 0.35, (n_items, 8))
    r = 3.0 + spread * q[i] + (us[u] * vs[i]).sum(1) + rng.normal(0, 0.3, len(u))
    r = np.clip(np.round(r * 2) / 2, 0.5, 5)
    return u.astype(np.int32), i.astype(np.int32), r.astype(np.float32)


def test_diversified_lists_cover_no_less_of_the_catalogue():
    """On a wide-pool explicit fit, trade-off 0.3 reaches at least as many items as trade-off
    1 over the same pool.  This is a property of the data, not of the kernels (the counts
    behind it are exact integers).  The data set was picked by the fp64 reference,
    diversify_ref.mmr run on the host over the fp32 factors this very fit produces: it covers
    40 items at trade-off 1 and 46 at 0.3 here (2000 users, 300 items, quality spread 1.5,
    seed 6); 17 and 19 at 400 users with spread 1, and 23 and 23 at 1000 users with spread 2.
    It is no law: on helpers.planted sets, whose plain lists already reach three quarters of
    the catalogue, the same reference covers FEWER items at 0.3 (223 -> 195 of 300 at 400
    users, seed 5)."""
    import pandas as pd

    from als_mi355x.ml.recommendation import ALS
    u, i, r = _blockbusters(2000, 300, 0.05, seed=6, spread=1.5)
    model = ALS(rank=8, maxIter=4, regParam=0.1, seed=1).fit(
        pd.DataFrame({"user": u, "item": i, "rating": r}))
    core = model.engine
    covered = {}
    for lam in (1.0, 0.3):
        recs = model.recommendForAllUsersDiverse(10, tradeOff=lam, pool=100)
        rows = model._padded_rows(recs)[2]
        counts, _ = E.list_exposure_rows(rows, int(rows.shape[1]), core.n_items)
        out = E.list_concentration(counts, core.n_items, None, len(recs), 10, core.ws).tolist()
        covered[lam] = int(out[1])
        assert out[1] / out[0] == model.evaluateListQuality(recs)["coverage"]
    print("covered items at trade-off 1 / 0.3:", covered[1.0], covered[0.3])
    assert covered[0.3] >= covered[1.0]
