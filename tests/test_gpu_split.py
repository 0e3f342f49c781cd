"""GPU tests of K20 (als_split_anchor / als_split_eligible / als_split_thresholds /
als_split_mark, ALSCore.holdout / split, datasets.user_holdout_split and the stratified tuners).

Everything is integers, or f32 ratings that are only copied: the bar is bit equality with the
numpy restatement (split_ref.py, held to its own properties by test_split_cpu.py) and with a
fresh ALSCore on the reference's kept triples.  Kernel shapes force row_cap = 64 so that the
radix path runs on rows of a few hundred entries, and run again at the default cap: the outputs
must not depend on it.
"""
import numpy as np
import pytest
import torch

import split_ref as SR
from als_mi355x import engine as E
from test_gpu_update import _assert_same_ratings

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = 64
SEED = 20


def _T():
    return E.csr_remove_tile()


# ---------------------------------------------------------------- shapes
def _edges(T):
    """Users 10, 11, ... with 1, 2, 63, 64, 65, 5 * 64 + 3 and 2 T + 3 ratings (the last one
    crosses K18 tiles and is longer than the anchor kernel's task and the default row_cap), a
    user whose row is five copies of one pair, a user who alone rated his items (every entry
    an anchor: no eligible entry) and, by more_users, two users without any rating."""
    rng = np.random.default_rng(3)
    n_items = 2 * T + 50
    u, i = [], []
    for k, ln in enumerate((1, 2, CAP - 1, CAP, CAP + 1, 5 * CAP + 3, 2 * T + 3)):
        u += [10 + k] * ln
        i += rng.choice(n_items, ln, replace=False).tolist()
    u += [40] * 5
    i += [7] * 5
    u += [41] * 4
    i += [n_items + 1, n_items + 2, n_items + 3, n_items + 2]
    u, i = np.array(u), np.array(i) - 25            # negative item ids too
    p = rng.permutation(len(u))
    return dict(users=u[p], items=i[p], more_users=(5, 99))


def _random(nnz, n_u, n_i, seed):
    rng = np.random.default_rng(seed)
    return dict(users=rng.integers(0, n_u, nnz), items=rng.integers(0, n_i, nnz))


def _shape(name):
    T = _T()
    if name == "edges":
        return _edges(T)
    if name.startswith("nnz"):
        return _random(T + int(name[3:]), 40, 90, 5)
    if name == "one_user":
        return dict(users=np.full(150, 3), items=np.random.default_rng(1).integers(0, 120, 150))
    if name == "one_item":
        return dict(users=np.random.default_rng(2).integers(0, 120, 150), items=np.full(150, -4))
    raise KeyError(name)


SHAPES = ("edges", "nnz-1", "nnz+0", "nnz+1", "one_user", "one_item")
WINDOWS = {
    "count1": dict(mode="count", value=1),
    "count3_keep2": dict(mode="count", value=3, min_keep=2),
    "fraction": dict(mode="fraction", value=0.2),
    "fold1of3": dict(mode="fold", value=(1, 3)),
    "empty": dict(win=lambda e: (0 * e, 0 * e)),
    "all": dict(win=lambda e: (0 * e, e)),
    "last": dict(win=lambda e: (np.maximum(e - 1, 0), e)),
    "fold_e_plus_1": dict(win=lambda e: ((e // 2) * e // (e + 1), (e // 2 + 1) * e // (e + 1))),
}
_CACHE = {}


def _ref(shape, user_side, keep):
    k = (shape, user_side, keep)
    if k not in _CACHE:
        _CACHE[k] = SR.Split(seed=SEED, keep_items=keep, user_side=user_side, **_shape(shape))
    return _CACHE[k]


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV)


def _kernels(sp, row_cap, seed=SEED):
    """The four entry points on the reference's two CSR sides: numpy outputs by name."""
    ws = E.Workspace(torch.device(DEV))
    sides = {}
    for user_rows in (True, False):
        row_ptr, col, _, n_rows, n_cols, row_ids, col_ids = sp.side(user_rows)
        sides[user_rows] = (_dev(row_ptr), _dev(col), n_cols, _dev(row_ids), _dev(col_ids),
                            user_rows)
    sel, oth = sides[sp.user_side], sides[not sp.user_side]
    out = {}
    anchor = None
    if sp.anchor is not None:
        anchor = E.split_anchor(*oth, seed, ws)
        out["anchor"] = anchor
    out["eligible"] = E.split_eligible(sel[0], sel[1], sel[2], anchor)
    thr = E.split_thresholds(*sel, seed, anchor, _dev(sp.lo), _dev(sp.hi), ws, row_cap)
    out.update(zip(("lo_key", "lo_col", "hi_key", "hi_col"), thr))
    for user_rows in (True, False):
        m = E.split_mark(*sides[user_rows], seed, user_rows == sp.user_side, thr, anchor, ws)
        out.update(zip((f"keep_bits{user_rows:d}", f"tile_off{user_rows:d}",
                        f"row_ptr_kept{user_rows:d}"), m))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _expected(sp):
    want = {"eligible": sp.eligible_counts()}
    if sp.anchor is not None:
        want["anchor"] = sp.anchor
    thr = sp.thresholds()
    want.update(lo_key=thr[0].view(np.int64), lo_col=thr[1], hi_key=thr[2].view(np.int64),
                hi_col=thr[3])
    for user_rows in (True, False):
        m = sp.marks(user_rows, _T())
        want.update({f"keep_bits{user_rows:d}": m[0].view(np.int64),
                     f"tile_off{user_rows:d}": m[1], f"row_ptr_kept{user_rows:d}": m[2]})
    return want


@pytest.mark.parametrize("user_side", [True, False])
@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_equal_the_reference(shape, keep, user_side):
    sp = _ref(shape, user_side, keep)
    for name, w in WINDOWS.items():
        sp.set_windows(w.get("mode"), w.get("value"), w.get("min_keep", 1), w.get("win"))
        want = _expected(sp)
        small, default = _kernels(sp, CAP), _kernels(sp, 0)
        assert sorted(small) == sorted(want)
        for k in want:
            assert small[k].dtype == want[k].dtype, (name, k)
            assert small[k].tobytes() == want[k].tobytes(), (name, k)
            assert default[k].tobytes() == small[k].tobytes(), (name, k, "row_cap changes it")
        assert small["tile_off1"][-1] == small["tile_off0"][-1] == int((~sp.held).sum())


@pytest.mark.parametrize("seed", [2 ** 63, 2 ** 63 + 12345, 2 ** 64 - 1, -3])
def test_kernels_take_every_64_bit_seed(seed):
    """The seed crosses the ABI as an int64 with the same bits: 2^63 and above arrive negative,
    and at 2^64 - 1 (and -1) seed + 1 wraps to 0."""
    sp = SR.Split(seed=seed, mode="count", value=2, **_shape("nnz+1"))
    assert (sp.keys != SR.key(SEED, sp.users, sp.items)).any()
    want, got = _expected(sp), _kernels(sp, CAP, seed)
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), k
    core = E.ALSCore(sp.users, sp.items, np.ones(len(sp.users), np.float32))
    held = core.holdout(count=2, seed=seed)
    assert sorted(zip(held[0].tolist(), held[1].tolist())) == sorted(
        zip(sp.users[sp.held].tolist(), sp.items[sp.held].tolist()))


def test_the_edge_shape_has_its_edges():
    T = _T()
    sp = _ref("edges", True, True)
    ln = np.bincount(sp.urow, minlength=len(sp.uids)).tolist()
    for want in (0, 1, 2, CAP - 1, CAP, CAP + 1, 5 * CAP + 3, 2 * T + 3):
        assert want in ln
    assert 2 * T + 3 > E.split_row_cap() > 5 * CAP + 3
    assert sp.e[list(sp.uids).index(41)] == 0 and ln[list(sp.uids).index(41)] == 4
    assert sp.e[list(sp.uids).index(40)] in (0, 5)     # copies share a fate


# ---------------------------------------------------------------- end to end
def _ratings():
    """300 users x 200 items, about 6,000 ratings, Zipf-skewed items, stored duplicates."""
    rng = np.random.default_rng(11)
    n = 5900
    u = rng.integers(0, 300, n)
    i = np.minimum(rng.zipf(1.3, n) - 1, 199)
    u, i = np.concatenate([u, u[:100]]), np.concatenate([i, i[:100]])     # copies
    u, i = np.concatenate([u, np.arange(300)]), np.concatenate([i, rng.integers(0, 200, 300)])
    r = np.clip(np.round(3.5 + rng.normal(0, 1, len(u))), 1, 5).astype(np.float32)
    return u.astype(np.int32) + 1000, i.astype(np.int32) - 50, r


E2E = {"count1": dict(count=1), "count3": dict(count=3), "fraction": dict(fraction=0.2),
       "fold1of3": dict(fold=(1, 3))}


def _ref_e2e(trip, kw, **more):
    (mode, value), = kw.items()
    return SR.Split(trip[0], trip[1], SEED, mode=mode, value=value, **more)


def _same_triples(got, want):
    for g, w in zip(got, want):
        g = g.cpu().numpy()
        assert g.dtype == np.asarray(w).dtype and g.tobytes() == np.asarray(w).tobytes()


def _csr_bits(core):
    out = []
    for b in (core.user_block, core.item_block):
        out += [b.row_ptr.clone(), b.col.clone(), b.val.clone()]
    return out + [core.uidx.map.clone(), core.iidx.map.clone()]


@pytest.mark.parametrize("name", E2E)
def test_holdout_leaves_the_core_of_the_kept_triples(name):
    trip = _ratings()
    sp = _ref_e2e(trip, E2E[name])
    assert 0 < sp.held.sum() < len(sp.held)
    core = E.ALSCore(*trip)
    held = core.holdout(seed=SEED, **E2E[name])
    _same_triples(held, sp.held_out(trip))
    _assert_same_ratings(core, E.ALSCore(*sp.kept(trip)))
    assert core.n_items == len(sp.iids)                       # keep_items: no item left
    core.add_ratings(*held)                                   # and back
    full = E.ALSCore(*trip)
    assert core.fingerprint() == full.fingerprint()
    for side in ("user_block", "item_block"):
        a, b = getattr(core, side), getattr(full, side)
        assert torch.equal(a.row_ptr, b.row_ptr)
        key = lambda blk: sorted(zip(np.repeat(np.arange(blk.n_rows), np.diff(
            blk.row_ptr.cpu().numpy())).tolist(), blk.col.cpu().numpy().tolist(),
            blk.val.cpu().numpy().tolist()))
        assert key(a) == key(b)


@pytest.mark.parametrize("name", E2E)
def test_split_leaves_the_source_alone(name):
    trip = _ratings()
    sp = _ref_e2e(trip, E2E[name])
    core = E.ALSCore(*trip)
    fp, bits = core.fingerprint(), _csr_bits(core)
    train, held = core.split(seed=SEED, **E2E[name])
    assert core.fingerprint() == fp
    assert all(torch.equal(a, b) for a, b in zip(bits, _csr_bits(core)))
    _same_triples(held, sp.held_out(trip))
    _assert_same_ratings(train, E.ALSCore(*sp.kept(trip)))
    assert train.U is None and train.rank == 0 and train.ws is not core.ws


def test_item_side_and_unprotected_holdouts():
    trip = _ratings()
    for more in (dict(user_side=False), dict(keep_items=False), dict(min_keep=0)):
        sp = _ref_e2e(trip, dict(count=2), **more)
        train, held = E.ALSCore(*trip).split(count=2, seed=SEED, **more)
        _same_triples(held, sp.held_out(trip))
        _assert_same_ratings(train, E.ALSCore(*sp.kept(trip)))


def test_holdout_on_a_fitted_core_keeps_the_factor_rows():
    trip = _ratings()
    one = np.array([5, 2000, 2001], np.int32)                 # three users with one rating
    trip = (np.concatenate([trip[0], one]), np.concatenate([trip[1], one * 0 + 3]),
            np.concatenate([trip[2], np.float32([1, 2, 3])]))
    sp = _ref_e2e(trip, dict(count=1), keep_items=False, min_keep=0)
    core = E.ALSCore(*trip)
    core.fit(8, 2, 0.1, seed=3)
    U0, ids0 = core.U.clone(), core.uidx.ids().clone()
    core.holdout(count=1, seed=SEED, keep_items=False, min_keep=0)
    assert core.n_users == len(ids0) - 3                      # one-rating users left
    rows = core.uidx.rows_of(ids0)
    assert torch.equal(core.U.view(torch.int32), U0[rows >= 0].view(torch.int32))
    _assert_same_ratings(core, E.ALSCore(*sp.kept(trip)))
    fresh = E.ALSCore(*sp.kept(trip))
    core.refit(2)
    fresh.fit(8, 2, 0.1, U0=U0[rows >= 0][:, :8])
    assert torch.equal(core.U.view(torch.int32), fresh.U.view(torch.int32))


def test_nothing_and_everything():
    trip = _ratings()
    core = E.ALSCore(*trip)
    before = (core.user_block, core.item_block, core.uidx, core.iidx)
    held = core.holdout(count=0)
    assert all(x.numel() == 0 for x in held) and held[2].dtype == torch.float32
    assert before == (core.user_block, core.item_block, core.uidx, core.iidx)
    with pytest.raises(ValueError, match="every rating"):
        core.holdout(fraction=1.0, min_keep=0, keep_items=False)
    with pytest.raises(ValueError, match="exactly one"):
        core.holdout(count=1, fraction=0.5)
    with pytest.raises(ValueError, match="exactly one"):
        core.split()
    assert before == (core.user_block, core.item_block, core.uidx, core.iidx)


def test_datasets_user_holdout_split():
    from als_mi355x import datasets as D
    trip = _ratings()
    sp = _ref_e2e(trip, dict(count=1))
    train, test = D.user_holdout_split(*trip, count=1, seed=SEED)
    _same_triples(test, sp.held_out(trip))
    # the training part comes back in the user side's stored order
    order = np.argsort(sp.urow[~sp.held], kind="stable")
    _same_triples(train, tuple(x[order] for x in sp.kept(trip)))


# ---------------------------------------------------------------- tuners and fitHoldout
def _frame(trip):
    return {"user": trip[0], "item": trip[1], "rating": trip[2]}


def _stand_alone(est, maps, evaluator, sp, trip):
    """Each map fitted stand-alone on the reference's kept triples, scored on its held-out."""
    from als_mi355x.ml.tuning import _score
    train, test = _frame(sp.kept(trip)), _frame(sp.held_out(trip))
    return [_score(evaluator, est.fit(train, m), test) for m in maps]


def test_stratified_tuners_equal_stand_alone_fits():
    from als_mi355x.ml.evaluation import RegressionEvaluator
    from als_mi355x.ml.recommendation import ALS
    from als_mi355x.ml.tuning import CrossValidator, ParamGridBuilder, TrainValidationSplit
    trip = _ratings()
    est = ALS(maxIter=2, regParam=0.1, seed=3, coldStartStrategy="drop")
    maps = ParamGridBuilder().addGrid("rank", [4, 8]).build()
    ev = RegressionEvaluator(metricName="rmse", labelCol="rating", predictionCol="prediction")
    tv = TrainValidationSplit(est, maps, ev, seed=SEED, stratify="user", holdOut=1).fit(
        _frame(trip))
    sp = SR.Split(trip[0], trip[1], SEED, mode="count", value=1)
    want = _stand_alone(est, maps, ev, sp, trip)
    assert tv.validationMetrics == want
    # no validation pair is cold: every held-out user and item is in the training part
    kept, held = sp.kept(trip), sp.held_out(trip)
    assert set(held[0].tolist()) <= set(kept[0].tolist())
    assert set(held[1].tolist()) <= set(kept[1].tolist())
    cv = CrossValidator(est, maps, ev, numFolds=3, seed=SEED, stratify="user").fit(_frame(trip))
    per_fold = []
    for f in range(3):
        sp.set_windows("fold", (f, 3))
        per_fold.append(_stand_alone(est, maps, ev, sp, trip))
    assert cv.avgMetrics == np.asarray(per_fold, np.float64).mean(axis=0).tolist()


def test_fit_holdout_is_the_hand_made_sequence():
    from als_mi355x.ml.recommendation import ALS
    trip = _ratings()
    est = ALS(rank=8, maxIter=2, regParam=0.1, seed=3)
    model, got = est.fitHoldout(_frame(trip), count=1, k=10, seed=SEED)
    sp = SR.Split(trip[0], trip[1], SEED, mode="count", value=1)
    hand = est.fit(_frame(sp.kept(trip)))
    test = _frame(sp.held_out(trip))
    want = dict(hand.evaluateRanking(test, 10, exclude="train"))
    full = hand.evaluateFullRanking(test, exclude="train")
    want.update({("fullRows" if k == "rows" else k): v for k, v in full.items()})
    assert got == want and "ndcg" in got and "mrr" in got
    _assert_same_ratings(model.engine if hasattr(model, "engine") else model._core,
                         E.ALSCore(*sp.kept(trip)))


class _MeanModel:
    def __init__(self, mean):
        self.mean = mean

    def transform(self, dataset):
        return dict(dataset, prediction=np.full(len(dataset["rating"]), self.mean))


class _MeanEstimator:
    """An estimator that is no ALS: predicts the training mean, records what it was given."""

    def __init__(self):
        self.seen = []

    def fit(self, dataset, params=None):
        self.seen.append(dataset)
        return _MeanModel(float(np.mean(dataset["rating"], dtype=np.float64)))


def test_other_estimators_get_host_datasets_of_the_same_split():
    from als_mi355x.ml.evaluation import RegressionEvaluator
    from als_mi355x.ml.tuning import CrossValidator, TrainValidationSplit
    trip = _ratings()
    ev = RegressionEvaluator(metricName="rmse", labelCol="rating", predictionCol="prediction")
    est = _MeanEstimator()
    tv = TrainValidationSplit(est, [{}], ev, seed=SEED, stratify="user", holdOut=1).fit(
        _frame(trip))
    sp = SR.Split(trip[0], trip[1], SEED, mode="count", value=1)
    order = np.argsort(sp.urow[~sp.held], kind="stable")       # the user side's stored order
    kept = tuple(x[order] for x in sp.kept(trip))
    for name, w in zip(("user", "item", "rating"), kept):
        assert est.seen[0][name].dtype == w.dtype and est.seen[0][name].tobytes() == w.tobytes()
    test = _frame(sp.held_out(trip))
    want = float(ev.evaluate(_MeanModel(float(np.mean(kept[2], dtype=np.float64))).transform(test)))
    assert tv.validationMetrics == [want]
    assert len(est.seen) == 2 and len(est.seen[1]["rating"]) == len(trip[2])    # the refit
    est = _MeanEstimator()
    CrossValidator(est, [{}], ev, numFolds=3, seed=SEED, stratify="user").fit(_frame(trip))
    assert len(est.seen) == 4
    sizes = [len(d["rating"]) for d in est.seen[:3]]
    assert sum(len(trip[2]) - n for n in sizes) == int(sp.eligible.sum())   # folds partition


def test_mllib_train_holdout():
    from als_mi355x.mllib.recommendation import ALS, Rating
    trip = _ratings()
    rows = list(zip(trip[0].tolist(), trip[1].tolist(), trip[2].tolist()))
    model, held = ALS.trainHoldout(rows, 8, iterations=2, lambda_=0.1, seed=5, holdOut=1,
                                   splitSeed=SEED)
    sp = SR.Split(trip[0], trip[1], SEED, mode="count", value=1)
    want = sp.held_out(trip)
    assert all(isinstance(x, Rating) for x in held)
    assert held == [Rating(*t) for t in zip(*(x.tolist() for x in want))]
    kept = sp.kept(trip)
    _assert_same_ratings(model.engine, E.ALSCore(*kept))
    hand = ALS.train(list(zip(*(x.tolist() for x in kept))), 8, iterations=2, lambda_=0.1, seed=5)
    assert torch.equal(model.engine.U.view(torch.int32), hand.engine.U.view(torch.int32))
    assert torch.equal(model.engine.V.view(torch.int32), hand.engine.V.view(torch.int32))
    with pytest.raises(ValueError, match="holdOut"):
        ALS.trainHoldout(rows, 8, holdOut=0)
