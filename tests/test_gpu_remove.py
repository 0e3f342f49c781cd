"""GPU tests of the removal path (K18 als_csr_remove_mark / als_csr_remove_compact,
ALSCore.remove_ratings / remove_users / remove_items / set_ratings and the public surfaces over
them).

Shapes come from T = als_csr_remove_tile(): remove_ref.base, about 45 x 345 rows with user-row
lengths 1, T - 1, T, T + 1, 2T + 3, 63, 64, 65, ... and the removals of remove_ref.CASES (held to
the oracle's csr_build of the filtered triples by test_remove_cpu.py).  The bar for everything
made of ratings is bit equality with a fresh ALSCore on the filtered triples; surviving factor
rows are compared bitwise, refreshed rows within the bar
test_gpu_update.py::test_refresh_solves_the_touched_rows_and_nothing_else holds them to.
"""
import numpy as np
import pytest
import torch

import remove_ref as RR
from als_mi355x import engine as E
from helpers import fold_in_oracle, rel_row_errs, report
from test_gpu_update import _assert_same_ratings, _bits, _cat, _rows_of, _trips

pytestmark = pytest.mark.gpu
DEV = "cuda"
REG = 0.1
REFRESH_BAR = 1e-4   # test_gpu_update.py's bar for refreshed rows against the fp64 oracle


def _T():
    return E.csr_remove_tile()


def _apply(core, spec):
    """Run a case's spec on the core; the reports of the calls, in order."""
    out = []
    if "pairs" in spec:
        out.append(core.remove_ratings(*spec["pairs"]))
    if "users" in spec:
        out.append(core.remove_users(spec["users"]))
    if "items" in spec:
        out.append(core.remove_items(spec["items"]))
    return out


def _check_info(info, want):
    assert info["removed"] == want["removed"] and info["missing"] == want["missing"]
    for key in ("left_users", "left_items", "touched_users", "touched_items"):
        assert info[key].cpu().numpy().tolist() == want[key].tolist(), key
    assert info["left_users"].dtype == torch.int32 and info["touched_users"].dtype == torch.int64


# ---------------------------------------------------------------- blocks are K1's, bit for bit
@pytest.mark.parametrize("name", RR.CASES)
def test_remove_gives_the_blocks_of_a_fresh_core(name):
    """Every case before any fit."""
    old, spec = RR.case(name, _T())
    core = E.ALSCore(*old)
    before = (core.user_block, core.item_block, core.uidx, core.iidx)
    infos = _apply(core, spec)
    assert core.rank == 0 and core.U is None
    pairs = RR.listed(old, spec)
    _assert_same_ratings(core, E.ALSCore(*RR.filtered(old, pairs)))
    want = RR.expected_info(old, pairs)
    if len(infos) == 1:
        _check_info(infos[0], want)
    else:   # whole users, then whole items: the second call sees the core the first left
        assert sum(x["removed"] for x in infos) == want["removed"]
        assert infos[0]["left_users"].cpu().numpy().tolist() == sorted(spec["users"])
        assert infos[1]["left_items"].cpu().numpy().tolist() == sorted(spec["items"])
    if name in ("c_missing", "l_nothing_to_do"):    # nothing moves: the same objects
        now = (core.user_block, core.item_block, core.uidx, core.iidx)
        assert all(a is b for a, b in zip(before, now)) and core._touched is None


def test_unknown_whole_rows_are_counted():
    old, spec = RR.case("j_whole_rows", _T())
    core = E.ALSCore(*old)
    info = core.remove_users(spec["users"] + [10 ** 6, spec["users"][0]])
    assert info["missing"] == 1 and info["left_users"].cpu().numpy().tolist() == sorted(spec["users"])
    assert core.remove_items([10 ** 6])["removed"] == 0


def test_add_then_remove_is_a_round_trip():
    old, _ = RR.case("l_nothing_to_do", _T())
    uid, iid = np.unique(old[0]), np.unique(old[1])
    short = uid[np.bincount(np.searchsorted(uid, old[0])) == 2][0]
    unrated = np.setdiff1d(iid, old[1][old[0] == short])[0]
    bu = np.array([10 ** 4, 10 ** 4 + 1, 10 ** 4, short, -3])
    bi = np.array([2 * 10 ** 4, 2 * 10 ** 4, iid[0], unrated, iid[5]])
    br = np.array([1.0, 2.5, 3.0, 4.5, 5.0], np.float32)
    core = E.ALSCore(*old)
    core.add_ratings(bu, bi, br)
    assert core.n_users == len(uid) + 3 and core.uidx.offset == -3
    info = core.remove_ratings(bu, bi)
    assert info["removed"] == 5 and info["missing"] == 0
    assert info["left_users"].cpu().numpy().tolist() == [-3, 10 ** 4, 10 ** 4 + 1]
    _assert_same_ratings(core, E.ALSCore(*old))


def test_two_removes_in_sequence_equal_one():
    T = _T()
    old, s1 = RR.case("f_both_leave", T)
    _, s2 = RR.case("i_tile_edges", T)
    twice, once = E.ALSCore(*old), E.ALSCore(*old)
    twice.remove_ratings(*s1["pairs"])
    twice.remove_ratings(*(torch.as_tensor(x, device=DEV) for x in s2["pairs"]))   # device too
    once.remove_ratings(*_cat(s1["pairs"], s2["pairs"]))
    _assert_same_ratings(twice, once)
    _assert_same_ratings(once, E.ALSCore(*RR.filtered(old, _cat(s1["pairs"], s2["pairs"]))))
    # the rows touched by either call, in the final numbering, are kept for refresh
    want = RR.expected_info(old, _cat(s1["pairs"], s2["pairs"]))
    assert twice._touched[0].tolist() == want["touched_users"].tolist()
    assert twice._touched[1].tolist() == want["touched_items"].tolist()


# ---------------------------------------------------------------- factors and caches
def _mixed_pairs(T):
    """Rows that leave at both ends of both sides, a row that loses one rating and one that
    loses stored duplicates."""
    old, a = RR.case("a_one_pair", T)
    _, b = RR.case("b_stored_duplicates", T)
    _, g = RR.case("g_first_and_last_rows_leave", T)
    return old, _cat(_cat(a["pairs"], b["pairs"]), g["pairs"])


@pytest.fixture(scope="module", params=[8, 64])
def fitted_then_removed(request):
    rank = request.param
    old, pairs = _mixed_pairs(_T())
    core = E.ALSCore(*old)
    core.fit(rank, 2, REG, seed=4)
    core.recommend_all(3, exclude="train")       # fills the exclusion cache with the old pairs
    b = dict(U=core.U.clone(), V=core.V.clone(), uids=core.uidx.ids().clone(),
             iids=core.iidx.ids().clone())
    info = core.remove_ratings(*pairs)
    return rank, old, pairs, core, b, info


def test_surviving_factor_rows_keep_their_bits(fitted_then_removed):
    rank, old, pairs, core, b, info = fitted_then_removed
    fresh = E.ALSCore(*RR.filtered(old, pairs))
    _assert_same_ratings(core, fresh)
    _check_info(info, RR.expected_info(old, pairs))
    assert info["left_users"].numel() == 2 and info["left_items"].numel() == 2
    for F, F0, idx, ids0, left in ((core.U, b["U"], core.uidx, b["uids"], info["left_users"]),
                                   (core.V, b["V"], core.iidx, b["iids"], info["left_items"])):
        assert F.shape == (idx.n, E.ld_for(rank)) and F.is_contiguous()
        rows = idx.rows_of(ids0)
        assert ids0[rows < 0].tolist() == left.tolist()          # rows that left are gone
        assert torch.equal(_bits(F[rows[rows >= 0]]), _bits(F0[rows >= 0]))
        assert torch.equal(rows[rows >= 0], torch.arange(idx.n, device=DEV))
    # the exclusion cache is rebuilt from the ratings that stay
    for a, f in zip(core.train_exclusion(True), fresh.train_exclusion(True)):
        assert torch.equal(a, f)
    assert core.fingerprint() == fresh.fingerprint()


def test_refresh_solves_the_touched_rows_and_nothing_else(fitted_then_removed):
    rank, old, pairs, core, b, info = fitted_then_removed
    U0, V0 = core.U.clone(), core.V.clone()
    tu, ti = core._touched
    assert tu.tolist() == info["touched_users"].tolist() and 0 < tu.numel() < core.n_users
    assert ti.tolist() == info["touched_items"].tolist() and 0 < ti.numel() < core.n_items
    try:
        assert core.refresh() is core
        for F, F0, t, block, Y, side in ((core.U, U0, tu, core.user_block, V0, "users"),
                                         (core.V, V0, ti, core.item_block, core.U, "items")):
            keep = torch.ones(F.shape[0], dtype=torch.bool, device=DEV)
            keep[t] = False
            assert torch.equal(_bits(F[keep]), _bits(F0[keep])), f"untouched {side} moved"
            assert not torch.equal(F[t], F0[t])
            want = fold_in_oracle(_rows_of(block, t), Y[:, :rank].cpu().numpy(), REG, False, 1.0)[0]
            errs = rel_row_errs(F[t, :rank].cpu().numpy(), want)
            report(f"remove_refresh_{side}_k{rank}", float(errs.max()))
            assert errs.max() < REFRESH_BAR, errs
    finally:    # the fixture is shared: the other tests see the factors the removal left
        core.U, core.V = U0, V0


def test_refit_is_a_fit_of_the_filtered_ratings_from_the_surviving_factors(fitted_then_removed):
    rank, old, pairs, core, b, info = fitted_then_removed
    U0, V0, touched = core.U.clone(), core.V.clone(), core._touched
    try:
        assert core.refit(2) is core and core.iterations_run == 2 and core._touched is None
        fresh = E.ALSCore(*RR.filtered(old, pairs))
        fresh.fit(rank, 2, REG, U0=U0[:, :rank])
        assert torch.equal(_bits(core.U), _bits(fresh.U))
        assert torch.equal(_bits(core.V), _bits(fresh.V))
    finally:
        core.U, core.V, core._touched = U0, V0, touched


# ---------------------------------------------------------------- set_ratings
def _dedup_last(batch):
    keys = list(zip(batch[0].tolist(), batch[1].tolist()))
    keep = np.array([k not in keys[j + 1:] for j, k in enumerate(keys)])
    return tuple(x[keep] for x in batch)


@pytest.mark.parametrize("what", ["stored", "new", "twice", "only_rating"])
def test_set_ratings_replaces(what):
    old, _ = RR.case("l_nothing_to_do", _T())
    u, i, _ = old
    uid, cnt = np.unique(u, return_counts=True)
    one = uid[cnt == 1][1]                                   # a user with a single rating
    dup = RR.case("b_stored_duplicates", _T())[1]["pairs"]   # a pair stored several times
    bu, bi, br = {
        "stored": ([dup[0][0], u[7]], [dup[1][0], i[7]], [0.5, 1.5]),
        "new": ([u[3], 10 ** 5], [10 ** 5, i[3]], [2.0, 3.0]),
        "twice": ([u[9], u[2], u[9]], [i[9], i[2], i[9]], [1.0, 2.0, 4.5]),
        "only_rating": ([one], [i[u == one][0]], [0.5]),
    }[what]
    batch = (np.asarray(bu, np.int64), np.asarray(bi, np.int64), np.asarray(br, np.float32))
    core = E.ALSCore(*old)
    core.fit(8, 1, REG, seed=3)
    U0, ids0 = core.U.clone(), core.uidx.ids().clone()
    info = core.set_ratings(*batch, seed=1)
    last = _dedup_last(batch)
    rest = RR.filtered(old, batch[:2])
    _assert_same_ratings(core, E.ALSCore(*_cat(rest, last)))
    assert info["added"] == len(last[0]) and info["replaced"] == len(old[0]) - len(rest[0])
    if what in ("new", "only_rating"):
        assert info["replaced"] == (what == "only_rating")
    if what == "stored":
        assert info["replaced"] >= 3                         # the duplicates all went
    # no row left on the way: every old user keeps the row and its bits until a refresh
    assert torch.equal(_bits(core.U[core.uidx.rows_of(ids0)]), _bits(U0))
    want = np.unique(core.uidx.rows_of(torch.as_tensor(last[0], device=DEV)).cpu().numpy())
    assert info["touched_users"].cpu().numpy().tolist() == want.tolist()
    if what == "twice":
        row = int(core.uidx.rows_of(torch.tensor([int(u[9])], device=DEV)))
        b = core.user_block
        vals = b.val[b.row_ptr[row]:b.row_ptr[row + 1]][
            b.col[b.row_ptr[row]:b.row_ptr[row + 1]] == int(core.iidx.rows_of(
                torch.tensor([int(i[9])], device=DEV)))]
        assert vals.tolist() == [4.5]                        # the last one won, alone


# ---------------------------------------------------------------- errors
def test_errors_leave_the_core_untouched():
    old, _ = RR.case("l_nothing_to_do", _T())
    core = E.ALSCore(*old)
    before = (core.user_block, core.item_block, core.uidx, core.iidx)
    with pytest.raises(ValueError, match="every rating"):
        core.remove_ratings(old[0], old[1])
    with pytest.raises(ValueError, match="every rating"):
        core.remove_users(np.unique(old[0]))
    with pytest.raises(ValueError, match="same length"):
        core.remove_ratings([1, 2], [1])
    with pytest.raises(ValueError, match="same length"):
        core.set_ratings([1, 2], [1, 2], [1.0])
    now = (core.user_block, core.item_block, core.uidx, core.iidx)
    assert all(a is b for a, b in zip(before, now)) and core.nnz == len(old[0])
    core.fit(4, 1, REG)
    loaded = E.ALSCore.from_factors(core.uidx.ids(), core.U[:, :4], core.iidx.ids(), core.V[:, :4])
    for call in (lambda: loaded.remove_ratings([1], [2]), lambda: loaded.remove_users([1]),
                 lambda: loaded.remove_items([1]), lambda: loaded.set_ratings([1], [2], [3.0])):
        with pytest.raises(ValueError, match="from_factors"):
            call()


# ---------------------------------------------------------------- public surfaces
def _after(eng, old, pairs, U0, ids0, mode, touched_ids):
    _assert_same_ratings(eng, E.ALSCore(*RR.filtered(old, pairs)))
    rows = eng.uidx.rows_of(ids0)
    moved, was = eng.U[rows[rows >= 0]], U0[rows >= 0]
    touched = torch.isin(ids0[rows >= 0], torch.as_tensor(touched_ids, device=DEV).int())
    if mode == "none":
        assert torch.equal(moved, was)
    elif mode == "refresh":
        assert torch.equal(moved[~touched], was[~touched])
        assert not torch.equal(moved[touched], was[touched])
    else:
        assert eng.iterations_run == 2 and not torch.equal(moved[~touched], was[~touched])


@pytest.mark.parametrize("mode", ["refit", "refresh", "none"])
def test_mllib_model_remove(mode):
    from als_mi355x.mllib.recommendation import ALS
    old, pairs = _mixed_pairs(_T())
    model = ALS.train(_trips(old), 8, iterations=2, lambda_=REG, seed=5)
    eng = model.engine
    U0, ids0 = eng.U.clone(), eng.uidx.ids().clone()
    want = RR.expected_info(old, pairs)
    touched_ids = np.unique(RR.filtered(old, pairs)[0])[want["touched_users"]]
    assert model.remove(list(zip(pairs[0].tolist(), pairs[1].tolist())), 2, mode=mode) is model
    assert model.engine is eng
    _after(eng, old, pairs, U0, ids0, mode, touched_ids)
    # whole users and whole products, on the model the removal left
    now = RR.filtered(old, pairs)
    gone_u, gone_p = [int(now[0][0])], [int(now[1][1])]
    assert model.removeUsers(gone_u, mode="none").removeProducts(gone_p, mode="none") is model
    rest = RR.filtered(now, RR.listed(now, dict(users=gone_u, items=gone_p)))
    _assert_same_ratings(eng, E.ALSCore(*rest))
    # replace=True: the stored ratings of the pair go, the new one stands alone
    p = (int(rest[0][0]), int(rest[1][0]))
    model.update([(p[0], p[1], 0.5)], 2, mode=mode, replace=True)
    kept = RR.filtered(rest, ([p[0]], [p[1]]))
    _assert_same_ratings(eng, E.ALSCore(*_cat(kept, (np.array([p[0]]), np.array([p[1]]),
                                                     np.array([0.5], np.float32)))))


@pytest.mark.parametrize("mode", ["refit", "refresh", "none"])
def test_ml_model_remove(mode):
    from als_mi355x.ml.recommendation import ALS
    old, pairs = _mixed_pairs(_T())
    frame = lambda t: {"u": t[0], "m": t[1], "r": t[2]} if len(t) == 3 else {"u": t[0], "m": t[1]}
    est = ALS(rank=8, maxIter=2, regParam=REG, userCol="u", itemCol="m", ratingCol="r", seed=5)
    model = est.fit(frame(old))
    eng = model.engine
    U0, ids0 = eng.U.clone(), eng.uidx.ids().clone()
    want = RR.expected_info(old, pairs)
    touched_ids = np.unique(RR.filtered(old, pairs)[0])[want["touched_users"]]
    assert model.remove(frame(pairs), maxIter=2, mode=mode) is model
    _after(eng, old, pairs, U0, ids0, mode, touched_ids)
    assert len(model.userFactors) == eng.n_users == len(ids0) - 2
    now = RR.filtered(old, pairs)
    gone_u, gone_i = [int(now[0][0])], [int(now[1][1])]
    assert model.removeUsers(gone_u, mode="none").removeItems(gone_i, mode="none") is model
    rest = RR.filtered(now, RR.listed(now, dict(users=gone_u, items=gone_i)))
    _assert_same_ratings(eng, E.ALSCore(*rest))
    p = (rest[0][:1], rest[1][:1], np.array([0.5], np.float32))
    assert model.update(frame(p), maxIter=2, mode=mode, replace=True) is model
    _assert_same_ratings(eng, E.ALSCore(*_cat(RR.filtered(rest, p[:2]), p)))


def test_personal_recommendations_update_replaces():
    from als_mi355x import personal
    from als_mi355x.mllib.recommendation import ALS
    old, _ = RR.case("l_nothing_to_do", _T())
    model = ALS.train(_trips(old), 8, iterations=2, lambda_=REG, seed=5)
    user = int(old[0][0])
    mine = np.unique(old[1][old[0] == user])[:2]
    rated = [(user, int(m), 0.5) for m in mine]
    movies = [(int(m), f"m{int(m)}") for m in np.unique(old[1])]
    got = personal.personal_recommendations_update(model, user, rated, movies, num=5,
                                                   min_ratings=0, iterations=1, replace=True)
    assert len(got) == 5
    batch = (np.array([user, user]), mine, np.array([0.5, 0.5], np.float32))
    _assert_same_ratings(model.engine, E.ALSCore(*_cat(RR.filtered(old, batch[:2]), batch)))
