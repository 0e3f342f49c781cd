"""K19 on the GPU: als_co_rated against the numpy restatement (co_rated_ref.py).

Shapes are the smallest that reach each path: the cache window W and the task length T come
from the library.  idx and common must equal the reference exactly and the scores bit for
bit; only the cosine, whose fp64 square root and quotient the device may round otherwise
than numpy, is allowed 1 fp32 ulp, and positions whose reference scores are within 1 ulp of
a neighbour's (without being equal) are compared as sets.
"""
import functools

import numpy as np
import pytest
import torch

import co_rated_ref as R
from als_mi355x import engine as E
from als_mi355x import filters as F

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(side):
    return tuple(torch.as_tensor(x, device=DEV) for x in side)


class Case:
    """One rating set: both CSR sides on the device, both multiplicity matrices on the host."""

    def __init__(self, users, items, n_u, n_i):
        self.n = {False: n_i, True: n_u}
        self.csr = {False: _dev(R.csr(items, users, n_i)), True: _dev(R.csr(users, items, n_u))}
        B = R.multiplicity(users, items, n_u, n_i)
        self.B = {False: B, True: B.T}
        self.ws = E.Workspace(torch.device(DEV))

    def run(self, q, top, measure="jaccard", min_common=1, allow=None, user_side=False, **kw):
        bits = None
        if allow is not None:
            rows = torch.as_tensor(np.nonzero(allow)[0], device=DEV)
            bits = F.pack_allow_bits(rows, self.n[user_side])
        out = E.co_rated_rows(self.csr[user_side], self.csr[not user_side],
                              torch.as_tensor(np.asarray(q, np.int32), device=DEV), top, measure,
                              min_common, bits, self.ws, **kw)
        torch.cuda.synchronize()
        return tuple(x.cpu().numpy() for x in out)

    def ref(self, q, top, measure="jaccard", min_common=1, allow=None, user_side=False):
        return R.co_rated(self.B[user_side], q, top, measure, min_common, allow)

    def check(self, q, top, measure="jaccard", min_common=1, allow=None, user_side=False, **kw):
        got = self.run(q, top, measure, min_common, allow, user_side, **kw)
        want = self.ref(q, top, measure, min_common, allow, user_side)
        if measure == "cosine":
            ext = self.ref(q, top + 1, measure, min_common, allow, user_side)
            _assert_cosine(got, want, ext)
        else:
            _assert_same(got, want)
        return got


def _assert_same(got, want):
    for g, w, name in zip(got, want, ("idx", "score", "common")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert g.tobytes() == w.tobytes(), f"{name} differs at {np.argwhere(g != w)[:5].tolist()}"


def _assert_cosine(got, want, ext):
    """idx / common exact and score within 1 ulp, except at the reference's near-tie
    positions (co_rated_ref.near_tie_positions over the list with one slot more), where the
    listed rows are compared as sets drawn from the tied rows."""
    (gi, gs, gc), (wi, ws, wc), (ei, es, ec) = got, want, ext
    top = wi.shape[1]
    near = R.near_tie_positions(es)
    firm = ~near[:, :top]
    assert (gi[firm] == wi[firm]).all() and (gc[firm] == wc[firm]).all()
    fin = np.isfinite(ws)
    assert (np.isfinite(gs) == fin).all()
    assert (R.ulp_apart(gs[fin], ws[fin]) <= 1).all()
    for r in np.nonzero(near[:, :top].any(1))[0]:
        pool = {int(i): int(c) for i, c in zip(ei[r][near[r]], ec[r][near[r]])}
        listed = gi[r, :top][near[r, :top]]
        assert len(set(listed.tolist())) == len(listed) and set(listed.tolist()) <= set(pool)
        assert all(pool[int(i)] == int(c) for i, c in zip(listed, gc[r, :top][near[r, :top]]))


# ---------------------------------------------------------------- parity
PARITY_SEED = 11


def _parity_pairs():
    rng = np.random.default_rng(PARITY_SEED)
    u = rng.integers(0, 300, 6000)
    i = np.minimum((rng.random(6000) ** 2 * 200).astype(np.int64), 199)   # a skewed catalogue
    return u, i


@functools.lru_cache(None)
def _parity():
    u, i = _parity_pairs()
    return Case(u, i, 300, 200)


@pytest.mark.parametrize("min_common", [1, 3])
@pytest.mark.parametrize("top", [1, 10, 256])
@pytest.mark.parametrize("measure", R.MEASURES)
@pytest.mark.parametrize("user_side", [False, True])
def test_parity_with_the_reference(user_side, measure, top, min_common):
    c = _parity()
    c.check(np.arange(c.n[user_side]), top, measure, min_common, user_side=user_side)


def test_cosine_near_ties_are_rare_for_the_parity_seed():
    """The set comparison of _assert_cosine may cover under 1 % of the listed entries
    (reference alone; this is how the seed was picked)."""
    u, i = _parity_pairs()
    B = R.multiplicity(u, i, 300, 200)
    for side in (B, B.T):
        for top in (1, 10, 256):
            for mc in (1, 3):
                ei, es, _ = R.co_rated(side, np.arange(side.shape[1]), top + 1, "cosine", mc)
                near = R.near_tie_positions(es)[:, :top]
                listed = (ei[:, :top] >= 0).sum()
                assert near.sum() < 0.01 * listed, (top, mc, int(near.sum()), int(listed))


# ---------------------------------------------------------------- cache collisions
def test_rows_that_share_a_cache_slot_keep_exact_counts():
    """Items j and j + W map to one LDS slot; both are heavy (every rater of the query rated
    both), so whichever loses the slot takes all its adds through memory."""
    W = E.co_rated_window()
    n_i, n_u, q = W + 37, 48, 50
    rng = np.random.default_rng(3)
    us, it = [], []
    for u in range(n_u):
        mine = [q, 3, 3 + W, 20, 20 + W, 36, 36 + W] + rng.integers(0, n_i, 30).tolist()
        us += [u] * len(mine)
        it += mine
    c = Case(np.array(us), np.array(it), n_u, n_i)
    for measure in ("count", "jaccard"):
        got = c.check([q, 3 + W, 36], 64, measure)
    _, _, com = c.run([q], 8, "count")
    assert (com[0, :6] >= n_u).all()           # the six heavy rows, each met by every user


# ---------------------------------------------------------------- task split
def test_task_split_is_bit_identical():
    T = E.co_rated_task()
    n_u, n_i = 3 * T, 60
    rng = np.random.default_rng(5)
    us = list(range(T + 1)) + list(range(3 * T))        # item 0: T + 1 raters, item 1: 3 T
    it = [0] * (T + 1) + [1] * (3 * T)
    for u in range(n_u):
        mine = rng.integers(2, n_i, 4).tolist()
        us += [u] * 4
        it += mine
    c = Case(np.array(us), np.array(it), n_u, n_i)
    q = [0, 1, 7]
    outs = [c.check(q, 20, "jaccard", task_entries=t) for t in (1, 7, None)]
    for o in outs[1:]:
        _assert_same(o, outs[0])
    c.check(q, 20, "count", task_entries=T - 1)


# ---------------------------------------------------------------- passes
def test_passes_and_a_reused_workspace():
    c = _parity()
    P = E.CO_RATED_PASS
    n = c.n[False]
    q = np.concatenate([np.arange(P - 1), [3, 3]])          # P + 1 queries, one given three times
    assert len(q) == P + 1
    one = c.run(q, 10, "jaccard", pass_queries=E.CO_RATED_MAX_PASS)     # a single pass
    _assert_same(one, c.ref(q, 10, "jaccard"))
    for p in (None, 1, 3):
        c.ws = E.Workspace(torch.device(DEV))
        a = c.run(q, 10, "jaccard", pass_queries=p)
        b = c.run(q, 10, "jaccard", pass_queries=p)         # the same workspace again
        _assert_same(a, one)
        _assert_same(b, one)
        strips = 4 * min(len(q), p or P) * n
        assert int(c.ws.buf[:strips].count_nonzero()) == 0, "the strips are not left zero"


def test_the_strips_are_cleared_whatever_the_workspace_held():
    c = _parity()
    q = np.arange(40)
    want = c.ref(q, 10, "count")
    c.ws = E.Workspace(torch.device(DEV))
    c.run(q, 10, "count")
    c.ws.buf.fill_(0x5A)
    _assert_same(c.run(q, 10, "count"), want)
    c.ws = E.Workspace(torch.device(DEV))


# ---------------------------------------------------------------- long user row
def test_a_user_who_rated_every_item():
    n_i, n_u = 700, 20                      # 700 > one wavefront's stride and the workgroup's
    rng = np.random.default_rng(8)
    us = [0] * n_i + rng.integers(1, n_u, 900).tolist()
    it = list(range(n_i)) + rng.integers(0, n_i, 900).tolist()
    c = Case(np.array(us), np.array(it), n_u, n_i)
    c.check([0, 5, 699], 256, "jaccard")
    c.check([0], 30, "count", user_side=True)


# ---------------------------------------------------------------- edges
@functools.lru_cache(None)
def _edges():
    """10 users x 30 items.
    item 0: rated by user 0 alone, who rated nothing else      -> all-open list
    item 1: users 1, 2; user 1 also rated 2, 3; user 2 rated 2 -> 2 (c = 2), 3 (c = 1)
    item 4: no entry at all (a zero-entry row), like items 27 .. 29
    items 5 .. 24: users 3, 4 rated each of them once          -> twenty rows tie for query 25
    item 25: users 3, 4 (the query of the tie); user 5 rated it twice and item 26 twice
    """
    pairs = [(0, 0), (1, 1), (2, 1), (1, 2), (1, 3), (2, 2)]
    for u in (3, 4):
        pairs += [(u, j) for j in range(5, 26)]
    pairs += [(5, 25), (5, 25), (5, 26), (5, 26)]
    u, i = np.array(pairs).T
    return Case(u, i, 10, 30)


def test_edge_lists():
    c = _edges()
    idx, sc, com = c.check([0, 1, 4, -1, 30, 1, 29], 5, "count")
    assert (idx[[0, 2, 3, 4, 6]] == -1).all() and np.isneginf(sc[[0, 2, 3, 4, 6]]).all()
    assert (com[[0, 2, 3, 4, 6]] == 0).all()
    assert idx[1].tolist() == [2, 3, -1, -1, -1] and com[1].tolist() == [2, 1, 0, 0, 0]
    assert idx[5].tolist() == idx[1].tolist()              # a row given twice: two lists
    for measure in R.MEASURES:
        c.check(np.arange(-2, 32), 7, measure)
        c.check(np.arange(10), 4, measure, user_side=True)


def test_candidates_and_min_common_thresholds():
    c = _edges()
    allow = np.ones(30, bool)
    allow[2] = False                                       # query 1's best neighbour
    idx, _, com = c.check([1], 3, "count", allow=allow)
    assert idx[0].tolist() == [3, -1, -1] and com[0].tolist() == [1, 0, 0]
    idx, _, _ = c.check([1], 3, "count", min_common=2)     # exactly the best pair's count: kept
    assert idx[0].tolist() == [2, -1, -1]
    idx, _, _ = c.check([1], 3, "count", min_common=3)     # one above it: dropped
    assert (idx == -1).all()


def test_twenty_tied_rows_come_in_ascending_order_and_duplicates_multiply():
    c = _edges()
    idx, sc, com = c.check([25], 22, "count")
    # c(25, 26) = 2 x 2 leads (user 5's duplicates); 5 .. 24 tie at 2: ascending rows
    assert idx[0].tolist() == [26] + list(range(5, 25)) + [-1]
    assert com[0, 0] == 4 and (com[0, 1:21] == 2).all() and sc[0, 1] == 2.0
    idx, _, _ = c.check([25], 10, "jaccard")
    assert idx[0].tolist() == [26] + list(range(5, 14))
    c.check([25], 20, "cosine")                            # the cut falls inside the tie
    _, _, com = c.check([5], 3, "count", user_side=True)   # user 5: (25, 25, 26, 26) vs 3, 4
    assert com[0].tolist() == [2, 2, 0]


# ---------------------------------------------------------------- slices
def test_more_than_64_slices_take_the_two_stage_merge():
    n_i, n_u, top = 65 * 512, 24, 256                     # a slice holds at least 512 rows
    rng = np.random.default_rng(13)
    us, it = [], []
    for u in range(n_u):
        mine = [7] + rng.integers(0, n_i, 300).tolist() + rng.integers(n_i - 600, n_i, 40).tolist()
        us += [u] * len(mine)
        it += mine
    c = Case(np.array(us), np.array(it), n_u, n_i)
    idx, _, _ = c.check([7, n_i - 1], top, "jaccard")
    assert (idx[0] >= 0).all() and len(set((idx[0] // 512).tolist())) > 32
    c.check([7], top, "count", min_common=2)


# ---------------------------------------------------------------- the public surface
@functools.lru_cache(None)
def _fitted():
    rng = np.random.default_rng(21)
    u = rng.integers(0, 90, 2500)
    i = np.minimum((rng.random(2500) ** 1.5 * 70).astype(np.int64), 69)
    keep = np.unique(np.stack([u, i], 1), axis=0)         # distinct pairs: a model's ratings
    u, i = keep[:, 0], keep[:, 1]
    uid, iid = (3 * u + 7).astype(np.int32), (5 * i + 11).astype(np.int32)    # ids are not rows
    r = rng.integers(1, 6, len(u)).astype(np.float32)
    return uid, iid, r


def _ref_by_id(uid, iid, ids, top, measure="jaccard", min_common=1, cand=None, user_side=False):
    """The reference over ids: {query id: [(neighbour id, score, common), ...]}."""
    us, ui = np.unique(uid, return_inverse=True)
    its, ii = np.unique(iid, return_inverse=True)
    B = R.multiplicity(ui, ii, len(us), len(its))
    table = us if user_side else its
    if user_side:
        B = B.T
    allow = None if cand is None else np.isin(table, cand)
    known = [x for x in sorted(set(int(v) for v in ids)) if x in set(table.tolist())]
    rows = np.searchsorted(table, known)
    idx, sc, com = R.co_rated(B, rows, top, measure, min_common, allow)
    return {k: [(int(table[a]), float(s), int(c)) for a, s, c in zip(idx[n], sc[n], com[n])
                if c > 0] for n, k in enumerate(known)}


def _lists(keys, ids, sc, com):
    keys, ids, sc, com = (x.cpu().numpy() for x in (keys, ids, sc, com))
    return {int(k): [(int(a), float(s), int(c)) for a, s, c in zip(ri, rs, rc) if c > 0]
            for k, ri, rs, rc in zip(keys, ids, sc, com)}


def test_engine_methods_return_ids():
    uid, iid, r = _fitted()
    core = E.ALSCore(uid, iid, r)
    core.fit(4, 1, 0.1)
    ask = [11, 16, 11, 9999, 356, -4]
    got = core.co_rated(ask, 6, measure="count", min_common=2)
    assert got[0].tolist() == [11, 16, 356] and got[1].dtype == torch.int32
    assert _lists(*got) == _ref_by_id(uid, iid, ask, 6, "count", 2)
    cand = np.unique(iid)[::2]
    assert _lists(*core.co_rated(ask, 6, candidates=cand)) == _ref_by_id(uid, iid, ask, 6,
                                                                          cand=cand)
    assert _lists(*core.co_rated([7, 10], 5, True)) == _ref_by_id(uid, iid, [7, 10], 5,
                                                                   user_side=True)
    every = core.co_rated_all(4)
    assert every[0].tolist() == np.unique(iid).tolist()
    assert _lists(*every) == _ref_by_id(uid, iid, np.unique(iid), 4)
    users = core.co_rated_all(3, True, measure="count")
    assert _lists(*users) == _ref_by_id(uid, iid, np.unique(uid), 3, "count", user_side=True)
    none = core.co_rated([9999], 3)
    assert none[0].numel() == 0 and tuple(none[1].shape) == (0, 3)
    bare = E.ALSCore.from_factors(np.unique(uid), core.U[:, :4], np.unique(iid), core.V[:, :4])
    with pytest.raises(ValueError, match="training ratings"):
        bare.co_rated([11], 3)
    with pytest.raises(ValueError, match="training ratings"):
        bare.co_rated_all(3)


def test_model_surfaces():
    import pandas as pd
    from als_mi355x import personal
    from als_mi355x.ml.recommendation import ALS
    from als_mi355x.mllib.recommendation import ALS as MLlibALS
    uid, iid, r = _fitted()
    model = ALS(rank=4, maxIter=1, regParam=0.1, seed=1).fit(
        pd.DataFrame({"user": uid, "item": iid, "rating": r}))

    def rows_of(df, col):
        return {int(k): [(a, s, c) for (a, s), c in zip(sim, com)]
                for k, sim, com in zip(df[col], df["similar"], df["common"])}

    ask = [16, 11, 9999]
    df = model.coRatedItems(pd.DataFrame({"item": ask}), 5)
    assert list(df.columns) == ["item", "similar", "common"]
    assert rows_of(df, "item") == _ref_by_id(uid, iid, ask, 5)
    df = model.coRatedItems(ask, 5, measure="cosine", minCommon=2)
    want = _ref_by_id(uid, iid, ask, 5, "cosine", 2)
    got = rows_of(df, "item")
    assert {k: [(a, c) for a, _, c in v] for k, v in got.items()} == \
           {k: [(a, c) for a, _, c in v] for k, v in want.items()}
    df = model.coRatedUsers([7, 10], 4, measure="count")
    assert rows_of(df, "user") == _ref_by_id(uid, iid, [7, 10], 4, "count", user_side=True)
    df = model.coRatedItemsForAllItems(3)
    assert rows_of(df, "item") == _ref_by_id(uid, iid, np.unique(iid), 3)

    agree = model.neighbourAgreement(np.unique(iid)[:20], 5)
    assert 0.0 <= agree <= 1.0
    # equal tables through a stubbed pair: the agreement of a list with itself is 1
    core = model.engine
    keys, ids, sc, com = core.co_rated(np.unique(iid)[:20], 5)
    full = (com > 0).all(1)
    stub_ids = keys[full]
    real = core.similar
    core.similar = lambda ids_, top, user_side=False, **kw: core.co_rated(ids_, top, user_side)[:3]
    try:
        assert full.any() and model.neighbourAgreement(stub_ids, 5) == 1.0
    finally:
        core.similar = real

    m2 = MLlibALS.train(list(zip(uid.tolist(), iid.tolist(), r.tolist())), 4, iterations=1,
                        seed=2)
    assert m2.coRatedProducts(16, 5) == _ref_by_id(uid, iid, [16], 5)[16]
    assert m2.coRatedUsers(7, 3, measure="count") == _ref_by_id(uid, iid, [7], 3, "count",
                                                                user_side=True)[7]
    with pytest.raises(KeyError):
        m2.coRatedProducts(9999, 5)

    movies = [(int(m), f"movie {m}") for m in np.unique(iid)[:-1]]      # the last has no title
    counts = dict(zip(*np.unique(iid, return_counts=True)))
    cut = int(np.median(list(counts.values())))
    out = personal.also_rated_movies(m2, movies, 16, 8, min_ratings=cut)
    cand = np.array([m for m, n in counts.items() if n > cut], np.int32)
    want = _ref_by_id(uid, iid, [16], 8, cand=cand)[16]
    titles = dict(movies)
    assert out == [(s, titles.get(a, str(a)), c, int(counts[a])) for a, s, c in want]
    assert out and all(n > cut for _, _, _, n in out)
    assert personal.also_rated_movies(m2, movies, 9999, 8) == []


def test_neighbours_follow_added_and_removed_ratings():
    uid, iid, r = _fitted()
    core = E.ALSCore(uid, iid, r)
    core.fit(4, 1, 0.1)
    add_u = np.array([7, 7, 1000, 1000, 10], np.int32)      # known and new users and items
    add_i = np.array([16, 2000, 16, 11, 2000], np.int32)
    have = set(zip(uid.tolist(), iid.tolist()))
    assert not have & set(zip(add_u.tolist(), add_i.tolist()))
    core.add_ratings(add_u, add_i, np.full(5, 4.0, np.float32))
    u2, i2 = np.concatenate([uid, add_u]), np.concatenate([iid, add_i])
    ask = [16, 11, 2000, 21]
    assert _lists(*core.co_rated(ask, 8, measure="count")) == _ref_by_id(u2, i2, ask, 8, "count")
    drop = np.arange(0, len(uid), 7)
    core.remove_ratings(uid[drop], iid[drop])
    keep = np.ones(len(u2), bool)
    keep[drop] = False
    u3, i3 = u2[keep], i2[keep]
    assert _lists(*core.co_rated(ask, 8)) == _ref_by_id(u3, i3, ask, 8)
    assert _lists(*core.co_rated([7, 1000], 5, True)) == _ref_by_id(u3, i3, [7, 1000], 5,
                                                                     user_side=True)
